"""CPU: MPC with tiled dynamics - what can be checked without a GPU: the two entry points are declared,
exported and bound, their argument checks answer before any launch, `TiledLinDx` and `MpcNet_dx(shared=True)` hold what
they say."""
import os
import re

import numpy as np
import torch

from chainer_differentiable_mpc_amd import LinDx, MpcNet_dx, TiledLinDx, _lib, expand_time_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dmpc_mpc_step_shared_grad_workspace_bytes", "dmpc_mpc_step_backward_shared")
F_TIME, CVEC_BATCH, FVEC_BATCH = 2, 8, 32


def test_entry_points_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "dmpc.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared in include/dmpc.h" % s
        assert hasattr(lib, s), "libdmpc_hip.so lacks %s" % s
        assert s in _lib.SIGNATURES
    assert lib.dmpc_version() == _lib.ABI_VERSION == 411          # adding symbols does not move the ABI number


def _call(lib, T, B, nx, nu, layout, F_hat=4096, ws=4096, ws_bytes=1 << 40):
    """made-up (aligned, never dereferenced) addresses: every answer below comes back before anything is launched"""
    p = 4096
    return lib.dmpc_mpc_step_backward_shared(T, B, nx, nu, layout, p, p, F_hat, p, p, p, p, p, p, p, None, None, p, None,
                                             None, None, 0.0, ws, ws_bytes, None, None)


def test_argument_errors_come_back_before_any_launch():
    lib = _lib.load()
    assert _call(lib, 5, 8, 3, 1, CVEC_BATCH) == _lib.E_BADARG
    assert _call(lib, 5, 8, 3, 1, F_TIME | FVEC_BATCH) == _lib.E_BADARG
    assert _call(lib, 5, 8, 3, 1, 0, F_hat=None) == _lib.E_BADARG
    assert _call(lib, 1, 8, 3, 1, 0) == _lib.E_BADARG                     # no dynamics to differentiate at T = 1
    need = lib.dmpc_mpc_step_shared_grad_workspace_bytes(5, 8, 3, 1)
    assert need > 0
    assert _call(lib, 5, 8, 3, 1, 0, ws_bytes=need - 1) == _lib.E_WORKSPACE
    assert _call(lib, 5, 8, 33, 1, 0) == _lib.E_UNSUPPORTED
    assert _call(lib, 5, 8, 3, 9, F_TIME) == _lib.E_UNSUPPORTED


def test_workspace_query():
    lib = _lib.load()
    assert lib.dmpc_mpc_step_shared_grad_workspace_bytes(5, 8, 33, 1) == 0
    assert lib.dmpc_mpc_step_shared_grad_workspace_bytes(5, 8, 3, 9) == 0
    assert lib.dmpc_mpc_step_shared_grad_workspace_bytes(1, 8, 3, 1) == 0
    small, large = (lib.dmpc_mpc_step_shared_grad_workspace_bytes(5, B, 32, 8) for B in (1, 1091))
    assert 0 < small < large
    # no dense gradient in it: far below the [T,B,ns,ns] + [T-1,B,nx,ns] floats the generic node allocates
    T, B, nx, nu = 50, 4096, 8, 2
    dense = 4 * (T * B * (nx + nu) ** 2 + (T - 1) * B * nx * (nx + nu))
    assert lib.dmpc_mpc_step_shared_grad_workspace_bytes(T, B, nx, nu) < dense


def test_tiled_lin_dx_tiles_equal_the_expanded_leaves_and_are_detached():
    T, B, nx, nu = 5, 4, 3, 2
    g = torch.Generator().manual_seed(0)
    AB = torch.randn(nx, nx + nu, generator=g, dtype=torch.float64, requires_grad=True)
    f0 = torch.randn(nx, generator=g, dtype=torch.float64, requires_grad=True)
    d = TiledLinDx(AB, f0, T, B)
    assert isinstance(d, LinDx) and d.AB is AB and d.f0 is f0
    assert torch.equal(d.F, expand_time_batch(AB.detach(), T - 1, B)) and torch.equal(d.f, expand_time_batch(f0.detach(), T - 1, B))
    assert d.F.is_contiguous() and d.f.is_contiguous() and not d.F.requires_grad and not d.f.requires_grad
    F_, f_ = d                                                          # still the namedtuple (F, f)
    assert F_ is d.F and f_ is d.f
    ABt = torch.randn(T - 1, nx, nx + nu, generator=g)                  # with a time axis, and no f
    dt = TiledLinDx(ABt, None, T, B)
    assert dt.f is None and dt.f0 is None and tuple(dt.F.shape) == (T - 1, B, nx, nx + nu)
    assert torch.equal(dt.F, ABt[:, None].expand(T - 1, B, nx, nx + nu))
    f0t = torch.randn(T - 1, nx, generator=g)
    assert torch.equal(TiledLinDx(ABt, f0t, T, B).f, f0t[:, None].expand(T - 1, B, nx))


def test_from_tiles_makes_no_copy():
    T, B, nx, nu = 4, 3, 2, 1
    AB = torch.ones(nx, nx + nu, requires_grad=True)
    F = expand_time_batch(AB.detach(), T - 1, B).contiguous()
    f = torch.zeros(T - 1, B, nx)
    d = TiledLinDx.from_tiles(F, f, AB, None)
    assert d.F is F and d.f is f and d.AB is AB and d.f0 is None
    assert d.F.data_ptr() == F.data_ptr()


def test_mpcnet_shared_draws_the_same_parameters_and_keeps_its_tiles():
    T, B, nx, nu = 5, 6, 3, 2
    lo, hi = torch.full((T, B, nu), -1.0), torch.full((T, B, nu), 1.0)
    dense = MpcNet_dx(T, lo, hi, B, nx, nu, seed=1, u_init=None, quiet=True)
    shared = MpcNet_dx(T, lo, hi, B, nx, nu, seed=1, u_init=None, quiet=True, shared=True)
    np.testing.assert_array_equal(shared.A.detach().numpy(), dense.A.detach().numpy())
    np.testing.assert_array_equal(shared.B.detach().numpy(), dense.B.detach().numpy())
    assert shared.shared and not dense.shared
    ab = torch.cat((shared.A, shared.B), dim=1)
    d1 = shared._shared_dynamics(ab)
    assert isinstance(d1, TiledLinDx) and d1.AB is ab and d1.f0 is None and not d1.F.requires_grad
    assert torch.equal(d1.F, expand_time_batch(ab.detach(), T - 1, B)) and float(d1.f.abs().max()) == 0.0
    p_F, p_f = d1.F.data_ptr(), d1.f.data_ptr()
    with torch.no_grad():
        shared.A.add_(1.0)
    ab2 = torch.cat((shared.A, shared.B), dim=1)
    d2 = shared._shared_dynamics(ab2)                                   # refreshed in place: same buffers, new values
    assert d2.F.data_ptr() == p_F and d2.f.data_ptr() == p_f
    assert torch.equal(d2.F, expand_time_batch(ab2.detach(), T - 1, B))
