"""CPU: LQR with batch-shared C and F - which inputs take the shared path, the expand fallback's shapes,
sharding of batch-free inputs, the C-ABI's argument checks, and the float64 reference the GPU tests hold the shared
gradients to (the oracle's dense gradient summed over the batch and time) against finite differences of the oracle."""
import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import _lib, dist as dmdist, lqr_shared
from tests import shared_lqr_problems as sp

T, B = 6, 5


def shapes(nx, nu):
    ns = nx + nu
    return dict(C={"full": (T, B, ns, ns), "time": (T, ns, ns), "shared": (ns, ns)},
                F={"full": (T - 1, B, nx, ns), "time": (T - 1, nx, ns), "shared": (nx, ns)},
                c={"full": (T, B, ns), "time": (T, ns), "shared": (ns,)},
                f={"none": None, "full": (T - 1, B, nx), "time": (T - 1, nx), "shared": (nx,)})


@pytest.mark.parametrize("nx,nu", [(3, 1), (8, 2), (32, 8), (40, 4), (12, 9)])
@pytest.mark.parametrize("precision", ["float32", "float64"])
def test_shape_classification_table(nx, nu, precision):
    S = shapes(nx, nu)
    z = lambda s: None if s is None else torch.zeros(s)
    for kC, sC in S["C"].items():
        for kF, sF in S["F"].items():
            for kc, sc in S["c"].items():
                for kf, sf in S["f"].items():
                    C, F, c, f = z(sC), z(sF), z(sc), z(sf)
                    lqr_shared.check_shapes(T, B, nx, nu, C, c, F, f)
                    got = lqr_shared.classify(T, nx, nu, C, c, F, f, precision)
                    if kC == kF == kc == "full" and kf in ("none", "full"):
                        want = "full"
                    elif kC != "full" and kF != "full" and precision == "float32" and nx <= 32 and nu <= 8:
                        want = "shared"
                    else:
                        want = "expand"
                    assert got == want, (kC, kF, kc, kf, precision, got)
                    if want == "full":
                        continue
                    eC, ec, eF, ef = lqr_shared.expand_full(T, B, C, c, F, f)
                    assert lqr_shared.is_full(eC, ec, eF, ef)
                    assert tuple(eC.shape) == S["C"]["full"] and tuple(ec.shape) == S["c"]["full"]
                    assert tuple(eF.shape) == S["F"]["full"] and (ef is None or tuple(ef.shape) == S["f"]["full"])


def test_layout_bits_and_full_shape_expand_views():
    nx, nu = 4, 2
    S = shapes(nx, nu)
    C, c, F, f = torch.zeros(S["C"]["time"]), torch.zeros(S["c"]["full"]), torch.zeros(S["F"]["shared"]), torch.zeros(
        S["f"]["time"])
    lay = lqr_shared.layout_of(C, c, F, f)
    assert lay == lqr_shared.SHARED_C_TIME | lqr_shared.SHARED_CVEC_TIME | lqr_shared.SHARED_CVEC_BATCH | \
        lqr_shared.SHARED_FVEC_TIME
    # an expand view of full shape is a full input: today's path, whatever its strides
    Cv = torch.eye(nx + nu).expand(*S["C"]["full"])
    Fv = torch.zeros(nx, nx + nu).expand(*S["F"]["full"])
    assert lqr_shared.classify(T, nx, nu, Cv, torch.zeros(S["c"]["full"]), Fv, None) == "full"


def test_expand_path_gradients_are_summed_to_the_input_shape():
    g = torch.arange(2 * 3 * 4, dtype=torch.float64).reshape(2, 3, 4)
    assert torch.equal(lqr_shared.reduce_to(g, (2, 4)), g.sum(1))
    assert torch.equal(lqr_shared.reduce_to(g, (4,)), g.sum((0, 1)))
    assert lqr_shared.reduce_to(g, (2, 3, 4)) is g


def test_shard_problem_passes_batch_free_inputs_through():
    nx, nu = 3, 1
    S = shapes(nx, nu)
    x0 = torch.randn(B, nx)
    C, c, F, f = torch.randn(S["C"]["shared"]), torch.randn(S["c"]["full"]), torch.randn(S["F"]["time"]), \
        torch.randn(S["f"]["shared"])
    parts = [dmdist.shard_problem(x0, C, c, F, f, rank=r, world=2) for r in range(2)]
    for r, (xs, Cs, cs, Fs, fs) in enumerate(parts):
        b0, b1 = dmdist.shard_bounds(B, r, 2)
        assert torch.equal(xs, x0[b0:b1]) and torch.equal(cs, c[:, b0:b1])
        assert Cs is C and Fs is F and fs is f
    full = dmdist.shard_problem(x0, torch.randn(S["C"]["full"]), c, torch.randn(S["F"]["full"]), None, rank=1, world=2)
    assert full[1].shape[1] == dmdist.shard_bounds(B, 1, 2)[1] - dmdist.shard_bounds(B, 1, 2)[0]


def _loss(p, wx, wu):
    x, u = sp.solve(p)
    return float((x * wx).sum() + (u * wu).sum())


@pytest.mark.parametrize("case", [
    dict(nx=3, nu=1, T=4, B=3, f_kind="shared"),
    dict(nx=2, nu=2, T=3, B=2, C_time=True, F_time=True, c_kind="time", f_kind="time"),
    dict(nx=3, nu=2, T=4, B=3, c_kind="batch", f_kind="batch"),
])
def test_summed_oracle_gradient_is_the_gradient_of_the_shared_inputs(case):
    """with strict_math the oracle's dense gradient, summed over the axes a reduced input lacks, is d loss / d input:
    central differences of the float64 oracle solve (symmetric C: the KKT gradient reads C's rows as its columns; for C
    itself, whose gradient is symmetrised, the symmetric part is compared)"""
    p = sp.make(seed=11, **case)
    rng = np.random.default_rng(2)
    T_, B_, nx, nu = p["T"], p["B"], p["nx"], p["nu"]
    wx, wu = rng.standard_normal((T_, B_, nx)), rng.standard_normal((T_, B_, nu))
    x, u = sp.solve(p)
    got = dict(zip(("x_init", "C", "c", "F", "f"), sp.grads(p, x, u, wx, wu, strict_math=True)))
    h = 1e-6
    for key in ("x_init", "C", "c", "F", "f"):
        if p[key] is None:
            continue
        a = p[key]
        num = np.zeros_like(a)
        for idx in np.ndindex(a.shape):
            keep = a[idx]
            a[idx] = keep + h
            lp = _loss(p, wx, wu)
            a[idx] = keep - h
            lm = _loss(p, wx, wu)
            a[idx] = keep
            num[idx] = (lp - lm) / (2 * h)
        g = got[key]
        if key == "C":
            sym = lambda m: 0.5 * (m + np.swapaxes(m, -1, -2))
            g, num = sym(g), sym(num)
        err = np.abs(g - num).max() / max(1.0, np.abs(num).max())
        assert err < 1e-5, (key, err)


def test_cabi_argument_checks_before_any_launch():
    lib = _lib.load()
    p = 0x1000
    assert lib.dmpc_lqr_shared_workspace_bytes(50, 4096, 8, 2) > 50 * 4096 * 2 * 4
    assert lib.dmpc_lqr_shared_saved_bytes(50, 8, 2) < lib.dmpc_lqr_shared_workspace_bytes(50, 4096, 8, 2)
    assert lib.dmpc_lqr_shared_grad_workspace_bytes(50, 4096, 8, 2) > 50 * 4096 * (10 + 16) * 4
    assert lib.dmpc_lqr_shared_workspace_bytes(50, 4096, 40, 4) == 0
    assert lib.dmpc_lqr_shared_workspace_bytes(0, 4096, 8, 2) == 0
    ws = lib.dmpc_lqr_shared_workspace_bytes(5, 16, 8, 2)
    args = lambda layout=0, nx=8, nu=2, T=5, C=p, ws_bytes=ws: (T, 16, nx, nu, layout, C, p, p, None, p, p, p, p, ws_bytes,
                                                                 None, None)
    assert lib.dmpc_lqr_shared_solve(*args(C=None)) == _lib.E_BADARG
    assert lib.dmpc_lqr_shared_solve(*args(T=0)) == _lib.E_BADARG
    assert lib.dmpc_lqr_shared_solve(*args(layout=64)) == _lib.E_BADARG
    assert lib.dmpc_lqr_shared_solve(*args(layout=lqr_shared.SHARED_CVEC_BATCH)) == _lib.E_BADARG
    assert lib.dmpc_lqr_shared_solve(*args(layout=lqr_shared.SHARED_FVEC_TIME | lqr_shared.SHARED_FVEC_BATCH)) == \
        _lib.E_BADARG          # f per trajectory, but f is NULL
    assert lib.dmpc_lqr_shared_solve(*args(C=p + 4)) == _lib.E_BADARG
    assert lib.dmpc_lqr_shared_solve(*args(nx=40, nu=4)) == _lib.E_UNSUPPORTED
    assert lib.dmpc_lqr_shared_solve(*args(nx=8, nu=9)) == _lib.E_UNSUPPORTED
    assert lib.dmpc_lqr_shared_solve(*args(ws_bytes=ws - 1)) == _lib.E_WORKSPACE
    gws = lib.dmpc_lqr_shared_grad_workspace_bytes(5, 16, 8, 2)
    g = lambda dc=p, ws_bytes=gws, nx=8: (5, 16, nx, 2, 0, p, p, p, p, p, p, p, p, 0, p, None, dc, None, None, p,
                                          ws_bytes, None, None)
    assert lib.dmpc_lqr_shared_kkt_grad(*g(dc=None)) == _lib.E_BADARG
    assert lib.dmpc_lqr_shared_kkt_grad(*g(nx=33)) == _lib.E_UNSUPPORTED
    assert lib.dmpc_lqr_shared_kkt_grad(*g(ws_bytes=gws - 1)) == _lib.E_WORKSPACE
