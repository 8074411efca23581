"""CPU: `MlpDx.rollout`, `MlpDx.prediction_loss` and the C ABI of `dmpc_mlp_rollout_grad` - exported, declared in
include/dmpc_mlp_rollout_grad.h, bound from `_lib.ROLLOUT_GRAD_SIGNATURES`, a memory-contract row for every symbol that takes a
pointer; the workspace formula and the partial counts; every argument and size check before any launch (no GPU is present
here) - the routes on CPU tensors, the start-major order of the window folding, `u` with T - 1 rows, and the sweep the kernels
evaluate restated in float64 against autograd of the live loop."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import MlpDx, _lib
from chainer_differentiable_mpc_amd.mlp_dx import _ACT_FN
from tests import mlp_rollout_grad_cases as rc
from tests.helpers import assert_close, npy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dmpc_mlp_rollout_grad_partials", "dmpc_mlp_rollout_grad_workspace_bytes", "dmpc_mlp_rollout_grad")
code = _lib.mlp_hidden2


def floats(nx, nu, H1, H2=0):
    if H2 == 0:
        return H1 * (nx + nu) + H1 + nx * H1 + nx
    return H1 * (nx + nu) + H1 + H2 * H1 + nx * H2 + H2 + nx


def test_the_symbols_are_exported_declared_and_bound_in_a_table_of_their_own():
    lib = _lib.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmpc_mlp_rollout_grad.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(dmpc_[a-z0-9_]+)\s*\(", txt))) == sorted(NEW) == sorted(_lib.ROLLOUT_GRAD_SIGNATURES)
    for name in NEW:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.ROLLOUT_GRAD_SIGNATURES[name][1]
        assert name not in _lib.SIGNATURES and name not in _lib.GRAD_SIGNATURES and name not in _lib.EPISODE_SIGNATURES
    assert _lib.ROLLOUT_GRAD_SIGNATURES["dmpc_mlp_rollout_grad"] == _lib.SIGNATURES["dmpc_mlp_param_grad"]     # the same argument list
    # the header's parameter count, read from its text
    decl = re.search(r"int\s+dmpc_mlp_rollout_grad\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
    assert len(decl.split(",")) == len(_lib.ROLLOUT_GRAD_SIGNATURES["dmpc_mlp_rollout_grad"][1]) == 23
    assert lib.dmpc_version() == _lib.ABI_VERSION == 411


def test_every_new_entry_point_with_a_device_pointer_has_a_memory_contract_row():
    from tests.arena import Builder
    from tests.test_mlp_rollout_grad_memory_gpu import ROWS
    lib = _lib.load()
    with_pointers = {name for name, (_, args) in _lib.ROLLOUT_GRAD_SIGNATURES.items() if ctypes.c_void_p in args}
    assert with_pointers == {"dmpc_mlp_rollout_grad"}
    assert {r.entry for r in ROWS} == with_pointers and len(ROWS) == 8
    for r in ROWS:
        b = Builder()
        prepare, (entry, args) = r.make(b, lib)
        assert entry == r.entry and len(args) == len(_lib.ROLLOUT_GRAD_SIGNATURES[entry][1]), r.id
        for layout in "AB":
            a = b.build(layout, "cpu")
            assert all(a.ptr(s) % 16 == 0 for s in b.specs) and a.nbytes < 8 << 20, r.id


def test_the_partials_and_the_workspace_are_those_of_the_weight_gradients():
    lib = _lib.load()
    part, need = lib.dmpc_mlp_rollout_grad_partials, lib.dmpc_mlp_rollout_grad_workspace_bytes
    two = code(5, 7)
    assert [part(B, 5) for B in (-3, 0, 1, 4, 5, 511, 512, 513, 1 << 30)] == [0, 0, 1, 4, 5, 511, 512, 512, 512]
    assert [part(B, two) for B in (-3, 0, 1, 4, 5, 8, 9, 1023, 1024, 1025, 1 << 30)] == [0, 0, 1, 1, 2, 2, 3, 256, 256, 256, 256]
    assert part(4, 0) == 0 and part(4, -1) == 0
    for B in (1, 4, 5, 7, 600, 100000):
        assert part(B, 5) == lib.dmpc_mlp_param_grad_partials(B) and part(B, two) == lib.dmpc_mlp2_param_grad_partials(B)
        for nx, nu, H1, H2 in ((3, 1, 5, 0), (16, 8, 256, 0), (1, 1, 1, 0), (3, 1, 5, 7), (16, 8, 128, 128), (1, 1, 1, 1)):
            h = H1 if H2 == 0 else code(H1, H2)
            assert need(B, nx, nu, h) == part(B, h) * floats(nx, nu, H1, H2) * 4 > 0
            other = lib.dmpc_mlp_param_grad_workspace_bytes if H2 == 0 else lib.dmpc_mlp2_param_grad_workspace_bytes
            assert need(B, nx, nu, h) == other(B, nx, nu, h)
    assert need(0, 3, 1, 5) == 0 and need(4, 0, 1, 5) == 0 and need(4, 3, 0, 5) == 0
    for nx, nu, h in ((17, 1, 5), (3, 9, 5), (3, 1, 257), (3, 1, 0), (3, 1, -1), (3, 1, code(129, 7)), (3, 1, code(5, 129)), (3, 1, code(0, 7))):
        assert need(4, nx, nu, h) == 0, (nx, nu, h)


def test_rollout_grad_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)       # a non-NULL pointer: the size checks come before anything reads it
    need = lib.dmpc_mlp_rollout_grad_workspace_bytes

    def grad(nx, nu, H, act, ptr=p, T=2, B=1, ws=p, ws_bytes=None, opt=p, grad_x=p):
        if ws_bytes is None:
            ws_bytes = 1 << 40
        return lib.dmpc_mlp_rollout_grad(T, B, nx, nu, H, act, 1, *([ptr] * 6), grad_x, *([ptr] * 4), opt, opt, ws, ws_bytes, None)

    for H in (5, code(5, 7)):
        assert grad(3, 1, H, 0, ptr=None) == _lib.E_BADARG                                      # NULL
        assert grad(3, 1, H, 0, ptr=None, opt=None, ws=None, ws_bytes=0) == _lib.E_BADARG
        assert grad(3, 1, H, 0, grad_x=None) == _lib.E_BADARG and grad(3, 1, H, 0, grad_x=None, T=1) == _lib.E_BADARG
        assert grad(3, 1, H, 0, T=0) == _lib.E_BADARG and grad(3, 1, H, 0, B=0) == _lib.E_BADARG
        assert grad(0, 1, H, 0) == _lib.E_BADARG and grad(3, 0, H, 0) == _lib.E_BADARG
        assert grad(17, 1, H, 0, ptr=None) == _lib.E_BADARG                                     # NULL before the size
        for act in (1, 5, -1):
            assert grad(3, 1, H, act) == _lib.E_UNSUPPORTED and grad(3, 1, H, act, ws_bytes=0) == _lib.E_UNSUPPORTED
        assert grad(17, 1, H, 0) == _lib.E_UNSUPPORTED and grad(3, 9, H, 0) == _lib.E_UNSUPPORTED
        assert grad(17, 1, H, 0, ws_bytes=0) == _lib.E_UNSUPPORTED                              # the size before the workspace
    for Hc in (257, 0, -1, code(129, 7), code(5, 129), code(0, 7)):
        assert grad(3, 1, Hc, 0) == _lib.E_UNSUPPORTED, Hc
    assert grad(16, 8, 256, 0, T=1 << 12, B=1 << 12) == _lib.E_UNSUPPORTED                      # the rollout's 2^31 limit
    assert grad(16, 8, code(128, 128), 0, T=1 << 12, B=1 << 12) == _lib.E_UNSUPPORTED
    for nx, nu, h in ((3, 1, 5), (16, 8, 256), (3, 1, code(5, 7)), (16, 8, code(128, 128)), (1, 1, code(1, 1))):
        for B in (1, 4, 5, 7, 100000):
            n = need(B, nx, nu, h)
            assert n > 0
            assert grad(nx, nu, h, 0, B=B, ws_bytes=n - 1) == _lib.E_WORKSPACE
            assert grad(nx, nu, h, 0, B=B, ws=None, ws_bytes=n) == _lib.E_WORKSPACE


# ---- the Python face on CPU tensors
def explicit_loop(m, x_init, u, T):
    xs = [x_init]
    for t in range(T - 1):
        xs.append(m(xs[t], u[t]))
    return torch.stack(xs, 0)


@pytest.mark.parametrize("case", [rc.ONE[0], rc.TWO["A"]], ids=["one", "two"])
@pytest.mark.parametrize("activation", ["tanh", "relu", "silu", "softplus"])
def test_cpu_tensors_take_the_live_route_whatever_the_keyword_says(activation, case):
    nx, nu, B, T, s = rc.dims(case)
    x_init, u, g = (torch.as_tensor(a) for a in rc.inputs(case))
    live = rc.run(rc.model(activation, case, "cpu", torch.float64), case, "cpu", torch.float64)
    m = rc.model(activation, case, "cpu", torch.float64, param_grad="device")
    got = rc.run(m, case, "cpu", torch.float64)
    for k in live:
        assert torch.equal(live[k], got[k]), k
    assert torch.equal(got["x"], explicit_loop(m, x_init, u, T).detach())
    with torch.no_grad():                        # no gradient wanted: the torch restatement of the one-launch rollout
        assert torch.equal(m.rollout(x_init, u), got["x"])
    assert float(got["x_init"].abs().max()) > 0 and float(got["u"][:-1].abs().max()) > 0 and not bool(got["u"][-1].any())


def test_u_with_one_row_less():
    case = rc.TWO["A"]
    nx, nu, B, T, s = rc.dims(case)
    m = rc.model("tanh", case, "cpu", torch.float64)
    full, short = rc.run(m, case, "cpu", torch.float64), rc.run(m, case, "cpu", torch.float64, u_rows=T - 1)
    assert tuple(short["u"].shape) == (T - 1, B, nu) and torch.equal(short["u"], full["u"][:-1])
    assert all(torch.equal(short[k], full[k]) for k in full if k != "u")
    x_init, u, _ = (torch.as_tensor(a) for a in rc.inputs(case))
    with torch.no_grad():
        assert torch.equal(m.rollout(x_init, u[:-1], T=T), full["x"])
        assert tuple(m.rollout(x_init, u[:-1]).shape) == (T - 1, B, nx)          # T is u's row count unless given
    for rows, bad in ((T - 1, T + 1), (T, T - 1), (T, T + 2), (T, 0)):
        with pytest.raises(ValueError, match="rows"):
            m.rollout(x_init, u[:rows], T=bad)


@pytest.mark.parametrize("n_hidden", rc.FIT_NETS, ids=["one", "two"])
@pytest.mark.parametrize("horizon", [None, 1, 3, 7])
def test_the_window_folding_against_a_hand_written_loop(n_hidden, horizon):
    """a window from every t = 0 .. T-1-h, each rolled h steps from the record's state under the record's controls; the mean over
    windows, steps >= 1 and components.  The folded batch is start-major: row start * B + b."""
    x, u = (torch.as_tensor(a) for a in rc.pendulum_record())
    T, B, nx = x.shape
    m = rc.fit_model(n_hidden, "cpu", torch.float64)
    weight = torch.tensor([1.0, 2.0, 0.25], dtype=torch.float64)
    h = T - 1 if horizon is None else horizon
    seen = {}
    plain = m.rollout
    m.rollout = lambda x0, uw, T=None: seen.setdefault("x", plain(x0, uw, T=T))
    try:
        got, got_w = m.prediction_loss(x, u, horizon=horizon), m.prediction_loss(x, u, horizon=horizon, weight=weight)
    finally:
        del m.rollout
    total, total_w, n = 0.0, 0.0, 0
    for start in range(T - h):
        xh = x[start]
        for s in range(1, h + 1):
            xh = m(xh, u[start + s - 1])
            assert torch.equal(seen["x"][s, start * B:(start + 1) * B], xh.detach())          # start-major
            total, total_w, n = total + ((xh - x[start + s]) ** 2).sum(), total_w + (weight * (xh - x[start + s]) ** 2).sum(), n + B * nx
    assert tuple(seen["x"].shape) == (h + 1, (T - h) * B, nx)
    assert_close(npy(got), npy(total / n), 1e-13, "prediction_loss")
    assert_close(npy(got_w), npy(total_w / n), 1e-13, "weighted prediction_loss")
    if horizon is None:
        assert torch.equal(got, m.prediction_loss(x, u, horizon=T - 1))
    u_full = torch.cat((u, torch.full((1, B, 1), 9.0, dtype=u.dtype)), 0)          # T rows: the last is never read
    assert torch.equal(m.prediction_loss(x, u_full, horizon=horizon), got)


def test_horizon_out_of_range_is_a_value_error():
    x, u = (torch.as_tensor(a) for a in rc.pendulum_record())
    m = rc.fit_model(16, "cpu", torch.float64)
    for bad in (0, -1, x.shape[0], x.shape[0] + 3):
        with pytest.raises(ValueError, match="horizon"):
            m.prediction_loss(x, u, horizon=bad)
    with pytest.raises(ValueError, match="horizon"):
        m.prediction_loss(x[:1], u[:0])                     # a record of one state has no step to predict
    with pytest.raises(ValueError, match="prediction_loss"):
        m.prediction_loss(x, u[:-1])                        # two rows short


def test_the_default_route_stays_live():
    assert MlpDx(3, 1, 5).param_grad == "live" and MlpDx(3, 1, (5, 7)).param_grad == "live"


# ---- the sweep of the kernels, restated in float64
@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("activation", ["tanh", "silu"])
@pytest.mark.parametrize("case", [rc.ONE[0], rc.ONE[2], rc.TWO["A"], rc.TWO["C"]], ids=["one-0", "one-2", "two-A", "two-C"])
def test_the_carried_co_state_against_float64_autograd_of_the_live_loop(case, activation, residual):
    """lam = g[T-1]; for t = T-2 .. 0: r = lam, the weight sums of the step, v = W1^T delta, d_u[t] = v[nx:],
    lam = g[t] + v[:nx] (+ r when residual); d_x_init = lam, d_u[T-1] = 0 - against autograd through the live loop at 1e-12"""
    nx, nu, B, T, s = rc.dims(case)
    ref = rc.reference(activation, case, residual)
    m = rc.model(activation, case, "cpu", torch.float64, residual)
    x_init, u, g = (torch.as_tensor(a) for a in rc.inputs(case))
    act, dact = _ACT_FN[activation]
    got = {k: torch.zeros_like(p) for k, p in zip(rc.names(case), m._weights())}
    du = torch.zeros_like(u)
    with torch.no_grad():
        x = explicit_loop(m, x_init, u, T)
        lam = g[T - 1]
        for t in range(T - 2, -1, -1):
            tau, r = torch.cat((x[t], u[t]), 1), lam
            z1 = tau @ m.W1.t() + m.b1
            a1, d1 = act(z1), dact(z1)
            if rc.depth(case) == 1:
                got["W2"] += r.t() @ a1
                got["b2"] += r.sum(0)
                e1 = d1 * (r @ m.W2)
            else:
                z2 = a1 @ m.W2.t() + m.b2
                a2, d2 = act(z2), dact(z2)
                got["W3"] += r.t() @ a2
                got["b3"] += r.sum(0)
                e2 = d2 * (r @ m.W3)
                got["W2"] += e2.t() @ a1
                got["b2"] += e2.sum(0)
                e1 = d1 * (e2 @ m.W2)
            got["W1"] += e1.t() @ tau
            got["b1"] += e1.sum(0)
            v = e1 @ m.W1
            du[t] = v[:, nx:]
            lam = g[t] + v[:, :nx] + (r if residual else 0.0)
    for name in rc.names(case):
        assert float(np.abs(ref[name]).max()) > 0, name
        assert_close(npy(got[name]), ref[name], 1e-12, "d/d" + name)
    assert_close(npy(lam), ref["x_init"], 1e-12, "d/dx_init")
    assert_close(npy(du), ref["u"], 1e-12, "d/du")
