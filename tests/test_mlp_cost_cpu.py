"""CPU: `MlpCost` - the torch module against the float64 numpy restatement of tests/mlp_cost_cases.py, the closed forms of its
Taylor model and of its parameter gradient against central differences and against `approximate_cost`'s autograd route, the
hooks' decisions on CPU tensors, `soft_box`, what the C ABI of include/dmpc_mlp_cost.h answers before its first launch (dummy
pointers, never dereferenced), and the conditions the GPU tests rely on, decided by the float64 oracle."""
import os
import re

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import MlpCost, _lib, approximate_cost
from tests import mlp_cost_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096          # a dummy device pointer: 16-byte aligned, never dereferenced by a refused call
CASES = [(act, name) for name in mc.CASE for act in mc.ACTS]
IDS = ["%s-%s" % (name, act) for act, name in CASES]


def cpu_module(Pb, **kw):
    return mc.module(Pb, device="cpu", dtype=torch.float64, **kw)


def points(Pb, seed=3):
    nx, nu, H, B, T = Pb["dims"]
    rs = np.random.RandomState(seed)
    return rs.randn(T, B, nx), rs.uniform(-0.6, 0.6, (T, B, nu))


@pytest.mark.parametrize("act,name", CASES, ids=IDS)
def test_the_module_is_the_numpy_cost_in_float64(act, name):
    Pb = mc.problem(act, name)
    x, u = points(Pb)
    tau = np.concatenate((x, u), axis=2)
    m = cpu_module(Pb)
    with torch.no_grad():
        got = torch.stack([m(torch.as_tensor(tau[t])) for t in range(tau.shape[0])]).numpy()
    np.testing.assert_allclose(got, Pb["cost"](tau), rtol=1e-12, atol=1e-12)
    assert m(torch.as_tensor(tau[0, 0])).shape == ()


@pytest.mark.parametrize("act", mc.ACTS)
def test_closed_forms_against_central_differences(act):
    Pb = mc.problem(act, "A")
    cost = Pb["cost"]
    x, u = points(Pb)
    tau = np.concatenate((x, u), axis=2).reshape(-1, 4)
    H, g0, _ = cost.taylor(tau)
    grad = g0 + np.einsum("bij,bj->bi", H, tau)
    h = 1e-5
    for j in range(4):
        e = np.zeros(4)
        e[j] = h
        np.testing.assert_allclose((cost(tau + e) - cost(tau - e)) / (2 * h), grad[:, j], rtol=1e-7, atol=1e-8)
        gp = cost.taylor(tau + e)
        gm = cost.taylor(tau - e)
        grad_p = gp[1] + np.einsum("bij,bj->bi", gp[0], tau + e)
        grad_m = gm[1] + np.einsum("bij,bj->bi", gm[0], tau - e)
        np.testing.assert_allclose((grad_p - grad_m) / (2 * h), H[:, :, j], rtol=1e-6, atol=1e-7)
    assert np.array_equal(H, np.swapaxes(H, 1, 2)) or np.abs(H - np.swapaxes(H, 1, 2)).max() < 1e-15


@pytest.mark.parametrize("act,name", CASES, ids=IDS)
def test_closed_forms_and_gradient_sums_against_the_autograd_route(act, name):
    """`approximate_cost` on CPU tensors in float64 (T (1 + ns) autograd calls) is the yardstick of every device route"""
    Pb = mc.problem(act, name)
    nx, nu, H, B, T = Pb["dims"]
    x, u = points(Pb)
    rs = np.random.RandomState(7)
    v, r = rs.randn(T, B, nx + nu), rs.randn(T, B)
    m = cpu_module(Pb)
    Hs, g0, costs = approximate_cost(torch.as_tensor(x), torch.as_tensor(u), m)
    assert not Hs.requires_grad and g0.requires_grad and costs.requires_grad
    ref = Pb["cost"].taylor(np.concatenate((x, u), axis=2))
    for got, want in zip((Hs, g0, costs), ref):
        assert np.abs(got.detach().numpy() - want).max() <= 1e-10
    for vv, rr in ((v, r), (v, None), (None, r)):
        m.zero_grad()
        loss = 0.0
        if vv is not None:
            loss = loss + (torch.as_tensor(vv) * g0).sum()
        if rr is not None:
            loss = loss + (torch.as_tensor(rr) * costs).sum()
        loss.backward(retain_graph=True)
        sums = Pb["cost"].grad_sums(np.concatenate((x, u), axis=2), vv, rr)
        for w, want in zip((m.Q, m.p, m.W1, m.b1, m.w2), sums):
            got = np.zeros_like(want) if w.grad is None else w.grad.numpy()
            assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())


def test_cpu_tensors_keep_the_autograd_route():
    Pb = mc.problem("softplus", "A")
    x, u = (torch.as_tensor(a) for a in points(Pb))
    for mode in ("live", "device"):
        m = cpu_module(Pb, param_grad=mode)
        assert m.approx_ok(x, u) is False
        with torch.no_grad():
            assert m.approx_ok(x, u) is False
        with pytest.raises(_lib.DmpcError):
            m.approximate(x, u)
        with pytest.raises(_lib.DmpcError):
            m.stage_costs(x, u)
        hidden = approximate_cost(x, u, lambda tau: m(tau))
        for got, want in zip(approximate_cost(x, u, m), hidden):
            assert torch.equal(got, want) and got.requires_grad == want.requires_grad


def test_constructor_defaults_and_arguments():
    m = MlpCost(3, 1, 5, seed=2)
    assert m.activation == "softplus" and m.param_grad == "live"
    assert torch.equal(m.Q.detach(), torch.eye(4)) and not m.p.detach().any() and not m.b1.detach().any()
    assert sorted(n for n, _ in m.named_parameters()) == ["Q", "W1", "b1", "p", "w2"]
    assert [tuple(w.shape) for w in (m.Q, m.p, m.W1, m.b1, m.w2)] == [(4, 4), (4,), (5, 4), (5,), (5,)]
    assert torch.equal(MlpCost(3, 1, 5, seed=2).W1, m.W1)
    assert "n_hidden=5" in repr(m) and "activation=softplus" in repr(m) and "param_grad" not in repr(m)
    assert "param_grad=device" in repr(MlpCost(3, 1, 5, param_grad="device"))
    Q = torch.arange(16.0).reshape(4, 4)
    assert torch.equal(MlpCost(3, 1, 5, Q=Q).Q.detach(), Q)            # as given: not symmetrised
    with pytest.raises(ValueError):
        MlpCost(3, 1, 5, activation="gelu")
    with pytest.raises(ValueError):
        MlpCost(3, 1, 5, param_grad="host")
    with pytest.raises(ValueError):
        MlpCost(3, 1, 0)
    with pytest.raises(ValueError):
        MlpCost(3, 1, 5, Q=torch.eye(3))
    assert [MlpCost(1, 1, 1, activation=a).act_code for a in mc.ACTS] == [0, 2, 3, 4]


def test_device_weights_are_made_on_every_call():
    m = MlpCost(3, 1, 5, seed=2).double()
    first = m.device_weights(torch.device("cpu"))
    assert all(w.dtype == torch.float32 and w.is_contiguous() and not w.requires_grad for w in first) and len(first) == 5
    with torch.no_grad():
        m.W1.mul_(0.5)
    again = m.device_weights(torch.device("cpu"))
    assert torch.equal(again[2], m.W1.detach().float()) and not torch.equal(again[2], first[2])


def test_soft_box_units_follow_their_formula():
    lo, hi = [-np.inf, -0.5, 0.25], [1.0, np.inf, 2.0]
    m = MlpCost.soft_box(3, 2, lo, hi, weight=3.0, sharpness=8.0)
    assert m.n_hidden == 4 and m.activation == "softplus"           # one unit per FINITE bound
    W1 = np.zeros((4, 5))
    W1[0, 0], W1[1, 1], W1[2, 2], W1[3, 2] = 8.0, -8.0, 8.0, -8.0
    assert np.array_equal(m.W1.detach().numpy(), W1)
    np.testing.assert_allclose(m.b1.detach().numpy(), [-8.0 * 1.0, 8.0 * -0.5, -8.0 * 2.0, 8.0 * 0.25])
    np.testing.assert_allclose(m.w2.detach().numpy(), np.full(4, 3.0 / 8.0))
    assert torch.equal(m.Q.detach(), torch.eye(5)) and not m.p.detach().any()
    m = MlpCost.soft_box(3, 2, lo, hi, weight=3.0, sharpness=8.0, Q=torch.zeros(5, 5))
    with torch.no_grad():
        inside = m(torch.tensor([[0.0, 0.5, 1.0, 9.0, -9.0]]))
        above = m(torch.tensor([[3.0, 0.5, 1.0, 0.0, 0.0]]))
        below = m(torch.tensor([[0.0, -2.5, 1.0, 0.0, 0.0]]))
    assert float(inside) < 3.0 / 8.0 * 4 * np.log1p(np.exp(-8.0 * 0.5)) + 1e-6      # every unit at least 0.5 inside its limit
    assert abs(float(above) - 3.0 * 2.0) < 0.01 and abs(float(below) - 3.0 * 2.0) < 0.01   # weight * violation
    with pytest.raises(ValueError):
        MlpCost.soft_box(2, 1, [-np.inf, -np.inf], [np.inf, np.inf])
    with pytest.raises(ValueError):
        MlpCost.soft_box(2, 1, [0.0], [1.0])
    sb = mc.soft_box_problem()
    m = MlpCost.soft_box(2, 1, sb["x_lower"], sb["x_upper"], weight=sb["weight"], sharpness=sb["sharpness"], Q=sb["Q"], p=sb["p"])
    for name in ("Q", "p", "W1", "b1", "w2"):
        np.testing.assert_allclose(getattr(m, name).detach().numpy(), getattr(sb["cost"], name), rtol=1e-7)


# ---------------------------------------------------------------------- the C ABI, before any launch
def test_the_header_declares_exactly_the_bound_symbols():
    txt = open(os.path.join(ROOT, "include", "dmpc_mlp_cost.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    assert sorted(set(re.findall(r"\b(dmpc_[a-z0-9_]+)\s*\(", txt))) == sorted(_lib.MLP_COST_SIGNATURES)
    for name, (res, args) in _lib.MLP_COST_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
        assert name not in _lib.SIGNATURES
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(decl.split(",")) == len(args), name
    assert lib.dmpc_version() == _lib.ABI_VERSION == 411


def test_supported_is_the_limits():
    lib = _lib.load()
    for act in (0, 2, 3, 4):
        assert lib.dmpc_mlp_cost_supported(16, 8, 256, act) == 1 and lib.dmpc_mlp_cost_supported(1, 1, 1, act) == 1
    for bad in ((17, 8, 256, 0), (16, 9, 256, 0), (16, 8, 257, 0), (3, 1, 5, 1), (3, 1, 5, 5), (3, 1, 5, -1), (0, 1, 5, 0),
                (3, 0, 5, 0), (3, 1, 0, 0)):
        assert lib.dmpc_mlp_cost_supported(*bad) == 0, bad
    assert MlpCost(3, 1, 5).supported() and not MlpCost(17, 1, 5).supported() and not MlpCost(3, 1, 257).supported()


def approx(lib, T=4, B=2, nx=3, nu=1, H=5, act=4, Q=P, x=P, Ho=P, go=P, co=P):
    return lib.dmpc_mlp_cost_approx(T, B, nx, nu, H, act, Q, P, P, P, P, x, P, Ho, go, co, None)


def search(lib, T=4, B=2, nx=3, nu=1, H=5, act=4, w2=P, F=P, f=None, costs=P):
    return lib.dmpc_mpc_forward_rec_mlp_cost(T, B, nx, nu, H, act, P, P, P, P, w2, P, P, P, P, P, P, F, f, 0.2, 10, P, P, costs,
                                             None, P, None, None, P, None, None)


def grad(lib, T=4, B=2, nx=3, nu=1, H=5, act=4, gg=P, gc=P, dQ=P, ws=P, short=0):
    need = lib.dmpc_mlp_cost_param_grad_workspace_bytes(T, B, nx, nu, H)
    return lib.dmpc_mlp_cost_param_grad(T, B, nx, nu, H, act, P, P, P, P, P, gg, gc, dQ, P, P, P, P, ws, max(need - short, 0), None)


def test_argument_errors_are_reported_before_any_launch():
    lib = _lib.load()
    for call in (approx, search, grad):
        for kw in (dict(T=0), dict(B=0), dict(nx=0), dict(nu=-1), dict(H=0)):
            assert call(lib, **kw) == _lib.E_BADARG, (call.__name__, kw)
        for kw in (dict(nx=17), dict(nu=9), dict(H=257), dict(act=1), dict(act=5)):
            assert call(lib, **kw) == _lib.E_UNSUPPORTED, (call.__name__, kw)
    assert approx(lib, Q=None) == approx(lib, x=None) == _lib.E_BADARG
    assert approx(lib, Ho=None) == approx(lib, go=None) == _lib.E_BADARG           # H and g0: both or neither
    assert approx(lib, Ho=None, go=None, co=None) == _lib.E_BADARG
    assert approx(lib, T=1 << 12, B=1 << 12, nx=16, nu=8, H=256) == _lib.E_UNSUPPORTED     # T B ns^2 >= 2^31
    assert search(lib, w2=None) == search(lib, costs=None) == _lib.E_BADARG
    assert search(lib, F=None) == _lib.E_BADARG                                     # (only T = 1 reads no F)
    assert grad(lib, gg=None, gc=None) == _lib.E_BADARG
    assert grad(lib, dQ=None) == _lib.E_BADARG
    assert grad(lib, ws=None) == _lib.E_WORKSPACE
    assert grad(lib, short=1) == _lib.E_WORKSPACE
    assert grad(lib, nx=16, nu=8, H=256, short=1) == _lib.E_WORKSPACE


def test_the_workspace_is_a_function_of_the_sizes_alone():
    lib = _lib.load()
    q = lib.dmpc_mlp_cost_param_grad_workspace_bytes
    per = lambda ns, H: 4 * (ns * ns + ns + H * ns + 2 * H)       # noqa: E731
    assert q(4, 5, 3, 1, 7) == 20 * per(4, 7)
    assert q(100, 100, 3, 1, 7) == 256 * per(4, 7)                # the cap on the partials
    assert q(3, 2, 16, 8, 256) == 6 * per(24, 256)
    assert q(0, 5, 3, 1, 7) == q(4, 5, 17, 1, 7) == q(4, 5, 3, 1, 257) == 0


# ---------------------------------------------------------------------- what the GPU tests rely on
@pytest.mark.parametrize("act,name", CASES, ids=IDS)
def test_the_oracle_iterates_meet_the_conditions_of_the_gpu_tests(act, name):
    first, second = mc.oracle_iterates(act, name)
    assert first["min_eig"] >= mc.MIN_EIG and second["min_eig"] >= mc.MIN_EIG
    assert first["ties"].sum() == 0
    if name in mc.NO_TIE_IN_SECOND:
        assert second["ties"].sum() == 0
    if act == "relu":
        assert mc.problem(act, name)["cost"].min_abs_z >= mc.KINK_MARGIN
    assert np.isfinite(second["x"]).all() and (first["n_ls"] >= 1).all()
