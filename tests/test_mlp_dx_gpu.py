"""GPU: `MlpDx` on the device - the one-launch rollout + linearisation and the line search with the network as the true
dynamics - against the float64 oracle running a numpy restatement of the network (tests/mlp_dx_cases.py)."""
import warnings

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import BoxDDP, MlpDx, MPCstep, QuadCost, _lib, linearize_dynamics
from chainer_differentiable_mpc_amd.util import get_traj
from tests.helpers import TOL_COSTATE, TOL_PRIMAL, TOL_STEP, assert_close, npy, tie_rows
from tests.mlp_dx_cases import BOUND, CASES, LS_DECAY, MAX_LS_ITER, oracle_loop, oracle_overshoot, oracle_two_steps, problem

pytestmark = pytest.mark.gpu

SEARCH_KERNEL = "mpc_forward_rec_mlp_kernel"


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(a, dtype=dtype, device="cuda")


def device_step(case, mlp, u_nom, rows=None):
    """rollout + linearisation and one `MPCstep.forward` on the device from the nominal controls u_nom (numpy);
    rows: solve these trajectories only"""
    nx, nu, H, B, T, s = case
    P = problem(case)
    sl = slice(None) if rows is None else rows
    x0, C, c = dev(P["x_init"][sl]), dev(P["C"][:, sl]), dev(P["c"][:, sl])
    lo, hi, ud = dev(P["lo"][:, sl]), dev(P["hi"][:, sl]), dev(u_nom[:, sl])
    with torch.no_grad():
        assert mlp.fused_ok(x0, ud)
        xd, Fd, fd = mlp.rollout_linearize(x0, ud)
        step = MPCstep(controls=ud, T=T, u_upper=hi, u_lower=lo, n_batch=x0.shape[0], n_state=nx, n_ctrl=nu, current_states=xd,
                       true_cost=QuadCost(C, c), true_dynamics=mlp, ls_decay=LS_DECAY, max_ls_iter=MAX_LS_ITER,
                       need_expand=True)
        x, u = step.forward((xd[0], C, c, Fd, fd))
        name = _lib.last_kernel_name()
    return dict(x_nom=xd, F=Fd, f=fd, x=x, u=u, costs=step.for_out.costs, alphas=step.alphas, n_ls=step.n_ls_iter, kernel=name)


_steps = {}


def device_two_steps(case):
    """the device's results for both iterates of `oracle_two_steps`, computed once and left unchanged"""
    if case not in _steps:
        mlp = problem(case)["net"].module("cuda")
        first, second = oracle_two_steps(case)
        _steps[case] = (mlp, device_step(case, mlp, first["u_nom"]), device_step(case, mlp, second["u_nom"]))
    return _steps[case]


@pytest.mark.parametrize("case", CASES)
def test_rollout_linearize_against_the_oracle(case):
    nx, nu, H, B, T, s = case
    mlp, got1, got2 = device_two_steps(case)
    for ref, got in zip(oracle_two_steps(case), (got1, got2)):
        assert_close(npy(got["x_nom"]), ref["x_nom"], TOL_PRIMAL, "x")
        assert_close(npy(got["F"]), ref["F"], TOL_PRIMAL, "F")
        assert_close(npy(got["f"]), ref["f"], TOL_COSTATE, "f")
        assert tuple(got["F"].shape) == (T - 1, B, nx, nx + nu) and tuple(got["f"].shape) == (T - 1, B, nx)
    P = problem(case)
    x0, ud = dev(P["x_init"]), dev(oracle_two_steps(case)[1]["u_nom"])
    with torch.no_grad():
        x_only, F_none, f_none = mlp.rollout_linearize(x0, ud, want_model=False)
        assert F_none is None and f_none is None
        assert torch.equal(x_only, got2["x_nom"])                 # the same states bit for bit, with or without the model
        x1, F1, f1 = mlp.rollout_linearize(x0, ud[:1])            # T = 1: no dynamics step
        assert torch.equal(x1, x0[None]) and tuple(F1.shape) == (0, B, nx, nx + nu) and tuple(f1.shape) == (0, B, nx)
        Fl, fl = mlp.linearize(got2["x_nom"], ud)                 # the hook of linearize_dynamics: the same launch
        assert torch.equal(Fl, got2["F"]) and torch.equal(fl, got2["f"])


@pytest.mark.parametrize("case", CASES)
def test_mpc_step_against_the_oracle(case):
    """backward sweep on the existing kernel, line search on the new one; two iterates per case"""
    mlp, got1, got2 = device_two_steps(case)
    for which, ref, got in zip(("step 1", "step 2"), oracle_two_steps(case), (got1, got2)):
        assert SEARCH_KERNEL in got["kernel"], got["kernel"]      # not the torch route around a callable
        assert tie_rows(ref["old_costs"], ref["costs"]).sum() == 0
        assert_close(npy(got["u"]), ref["u"], TOL_STEP, which + " u")
        assert_close(npy(got["x"]), ref["x"], TOL_STEP, which + " x")
        assert_close(npy(got["costs"]), ref["costs"], TOL_STEP, which + " costs")
        np.testing.assert_array_equal(got["n_ls"].cpu().numpy(), ref["n_ls"])
        assert_close(npy(got["alphas"]), ref["alphas"], 1e-6, which + " alphas")


@pytest.mark.parametrize("case", CASES)
def test_zero_gains_reproduce_the_nominal_trajectory_bit_for_bit(case):
    """Ks = 0, ks = 0: the candidate IS the nominal trajectory - one step function for both kernels"""
    nx, nu, H, B, T, s = case
    P = problem(case)
    mlp, _, got2 = device_two_steps(case)
    lib = _lib.load()
    ud = dev(oracle_two_steps(case)[1]["u_nom"])
    xs = got2["x_nom"]
    C, c, lo, hi = dev(P["C"]), dev(P["c"]), dev(P["lo"]), dev(P["hi"])
    W1, b1, W2, b2 = mlp.device_weights(ud.device)
    f32 = dict(dtype=torch.float32, device="cuda")
    Ks, ks = torch.zeros((T, B, nu, nx), **f32), torch.zeros((T, B, nu), **f32)
    x, u, u1 = torch.empty((T, B, nx), **f32), torch.empty((T, B, nu), **f32), torch.empty((T, B, nu), **f32)
    costs, old, alphas, objs = (torch.empty(sh, **f32) for sh in ((B,), (B,), (B,), (T, B)))
    nls = torch.zeros((B,), dtype=torch.int32, device="cuda")
    info = torch.zeros((B,), dtype=torch.int32, device="cuda")
    ptr = _lib.ptr
    rc = lib.dmpc_mpc_forward_rec_mlp(T, B, nx, nu, H, 0, 1, ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(Ks), ptr(ks), ptr(ud),
                                      ptr(xs), ptr(lo), ptr(hi), ptr(C), ptr(c), LS_DECAY, MAX_LS_ITER, ptr(x), ptr(u),
                                      ptr(costs), ptr(old), ptr(alphas), ptr(objs), ptr(u1), ptr(nls), ptr(info),
                                      _lib.stream_ptr(ud.device))
    assert rc == 0
    assert torch.equal(x, xs) and torch.equal(u, ud) and torch.equal(u1, ud)
    assert torch.equal(costs, old)
    assert bool((alphas == 1).all()) and bool((nls == 1).all()) and not bool(info.any())


@pytest.mark.parametrize("case", CASES[:4])
def test_search_that_backtracks(case):
    """the five cases accept their first candidate; here the feed-forward gains overshoot, so trajectories of one batch stop
    after different numbers of passes"""
    nx, nu, H, B, T, s = case
    P = problem(case)
    mlp, got1, _ = device_two_steps(case)
    ref = oracle_overshoot(case)
    assert tie_rows(ref["old_costs"], ref["costs"]).sum() == 0 and ref["n_ls"].max() == 2
    with torch.no_grad():
        step = MPCstep(controls=dev(oracle_two_steps(case)[0]["u_nom"]), T=T, u_upper=dev(ref["hi"]), u_lower=dev(ref["lo"]),
                       n_batch=B, n_state=nx, n_ctrl=nu, current_states=got1["x_nom"], true_cost=None, true_dynamics=None,
                       ls_decay=LS_DECAY, max_ls_iter=MAX_LS_ITER)
        x, u, fo = step.forward_rec(dev(ref["Ks"]), dev(ref["ks"]), QuadCost(dev(P["C"]), dev(P["c"])), mlp, LS_DECAY, MAX_LS_ITER)
    assert SEARCH_KERNEL in _lib.last_kernel_name()
    np.testing.assert_array_equal(step.n_ls_iter.cpu().numpy(), ref["n_ls"])
    assert_close(npy(step.alphas), ref["alphas"], 1e-6, "alphas")
    assert_close(npy(u), ref["u"], TOL_STEP, "u")
    assert_close(npy(x), ref["x"], TOL_STEP, "x")
    assert_close(npy(fo.costs), ref["costs"], TOL_STEP, "costs")


@pytest.mark.parametrize("case", CASES[:2])
def test_a_trajectory_does_not_depend_on_its_batch(case):
    """row b of the B = 5 and B = 6 solves equals the same trajectory solved alone, bit for bit"""
    B = case[3]
    mlp, got1, got2 = device_two_steps(case)
    for ref, got in zip(oracle_two_steps(case), (got1, got2)):
        for b in range(B):
            alone = device_step(case, mlp, ref["u_nom"], rows=slice(b, b + 1))
            assert SEARCH_KERNEL in alone["kernel"]
            for k in ("x_nom", "F", "f", "x", "u"):
                assert torch.equal(alone[k][:, 0], got[k][:, b]), (k, b)
            for k in ("costs", "alphas", "n_ls"):
                assert torch.equal(alone[k][0], got[k][b]), (k, b)


def _solver(case, **kw):
    nx, nu, H, B, T, s = case
    return BoxDDP(T, -BOUND, BOUND, B, nx, nu, None, eps=1e-3, max_iter=10, line_search_decay=LS_DECAY,
                  max_line_search_iter=MAX_LS_ITER, quiet=True, **kw)


@pytest.mark.parametrize("case", CASES[:2])
def test_box_ddp_with_the_network(case):
    """x and u are NOT compared with the oracle loop: these problems have a flat valley (float32-model and float64 loops end up
    to 1.5e-3 apart in u on the CPU); the costs, the bounds and the consistency of the returned pair are what is pinned"""
    nx, nu, H, B, T, s = case
    P = problem(case)
    mlp = problem(case)["net"].module("cuda")
    ref = oracle_loop(case)
    solver = _solver(case)
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        x, u, costs = solver((dev(P["x_init"]), QuadCost(dev(P["C"]), dev(P["c"])), mlp))     # (3,1): not taken for the pendulum
    assert SEARCH_KERNEL in _lib.last_kernel_name()
    assert_close(npy(costs), ref["costs"], TOL_PRIMAL, "costs")
    assert bool((u.abs() <= BOUND).all())
    with torch.no_grad():
        again = get_traj(T, u, dev(P["x_init"]), lambda a, b: mlp(a, b))
    assert float((again - x).abs().max()) <= 1e-5


@pytest.mark.parametrize("case", CASES[:2])
def test_linearize_with_a_gradient_against_autograd(case):
    nx, nu, H, B, T, s = case
    mlp = problem(case)["net"].module("cuda")
    ref = oracle_loop(case)
    x, u = dev(ref["x"]), dev(ref["u"])
    g = dev(np.random.RandomState(s + 30).randn(T - 1, B, nx))
    params = [mlp.W1, mlp.b1, mlp.W2, mlp.b2]
    assert not mlp.fused_ok(x[0], u)
    F, f = mlp.linearize(x, u)
    Fa, fa = linearize_dynamics(x, u, lambda a, b: mlp(a, b))
    assert not F.requires_grad and f.requires_grad
    assert_close(npy(F), npy(Fa), TOL_COSTATE, "F")
    assert_close(npy(f), npy(fa), TOL_COSTATE, "f")
    own = torch.autograd.grad((f * g).sum(), params)
    auto = torch.autograd.grad((fa * g).sum(), params)
    for name, a, b in zip(("W1", "b1", "W2", "b2"), own, auto):
        assert float(b.abs().max()) > 0
        assert_close(npy(a), npy(b), TOL_COSTATE, "d/d" + name)


@pytest.mark.parametrize("case", CASES[:2])
def test_box_ddp_gradient_reaches_the_weights(case):
    nx, nu, H, B, T, s = case
    P = problem(case)
    mlp = problem(case)["net"].module("cuda")
    x0, C, c = dev(P["x_init"]), dev(P["C"]), dev(P["c"])
    rng = np.random.RandomState(s + 40)
    gx, gu = dev(rng.randn(T, B, nx)), dev(rng.randn(T, B, nu))
    params = [mlp.W1, mlp.b1, mlp.W2, mlp.b2]
    solver = _solver(case, detach_unconverged=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, u, _ = solver((x0, QuadCost(C, c), mlp))
    assert x.requires_grad and u.requires_grad
    got = torch.autograd.grad((x * gx).sum() + (u * gu).sum(), params)
    # by hand: the returned pair through a no-op MPCstep node with linearize's models
    xd, ud = x.detach(), u.detach()
    Fm, fm = mlp.linearize(xd, ud)
    node = MPCstep(controls=ud, T=T, u_upper=dev(P["hi"]), u_lower=dev(P["lo"]), n_batch=B, n_state=nx, n_ctrl=nu,
                   current_states=xd, true_cost=QuadCost(C, c), true_dynamics=mlp, ls_decay=LS_DECAY, max_ls_iter=MAX_LS_ITER,
                   need_expand=True, no_op_forward=True)
    x2, u2 = node.apply((xd[0], C, c, Fm, fm))
    assert torch.equal(x2, xd) and torch.equal(u2, ud)
    want = torch.autograd.grad((x2 * gx).sum() + (u2 * gu).sum(), params)
    for name, a, b in zip(("W1", "b1", "W2", "b2"), got, want):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name
        assert_close(npy(a), npy(b), TOL_COSTATE, "d/d" + name)


def test_a_size_outside_the_limits_takes_the_generic_route():
    nx, nu, H, B, T = 3, 1, 300, 2, 4
    P = problem((nx, nu, 5, B, T, 6))
    mlp = MlpDx(nx, nu, H, seed=0).cuda()
    x0, ud = dev(P["x_init"]), torch.zeros((T, B, nu), device="cuda")
    assert not mlp.supported() and not mlp.fused_ok(x0, ud)
    solver = BoxDDP(T, -BOUND, BOUND, B, nx, nu, None, eps=1e-3, max_iter=2, quiet=True)
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        x, u, costs = solver((x0, QuadCost(dev(P["C"]), dev(P["c"])), mlp))
        xr, Fr, fr = mlp.rollout_linearize(x0, u)                 # never raises for size: the same results from torch
    assert SEARCH_KERNEL not in _lib.last_kernel_name()
    assert bool(torch.isfinite(x).all()) and bool((u.abs() <= BOUND).all()) and bool(torch.isfinite(costs).all())
    assert float((xr - x).abs().max()) <= 1e-5 and tuple(Fr.shape) == (T - 1, B, nx, nx + nu)
