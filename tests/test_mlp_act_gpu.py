"""GPU: `MlpDx` with the relu, silu and softplus activations on the device - the one-launch rollout + linearisation and the
line search with the network as the true dynamics - against the float64 oracle running the numpy restatement of the network
(tests/mlp_act_cases.py).  The tests of tests/test_mlp_dx_gpu.py per activation, at the same tolerances.

relu: every comparison of a Jacobian asserts that the float64 side stays KINK_MARGIN away from a kink, and the ten-iteration
loop is not compared with the oracle's (its linearisation points come within 9.8e-8 of one)."""
import warnings

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import BoxDDP, MPCstep, QuadCost, _lib
from chainer_differentiable_mpc_amd.util import get_traj
from tests.helpers import TOL_COSTATE, TOL_PRIMAL, TOL_STEP, assert_close, npy, tie_rows
from tests.mlp_act_cases import (ACT_CODES, ACTIVATIONS, KINK_MARGIN, oracle_loop, oracle_overshoot, oracle_two_steps,
                                 problem)
from tests.mlp_dx_cases import BOUND, CASES, LS_DECAY, MAX_LS_ITER

pytestmark = pytest.mark.gpu

SEARCH_KERNEL = "mpc_forward_rec_mlp_kernel"
ROLLOUT_KERNEL = "mlp_rollout_linearize_kernel"


def act_cases(cases, activations=ACTIVATIONS):
    return pytest.mark.parametrize("activation,case", [(a, c) for a in activations for c in cases])


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(a, dtype=dtype, device="cuda")


def device_step(activation, case, mlp, u_nom, rows=None):
    """rollout + linearisation and one `MPCstep.forward` on the device from the nominal controls u_nom (numpy);
    rows: solve these trajectories only"""
    nx, nu, H, B, T, s = case
    P = problem(activation, case)
    sl = slice(None) if rows is None else rows
    x0, C, c = dev(P["x_init"][sl]), dev(P["C"][:, sl]), dev(P["c"][:, sl])
    lo, hi, ud = dev(P["lo"][:, sl]), dev(P["hi"][:, sl]), dev(u_nom[:, sl])
    with torch.no_grad():
        assert mlp.fused_ok(x0, ud)
        xd, Fd, fd = mlp.rollout_linearize(x0, ud)
        rollout_name = _lib.last_kernel_name()
        step = MPCstep(controls=ud, T=T, u_upper=hi, u_lower=lo, n_batch=x0.shape[0], n_state=nx, n_ctrl=nu, current_states=xd,
                       true_cost=QuadCost(C, c), true_dynamics=mlp, ls_decay=LS_DECAY, max_ls_iter=MAX_LS_ITER,
                       need_expand=True)
        x, u = step.forward((xd[0], C, c, Fd, fd))
        name = _lib.last_kernel_name()
    return dict(x_nom=xd, F=Fd, f=fd, x=x, u=u, costs=step.for_out.costs, alphas=step.alphas, n_ls=step.n_ls_iter, kernel=name,
                rollout_kernel=rollout_name)


_steps = {}


def device_two_steps(activation, case):
    """the device's results for both iterates of `oracle_two_steps`, computed once and left unchanged"""
    key = (activation, case)
    if key not in _steps:
        mlp = problem(activation, case)["net"].module("cuda")
        first, second = oracle_two_steps(activation, case)
        _steps[key] = (mlp, device_step(activation, case, mlp, first["u_nom"]),
                       device_step(activation, case, mlp, second["u_nom"]))
    return _steps[key]


@act_cases(CASES)
def test_rollout_linearize_against_the_oracle(activation, case):
    nx, nu, H, B, T, s = case
    mlp, got1, got2 = device_two_steps(activation, case)
    assert mlp.activation == activation and mlp.supported()
    for ref, got in zip(oracle_two_steps(activation, case), (got1, got2)):
        if activation == "relu":
            assert ref["min_abs_z"] >= KINK_MARGIN, ref["min_abs_z"]
        assert ROLLOUT_KERNEL in got["rollout_kernel"], got["rollout_kernel"]
        assert_close(npy(got["x_nom"]), ref["x_nom"], TOL_PRIMAL, "x")
        assert_close(npy(got["F"]), ref["F"], TOL_PRIMAL, "F")
        assert_close(npy(got["f"]), ref["f"], TOL_COSTATE, "f")
        assert tuple(got["F"].shape) == (T - 1, B, nx, nx + nu) and tuple(got["f"].shape) == (T - 1, B, nx)
    P = problem(activation, case)
    x0, ud = dev(P["x_init"]), dev(oracle_two_steps(activation, case)[1]["u_nom"])
    with torch.no_grad():
        x_only, F_none, f_none = mlp.rollout_linearize(x0, ud, want_model=False)
        assert F_none is None and f_none is None
        assert torch.equal(x_only, got2["x_nom"])                 # the same states bit for bit, with or without the model
        x1, F1, f1 = mlp.rollout_linearize(x0, ud[:1])            # T = 1: no dynamics step
        assert torch.equal(x1, x0[None]) and tuple(F1.shape) == (0, B, nx, nx + nu) and tuple(f1.shape) == (0, B, nx)
        Fl, fl = mlp.linearize(got2["x_nom"], ud)                 # the hook of linearize_dynamics: the same launch
        assert torch.equal(Fl, got2["F"]) and torch.equal(fl, got2["f"])


@act_cases(CASES)
def test_mpc_step_against_the_oracle(activation, case):
    """backward sweep on the existing kernel, line search on the activation's instance; two iterates per case"""
    mlp, got1, got2 = device_two_steps(activation, case)
    for which, ref, got in zip(("step 1", "step 2"), oracle_two_steps(activation, case), (got1, got2)):
        assert SEARCH_KERNEL in got["kernel"], got["kernel"]      # not the torch route around a callable
        assert tie_rows(ref["old_costs"], ref["costs"]).sum() == 0
        assert_close(npy(got["u"]), ref["u"], TOL_STEP, which + " u")
        assert_close(npy(got["x"]), ref["x"], TOL_STEP, which + " x")
        assert_close(npy(got["costs"]), ref["costs"], TOL_STEP, which + " costs")
        np.testing.assert_array_equal(got["n_ls"].cpu().numpy(), ref["n_ls"])
        assert_close(npy(got["alphas"]), ref["alphas"], 1e-6, which + " alphas")


def _search_through_the_abi(activation, case, act_code):
    """`dmpc_mpc_forward_rec_mlp` with zero gains from the second iterate's nominal trajectory -> (rc, outputs, inputs)"""
    nx, nu, H, B, T, s = case
    P = problem(activation, case)
    mlp, _, got2 = device_two_steps(activation, case)
    lib = _lib.load()
    ud = dev(oracle_two_steps(activation, case)[1]["u_nom"])
    xs = got2["x_nom"]
    C, c, lo, hi = dev(P["C"]), dev(P["c"]), dev(P["lo"]), dev(P["hi"])
    W1, b1, W2, b2 = mlp.device_weights(ud.device)
    f32 = dict(dtype=torch.float32, device="cuda")
    Ks, ks = torch.zeros((T, B, nu, nx), **f32), torch.zeros((T, B, nu), **f32)
    out = dict(x=torch.full((T, B, nx), -7.0, **f32), u=torch.full((T, B, nu), -7.0, **f32), u1=torch.full((T, B, nu), -7.0, **f32))
    out.update({k: torch.full(sh, -7.0, **f32) for k, sh in (("costs", (B,)), ("old", (B,)), ("alphas", (B,)), ("objs", (T, B)))})
    out.update(nls=torch.zeros((B,), dtype=torch.int32, device="cuda"), info=torch.zeros((B,), dtype=torch.int32, device="cuda"))
    ptr = _lib.ptr
    rc = lib.dmpc_mpc_forward_rec_mlp(T, B, nx, nu, H, act_code, 1, ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(Ks), ptr(ks), ptr(ud),
                                      ptr(xs), ptr(lo), ptr(hi), ptr(C), ptr(c), LS_DECAY, MAX_LS_ITER, ptr(out["x"]),
                                      ptr(out["u"]), ptr(out["costs"]), ptr(out["old"]), ptr(out["alphas"]), ptr(out["objs"]),
                                      ptr(out["u1"]), ptr(out["nls"]), ptr(out["info"]), _lib.stream_ptr(ud.device))
    return rc, out, xs, ud


@act_cases(CASES)
def test_zero_gains_reproduce_the_nominal_trajectory_bit_for_bit(activation, case):
    """Ks = 0, ks = 0: the candidate IS the nominal trajectory - one step function for both kernels of an activation"""
    rc, out, xs, ud = _search_through_the_abi(activation, case, ACT_CODES[activation])
    assert rc == 0
    assert SEARCH_KERNEL in _lib.last_kernel_name()
    assert torch.equal(out["x"], xs) and torch.equal(out["u"], ud) and torch.equal(out["u1"], ud)
    assert torch.equal(out["costs"], out["old"])
    assert bool((out["alphas"] == 1).all()) and bool((out["nls"] == 1).all()) and not bool(out["info"].any())


def test_act_code_one_is_refused_with_nothing_launched():
    case = CASES[0]
    rc, out, xs, ud = _search_through_the_abi("relu", case, 1)
    torch.cuda.synchronize()
    assert rc == _lib.E_UNSUPPORTED
    for k in ("x", "u", "u1", "costs", "old", "alphas", "objs"):
        assert bool((out[k] == -7.0).all()), k                    # nothing was written
    assert not bool(out["nls"].any())
    nx, nu, H, B, T, s = case
    mlp = device_two_steps("relu", case)[0]
    lib, ptr = _lib.load(), _lib.ptr
    W1, b1, W2, b2 = mlp.device_weights(ud.device)
    x, x0 = torch.full((T, B, nx), -7.0, device="cuda"), xs[0].contiguous()
    rc = lib.dmpc_mlp_rollout_linearize(T, B, nx, nu, H, 1, 1, ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(x0), ptr(ud), ptr(x),
                                        None, None, _lib.stream_ptr(ud.device))
    torch.cuda.synchronize()
    assert rc == _lib.E_UNSUPPORTED and bool((x == -7.0).all())
    assert lib.dmpc_mlp_dx_supported(nx, nu, H, 1) == 0


@act_cases(CASES[:4])
def test_search_that_backtracks(activation, case):
    """the five cases accept their first candidate; here the feed-forward gains overshoot, so trajectories of one batch stop
    after different numbers of passes"""
    nx, nu, H, B, T, s = case
    P = problem(activation, case)
    mlp, got1, _ = device_two_steps(activation, case)
    ref = oracle_overshoot(activation, case)
    assert tie_rows(ref["old_costs"], ref["costs"]).sum() == 0 and ref["n_ls"].max() == 2
    with torch.no_grad():
        step = MPCstep(controls=dev(oracle_two_steps(activation, case)[0]["u_nom"]), T=T, u_upper=dev(ref["hi"]),
                       u_lower=dev(ref["lo"]), n_batch=B, n_state=nx, n_ctrl=nu, current_states=got1["x_nom"], true_cost=None,
                       true_dynamics=None, ls_decay=LS_DECAY, max_ls_iter=MAX_LS_ITER)
        x, u, fo = step.forward_rec(dev(ref["Ks"]), dev(ref["ks"]), QuadCost(dev(P["C"]), dev(P["c"])), mlp, LS_DECAY, MAX_LS_ITER)
    assert SEARCH_KERNEL in _lib.last_kernel_name()
    np.testing.assert_array_equal(step.n_ls_iter.cpu().numpy(), ref["n_ls"])
    assert_close(npy(step.alphas), ref["alphas"], 1e-6, "alphas")
    assert_close(npy(u), ref["u"], TOL_STEP, "u")
    assert_close(npy(x), ref["x"], TOL_STEP, "x")
    assert_close(npy(fo.costs), ref["costs"], TOL_STEP, "costs")


@act_cases(CASES[:2])
def test_a_trajectory_does_not_depend_on_its_batch(activation, case):
    """row b of the B = 5 and B = 6 solves equals the same trajectory solved alone, bit for bit"""
    B = case[3]
    mlp, got1, got2 = device_two_steps(activation, case)
    for ref, got in zip(oracle_two_steps(activation, case), (got1, got2)):
        for b in range(B):
            alone = device_step(activation, case, mlp, ref["u_nom"], rows=slice(b, b + 1))
            assert SEARCH_KERNEL in alone["kernel"]
            for k in ("x_nom", "F", "f", "x", "u"):
                assert torch.equal(alone[k][:, 0], got[k][:, b]), (k, b)
            for k in ("costs", "alphas", "n_ls"):
                assert torch.equal(alone[k][0], got[k][b]), (k, b)


_loops = {}


def device_loop(activation, case):
    """the BoxDDP solve with the network, computed once: (mlp, x, u, costs, name of the last kernel)"""
    key = (activation, case)
    if key not in _loops:
        nx, nu, H, B, T, s = case
        P = problem(activation, case)
        mlp = P["net"].module("cuda")
        solver = BoxDDP(T, -BOUND, BOUND, B, nx, nu, None, eps=1e-3, max_iter=10, line_search_decay=LS_DECAY,
                        max_line_search_iter=MAX_LS_ITER, quiet=True)
        with warnings.catch_warnings(), torch.no_grad():
            warnings.simplefilter("ignore")
            x, u, costs = solver((dev(P["x_init"]), QuadCost(dev(P["C"]), dev(P["c"])), mlp))
        _loops[key] = (mlp, x, u, costs, _lib.last_kernel_name())
    return _loops[key]


@act_cases(CASES[:2])
def test_box_ddp_with_the_network(activation, case):
    """the loop on the device route: the bounds, finite results and the consistency of the returned pair"""
    nx, nu, H, B, T, s = case
    P = problem(activation, case)
    mlp, x, u, costs, name = device_loop(activation, case)
    assert SEARCH_KERNEL in name, name
    assert bool((u.abs() <= BOUND).all())
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(u).all()) and bool(torch.isfinite(costs).all())
    with torch.no_grad():
        again = get_traj(T, u, dev(P["x_init"]), lambda a, b: mlp(a, b))
    assert float((again - x).abs().max()) <= 1e-5


@act_cases(CASES[:2], ("silu", "softplus"))
def test_box_ddp_costs_against_the_oracle_loop(activation, case):
    """x and u are NOT compared with the oracle loop (a flat valley, as for tanh); relu is not compared at all: inside the
    oracle's loop its linearisation points come within 9.8e-8 of a kink, which float32 cannot resolve"""
    _, _, _, costs, _ = device_loop(activation, case)
    assert_close(npy(costs), oracle_loop(activation, case)["costs"], TOL_PRIMAL, "costs")
