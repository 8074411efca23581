"""GPU: `MlpDx` with TWO hidden layers on the device kernels (depth-two instances of mlp_rollout_linearize_kernel and
mpc_forward_rec_mlp_kernel) and inside the box-DDP chain, against the float64 oracle running the numpy restatement of
tests/mlp2_cases.py.  Tolerances are the project's own (tests/helpers.py); what each case is for, the tie rows that a step
comparison may leave out (at most one) and the relu cases with a resolvable margin to a kink are stated in tests/mlp2_cases.py."""
import warnings

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import BoxDDP, MlpDx, MPCstep, QuadCost, _lib
from chainer_differentiable_mpc_amd.util import get_traj
from tests.helpers import TOL_COSTATE, TOL_PRIMAL, assert_close, npy, tie_rows
from tests.mlp2_cases import (ACT_CODES, CASE, CASES, KINK_MARGIN, MAX_TIE_ROWS, RELU_CASES, oracle_loop, oracle_one_iteration,
                              oracle_overshoot, oracle_two_steps, problem)
from tests.mlp_dx_cases import BOUND, LS_DECAY, MAX_LS_ITER

pytestmark = pytest.mark.gpu

SEARCH_KERNEL = "mpc_forward_rec_mlp_kernel"
ROLLOUT_KERNEL = "mlp_rollout_linearize_kernel"
CHAIN_END = "box_ddp_summary_kernel"
TOL_F_SMALL = 5e-4        # f = next - F [x;u]
ACF = [CASE[k] for k in "ACF"]

ROLLOUT = [("tanh", c) for c in CASES] + [(a, c) for a in ("relu", "silu", "softplus") for c in ACF] + [("silu", CASE["D"])]
STEPS = [("tanh", c) for c in CASES] + [(a, c) for a in ("silu", "relu") for c in ACF]
BITS = [("tanh", CASE[k]) for k in "ACD"]


def ids(pairs):
    names = {v: k for k, v in CASE.items()}
    return ["%s-%s" % (a, names[c]) for a, c in pairs]


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(a, dtype=dtype, device="cuda")


def device_step(activation, case, mlp, u_nom, rows=None):
    """rollout + linearisation and one `MPCstep.forward` on the device from the nominal controls u_nom (numpy);
    rows: solve these trajectories only"""
    nx, nu, H1, H2, B, T, s = case
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


# ---- 1. rollout and linearisation
@pytest.mark.parametrize("activation,case", ROLLOUT, ids=ids(ROLLOUT))
def test_rollout_linearize_against_the_oracle(activation, case):
    nx, nu, H1, H2, B, T, s = case
    mlp, got1, got2 = device_two_steps(activation, case)
    assert mlp.activation == activation and mlp.depth == 2 and mlp.supported()
    for ref, got in zip(oracle_two_steps(activation, case), (got1, got2)):
        if activation == "relu":
            assert case in RELU_CASES and ref["min_abs_z"] >= KINK_MARGIN, ref["min_abs_z"]
        assert ROLLOUT_KERNEL in got["rollout_kernel"], got["rollout_kernel"]
        assert_close(npy(got["x_nom"]), ref["x_nom"], TOL_PRIMAL, "x")
        assert_close(npy(got["F"]), ref["F"], TOL_PRIMAL, "F")
        assert_close(npy(got["f"]), ref["f"], TOL_F_SMALL, "f")
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


@pytest.mark.parametrize("case", [CASE["B"], CASE["D"]], ids=["B", "D"])
def test_relu_rollout_states_where_the_jacobian_is_not_compared(case):
    """B and D come within 1.8e-6 / 5.1e-6 of a kink: their F and f are not compared, their states are"""
    mlp, got1, got2 = device_two_steps("relu", case)
    for ref, got in zip(oracle_two_steps("relu", case), (got1, got2)):
        assert ROLLOUT_KERNEL in got["rollout_kernel"]
        assert_close(npy(got["x_nom"]), ref["x_nom"], TOL_PRIMAL, "x")


# ---- 2. bit-equality
def _search_through_the_abi(activation, case, rows=None):
    """`dmpc_mpc_forward_rec_mlp` with zero gains from the second iterate's nominal trajectory -> (rc, outputs, xs, u)"""
    nx, nu, H1, H2, B, T, s = case
    P = problem(activation, case)
    mlp, _, got2 = device_two_steps(activation, case)
    sl = slice(None) if rows is None else rows
    lib = _lib.load()
    ud = dev(oracle_two_steps(activation, case)[1]["u_nom"][:, sl])
    xs = got2["x_nom"][:, sl].contiguous()
    C, c, lo, hi = dev(P["C"][:, sl]), dev(P["c"][:, sl]), dev(P["lo"][:, sl]), dev(P["hi"][:, sl])
    B = ud.shape[1]
    W1, b1, W23, b23 = mlp.device_weights(ud.device)
    f32 = dict(dtype=torch.float32, device="cuda")
    Ks, ks = torch.zeros((T, B, nu, nx), **f32), torch.zeros((T, B, nu), **f32)
    out = dict(x=torch.full((T, B, nx), -7.0, **f32), u=torch.full((T, B, nu), -7.0, **f32), u1=torch.full((T, B, nu), -7.0, **f32))
    out.update({k: torch.full(sh, -7.0, **f32) for k, sh in (("costs", (B,)), ("old", (B,)), ("alphas", (B,)), ("objs", (T, B)))})
    out.update(nls=torch.zeros((B,), dtype=torch.int32, device="cuda"), info=torch.zeros((B,), dtype=torch.int32, device="cuda"))
    ptr = _lib.ptr
    rc = lib.dmpc_mpc_forward_rec_mlp(T, B, nx, nu, _lib.mlp_hidden2(H1, H2), ACT_CODES[activation], 1, ptr(W1), ptr(b1), ptr(W23),
                                      ptr(b23), ptr(Ks), ptr(ks), ptr(ud), ptr(xs), ptr(lo), ptr(hi), ptr(C), ptr(c), LS_DECAY,
                                      MAX_LS_ITER, ptr(out["x"]), ptr(out["u"]), ptr(out["costs"]), ptr(out["old"]),
                                      ptr(out["alphas"]), ptr(out["objs"]), ptr(out["u1"]), ptr(out["nls"]), ptr(out["info"]),
                                      _lib.stream_ptr(ud.device))
    return rc, out, xs, ud


@pytest.mark.parametrize("activation,case", BITS, ids=ids(BITS))
def test_zero_gains_reproduce_the_nominal_trajectory_bit_for_bit(activation, case):
    """Ks = 0, ks = 0: the candidate IS the nominal trajectory - one step function for both kernels of a depth"""
    rc, out, xs, ud = _search_through_the_abi(activation, case)
    assert rc == 0
    assert SEARCH_KERNEL in _lib.last_kernel_name()
    assert torch.equal(out["x"], xs) and torch.equal(out["u"], ud) and torch.equal(out["u1"], ud)
    assert torch.equal(out["costs"], out["old"])
    assert bool((out["alphas"] == 1).all()) and bool((out["nls"] == 1).all()) and not bool(out["info"].any())


@pytest.mark.parametrize("activation,case", BITS, ids=ids(BITS))
def test_a_trajectory_does_not_depend_on_its_batch(activation, case):
    """row b of a batch equals the same trajectory solved alone, bit for bit: the rollout with its Jacobians and the search"""
    B = case[4]
    mlp, got1, got2 = device_two_steps(activation, case)
    for ref, got in zip(oracle_two_steps(activation, case), (got1, got2)):
        for b in range(B):
            alone = device_step(activation, case, mlp, ref["u_nom"], rows=slice(b, b + 1))
            assert SEARCH_KERNEL in alone["kernel"] and ROLLOUT_KERNEL in alone["rollout_kernel"]
            for k in ("x_nom", "F", "f", "x", "u"):
                assert torch.equal(alone[k][:, 0], got[k][:, b]), (k, b)
            for k in ("costs", "alphas", "n_ls"):
                assert torch.equal(alone[k][0], got[k][b]), (k, b)
    b = B - 1
    rc, whole, _, _ = _search_through_the_abi(activation, case)
    rc1, alone, _, _ = _search_through_the_abi(activation, case, rows=slice(b, b + 1))
    assert rc == 0 and rc1 == 0
    for k in ("x", "u", "u1", "objs"):
        assert torch.equal(alone[k][:, 0], whole[k][:, b]), k


# ---- 3. one MPC step
@pytest.mark.parametrize("activation,case", STEPS, ids=ids(STEPS))
def test_mpc_step_against_the_oracle(activation, case):
    """backward sweep on the existing kernel, line search on the depth-two instance; two iterates per case"""
    mlp, got1, got2 = device_two_steps(activation, case)
    for which, ref, got in zip(("step 1", "step 2"), oracle_two_steps(activation, case), (got1, got2)):
        if activation == "relu":
            assert ref["min_abs_z"] >= KINK_MARGIN, ref["min_abs_z"]
        assert SEARCH_KERNEL in got["kernel"], got["kernel"]      # not the torch route around a callable
        keep = ~tie_rows(ref["old_costs"], ref["costs"])
        assert (~keep).sum() <= MAX_TIE_ROWS
        if not keep.any():
            assert case == CASE["E"] and which == "step 2"        # B = 1: a tie leaves nothing to compare
            continue
        assert_close(npy(got["u"])[:, keep], ref["u"][:, keep], TOL_PRIMAL, which + " u")
        assert_close(npy(got["x"])[:, keep], ref["x"][:, keep], TOL_PRIMAL, which + " x")
        assert_close(npy(got["costs"])[keep], ref["costs"][keep], TOL_PRIMAL, which + " costs")
        np.testing.assert_array_equal(got["n_ls"].cpu().numpy()[keep], ref["n_ls"][keep])
        assert_close(npy(got["alphas"])[keep], ref["alphas"][keep], 1e-6, which + " alphas")


@pytest.mark.parametrize("activation,case", STEPS, ids=ids(STEPS))
def test_search_that_backtracks(activation, case):
    """the feed-forward gains overshoot (tests/mlp_dx_cases.py::oracle_overshoot): `forward_rec` alone, per trajectory"""
    nx, nu, H1, H2, B, T, s = case
    P = problem(activation, case)
    mlp, got1, _ = device_two_steps(activation, case)
    ref = oracle_overshoot(activation, case)
    keep = ~tie_rows(ref["old_costs"], ref["costs"])
    assert (~keep).sum() <= MAX_TIE_ROWS
    with torch.no_grad():
        step = MPCstep(controls=dev(oracle_two_steps(activation, case)[0]["u_nom"]), T=T, u_upper=dev(ref["hi"]),
                       u_lower=dev(ref["lo"]), n_batch=B, n_state=nx, n_ctrl=nu, current_states=got1["x_nom"], true_cost=None,
                       true_dynamics=None, ls_decay=LS_DECAY, max_ls_iter=MAX_LS_ITER)
        x, u, fo = step.forward_rec(dev(ref["Ks"]), dev(ref["ks"]), QuadCost(dev(P["C"]), dev(P["c"])), mlp, LS_DECAY, MAX_LS_ITER)
    assert SEARCH_KERNEL in _lib.last_kernel_name()
    if not keep.any():
        return
    np.testing.assert_array_equal(step.n_ls_iter.cpu().numpy()[keep], ref["n_ls"][keep])
    assert_close(npy(step.alphas)[keep], ref["alphas"][keep], 1e-6, "alphas")
    assert_close(npy(u)[:, keep], ref["u"][:, keep], TOL_PRIMAL, "u")
    assert_close(npy(x)[:, keep], ref["x"][:, keep], TOL_PRIMAL, "x")
    assert_close(npy(fo.costs)[keep], ref["costs"][keep], TOL_PRIMAL, "costs")


# ---- 4. / 5. BoxDDP: the host loop and the chain
LOOPS = [("tanh", CASE["A"]), ("tanh", CASE["B"]), ("silu", CASE["A"])]


def make_solver(case, max_iter=10, **kw):
    nx, nu, H1, H2, B, T, s = case
    return BoxDDP(T, -BOUND, BOUND, B, nx, nu, None, eps=1e-3, max_iter=max_iter, line_search_decay=LS_DECAY,
                  max_line_search_iter=MAX_LS_ITER, quiet=True, **kw)


def inputs(activation, case):
    P = problem(activation, case)
    return dev(P["x_init"]), QuadCost(dev(P["C"]), dev(P["c"]))


def solve(solver, x0, cost, mlp):
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        x, u, costs = solver((x0, cost, mlp))
    return x, u, costs, _lib.last_kernel_name()


_host = {}


def host_loop(activation, case):
    key = (activation, case)
    if key not in _host:
        x0, cost = inputs(activation, case)
        _host[key] = solve(make_solver(case), x0, cost, problem(activation, case)["net"].module("cuda"))
    return _host[key]


@pytest.mark.parametrize("activation,case", LOOPS, ids=ids(LOOPS))
def test_box_ddp_host_loop_against_the_oracle_loop(activation, case):
    x, u, costs, name = host_loop(activation, case)
    assert SEARCH_KERNEL in name, name
    assert_close(npy(costs), oracle_loop(activation, case)["costs"], TOL_PRIMAL, "costs")
    assert bool((u.abs() <= BOUND).all())


@pytest.mark.parametrize("case", CASES, ids=list("ABCDEF"))
def test_chain_one_iteration_against_the_oracle(case):
    ref = oracle_one_iteration("tanh", case)
    first = oracle_two_steps("tanh", case)[0]
    keep = ~tie_rows(first["old_costs"], first["costs"])
    assert (~keep).sum() <= MAX_TIE_ROWS and keep.any()
    x0, cost = inputs("tanh", case)
    x, u, costs, name = solve(make_solver(case, max_iter=1), x0, cost, problem("tanh", case)["net"].module("cuda", device_loop=True))
    assert CHAIN_END in name, name
    assert_close(npy(u)[:, keep], ref["u"][:, keep], TOL_PRIMAL, "u")
    assert_close(npy(x)[:, keep], ref["x"][:, keep], TOL_PRIMAL, "x")
    assert_close(npy(costs)[keep], ref["costs"][keep], TOL_PRIMAL, "costs")


@pytest.mark.parametrize("activation,case", LOOPS, ids=ids(LOOPS))
def test_chain_loop_against_the_oracle_and_the_host_loop(activation, case):
    nx, nu, H1, H2, B, T, s = case
    x0, cost = inputs(activation, case)
    mlp = problem(activation, case)["net"].module("cuda", device_loop=True)
    solver = make_solver(case)
    x, u, costs, name = solve(solver, x0, cost, mlp)
    assert CHAIN_END in name, name
    assert_close(npy(costs), oracle_loop(activation, case)["costs"], TOL_PRIMAL, "costs")
    assert_close(npy(costs), npy(host_loop(activation, case)[2]), TOL_PRIMAL, "costs, chain against host loop")
    assert bool((u.abs() <= BOUND).all())
    with torch.no_grad():
        again = get_traj(T, u, x0, lambda a, b: mlp(a, b))
    assert float((again - x).abs().max()) <= 1e-5
    assert 1 <= solver.n_iter <= 10


def test_a_recorded_chain_follows_the_weights():
    activation, case = LOOPS[1]
    x0, cost = inputs(activation, case)
    net = problem(activation, case)["net"]
    mlp = net.module("cuda", device_loop=True)
    solver = make_solver(case)
    first = solve(solver, x0, cost, mlp)
    assert CHAIN_END in first[3]
    recorded = solve(solver, x0, cost, mlp)
    assert any(e[0] is not None for e in solver._graphs.values())           # the second call recorded the chain
    replayed = solve(solver, x0, cost, mlp)
    for other in (recorded, replayed):
        for a, b in zip(first[:3], other[:3]):
            assert torch.equal(a, b)
    with torch.no_grad():
        mlp.W2.mul_(0.9)
        mlp.W3.mul_(1.1)
    moved = solve(solver, x0, cost, mlp)                                    # a replay, on the new weights
    fresh_mlp = net.module("cuda", device_loop=True)
    with torch.no_grad():
        fresh_mlp.W2.copy_(mlp.W2)
        fresh_mlp.W3.copy_(mlp.W3)
    fresh = solve(make_solver(case), x0, cost, fresh_mlp)
    for a, b in zip(moved[:3], fresh[:3]):
        assert torch.equal(a, b)
    assert not torch.equal(moved[1], first[1])


# ---- 6. beyond the limits: the torch route
def test_a_size_beyond_the_limits_takes_the_torch_route():
    nx, nu, B, T = 3, 1, 4, 5
    mlp = MlpDx(nx, nu, (5, 129), seed=2).cuda()
    assert not mlp.supported()
    rng = np.random.RandomState(3)
    x0, u = dev(rng.randn(B, nx)), dev(0.5 * rng.randn(T, B, nu))
    with torch.no_grad():
        assert not mlp.fused_ok(x0, u)
        x, F, f = mlp.rollout_linearize(x0, u)
        xt, Ft, ft = mlp._rollout_linearize_torch(x0, u, True)
    assert "mlp" not in _lib.last_kernel_name()
    assert torch.equal(x, xt) and torch.equal(F, Ft) and torch.equal(f, ft)
    ref = mlp.double().cpu()
    with torch.no_grad():
        xr, Fr, fr = ref._rollout_linearize_torch(x0.double().cpu(), u.double().cpu(), True)
    assert_close(npy(x), npy(xr), TOL_PRIMAL, "x")
    assert_close(npy(F), npy(Fr), TOL_PRIMAL, "F")
    P = problem("tanh", CASE["A"])
    big = MlpDx(3, 1, (5, 129), seed=2, device_loop=True).cuda()
    solver = BoxDDP(7, -BOUND, BOUND, 5, 3, 1, None, eps=1e-3, max_iter=2, quiet=True)
    x, u, costs, name = solve(solver, dev(P["x_init"]), QuadCost(dev(P["C"]), dev(P["c"])), big)
    assert CHAIN_END not in name and SEARCH_KERNEL not in name, name
    assert bool(torch.isfinite(x).all()) and bool((u.abs() <= BOUND).all()) and bool(torch.isfinite(costs).all())


# ---- 7. the gradient of a two-layer solve: the live route
GRAD_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")


@pytest.mark.parametrize("activation,case", LOOPS, ids=ids(LOOPS))
def test_box_ddp_gradient_reaches_all_six_weights(activation, case):
    """`backward` of sum(x) + sum(u) through BoxDDP(update_dynamics=True).  The MPC step's backward exists in float32 on the
    device only, so the reference is the one of tests/test_mlp_act_grad_gpu.py: float64 autograd of the live route on the CPU
    for the (x, u, dL/df) that this backward hands to `linearize` - recorded by a hook on f."""
    nx, nu, H1, H2, B, T, s = case
    P = problem(activation, case)
    mlp = P["net"].module("cuda")
    seen, linearize = [], mlp.linearize

    def recording(x, u):
        F, f = linearize(x, u)
        if f.requires_grad:
            f.register_hook(lambda g: seen.append((x.detach(), u.detach(), g.detach())))
        return F, f
    mlp.linearize = recording
    x0, C, c = dev(P["x_init"]), dev(P["C"]), dev(P["c"])
    solver = make_solver(case, update_dynamics=True, detach_unconverged=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, u, _ = solver((x0, QuadCost(C, c), mlp))
    assert x.requires_grad and u.requires_grad
    got = torch.autograd.grad(x.sum() + u.sum(), [getattr(mlp, n) for n in GRAD_NAMES])
    assert len(seen) == 1
    xs, us, g = (t.double().cpu() for t in seen[0])
    assert torch.equal(us, u.detach().double().cpu()) and float(g.abs().max()) > 0
    ref = P["net"].module("cpu", dtype=torch.float64)
    Fr, fr = ref.linearize(xs, us)
    assert fr.requires_grad and not Fr.requires_grad
    want = torch.autograd.grad((fr * g).sum(), [getattr(ref, n) for n in GRAD_NAMES])
    for name, a, b in zip(GRAD_NAMES, got, want):
        assert bool(torch.isfinite(a).all()) and float(b.abs().max()) > 0, name
        assert_close(npy(a), npy(b), TOL_COSTATE, "d/d" + name)
