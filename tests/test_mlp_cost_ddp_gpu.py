"""GPU: `BoxDDP` with an `MlpCost(device_loop=True)` and a dense `LinDx` - the whole iLQR loop as one chain of launches
(`dmpc_box_ddp_mlp_cost`, include/dmpc_mlp_cost.h): against the float64 oracle's iterates and loop, against the host loop over
the same kernels, the two modes of the chain against each other bit for bit, a stopped chain, row isolation, the solver's own
hipGraph under changing weights, a caller's capture, the gradient behind the chain, and what falls through to the host loop."""
import warnings

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import BoxDDP, LinDx, MlpCost, MlpDx, _lib
from tests import mlp_cost_cases as mc
from tests import mlp_cost_ddp_cases as dc
from tests.helpers import TOL_COSTATE, TOL_PRIMAL, TOL_STEP, assert_close, npy
from tests.mlp_cost_ddp_cases import BEST_COST_EPS, CHAIN_END, EPS, NOT_IMPROVED_LIM, SEARCH_KERNEL

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def module(key, **kw):
    P = dc.problem(key)
    if key == dc.SOFT_BOX:
        m = MlpCost.soft_box(2, 1, P["x_lower"], P["x_upper"], weight=P["weight"], sharpness=P["sharpness"], Q=P["Q"], p=P["p"])
        m.device_loop = bool(kw.pop("device_loop", False))
        m.param_grad = kw.pop("param_grad", "live")
        assert not kw
        return m.to("cuda")
    return mc.module(P, **kw)


def make_solver(key, max_iter=dc.MAX_ITER, bounds=None, **kw):
    P = dc.problem(key)
    nx, nu, H, B, T = P["dims"]
    lo, hi = bounds or (dev(P["lo"]), dev(P["hi"]))
    return BoxDDP(T, lo, hi, B, nx, nu, None, eps=EPS, not_improved_lim=NOT_IMPROVED_LIM, max_iter=max_iter,
                  line_search_decay=mc.LS_DECAY, max_line_search_iter=mc.MAX_LS_ITER, best_cost_eps=BEST_COST_EPS, quiet=True, **kw)


def inputs(key):
    P = dc.problem(key)
    return dev(P["x_init"]), LinDx(dev(P["F"]), dev(P["f"]))


def solve(solver, x0, cost, dyn):
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        x, u, costs = solver((x0, cost, dyn))
    return x, u, costs, _lib.last_kernel_name()


# ---- 1. one iteration against the oracle's first iterate
@pytest.mark.parametrize("key", dc.ONE_ITERATION, ids=dc.name)
def test_one_iteration_against_the_oracle(key):
    ref = mc.oracle_iterates(*key)[0]
    x0, dyn = inputs(key)
    x, u, costs, name = solve(make_solver(key, max_iter=1), x0, module(key, device_loop=True), dyn)
    assert CHAIN_END in name, name
    assert_close(npy(u), ref["u"], TOL_STEP, "chain u")
    assert_close(npy(x), ref["x"], TOL_STEP, "chain x")
    assert_close(npy(costs), ref["costs"], TOL_STEP, "chain costs")


# ---- 2. the loop
@pytest.mark.parametrize("key", dc.LOOP, ids=dc.name)
def test_the_loop_against_the_oracle_and_the_host_loop(key):
    P = dc.problem(key)
    nx, nu, H, B, T = P["dims"]
    x_ref, u_ref, c_ref, n_ref = dc.oracle_loop(key)
    x0, dyn = inputs(key)
    solver = make_solver(key)
    x, u, costs, name = solve(solver, x0, module(key, device_loop=True), dyn)
    assert CHAIN_END in name, name                                # the route was taken
    print("%s: chain %d iterations (oracle %d), costs error %.3e" % (dc.name(key), solver.n_iter, n_ref, np.abs(npy(costs) - c_ref).max()))
    assert_close(npy(costs), c_ref, 1e-4, "chain costs against the oracle's loop")
    host_solver = make_solver(key)
    xh, uh, costs_host, name_host = solve(host_solver, x0, module(key, device_loop=False), dyn)
    assert SEARCH_KERNEL in name_host and CHAIN_END not in name_host, name_host      # the default stays the host loop
    assert_close(npy(costs), npy(costs_host), TOL_PRIMAL, "costs, chain against host loop")
    assert 2 <= solver.n_iter <= 10
    assert bool((u >= dev(P["lo"])).all()) and bool((u <= dev(P["hi"])).all())
    again = torch.empty_like(x)
    rc = _lib.load().dmpc_lin_rollout(T, B, nx, nu, _lib.ptr(x0), _lib.ptr(u.contiguous()), _lib.ptr(dyn.F), _lib.ptr(dyn.f),
                                      _lib.ptr(again), _lib.stream_ptr(x0.device))
    assert rc == 0
    assert float((again - x).abs().max()) <= 1e-5
    if key == dc.SOFT_BOX:       # the limit is felt: the second trajectory ends at it, not at the linear cost's pull
        assert npy(x)[:, 1, 0].max() < 1.1


# ---- 3. - 5. the C ABI directly
def chain(key, mode, max_iter, rows=None):
    """dmpc_box_ddp_mlp_cost through ctypes -> dict of its outputs (and rc, and the kernel launched last)"""
    P = dc.problem(key)
    nx, nu, H, B, T = P["dims"]
    sl = slice(None) if rows is None else rows
    x0, F, f = dev(P["x_init"][sl]), dev(P["F"][:, sl]).contiguous(), None if P["f"] is None else dev(P["f"][:, sl]).contiguous()
    lo, hi = dev(P["lo"][:, sl]).contiguous(), dev(P["hi"][:, sl]).contiguous()
    B = x0.shape[0]
    m = module(key)
    packed = m.packed_weights(x0.device).clone()
    f32 = dict(dtype=torch.float32, device="cuda")
    u0 = torch.zeros((T, B, nu), **f32)
    out = dict(x=torch.full((T, B, nx), np.nan, **f32), u=torch.full((T, B, nu), np.nan, **f32), costs=torch.full((B,), np.nan, **f32),
               norm_best=torch.full((B,), np.nan, **f32), norm_last=torch.full((B,), np.nan, **f32),
               state=torch.full((8,), -1, dtype=torch.int32, device="cuda"), info=torch.full((B,), -1, dtype=torch.int32, device="cuda"))
    lib = _lib.load()
    need = lib.dmpc_box_ddp_mlp_cost_workspace_bytes(T, B, nx, nu)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    ptr = _lib.ptr
    rc = lib.dmpc_box_ddp_mlp_cost(T, B, nx, nu, ptr(x0), ptr(packed), m.n_hidden, m.act_code, mode, ptr(F), ptr(f), 0, None, ptr(u0),
                                   ptr(lo), ptr(hi), EPS, NOT_IMPROVED_LIM, mc.LS_DECAY, mc.MAX_LS_ITER, BEST_COST_EPS, max_iter, 20, 1, 0,
                                   ptr(out["x"]), ptr(out["u"]), ptr(out["costs"]), ptr(out["norm_best"]), ptr(out["norm_last"]),
                                   ptr(out["state"]), ptr(ws), need, ptr(out["info"]), _lib.stream_ptr(x0.device))
    out["kernel"] = _lib.last_kernel_name()
    torch.cuda.synchronize()
    out["rc"] = rc
    return out


OUTPUTS = ("x", "u", "costs", "norm_best", "norm_last", "state", "info")


@pytest.mark.parametrize("max_iter", [1, 2, 10])
@pytest.mark.parametrize("key", dc.SAME_BITS, ids=dc.name)
def test_the_search_that_approximates_returns_the_same_bits(key, max_iter):
    a, b = chain(key, 0, max_iter), chain(key, 1, max_iter)
    assert a["rc"] == 0 and b["rc"] == 0
    assert CHAIN_END in a["kernel"] and CHAIN_END in b["kernel"]
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    for k in ("x", "u", "costs", "norm_best", "norm_last"):
        assert bool(torch.isfinite(a[k]).all()), k
    assert 1 <= int(a["state"][1]) <= max_iter


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("key", [("softplus", "A"), ("softplus", "D")], ids=dc.name)
def test_a_stopped_chain_is_inert(key, mode):
    """the launches behind the stop are no-ops through the device flag: the chain that stops by itself leaves what a chain
    leaves that was given exactly that many iterations"""
    long = chain(key, mode, 10)
    assert long["rc"] == 0
    n = int(long["state"][1])
    assert int(long["state"][0]) == 1 and n < 10          # (it did stop early: the launches behind the stop exist)
    short = chain(key, mode, n)
    assert short["rc"] == 0
    for k in OUTPUTS:
        assert torch.equal(long[k], short[k]), k


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("key", [("softplus", "A"), ("softplus", "B")], ids=dc.name)
def test_a_trajectory_does_not_depend_on_its_batch(key, mode):
    """max_iter = 1 (the stop tests of a longer loop are batch-global); the norms are not compared: the reference's reshape in
    full_du_norm mixes the rows of a batch"""
    B = dc.problem(key)["dims"][3]
    whole = chain(key, mode, 1)
    assert whole["rc"] == 0
    for b in range(B):
        alone = chain(key, mode, 1, rows=slice(b, b + 1))
        assert alone["rc"] == 0
        for k in ("x", "u"):
            assert torch.equal(alone[k][:, 0], whole[k][:, b]), (k, b)
        assert torch.equal(alone["costs"][0], whole["costs"][b]), b


# ---- 6. the packed weights under the solver's own hipGraph
def test_a_recorded_chain_follows_the_weights():
    key = ("softplus", "B")
    x0, dyn = inputs(key)
    m = module(key, device_loop=True)
    solver = make_solver(key)
    first = solve(solver, x0, m, dyn)
    assert CHAIN_END in first[3] and solver._fast is None
    recorded = solve(solver, x0, m, dyn)
    assert any(e[0] is not None for e in solver._graphs.values())           # the second call recorded the chain ...
    assert solver._fast is None
    replayed = solve(solver, x0, m, dyn)
    assert solver._fast is None                                             # ... and no call goes round the refill of the pack
    for other in (recorded, replayed):
        for a, b in zip(first[:3], other[:3]):
            assert torch.equal(a, b)
    with torch.no_grad():
        m.W1.mul_(0.9)
    moved = solve(solver, x0, m, dyn)                                       # a replay, on the new weights
    assert solver._fast is None
    fresh_m = module(key, device_loop=True)
    with torch.no_grad():
        fresh_m.W1.copy_(m.W1)
    fresh = solve(make_solver(key), x0, fresh_m, dyn)
    for a, b in zip(moved[:3], fresh[:3]):
        assert torch.equal(a, b)
    assert not torch.equal(moved[1], first[1])


# ---- 7. a caller's capture: the chain holds no host synchronisation
def test_a_solve_can_be_captured_by_the_caller():
    key = ("softplus", "A")
    P = dc.problem(key)
    x0, dyn = inputs(key)
    m = module(key, device_loop=True)
    lo, hi = dev(P["lo"]), dev(P["hi"])

    def make():         # (bounds on the device: a capture takes no copy from pageable host memory)
        return make_solver(key, bounds=(lo, hi), graph=False, lazy_status=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up on a side stream (allocations, library load); also the eager result
        eager = solve(make(), x0, m, dyn)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert CHAIN_END in eager[3]
    solver = make()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = solve(solver, x0, m, dyn)
    assert solver._pending is None and CHAIN_END in got[3]
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(got[:3], eager[:3]):
            assert torch.equal(a, b)


# ---- 8. the gradient: the chain replaces the loop only
@pytest.mark.parametrize("param_grad", ["device", "live"])
@pytest.mark.parametrize("act", ["softplus", "relu"])
def test_the_gradient_behind_the_chain_is_the_host_loops(act, param_grad):
    key = (act, "A")
    P = dc.problem(key)
    nx, nu, H, B, T = P["dims"]
    rng = np.random.RandomState(77)
    gx, gu = dev(rng.randn(T, B, nx)), dev(rng.randn(T, B, nu))
    x0, dyn = inputs(key)
    grads = {}
    for loop in (True, False):
        m = module(key, device_loop=loop, param_grad=param_grad)
        solver = make_solver(key, max_iter=6, detach_unconverged=False, update_dynamics=False)     # the cost is what is learnt
        solver.__dict__.pop("_loop_flag", None)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x, u, _ = solver((x0, m, dyn))
        assert (solver.__dict__.get("_loop_flag") is not None) == loop      # the device loop ran (the host loop leaves no such flag)
        assert x.requires_grad and u.requires_grad
        grads[loop] = [npy(g) for g in torch.autograd.grad((x * gx).sum() + (u * gu).sum(), [m.Q, m.p, m.W1, m.b1, m.w2])]
    for got, want, what in zip(grads[True], grads[False], ("Q", "p", "W1", "b1", "w2")):
        assert np.isfinite(got).all(), what
        assert_close(got, want, TOL_COSTATE, "gradient %s (%s), chain against host loop" % (what, param_grad))
        if act == "relu" and what == "b1":
            assert not got.any()        # db1 = w2 act''(z) q + r w2 act'(z): relu has act'' = 0, and the loss does not read the costs
        else:
            assert np.abs(got).max() > 0, what


def test_nothing_to_differentiate_ends_with_the_chain():
    """grad mode on, no leaf wants a gradient: no launch behind the chain's one read-back"""
    key = ("softplus", "A")
    x0, dyn = inputs(key)
    m = module(key, device_loop=True).requires_grad_(False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, u, costs = make_solver(key)((x0, m, dyn))
    assert CHAIN_END in _lib.last_kernel_name() and not x.requires_grad and not u.requires_grad


# ---- 9. what the chain does not take falls through to today's route
def in_bounds(P, x, u, costs):
    return bool(torch.isfinite(x).all()) and bool(torch.isfinite(costs).all()) and bool((u >= dev(P["lo"])).all()) and \
        bool((u <= dev(P["hi"])).all())


def test_a_size_outside_the_limits_solves_on_todays_route():
    key = ("softplus", "A")
    P = dc.problem(key)
    x0, dyn = inputs(key)
    m = MlpCost(3, 1, 257, seed=0, device_loop=True).cuda()
    assert _lib.load().dmpc_mlp_cost_supported(3, 1, 257, m.act_code) == 0
    x, u, costs, name = solve(make_solver(key, max_iter=2), x0, m, dyn)
    assert CHAIN_END not in name, name
    assert in_bounds(P, x, u, costs)


def test_a_batch_coupled_solve_stays_on_the_host_loop():
    key = ("softplus", "A")
    P = dc.problem(key)
    x0, dyn = inputs(key)
    x, u, costs, name = solve(make_solver(key, max_iter=2, batch_coupled=True), x0, module(key, device_loop=True), dyn)
    assert CHAIN_END not in name, name
    assert in_bounds(P, x, u, costs)
    xh, uh, costs_h, _ = solve(make_solver(key, max_iter=2, batch_coupled=True), x0, module(key, device_loop=False), dyn)
    assert torch.equal(x, xh) and torch.equal(u, uh) and torch.equal(costs, costs_h)


def test_learned_dynamics_keep_the_host_loop():
    key = ("softplus", "A")
    P = dc.problem(key)
    x0, _ = inputs(key)
    x, u, costs, name = solve(make_solver(key, max_iter=2), x0, module(key, device_loop=True), MlpDx(3, 1, 8, seed=1).cuda())
    assert CHAIN_END not in name, name
    assert in_bounds(P, x, u, costs)


def test_a_single_timestep_is_refused_by_the_gate():
    key = ("softplus", "E")
    x0, dyn = inputs(key)
    assert make_solver(key, max_iter=2)._cost_chain_ok(module(key, device_loop=True), dyn, x0) is False
    assert make_solver(("softplus", "A"))._cost_chain_ok(module(("softplus", "A"), device_loop=True), inputs(("softplus", "A"))[1],
                                                         inputs(("softplus", "A"))[0]) is True


def test_a_single_timestep_keeps_the_host_loop():
    """case E (T = 1): the gate above refuses it, and the host loop solves it - `MPCstep.backward_rec` serves a single
    timestep by the box QP alone (`dmpc_mpc_backward_rec` starts at T = 2), the search is `dmpc_mpc_forward_rec_mlp_cost`'s"""
    key = ("softplus", "E")
    P = dc.problem(key)
    x0, dyn = inputs(key)
    x, u, costs, name = solve(make_solver(key, max_iter=2), x0, module(key, device_loop=True), dyn)
    assert CHAIN_END not in name, name
    assert in_bounds(P, x, u, costs)
    ref = mc.oracle_iterates(*key)[0]
    x, u, costs, name = solve(make_solver(key, max_iter=1), x0, module(key, device_loop=True), dyn)
    assert SEARCH_KERNEL in name, name
    assert_close(npy(u), ref["u"], TOL_STEP, "T = 1 u")
    assert_close(npy(x), ref["x"], TOL_STEP, "T = 1 x")
    assert_close(npy(costs), ref["costs"], TOL_STEP, "T = 1 costs")


@pytest.mark.parametrize("nx,nu,B", [(2, 1, 6), (4, 2, 5), (5, 3, 3)])
def test_the_single_timestep_recursion_against_the_oracle(nx, nu, B):
    """`MPCstep.backward_rec` at T = 1 against oracle.mpc.mpc_backward_rec (per-trajectory termination): gains, feed-forward
    and the rows of clamped controls.  Bounds tight enough that some controls clamp and some stay free."""
    from chainer_differentiable_mpc_amd import MPCstep
    from oracle import mpc as ompc
    ns = nx + nu
    rs = np.random.RandomState(100 + ns)
    A = rs.randn(1, B, ns, ns)
    C = A @ np.transpose(A, (0, 1, 3, 2)) + 0.5 * np.eye(ns)
    c = rs.randn(1, B, ns)
    u0 = 0.1 * rs.randn(1, B, nu)
    lo, hi = np.full((1, B, nu), -0.3), np.full((1, B, nu), 0.3)
    F = np.zeros((0, B, nx, ns))
    Ks_ref, ks_ref, _, free = ompc.mpc_backward_rec(C, c, F, None, u0, lo, hi, 1, nx, nu, batch_coupled=False)
    assert 0 < free.sum() < free.size                                  # both kinds of row are there
    step = MPCstep(controls=dev(u0), T=1, u_upper=dev(hi), u_lower=dev(lo), n_batch=B, n_state=nx, n_ctrl=nu,
                   current_states=dev(rs.randn(1, B, nx)), true_cost=None, true_dynamics=None, ls_decay=mc.LS_DECAY,
                   max_ls_iter=mc.MAX_LS_ITER, need_expand=True)
    Ks, ks, back = step.backward_rec(dev(C), dev(c), dev(F), None)
    assert list(Ks.shape) == [1, B, nu, nx] and list(ks.shape) == [1, B, nu] and back.n_total_qp_iter >= 1
    assert_close(npy(ks), ks_ref, TOL_PRIMAL, "T = 1 ks")
    assert_close(npy(Ks), Ks_ref, TOL_PRIMAL, "T = 1 Ks")
    assert not npy(Ks)[0][free[0] == 0].any()                          # exact-zero gain rows where the control is clamped


def test_cpu_tensors_keep_the_autograd_route():
    key = ("softplus", "A")
    P = dc.problem(key)
    nx, nu, H, B, T = P["dims"]
    cpu = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)       # noqa: E731
    solver = BoxDDP(T, cpu(P["lo"]), cpu(P["hi"]), B, nx, nu, None, eps=EPS, max_iter=2, line_search_decay=mc.LS_DECAY,
                    max_line_search_iter=mc.MAX_LS_ITER, quiet=True)
    x0, dyn = inputs(key)
    assert CHAIN_END not in solve(make_solver(key, max_iter=1), x0, module(key), dyn)[3]      # (the name is no stale one)
    x, u, costs, name = solve(solver, cpu(P["x_init"]), mc.module(P, device="cpu", device_loop=True), LinDx(cpu(P["F"]), cpu(P["f"])))
    assert CHAIN_END not in name and not x.is_cuda, name
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(costs).all())
    assert bool((u >= cpu(P["lo"])).all()) and bool((u <= cpu(P["hi"])).all())
