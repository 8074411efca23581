"""GPU: BoxDDP's iLQR loop with an `MlpDx` as ONE chain of launches (`dmpc_box_ddp`, dyn_kind 2; `MlpDx(device_loop=True)`):
against the float64 oracle's loop, against the host loop it replaces, `search_linearizes` 1 against 0 bit for bit, the packed
weight buffer under a recorded hipGraph, a caller's capture, the gradient, and the problems the chain does not take."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import BoxDDP, MlpDx, MPCstep, QuadCost, _lib
from chainer_differentiable_mpc_amd.util import get_traj
from tests import box_ddp_mlp_cases as cases
from tests.helpers import TOL_COSTATE, TOL_PRIMAL, assert_close, npy, tie_rows
from tests.mlp_dx_cases import BOUND, CASES, LS_DECAY, MAX_LS_ITER

pytestmark = pytest.mark.gpu

SEARCH_KERNEL = "mpc_forward_rec_mlp_kernel"
CHAIN_END = "box_ddp_summary_kernel"
EPS = 1e-3


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(a, dtype=dtype, device="cuda")


def make_solver(key, max_iter=10, bounds=(-BOUND, BOUND), **kw):
    nx, nu, H, B, T, s = key[1]
    return BoxDDP(T, bounds[0], bounds[1], B, nx, nu, None, eps=EPS, max_iter=max_iter, line_search_decay=LS_DECAY,
                  max_line_search_iter=MAX_LS_ITER, quiet=True, **kw)


def inputs(key):
    P = cases.problem(key)
    return dev(P["x_init"]), QuadCost(dev(P["C"]), dev(P["c"]))


def solve(solver, x0, cost, mlp):
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        x, u, costs = solver((x0, cost, mlp))
    return x, u, costs, _lib.last_kernel_name()


# ---- 1. one iteration against the oracle's loop stopped after one
@pytest.mark.parametrize("key", cases.ONE_ITERATION, ids=cases.name)
def test_one_iteration_against_the_oracle(key):
    ref = cases.oracle_one_iteration(key)
    keep = ~tie_rows(ref["old_costs"], ref["costs"])
    assert (~keep).sum() <= 1
    x0, cost = inputs(key)
    x, u, costs, name = solve(make_solver(key, max_iter=1), x0, cost, cases.module(key, device_loop=True))
    assert CHAIN_END in name, name
    assert_close(npy(u)[:, keep], ref["u"][:, keep], TOL_PRIMAL, "u")
    assert_close(npy(x)[:, keep], ref["x"][:, keep], TOL_PRIMAL, "x")
    assert_close(npy(costs)[keep], ref["costs"][keep], TOL_PRIMAL, "costs")


# ---- 2. the loop
@pytest.mark.parametrize("key", cases.LOOP, ids=cases.name)
def test_the_loop_against_the_oracle_and_the_host_loop(key):
    """x and u are not compared with the oracle's: the flat valley tests/test_mlp_dx_gpu.py::test_box_ddp_with_the_network documents"""
    nx, nu, H, B, T, s = key[1]
    ref = cases.oracle_loop(key)
    x0, cost = inputs(key)
    mlp = cases.module(key, device_loop=True)
    solver = make_solver(key)
    x, u, costs, name = solve(solver, x0, cost, mlp)
    assert CHAIN_END in name, name                                # the route was taken
    assert_close(npy(costs), ref["costs"], TOL_PRIMAL, "costs")
    assert bool((u.abs() <= BOUND).all())
    with torch.no_grad():
        again = get_traj(T, u, x0, lambda a, b: mlp(a, b))
    assert float((again - x).abs().max()) <= 1e-5
    assert 1 <= solver.n_iter <= 10
    host = cases.module(key, device_loop=False)
    _, uh, costs_host, name_host = solve(make_solver(key), x0, cost, host)
    assert SEARCH_KERNEL in name_host, name_host                  # the default stays the host loop
    assert_close(npy(costs), npy(costs_host), TOL_PRIMAL, "costs, chain against host loop")


# ---- 3. / 4. the C ABI directly
def chain(key, search_linearizes, max_iter, rows=None):
    """dmpc_box_ddp(dyn_kind = 2) through ctypes -> dict of its outputs (and rc)"""
    nx, nu, H, B, T, s = key[1]
    P = cases.problem(key)
    sl = slice(None) if rows is None else rows
    x0, C, c = dev(P["x_init"][sl]), dev(P["C"][:, sl]), dev(P["c"][:, sl])
    lo, hi = dev(P["lo"][:, sl]), dev(P["hi"][:, sl])
    B = x0.shape[0]
    mlp = cases.module(key)
    packed = mlp.packed_weights(x0.device).clone()
    params = (ctypes.c_float * 4)(float(H), float(mlp.act_code), 1.0, float(search_linearizes))
    f32 = dict(dtype=torch.float32, device="cuda")
    u0 = torch.zeros((T, B, nu), **f32)
    out = dict(x=torch.full((T, B, nx), np.nan, **f32), u=torch.full((T, B, nu), np.nan, **f32), costs=torch.full((B,), np.nan, **f32),
               norm_best=torch.full((B,), np.nan, **f32), norm_last=torch.full((B,), np.nan, **f32),
               state=torch.full((8,), -1, dtype=torch.int32, device="cuda"), info=torch.full((B,), -1, dtype=torch.int32, device="cuda"))
    lib = _lib.load()
    need = lib.dmpc_box_ddp_workspace_bytes(T, B, nx, nu)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    ptr = _lib.ptr
    rc = lib.dmpc_box_ddp(T, B, nx, nu, ptr(x0), ptr(C), ptr(c), ptr(packed), None, 2, ctypes.cast(params, ctypes.c_void_p), ptr(u0),
                          ptr(lo), ptr(hi), EPS, 5, LS_DECAY, MAX_LS_ITER, 1e-4, max_iter, 20, 1, 0, ptr(out["x"]), ptr(out["u"]),
                          ptr(out["costs"]), ptr(out["norm_best"]), ptr(out["norm_last"]), ptr(out["state"]), ptr(ws), need,
                          ptr(out["info"]), _lib.stream_ptr(x0.device))
    out["kernel"] = _lib.last_kernel_name()
    torch.cuda.synchronize()
    out["rc"] = rc
    return out


@pytest.mark.parametrize("max_iter", [1, 2, 10])
@pytest.mark.parametrize("key", cases.LOOP, ids=cases.name)
def test_the_search_that_linearizes_returns_the_same_bits(key, max_iter):
    a, b = chain(key, 0, max_iter), chain(key, 1, max_iter)
    assert a["rc"] == 0 and b["rc"] == 0
    assert CHAIN_END in a["kernel"] and CHAIN_END in b["kernel"]
    for k in ("x", "u", "costs", "norm_best", "norm_last", "state", "info"):
        assert torch.equal(a[k], b[k]), k
    assert bool(torch.isfinite(a["x"]).all()) and 1 <= int(a["state"][1]) <= max_iter


@pytest.mark.parametrize("search_linearizes", [0, 1])
@pytest.mark.parametrize("key", cases.LOOP[:2], ids=cases.name)
def test_a_trajectory_does_not_depend_on_its_batch(key, search_linearizes):
    """max_iter = 1 (the stop tests of a longer loop are batch-global); the norms are not compared: the reference's reshape in
    full_du_norm mixes the rows of a batch"""
    B = key[1][3]
    whole = chain(key, search_linearizes, 1)
    assert whole["rc"] == 0
    for b in range(B):
        alone = chain(key, search_linearizes, 1, rows=slice(b, b + 1))
        assert alone["rc"] == 0
        for k in ("x", "u"):
            assert torch.equal(alone[k][:, 0], whole[k][:, b]), (k, b)
        assert torch.equal(alone["costs"][0], whole["costs"][b]), b


# ---- 5. the packed weights under the solver's own hipGraph
def test_a_recorded_chain_follows_the_weights():
    key = cases.LOOP[1]
    x0, cost = inputs(key)
    mlp = cases.module(key, device_loop=True)
    solver = make_solver(key)
    first = solve(solver, x0, cost, mlp)
    assert CHAIN_END in first[3]
    recorded = solve(solver, x0, cost, mlp)
    assert any(e[0] is not None for e in solver._graphs.values())           # the second call recorded the chain ...
    replayed = solve(solver, x0, cost, mlp)
    assert solver._fast is None                                             # ... and no call goes round the refill of the pack
    for other in (recorded, replayed):
        for a, b in zip(first[:3], other[:3]):
            assert torch.equal(a, b)
    with torch.no_grad():
        mlp.W1.mul_(0.9)
    moved = solve(solver, x0, cost, mlp)                                    # a replay, on the new weights
    fresh_mlp = cases.module(key, device_loop=True)
    with torch.no_grad():
        fresh_mlp.W1.copy_(mlp.W1)
    fresh = solve(make_solver(key), x0, cost, fresh_mlp)
    for a, b in zip(moved[:3], fresh[:3]):
        assert torch.equal(a, b)
    assert not torch.equal(moved[1], first[1])


# ---- 6. a caller's capture: the chain holds no host synchronisation
def test_a_solve_can_be_captured_by_the_caller():
    key = cases.LOOP[0]
    x0, cost = inputs(key)
    nx, nu, H, B, T, s = key[1]
    mlp = cases.module(key, device_loop=True)
    lo, hi = torch.full((T, B, nu), -BOUND, device="cuda"), torch.full((T, B, nu), BOUND, device="cuda")

    def make():         # (bounds on the device: a capture takes no copy from pageable host memory)
        return make_solver(key, bounds=(lo, hi), graph=False, lazy_status=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up on a side stream (allocations, library load); also the eager result
        eager = solve(make(), x0, cost, mlp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert CHAIN_END in eager[3]
    solver = make()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = solve(solver, x0, cost, mlp)
    assert solver._pending is None and CHAIN_END in got[3]
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(got[:3], eager[:3]):
        assert torch.equal(a, b)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(got[:3], eager[:3]):
        assert torch.equal(a, b)


# ---- 7. the gradient: the chain replaces the loop only
@pytest.mark.parametrize("device_grad", [False, True])
@pytest.mark.parametrize("case", CASES[:2])
def test_the_gradient_reaches_the_weights(case, device_grad):
    """tests/test_mlp_dx_gpu.py::test_box_ddp_gradient_reaches_the_weights with the loop on the chain"""
    nx, nu, H, B, T, s = case
    key = ("tanh", case)
    P = cases.problem(key)
    mlp = cases.module(key, device_loop=True, device_grad=device_grad)
    x0, C, c = dev(P["x_init"]), dev(P["C"]), dev(P["c"])
    rng = np.random.RandomState(s + 40)
    gx, gu = dev(rng.randn(T, B, nx)), dev(rng.randn(T, B, nu))
    params = [mlp.W1, mlp.b1, mlp.W2, mlp.b2]
    solver = make_solver(key, detach_unconverged=False)
    solver.__dict__.pop("_loop_flag", None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, u, _ = solver((x0, QuadCost(C, c), mlp))
    assert solver.__dict__.get("_loop_flag") is not None            # the device loop ran (the host loop leaves no such flag)
    assert x.requires_grad and u.requires_grad
    got = torch.autograd.grad((x * gx).sum() + (u * gu).sum(), params)
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


# ---- 8. what the chain does not take falls through to the host loop
def test_a_size_outside_the_limits_solves_on_the_host_loop():
    nx, nu, H, B, T = 3, 1, 300, 2, 4
    P = cases.problem(("tanh", (nx, nu, 5, B, T, 6)))
    mlp = MlpDx(nx, nu, H, seed=0, device_loop=True).cuda()
    solver = BoxDDP(T, -BOUND, BOUND, B, nx, nu, None, eps=EPS, max_iter=2, quiet=True)
    x, u, costs, name = solve(solver, dev(P["x_init"]), QuadCost(dev(P["C"]), dev(P["c"])), mlp)
    assert CHAIN_END not in name and SEARCH_KERNEL not in name, name
    assert bool(torch.isfinite(x).all()) and bool((u.abs() <= BOUND).all()) and bool(torch.isfinite(costs).all())


def test_a_batch_coupled_solve_stays_on_the_host_loop():
    key = cases.LOOP[0]
    x0, cost = inputs(key)
    x, u, costs, name = solve(make_solver(key, max_iter=2, batch_coupled=True), x0, cost, cases.module(key, device_loop=True))
    assert SEARCH_KERNEL in name, name
    assert bool(torch.isfinite(x).all()) and bool((u.abs() <= BOUND).all()) and bool(torch.isfinite(costs).all())
    xh, uh, costs_h, _ = solve(make_solver(key, max_iter=2, batch_coupled=True), x0, cost, cases.module(key, device_loop=False))
    assert torch.equal(x, xh) and torch.equal(u, uh) and torch.equal(costs, costs_h)
