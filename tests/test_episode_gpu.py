"""GPU: a closed-loop MPC episode as one chain of launches (`dmpc_mpc_episode`, include/dmpc_episode.h; `ClosedLoop`): bit for
bit against the pieces it is made of - `dmpc_box_ddp`, the plant's own rollout entry point at T = 2, a torch shift - driven
step by step from here; the stage cost against float64 numpy; `ClosedLoop`'s host route against its chain route; the float64
oracle's episode; one step; weights that are read, not cached; a caller's capture.  Every case runs at most 4 steps of at most 5
iterations at the sizes of tests/episode_cases.py."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import BoxDDP, ClosedLoop, LinDx, PendulumDx, QuadCost, _lib
from tests import episode_cases as ec
from tests import mlp_dx_cases
from tests.abi_calls import pendulum_start
from tests.helpers import TOL_PRIMAL, assert_close, npy

pytestmark = pytest.mark.gpu

ADVANCE = "episode_advance_kernel"
F32 = dict(dtype=torch.float32, device="cuda")
I32 = dict(dtype=torch.int32, device="cuda")


def dev(a):
    return None if a is None else torch.as_tensor(np.asarray(a), **F32).contiguous()


def floats(v):
    return None if v is None else ctypes.cast((ctypes.c_float * len(v))(*v), ctypes.c_void_p)


class Net:
    """a network of tests/mlp_dx_cases or tests/mlp2_cases as the C ABI takes it"""

    def __init__(self, net):
        self.net = net
        self.two = hasattr(net, "W3")
        self.code = _lib.mlp_hidden2(net.H1, net.H2) if self.two else net.H
        self.act = 0                                   # tanh
        self.packed = ec.mlp_packed(net)

    def rollout_weights(self):
        """(W1, b1, W2, b2) of dmpc_mlp_rollout_linearize: with two layers [W2 | W3] and [b2 | b3]"""
        n = self.net
        if self.two:
            return [dev(n.W1), dev(n.b1), dev(np.concatenate((n.W2.reshape(-1), n.W3.reshape(-1)))), dev(np.concatenate((n.b2, n.b3)))]
        return [dev(n.W1), dev(n.b1), dev(n.W2), dev(n.b2)]

    def module(self, device_loop=True):
        m = self.net.module(device="cuda")
        m.device_loop = device_loop
        return m


def pendulum_problem(B, T, seed):
    p = ec.synthetic.make_lqr_problem(B, T, 3, 1, seed=seed)
    return dict(C=p["C"], c=p["c"], x_init=pendulum_start(B, seed + 1), lo=np.full((T, B, 1), -2.0), hi=np.full((T, B, 1), 2.0))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(T, B, nx, nu, C, c, x_init, lo, hi, model=(kind, what), plant=(kind, what)): kind 0 what = (F, f), kind 1 what = None,
    kind 2 what = Net"""
    if name == "lin":
        P, k = ec.lin_problem(), ec.LIN
        return dict(P, T=k["T"], B=k["B"], nx=k["nx"], nu=k["nu"], model=(0, (P["F"], P["f"])), plant=(0, (P["plant_F"], P["plant_f"])))
    if name in ("pendulum_B4", "pendulum_B5"):      # B = 4: one launch per iteration; B = 5: sweep and search as launches of their own
        B = int(name[-1])
        return dict(pendulum_problem(B, 8, 24), T=8, B=B, nx=3, nu=1, model=(1, None), plant=(1, None))
    mc, plant = {"mlp_small": (ec.MLP_SMALL, "pendulum"), "mlp_wide": (ec.MLP_WIDE, "two"), "mlp_limit": (ec.MLP_LIMIT, "same"),
                 "mlp_one": (ec.MLP_ONE, "pendulum")}[name]
    nx, nu, H, B, T, s = mc
    P = mlp_dx_cases.problem(mc)
    model = Net(P["net"])
    pl = (1, None) if plant == "pendulum" else (2, model if plant == "same" else Net(ec.mlp2_plant_net()))
    return dict(C=P["C"], c=P["c"], x_init=P["x_init"], lo=P["lo"], hi=P["hi"], T=T, B=B, nx=nx, nu=nu, model=(2, model), plant=pl)


CASES = ["lin", "pendulum_B4", "pendulum_B5", "mlp_small", "mlp_wide", "mlp_limit", "mlp_one"]
SCALARS = (ec.EPS, 5, ec.LS_DECAY, ec.MAX_LS_ITER, 1e-4)      # eps, not_improved_lim, ls_decay, max_ls_iter, best_cost_eps
N_QP, SCRAMBLED = 20, 1


def abi_args(kind, what):
    """(F, f, host params) of a model or a plant for the C ABI; the tensors must be kept alive by the caller"""
    if kind == 0:
        return dev(what[0]), dev(what[1]), None
    if kind == 1:
        return None, None, ec.PENDULUM + (1.0,)
    return dev(what.packed), None, (float(what.code), float(what.act), 1.0, 0.0)


def episode(name, n_steps, max_iter, model_packed=None):
    """dmpc_mpc_episode through ctypes -> dict of its outputs (prefilled with NaN / -1), rc and the kernel launched last"""
    k = case(name)
    T, B, nx, nu = k["T"], k["B"], k["nx"], k["nu"]
    lib = _lib.load()
    x0, C, c, lo, hi = dev(k["x_init"]), dev(k["C"]), dev(k["c"]), dev(k["lo"]), dev(k["hi"])
    mF, mf, mp = abi_args(*k["model"])
    if model_packed is not None:
        mF = model_packed
    pF, pf, pp = (mF, mf, mp) if k["plant"][1] is k["model"][1] and k["plant"][0] == 2 else abi_args(*k["plant"])
    if k["plant"][0] == 2:
        pp = pp[:3]
    u0 = torch.zeros((T, B, nu), **F32)
    out = dict(x=torch.full((n_steps + 1, B, nx), np.nan, **F32), u=torch.full((n_steps, B, nu), np.nan, **F32),
               stage=torch.full((n_steps, B), np.nan, **F32), x_plan=torch.full((T, B, nx), np.nan, **F32),
               u_plan=torch.full((T, B, nu), np.nan, **F32), state=torch.full((n_steps, 8), -1, **I32), info=torch.full((B,), -1, **I32))
    need = lib.dmpc_mpc_episode_workspace_bytes(T, B, nx, nu)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    ptr = _lib.ptr
    rc = lib.dmpc_mpc_episode(n_steps, T, B, nx, nu, ptr(x0), ptr(C), ptr(c), ptr(mF), ptr(mf), k["model"][0], floats(mp), ptr(pF), ptr(pf),
                              k["plant"][0], floats(pp), ptr(u0), ptr(lo), ptr(hi), *SCALARS, max_iter, N_QP, SCRAMBLED, ptr(out["x"]),
                              ptr(out["u"]), ptr(out["stage"]), ptr(out["x_plan"]), ptr(out["u_plan"]), ptr(out["state"]), ptr(ws), need,
                              ptr(out["info"]), _lib.stream_ptr(x0.device))
    out["kernel"] = _lib.last_kernel_name()
    torch.cuda.synchronize()
    out["rc"] = rc
    return out


def plant_once(lib, k, x, u0):
    """one plant step through the plant's existing rollout entry point at T = 2"""
    B, nx, nu = k["B"], k["nx"], k["nu"]
    kind, what = k["plant"]
    u2 = torch.stack((u0, u0), dim=0).contiguous()
    xs = torch.full((2, B, nx), np.nan, **F32)
    ptr, stream = _lib.ptr, _lib.stream_ptr(x.device)
    if kind == 0:
        F, f = dev(what[0])[None].contiguous(), dev(what[1])[None].contiguous()
        rc = lib.dmpc_lin_rollout(2, B, nx, nu, ptr(x), ptr(u2), ptr(F), ptr(f), ptr(xs), stream)
    elif kind == 1:
        rc = lib.dmpc_pendulum_rollout_linearize(2, B, ptr(x), ptr(u2), *ec.PENDULUM, 1, ptr(xs), None, None, stream)
    else:
        w = what.rollout_weights()
        rc = lib.dmpc_mlp_rollout_linearize(2, B, nx, nu, what.code, what.act, 1, *(ptr(t) for t in w), ptr(x), ptr(u2), ptr(xs), None,
                                            None, stream)
    assert rc == 0
    torch.cuda.synchronize()
    return xs[1].clone()


def pieces(name, n_steps, max_iter):
    """the same episode from dmpc_box_ddp, the plant's rollout entry point and a torch shift, step by step"""
    k = case(name)
    T, B, nx, nu = k["T"], k["B"], k["nx"], k["nu"]
    lib = _lib.load()
    C, c, lo, hi = dev(k["C"]), dev(k["c"]), dev(k["lo"]), dev(k["hi"])
    mF, mf, mp = abi_args(*k["model"])
    x, warm = dev(k["x_init"]), torch.zeros((T, B, nu), **F32)
    need = lib.dmpc_box_ddp_workspace_bytes(T, B, nx, nu)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    ptr = _lib.ptr
    xs, us, states = [x.clone()], [], []
    info = torch.zeros((B,), **I32)
    for _ in range(n_steps):
        bx, bu = torch.full((T, B, nx), np.nan, **F32), torch.full((T, B, nu), np.nan, **F32)
        tail, st, inf = torch.empty((3, B), **F32), torch.full((8,), -1, **I32), torch.full((B,), -1, **I32)
        rc = lib.dmpc_box_ddp(T, B, nx, nu, ptr(x), ptr(C), ptr(c), ptr(mF), ptr(mf), k["model"][0], floats(mp), ptr(warm), ptr(lo), ptr(hi),
                              *SCALARS, max_iter, N_QP, SCRAMBLED, 0, ptr(bx), ptr(bu), ptr(tail[0]), ptr(tail[1]), ptr(tail[2]), ptr(st),
                              ptr(ws), need, ptr(inf), _lib.stream_ptr(x.device))
        assert rc == 0
        torch.cuda.synchronize()
        x = plant_once(lib, k, x, bu[0].contiguous())
        xs.append(x.clone()), us.append(bu[0].clone()), states.append(st.clone())
        info |= inf
        warm = torch.cat((bu[1:], bu[-1:]), dim=0).contiguous()
    return dict(x=torch.stack(xs), u=torch.stack(us), state=torch.stack(states), info=info, x_plan=bx, u_plan=bu)


@functools.lru_cache(maxsize=None)
def chain(name, n_steps=ec.N_STEPS, max_iter=ec.MAX_ITER):
    return episode(name, n_steps, max_iter)


# ---- 1. the same bits as the pieces
@pytest.mark.parametrize("name", CASES)
def test_the_chain_has_the_bits_of_its_pieces(name):
    got, want = chain(name), pieces(name, ec.N_STEPS, ec.MAX_ITER)
    assert got["rc"] == 0 and ADVANCE in got["kernel"], got["kernel"]
    for key in ("x", "u", "state", "x_plan", "u_plan", "info"):
        assert torch.equal(got[key], want[key]), key
    assert bool(torch.isfinite(got["x"]).all()) and bool(torch.isfinite(got["stage"]).all())
    assert bool((got["state"][:, 1] >= 1).all()) and bool((got["state"][:, 1] <= ec.MAX_ITER).all())
    k = case(name)
    assert torch.equal(got["x"][0], dev(k["x_init"]))
    assert bool((got["u"].abs() <= float(np.abs(k["hi"]).max())).all())


# ---- 2. the stage cost
@pytest.mark.parametrize("name", CASES)
def test_the_stage_cost_against_float64_numpy(name):
    got, k = chain(name), case(name)
    x, u = npy(got["x"]), npy(got["u"])
    want = np.stack([ec.stage_cost(k["C"][0], k["c"][0], x[s], u[s]) for s in range(ec.N_STEPS)])
    assert_close(npy(got["stage"]), want, TOL_PRIMAL, "stage cost")


# ---- 3. ClosedLoop: the host route against the chain route
def loop_objects(name, **solver_kw):
    k = case(name)
    T, B, nx, nu = k["T"], k["B"], k["nx"], k["nu"]
    kw = dict(eps=ec.EPS, max_iter=ec.MAX_ITER, line_search_decay=ec.LS_DECAY, max_line_search_iter=ec.MAX_LS_ITER, quiet=True)
    kw.update(solver_kw)
    solver = BoxDDP(T, dev(k["lo"]), dev(k["hi"]), B, nx, nu, None, **kw)

    def obj(kind, what, is_plant):
        if kind == 0:
            return LinDx(dev(what[0])[None], dev(what[1])[None]) if is_plant else LinDx(dev(what[0]), dev(what[1]))
        if kind == 1:
            return PendulumDx()
        return what.module(device_loop=True)
    model = obj(*k["model"], False)
    plant = model if k["plant"][1] is k["model"][1] and k["plant"][0] != 0 and k["plant"][0] == k["model"][0] else obj(*k["plant"], True)
    return solver, plant, dev(k["x_init"]), QuadCost(dev(k["C"]), dev(k["c"])), model


def run_loop(loop, x0, cost, model):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return loop(x0, cost, model)


@pytest.mark.parametrize("name", ["lin", "pendulum_B4", "pendulum_B5", "mlp_small"])
def test_closed_loop_host_route_against_chain_route(name):
    solver, plant, x0, cost, model = loop_objects(name)
    on_chain = ClosedLoop(solver, plant, ec.N_STEPS, device_episode=True)
    a = run_loop(on_chain, x0, cost, model)
    assert on_chain.route == "chain" and ADVANCE in _lib.last_kernel_name()
    raw = chain(name)
    for got, key in ((a.x, "x"), (a.u, "u"), (a.stage_costs, "stage"), (a.state, "state"), (a.info, "info"), (a.x_plan, "x_plan"),
                     (a.u_plan, "u_plan")):
        assert torch.equal(got, raw[key]), key                  # the class adds nothing to the C call
    on_host = ClosedLoop(solver, plant, ec.N_STEPS, device_episode=False)
    b = run_loop(on_host, x0, cost, model)
    assert on_host.route == "host" and solver.u_init is None
    assert_close(npy(b.x), npy(a.x), TOL_PRIMAL, "x, host route against chain")
    assert_close(npy(b.u), npy(a.u), TOL_PRIMAL, "u, host route against chain")
    assert_close(npy(b.stage_costs), npy(a.stage_costs), TOL_PRIMAL, "stage costs, host route against chain")
    assert torch.equal(b.state[:, 1], a.state[:, 1])            # iterations run
    assert tuple(b.state.shape) == (ec.N_STEPS, 8) and b.state.dtype == torch.int32 and tuple(b.info.shape) == tuple(a.info.shape)


# ---- 4. the float64 oracle (LinDx -> linear)
def test_the_linear_episode_against_the_float64_oracle():
    got, ref = chain("lin"), ec.oracle_lin_episode()
    assert got["rc"] == 0
    assert_close(npy(got["u"]), ref["u"], TOL_PRIMAL, "u")
    assert_close(npy(got["x"]), ref["x"], TOL_PRIMAL, "x")
    assert np.array_equal(got["state"][:, 1].cpu().numpy(), ref["n_iter"])
    on = np.abs(ref["u"]) == ec.LIN["bound"]
    # controls on a bound sit on it exactly: on the float32 bound the kernels were given
    assert np.array_equal(np.abs(got["u"].cpu().numpy())[on], np.full(int(on.sum()), np.float32(ec.LIN["bound"])))


# ---- 5. one step
@pytest.mark.parametrize("name", ["lin", "pendulum_B4", "mlp_small", "mlp_one"])
def test_one_step_is_one_solve_and_one_plant_step(name):
    got, want = episode(name, 1, ec.MAX_ITER), pieces(name, 1, ec.MAX_ITER)
    assert got["rc"] == 0
    for key in ("x", "u", "state", "x_plan", "u_plan", "info"):
        assert torch.equal(got[key], want[key]), key
    assert tuple(got["x"].shape[:1]) == (2,) and torch.equal(got["u"][0], got["u_plan"][0])


# ---- 6. the weights are read, not cached
def test_an_in_place_step_on_the_weights_is_seen_and_undone():
    solver, plant, x0, cost, model = loop_objects("mlp_small")
    loop = ClosedLoop(solver, plant, 2)
    first = run_loop(loop, x0, cost, model)
    assert loop.route == "chain"
    saved = model.W1.detach().clone()
    with torch.no_grad():
        model.W1.add_(0.05)
    moved = run_loop(loop, x0, cost, model)
    assert not torch.equal(moved.u, first.u)
    with torch.no_grad():
        model.W1.copy_(saved)
    back = run_loop(loop, x0, cost, model)
    for a, b in zip(back, first):
        assert torch.equal(a, b)
    # the same through the C ABI, on ONE packed buffer changed in place
    k = case("mlp_small")
    packed = dev(k["model"][1].packed)
    n1 = k["model"][1].net.W1.size
    one = episode("mlp_small", 2, ec.MAX_ITER, model_packed=packed)
    packed[:n1] += 0.05
    two = episode("mlp_small", 2, ec.MAX_ITER, model_packed=packed)
    packed[:n1] = dev(k["model"][1].packed)[:n1]
    three = episode("mlp_small", 2, ec.MAX_ITER, model_packed=packed)
    assert not torch.equal(one["u"], two["u"])
    for key in ("x", "u", "stage", "state", "x_plan", "u_plan"):
        assert torch.equal(one[key], three[key]), key


# ---- 7. a caller's capture: the chain holds no host synchronisation
def test_an_episode_can_be_captured_by_the_caller():
    def make():         # (bounds on the device: a capture takes no copy from pageable host memory)
        return loop_objects("mlp_small", graph=False, lazy_status=True)
    solver, plant, x0, cost, model = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up on a side stream (allocations, library load); also the eager result
        warm = ClosedLoop(solver, plant, 2)
        eager = run_loop(warm, x0, cost, model)
        warm.resolve()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert warm.route == "chain"
    solver2 = make()[0]
    loop = ClosedLoop(solver2, plant, 2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run_loop(loop, x0, cost, model)
    assert loop.route == "chain" and loop._pending is None
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert torch.equal(a, b)


def test_a_deferred_read_back_raises_at_resolve():
    """lazy_status: the state log is read when asked for; lower > upper is the solver's input assert, raised as BoxDDP raises it"""
    k = case("lin")
    solver, plant, x0, cost, model = loop_objects("lin", lazy_status=True)
    loop = ClosedLoop(solver, plant, 1)
    out = run_loop(loop, x0, cost, model)
    assert loop._pending is not None
    loop.resolve()
    assert loop._pending is None and int(out.state[0, 1]) >= 1
    bad = BoxDDP(k["T"], dev(k["hi"]), dev(k["lo"]), k["B"], k["nx"], k["nu"], None, eps=ec.EPS, max_iter=1, quiet=True, lazy_status=True)
    loop = ClosedLoop(bad, plant, 1)
    run_loop(loop, x0, cost, model)
    with pytest.raises(AssertionError, match="lower is larger than upper"):
        loop.resolve()
