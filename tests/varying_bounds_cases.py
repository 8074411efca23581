"""Problems of the varying-bounds tests (tests/test_varying_bounds_cpu.py, tests/test_varying_bounds_gpu.py): control bounds
that depend on the time step, the trajectory and the control index, asymmetric about zero, with some controls pinned by
lower == upper; one MPC step per kernel family the step's dispatch can take (csrc/mpc_api.hip); the numpy oracle's answers,
computed once per case and shared; and the figures the CPU test holds the cases to, so that a kernel which misreads its bounds
cannot pass the GPU comparison."""
import collections
import functools

import numpy as np

from chainer_differentiable_mpc_amd import synthetic
from oracle import mpc as ompc
from tests.helpers import tie_rows

LS_DECAY, MAX_LS_ITER = 0.2, 5
PIN_SHARE = 0.08


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def bounds(T, B, nu, bound, seed, pin):
    """lower in -bound * [0.3, 1.7), upper in bound * [0.3, 1.7), every entry its own draw; with `pin` about 8 % of the entries
    get lower == upper == half of one of their two bounds.  float32-representable float64 arrays."""
    r = np.random.RandomState(1000 + seed)
    lo = -bound * (0.3 + 1.4 * r.rand(T, B, nu))
    hi = bound * (0.3 + 1.4 * r.rand(T, B, nu))
    if pin:
        picked = r.rand(T, B, nu) < PIN_SHARE
        coin = r.rand(T, B, nu) < 0.5
        value = 0.5 * np.where(coin, lo, hi)
        lo, hi = np.where(picked, value, lo), np.where(picked, value, hi)
    return f32(lo), f32(hi)


def rollout(p, u):
    xs = [p["x_init"]]
    for t in range(u.shape[0] - 1):
        xs.append(np.einsum("bij,bj->bi", p["F"][t], np.concatenate((xs[t], u[t]), axis=1)) + p["f"][t])
    return f32(np.stack(xs))


def step_case(B, T, nx, nu, bound, seed):
    """-> (p, lo, hi, u_nom, x_nom): the synthetic problem, pinned varying bounds, a non-zero nominal plan clipped into them
    (some of its entries exactly on a bound: that QP bound is exactly 0) and its float32-rounded rollout"""
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=seed, with_f=True)
    lo, hi = bounds(T, B, nu, bound, seed, pin=True)
    r = np.random.RandomState(2000 + seed)
    u_nom = f32(np.clip(0.6 * bound * r.randn(T, B, nu), lo, hi))
    return p, lo, hi, u_nom, rollout(p, u_nom)


# One row per kernel family: the substrings are of what `dmpc_last_kernel_name` reports after `backward_rec` and after
# `forward_rec` (tests/golden/mpc_routes.json has the spelling).  B = 8 where a family wants whole wavefronts (two groups of four
# trajectories, so a roll of the bounds by four is visible), the smallest ragged batch where it does not.  `seed` is the row's
# own: 7 where the oracle meets every condition of tests/test_varying_bounds_cpu.py with it in both need_expand forms, otherwise
# the first of 0, 1, 2, ... that does.  (17,1) has 20 controls in all and met them with no seed below 80 at a scale of 0.5: 0.25.
Row = collections.namedtuple("Row", "id B T nx nu bound env sweep search seed")
ROUTES = [
    Row("stream-8-2", 8, 4, 8, 2, 0.25, {}, "mpc_backward_asm_kernel<8, 2", "mpc_forward_asm_kernel<8, 2>", 45),
    Row("stream-3-1", 8, 4, 3, 1, 0.5, {}, "mpc_backward_asm_kernel<3, 1", "mpc_forward_asm_kernel<3, 1>", 10),
    Row("ring-4-4", 8, 4, 4, 4, 0.375, {}, "mpc_backward_rec_dma_kernel<4, 4", "mpc_forward_rec_kernel<4, 4, 16, true, false>", 7),
    Row("ring-sweep-stream-search-6-2", 8, 4, 6, 2, 0.25, {}, "mpc_backward_rec_dma_kernel<6, 2", "mpc_forward_asm_kernel<6, 2>", 0),
    Row("ring-sweep-bank-search-12-3", 8, 4, 12, 3, 0.25, {}, "mpc_backward_rec_dma_kernel<12, 3",
        "mpc_forward_rec_kernel<12, 3, 16, false, false>", 1),
    Row("ring-8-2-no-stream", 8, 4, 8, 2, 0.25, {"DMPC_NO_MPC_ASM": "1"}, "mpc_backward_rec_dma_kernel<8, 2",
        "mpc_forward_rec_kernel<8, 2, 16, true, false>", 45),
    Row("banks-ragged-8-2", 6, 5, 8, 2, 0.25, {}, "mpc_backward_rec_kernel<8, 2, 16, false>",
        "mpc_forward_rec_kernel<8, 2, 16, false, false>", 0),
    Row("banks-ragged-3-1", 5, 5, 3, 1, 0.5, {}, "mpc_backward_rec_kernel<3, 1, 16, false>",
        "mpc_forward_rec_kernel<3, 1, 16, false, false>", 13),
    Row("banks-ragged-4-4", 5, 5, 4, 4, 0.375, {}, "mpc_backward_rec_kernel<4, 4, 16, false>",
        "mpc_forward_rec_kernel<4, 4, 16, false, false>", 7),
    Row("container-5-3", 8, 4, 5, 3, 0.375, {}, "mpc_backward_rec_kernel<8, 4, 16, true>",
        "mpc_forward_rec_kernel<8, 4, 16, false, true>", 2),
    Row("container-9-2", 5, 5, 9, 2, 0.25, {}, "mpc_backward_rec_kernel<13, 2, 16, true>",
        "mpc_forward_rec_kernel<13, 2, 16, false, true>", 2),
    Row("wide-12-4", 8, 4, 12, 4, 0.25, {}, "lqr_wide_kernel<12, 4, 2, 2, false, false, true>",
        "mpc_wide_forward_kernel<12, 4, 2, false>", 1),
    Row("wide-16-8", 8, 4, 16, 8, 0.25, {}, "lqr_wide_kernel<16, 8, 2, 2, false, false, true>",
        "mpc_wide_forward_kernel<16, 8, 2, false>", 0),
    Row("wide-padded-5-5", 8, 4, 5, 5, 0.25, {}, "lqr_wide_kernel<12, 8, 2, 2, true", "mpc_wide_forward_kernel<12, 8, 2, true>", 7),
    Row("wide-padded-9-4", 8, 4, 9, 4, 0.25, {}, "lqr_wide_kernel<12, 4, 2, 2, true", "mpc_wide_forward_kernel<12, 4, 2, true>", 7),
    Row("matrix-core-32-8", 4, 5, 32, 8, 0.25, {}, "lqr_wave_mfma_backward<32, 8, false, false, false, true>",
        "mpc_staged_forward_kernel", 7),
    Row("matrix-core-16-8", 3, 5, 16, 8, 0.25, {}, "lqr_wave_mfma_backward<16, 8, false, false, false, true>",
        "mpc_staged_forward_kernel", 7),
    Row("matrix-core-padded-24-8", 4, 5, 24, 8, 0.25, {}, "lqr_wave_mfma_backward<32, 8, false, false, true, true>",
        "mpc_staged_forward_kernel", 7),
    Row("matrix-core-padded-21-3", 4, 5, 21, 3, 0.25, {}, "lqr_wave_mfma_backward<32, 8, false, false, true, true>",
        "mpc_staged_forward_kernel", 7),
    Row("matrix-core-padded-12-8", 3, 5, 12, 8, 0.25, {}, "lqr_wave_mfma_backward<16, 8, false, false, true, true>",
        "mpc_staged_forward_kernel", 7),
    Row("runtime-17-1", 4, 5, 17, 1, 0.25, {}, "mpc_generic_backward_kernel<1>", "mpc_staged_forward_kernel", 22),
    Row("runtime-40-5", 4, 5, 40, 5, 0.25, {}, "mpc_generic_backward_kernel<5>", "mpc_staged_forward_kernel", 0),
    Row("runtime-12-4", 3, 5, 12, 4, 0.25, {}, "mpc_generic_backward_kernel<4>", "mpc_staged_forward_kernel", 1),
    Row("runtime-17-1-plain-search", 4, 5, 17, 1, 0.25, {"DMPC_NO_MPC_STAGED_FWD": "1"}, "mpc_generic_backward_kernel<1>",
        "mpc_generic_forward_kernel", 22),
    Row("tiled-4-10", 3, 5, 4, 10, 0.25, {}, "mpc_tiled_backward_kernel", "mpc_tiled_forward_kernel", 7),
    Row("tiled-70-3", 3, 5, 70, 3, 0.25, {}, "mpc_tiled_backward_kernel", "mpc_tiled_forward_kernel", 7),
]
ROUTE = {r.id: r for r in ROUTES}


@functools.lru_cache(maxsize=None)
def route_problem(row_id):
    r = ROUTE[row_id]
    return step_case(r.B, r.T, r.nx, r.nu, r.bound, r.seed)


def oracle_forward(p, lo, hi, u_nom, x_nom, need_expand, batch_coupled=False):
    T, B, nu = u_nom.shape
    nx = x_nom.shape[2]
    x, u, bo, fo, Ks, ks = ompc.mpc_forward(p["C"], p["c"], p["F"], p["f"], u_nom, x_nom, lo, hi, ompc.QuadCost(p["C"], p["c"]),
                                            ompc.LinDx(p["F"], p["f"]), LS_DECAY, MAX_LS_ITER, T, nx, nu, need_expand=need_expand,
                                            batch_coupled=batch_coupled)
    return dict(x=x, u=u, Ks=Ks, ks=ks, costs=fo.costs, n_total_qp_iter=bo.n_total_qp_iter)


def taylor_model(p, u_nom, x_nom, need_expand):
    """(c_hat, f_hat) as `MPCstep.forward` hands them to backward_rec (mpc_step.py:305-317)"""
    if not need_expand:
        return p["c"], p["f"]
    tau = np.concatenate((x_nom, u_nom), axis=2)
    return np.einsum("tbij,tbj->tbi", p["C"], tau) + p["c"], None


@functools.lru_cache(maxsize=None)
def oracle_step(row_id, need_expand, batch_coupled=False):
    """the oracle's step of a row; per-trajectory termination also gives `n_qp` [B]: every trajectory's own QP pass total,
    from the sweep run on that trajectory alone"""
    r = ROUTE[row_id]
    p, lo, hi, u_nom, x_nom = route_problem(row_id)
    out = oracle_forward(p, lo, hi, u_nom, x_nom, need_expand, batch_coupled)
    if not batch_coupled:
        c_hat, f_hat = taylor_model(p, u_nom, x_nom, need_expand)
        one = lambda a, b: None if a is None else a[:, b:b + 1]     # noqa: E731
        out["n_qp"] = np.array([ompc.mpc_backward_rec(one(p["C"], b), one(c_hat, b), one(p["F"], b), one(f_hat, b), one(u_nom, b),
                                                      one(lo, b), one(hi, b), r.T, r.nx, r.nu, batch_coupled=False)[2].n_total_qp_iter
                                for b in range(r.B)])
    return out


def on_lower(u, lo):
    return np.abs(u - lo) <= 1e-8           # the reference's test, mpc_step.py:363


def on_upper(u, hi):
    return np.abs(u - hi) <= 1e-8


def mutations(lo, hi):
    """the ways a kernel can misread its bounds -> (name, lower, upper)"""
    T, B, nu = lo.shape
    out = [("rolled along t", np.roll(lo, 1, axis=0), np.roll(hi, 1, axis=0)),
           ("rolled along b", np.roll(lo, 1, axis=1), np.roll(hi, 1, axis=1))]
    if B > 4:
        out.append(("rolled by four along b", np.roll(lo, 4, axis=1), np.roll(hi, 4, axis=1)))
    if nu > 1:
        out.append(("rolled along the control axis", np.roll(lo, 1, axis=2), np.roll(hi, 1, axis=2)))
    out.append(("replaced by their mean", f32(np.full_like(lo, lo.mean())), f32(np.full_like(hi, hi.mean()))))
    out.append(("lower and upper exchanged in magnitude", -hi, -lo))
    return out


def figures(row_id, need_expand):
    """what tests/test_varying_bounds_cpu.py asserts of a row, measured on the oracle alone"""
    p, lo, hi, u_nom, x_nom = route_problem(row_id)
    ref = oracle_step(row_id, need_expand)
    pinned = lo == hi
    free = ~pinned
    low, up = on_lower(ref["u"], lo) & free, on_upper(ref["u"], hi) & free
    on = low | up
    values = np.concatenate((lo[free], hi[free])).astype(np.float32)
    sens = {}
    for name, mlo, mhi in mutations(lo, hi):
        mu = f32(np.clip(u_nom, mlo, mhi))
        sens[name] = float(np.abs(oracle_forward(p, mlo, mhi, mu, rollout(p, mu), need_expand)["u"] - ref["u"]).max())
    T, B, nu = lo.shape
    old = ompc.get_cost(T, u_nom, ompc.QuadCost(p["C"], p["c"]), x=x_nom)
    return dict(ordered=bool((lo <= hi).all()), strict=bool((lo[free] < hi[free]).all()), pinned_share=float(pinned.mean()),
                distinct=len(np.unique(values)) == values.size, lower_share=float(low.sum() / free.sum()),
                upper_share=float(up.sum() / free.sum()), inside_share=float((free & ~on).sum() / free.sum()),
                every_t=bool(on.any(axis=(1, 2)).all()), every_b=bool(on.any(axis=(0, 2)).all()),
                every_m=bool(on.any(axis=(0, 1)).all()), sensitivity=sens, ties=int(tie_rows(old, ref["costs"]).sum()),
                finite=bool(np.isfinite(ref["u"]).all() and np.isfinite(ref["Ks"]).all()))


# ---- batch-coupled termination: `form` register = the cooperative launch, fixed_grid = DMPC_NO_COOP_REGISTER=1 (read per call);
# `kernel`: a substring of the sweep's name
Coupled = collections.namedtuple("Coupled", "id B T nx nu bound seed form kernel")
COUPLED = [
    Coupled("register-8-2", 8, 4, 8, 2, 0.25, 7, "register", "mpc_backward_rec_kernel<8, 2, 16, false>"),
    Coupled("fixed-grid-8-2", 8, 4, 8, 2, 0.25, 7, "fixed_grid", "mpc_coupled_backward_kernel"),
    Coupled("register-5-3", 4, 5, 5, 3, 0.375, 7, "register", "mpc_backward_rec_kernel<8, 4, 16, true>"),
    Coupled("fixed-grid-5-3", 4, 5, 5, 3, 0.375, 7, "fixed_grid", "mpc_coupled_backward_kernel"),
    Coupled("cooperative-runtime-16-8", 3, 5, 16, 8, 0.25, 7, "register", "mpc_generic_backward_kernel<8>"),
    Coupled("fixed-grid-4-10", 3, 5, 4, 10, 0.25, 7, "fixed_grid", "mpc_coupled_backward_kernel"),
]


@functools.lru_cache(maxsize=None)
def coupled_case(B, T, nx, nu, bound, seed, need_expand):
    p, lo, hi, u_nom, x_nom = step_case(B, T, nx, nu, bound, seed)
    return (p, lo, hi, u_nom, x_nom), oracle_forward(p, lo, hi, u_nom, x_nom, need_expand, batch_coupled=True)


# ---- PNQP with pinned coordinates
@functools.lru_cache(maxsize=None)
def pinned_qp(n):
    """tests/test_pnqp_gpu.py's factorisation problem with about 30 % of its entries pinned to one of their own bounds; row 0 is
    pinned in every coordinate, row 1 in none"""
    B = 12
    p = synthetic.make_box_qp(B, n, seed=90 + n, bound=0.4)
    r = np.random.RandomState(500 + n)
    picked = r.rand(B, n) < 0.3
    picked[0], picked[1] = True, False
    value = np.where(r.rand(B, n) < 0.5, p["lower"], p["upper"])
    lower, upper = np.where(picked, value, p["lower"]), np.where(picked, value, p["upper"])
    return dict(H=p["H"], q=p["q"], lower=lower, upper=upper, pinned=picked)


# ---- the linear episode of tests/episode_cases.py with varying bounds, no pins
EPISODE_SEED = 201


@functools.lru_cache(maxsize=None)
def lin_episode_bounds():
    from tests import episode_cases as ec
    k = ec.LIN
    return bounds(k["T"], k["B"], k["nu"], k["bound"], EPISODE_SEED, pin=False)


@functools.lru_cache(maxsize=None)
def lin_episode():
    """the float64 episode under those bounds; `warm_outside`: entries of the shifted plans that lie outside the box, which does
    not shift with them"""
    from tests import episode_cases as ec
    lo, hi = lin_episode_bounds()
    ep = dict(ec.oracle_lin_episode(bounds=(lo, hi)))
    ep["warm_outside"] = int(((ep["warm"] < lo[None]) | (ep["warm"] > hi[None])).sum())
    return ep


# ---- BoxDDP with array bounds (no pins, lower < 0 < upper: u_init = None is feasible): (B, T, nx, nu, bound, seed)
DDP_LIN = [(8, 6, 3, 1, 0.5, 7), (6, 5, 8, 2, 0.25, 7), (8, 5, 12, 4, 0.25, 7)]
DDP_PENDULUM = [(8, 5, "mpc_forward_rec_pendulum_spec4_kernel"), (8, 33, "mpc_forward_rec_pendulum_spec_kernel<true>"),
                (5, 33, "mpc_forward_rec_pendulum_spec_kernel<false>")]


@functools.lru_cache(maxsize=None)
def ddp_lin_case(B, T, nx, nu, bound, seed):
    """-> (p, lo, hi, ref): ref = the float64 loop from u = 0 stopped after one iteration, and the nominal trajectory's cost"""
    from oracle import box_ddp as obox
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=seed, with_f=True)
    lo, hi = bounds(T, B, nu, bound, seed, pin=False)
    cost, dyn = ompc.QuadCost(p["C"], p["c"]), ompc.LinDx(p["F"], p["f"])
    x, u, costs, *_ = obox.box_ddp(p["x_init"], cost, dyn, T, lo, hi, nx, nu, max_iter=1, batch_coupled=False)
    u0 = np.zeros((T, B, nu))
    old = ompc.get_cost(T, u0, cost, obox.get_traj(T, u0, p["x_init"], dyn))
    return p, lo, hi, dict(x=x, u=u, costs=costs, old_costs=old)


PENDULUM_BOUND, PENDULUM_SEED = 1.0, 7          # bounds within +-1.7: inside the model's own torque limit of 2


@functools.lru_cache(maxsize=None)
def ddp_pendulum_case(B, T):
    """the built-in pendulum with its true cost -> dict(x0, Q, pv, lo, hi, step = one iLQR step from u = 0 (x, u, costs, Ks, ks),
    first = the loop stopped after one iteration, old_costs, kw = the model's search settings)"""
    from chainer_differentiable_mpc_amd import PendulumDx
    from chainer_differentiable_mpc_amd.pendulum import sample_xinit
    from oracle import box_ddp as obox
    dx = PendulumDx()
    q, pp = dx.get_true_obj()
    x0 = f32(sample_xinit(B, seed=PENDULUM_SEED))
    Q = np.tile(np.diag(q.numpy().astype(np.float64)), (T, B, 1, 1))
    pv = np.tile(pp.numpy().astype(np.float64), (T, B, 1))
    lo, hi = bounds(T, B, 1, PENDULUM_BOUND, PENDULUM_SEED, pin=False)
    kw = dict(eps=dx.mpc_eps, line_search_decay=dx.linesearch_decay, max_line_search_iter=dx.max_linesearch_iter)
    cost = ompc.QuadCost(Q, pv)
    u0 = np.zeros((T, B, 1))
    xk = obox.get_traj(T, u0, x0, obox.pendulum_step)
    Fm, fm = obox.pendulum_linearize(xk, u0)
    xs, us, _, fo, Ks, ks = ompc.mpc_forward(Q, pv, Fm, fm, u0, xk, lo, hi, cost, obox.pendulum_step, dx.linesearch_decay,
                                             dx.max_linesearch_iter, T, 3, 1, need_expand=True, batch_coupled=False)
    x, u, costs, *_ = obox.box_ddp(x0, cost, obox.pendulum_step, T, lo, hi, 3, 1, max_iter=1, linearize=obox.pendulum_linearize,
                                   batch_coupled=False, **kw)
    return dict(x0=x0, Q=Q, pv=pv, lo=lo, hi=hi, kw=kw, x_nom=xk, old_costs=ompc.get_cost(T, u0, cost, xk),
                step=dict(x=xs, u=us, costs=fo.costs, Ks=Ks, ks=ks), first=dict(x=x, u=u, costs=costs))


@functools.lru_cache(maxsize=None)
def ddp_mlp_case():
    """tests/mlp_dx_cases.CASES[1] with its bounds replaced -> (key of tests/box_ddp_mlp_cases, lo, hi, the float64 loop stopped
    after one iteration)"""
    from oracle import box_ddp as obox
    from tests import box_ddp_mlp_cases as cases
    from tests.mlp_dx_cases import BOUND, CASES
    key = ("tanh", CASES[1])
    nx, nu, H, B, T, s = key[1]
    P = cases.problem(key)
    lo, hi = bounds(T, B, nu, BOUND, 7, pin=False)
    x, u, costs, *_ = obox.box_ddp(P["x_init"], P["cost"], P["net"].step, T, lo, hi, nx, nu, eps=1e-3, max_iter=1,
                                   linearize=P["net"].linearize, batch_coupled=False, line_search_decay=cases.LS_DECAY,
                                   max_line_search_iter=cases.MAX_LS_ITER)
    u0 = np.zeros((T, B, nu))
    old = ompc.get_cost(T, u0, P["cost"], obox.get_traj(T, u0, P["x_init"], P["net"].step))
    return key, lo, hi, dict(x=x, u=u, costs=costs, old_costs=old)


# ---- MPCstep.backward through the shared-parameter entry point: tests/test_shared_mpc_gpu.py's hand-built inputs at one of its
# shapes, with varying bounds and the controls on them
SHARED_SHAPE = (3, 8, 8, 2)       # T, B, nx, nu: the LDS-DMA co-state kernel


@functools.lru_cache(maxsize=None)
def shared_case():
    T, B, nx, nu = SHARED_SHAPE
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=100 + T + 7 * B + 31 * nx + nu, with_f=False)
    rng = np.random.RandomState(1000 + B + nx)
    lo, hi = bounds(T, B, nu, 0.25, 7, pin=True)
    F = np.ascontiguousarray(np.broadcast_to(p["F"][0, 0], (T - 1, B, nx, nx + nu)))
    u = f32(lo + (0.05 + 0.9 * rng.rand(T, B, nu)) * (hi - lo))
    on = rng.rand(T, B, nu)
    u = np.where(on < 0.2, lo, np.where(on > 0.8, hi, u))
    x = f32(rng.randn(T, B, nx))
    gx, gu = f32(rng.randn(T, B, nx)), f32(rng.randn(T, B, nu))
    ref = ompc.mpc_backward(x[0], p["C"], p["c"], F, np.zeros((T - 1, B, nx)), x, u, lo, hi, gx, gu, T, nx, nu)
    return dict(C=p["C"], c=p["c"], F=F, x=x, u=u, gx=gx, gu=gu, lo=lo, hi=hi, dx0=ref[0], dF=ref[3][:T - 1], df=ref[4])
