"""The case table of the C-ABI's memory contract (tests/test_abi_memory_gpu.py): for every entry point of include/dmpc.h that
takes a device pointer, the smallest calls that reach each branch of its host code, with every array declared by its role
(tests/arena.py).  A row is a Case: an id, the entry point, and `make(b, lib)` which declares the arrays on the Builder `b`
and returns `(prepare, call)` - each a `(entry point, argument list)` with the arrays' handles in the list, or a callable of
`ptr` (the rows taken from tests/golden/make_lqr_routes.py).  `prepare` (a list) runs first and is not examined: it leaves
what the checked call reads (saved gains, a factorisation, a rollout's states, the shared solve's blocks).

Workspaces have exactly the size the entry point's own query states.  Nothing here needs a GPU to be imported; the data of a
row is made when the row is run."""
import ctypes

import numpy as np

import torch

from chainer_differentiable_mpc_amd import _lib, pendulum_net, synthetic
from oracle import lqr as olqr
from tests import mlp_dx_cases, shared_lqr_problems
from tests.arena import Spec
from tests.helpers import COSTATE_PATHS, TOL_PRIMAL, load_routes_script

ROUTES = load_routes_script()
LQR_ENTRY = dict(solve="dmpc_lqr_solve", backward="dmpc_lqr_backward_sweep", backward_ws="dmpc_lqr_backward_sweep_ws",
                 forward="dmpc_lqr_forward_sweep", solve_saving="dmpc_lqr_solve_saving", saved_solve="dmpc_lqr_saved_solve",
                 kkt_grad_saved="dmpc_lqr_kkt_grad_saved", kkt_grad="dmpc_lqr_kkt_grad")
PENDULUM = (10.0, 1.0, 1.0, 0.05, 2.0)       # g, m, l, dt, max_torque (env_dx/pendulum.py's defaults)
I32, F64, U8 = np.int32, np.float64, np.uint8


class Case:
    def __init__(self, id, entry, make, **meta):
        self.id, self.entry, self.make, self.meta = id, entry, make, meta

    def __repr__(self):
        return self.id


CASES = []


def add(id, entry, make, **meta):
    CASES.append(Case(id, entry, make, **meta))


def invoke(lib, call, ptr):
    if callable(call):
        return call(ptr)
    entry, args = call
    return getattr(lib, entry)(*[ptr(a) if isinstance(a, Spec) else a for a in args])


def run(case, layout, lib, device, sync):
    """the row in one layout -> (arena, rc), examined by the caller (arena.check(rc), arena.compare(other))"""
    from tests.arena import Builder
    b = Builder()
    prepare, call = case.make(b, lib)
    a = b.build(layout, device)
    for pre in prepare or []:
        rc = invoke(lib, pre, a.ptr)
        if rc > 0:
            raise RuntimeError("%s: HIP error %d from a preparing call" % (case.id, rc))
        if rc < 0:      # (refused: what it would have left reads as zeros, as in the routes' recording)
            for s in a.specs:
                if s.prefill:
                    a.view(s).zero_()
    sync()
    a.snapshot()
    rc = invoke(lib, call, a.ptr)
    a.kernel = _lib.last_kernel_name()       # (the kernel the call launched last; a refused call leaves the one before it)
    sync()
    return a, rc


def f32(a):
    return np.asarray(a, dtype=np.float32)


def lqr_problem(B, T, nx, nu, seed, with_f=True):
    return synthetic.make_lqr_problem(B, T, nx, nu, seed=seed, with_f=with_f)


def mpc_problem(B, T, nx, nu, bound, seed):
    """an MPC step from u = 0 and its nominal rollout (tests/test_mpc_paths_gpu.py's)"""
    p = lqr_problem(B, T, nx, nu, seed)
    lo, hi = -bound * np.ones((T, B, nu)), bound * np.ones((T, B, nu))
    u0 = np.zeros((T, B, nu))
    xs = [p["x_init"]]
    for t in range(T - 1):
        xs.append(np.einsum("bij,bj->bi", p["F"][t], np.concatenate((xs[t], u0[t]), axis=1)) + p["f"][t])
    return p, lo, hi, u0, np.stack(xs).astype(np.float32).astype(np.float64)


# ---- the LQR family: the case table of the routes' recording (solve, sweeps, saving solve, saved gains, both gradients) ----
def _route(c):
    def make(b, lib):
        prepare, fn = ROUTES.call(c, lib, b)
        return (None if prepare is None else [prepare]), fn
    return make


for _c in ROUTES.cases():
    add("lqr:" + _c["id"], LQR_ENTRY[_c["fn"]], _route(_c), lqr=_c)


# ---- the co-state sweep: one row per kernel it can take (tests/test_kkt_gpu.py), both dC conventions ----
def kkt_inputs(b, T, B, nx, nu, seed, dtype=np.float32):
    p = lqr_problem(B, T, nx, nu, seed)
    rng = np.random.RandomState(nx * 23 + nu + B)
    gx, gu = f32(rng.randn(T, B, nx)), f32(rng.randn(T, B, nu))
    xr, ur = olqr.lqr_solve(p["x_init"], p["C"], p["c"], p["F"], p["f"], T, nx, nu)
    if dtype == np.float32:
        xr, ur = f32(xr), f32(ur)
    ins = [b.inp(k, v, dtype) for k, v in (("C", p["C"]), ("c", p["c"]), ("F", p["F"]), ("x", xr), ("u", ur), ("gx", gx), ("gu", gu))]
    ns = nx + nu
    outs = [b.out("dx0", (B, nx), dtype), b.out("dC", (T, B, ns, ns), dtype), b.out("dc", (T, B, ns), dtype),
            b.out("dF", (T - 1, B, nx, ns), dtype), b.out("df", (T - 1, B, nx), dtype)]
    return ins, outs


def _costate(T, B, nx, nu, strict):
    def make(b, lib):
        ins, outs = kkt_inputs(b, T, B, nx, nu, 700 + 3 * nx + B)
        need = lib.dmpc_lqr_kkt_workspace_bytes(T, B, nx, nu)
        return None, ("dmpc_lqr_kkt_grad", [T, B, nx, nu] + ins + [strict] + outs + [b.ws("ws", need), need, b.info("info", B), None])
    return make


for (_T, _B, _nx, _nu), _ in COSTATE_PATHS:
    for _s in (0, 1):
        add("costate:T%d_B%d_%dx%d_strict%d" % (_T, _B, _nx, _nu, _s), "dmpc_lqr_kkt_grad", _costate(_T, _B, _nx, _nu, _s))


# ---- float64: one shape per dmpc_lqr_f64_path value, the tile shapes, a masked solve; gains taken and not ----
def _solve_f64(nx, nu, gains, mask):
    T, B = 3, 5

    def make(b, lib):
        p = lqr_problem(B, T, nx, nu, 31 + nx)
        ins = [b.inp(k, p[k], F64) for k in ("C", "c", "F", "f", "x_init")]
        m = b.inp("mask", np.arange(T * B * nu).reshape(T, B, nu) % 3 == 0, U8) if mask else None
        Ks, ks = (b.out("Ks", (T, B, nu, nx), F64), b.out("ks", (T, B, nu), F64)) if gains else (None, None)
        need = lib.dmpc_lqr_f64_workspace_bytes(T, B, nx, nu)
        return None, ("dmpc_lqr_solve_f64", [T, B, nx, nu] + ins + [m, Ks, ks, b.out("x", (T, B, nx), F64), b.out("u", (T, B, nu), F64),
                                                                  b.ws("ws", need), need, b.info("info", B), None])
    return make


def _kkt_f64(nx, nu, strict):
    T, B = 3, 5

    def make(b, lib):
        ins, outs = kkt_inputs(b, T, B, nx, nu, 31 + nx, F64)
        need = lib.dmpc_lqr_f64_workspace_bytes(T, B, nx, nu)
        return None, ("dmpc_lqr_kkt_grad_f64", [T, B, nx, nu] + ins + [strict] + outs + [b.ws("ws", need), need, b.info("info", B), None])
    return make


for _nx, _nu in ((5, 3), (3, 1), (32, 8), (16, 4), (16, 8)):
    for _g in (False, True):
        add("f64:solve(%d,%d)%sgains" % (_nx, _nu, "+" if _g else "-"), "dmpc_lqr_solve_f64", _solve_f64(_nx, _nu, _g, False),
            kernel={(5, 3): "lqr_f64_kernel", (3, 1): "lqr_f64_row_kernel<3, 1, 16, false>"}.get((_nx, _nu), "lqr_tile16_f64_kernel<%d, %d>" % (_nx, _nu)))
    add("f64:kkt_grad(%d,%d)" % (_nx, _nu), "dmpc_lqr_kkt_grad_f64", _kkt_f64(_nx, _nu, 0))
add("f64:solve(3,1)+mask", "dmpc_lqr_solve_f64", _solve_f64(3, 1, True, True))
add("f64:solve(5,3)+mask-gains", "dmpc_lqr_solve_f64", _solve_f64(5, 3, False, True))
add("f64:kkt_grad(3,1)strict", "dmpc_lqr_kkt_grad_f64", _kkt_f64(3, 1, 1))


# ---- PNQP ----
def _pnqp(n, coupled, warm=False, B=5, n_iter=20):
    def make(b, lib):
        q = synthetic.make_box_qp(B, n, seed=3 + n)
        ins = [b.inp(k, q[k]) for k in ("H", "q", "lower", "upper")]
        x0 = b.inp("x_init", np.clip(0.1 * np.ones((B, n)), q["lower"], q["upper"])) if warm else None
        need = lib.dmpc_pnqp_workspace_bytes(B, n, n_iter, coupled)
        ws = b.ws("ws", need) if need else None
        outs = [b.out("x", (B, n)), b.out("fac", (B, n, n)), b.out("piv", (B, n), I32), b.out("index_f", (B, n)),
                b.out("n_iter_out", (B,), I32)]
        return None, ("dmpc_pnqp", [B, n] + ins + [x0, n_iter, coupled] + outs + [ws, need, b.info("info", B), None])
    return make


for _n in (1, 4, 8, 9):
    add("pnqp:n%d" % _n, "dmpc_pnqp", _pnqp(_n, 0), kernel="pnqp_kernel<%d>" % _n if _n <= 8 else "pnqp_tiled_kernel")
add("pnqp:n4+warm", "dmpc_pnqp", _pnqp(4, 0, warm=True))
for _n in (4, 9):
    add("pnqp:n%d+coupled" % _n, "dmpc_pnqp", _pnqp(_n, 1), kernel="pnqp_kernel<4>" if _n == 4 else "pnqp_coupled_kernel")


# ---- batched LU ----
def _lu_matrix(B, n):
    rng = np.random.RandomState(50 + n)
    return f32(rng.randn(B, n, n) + 0.5 * n * np.eye(n))


def _lu_factor(n, B=5):
    def make(b, lib):
        return None, ("dmpc_batch_lu_factor", [B, n, b.inp("A", _lu_matrix(B, n)), b.out("LU", (B, n, n)), b.out("piv", (B, n), I32),
                                               b.info("info", B), None])
    return make


def _lu_solve(n, k, B=5):
    def make(b, lib):
        A, LU, piv = b.inp("A", _lu_matrix(B, n)), b.produced("LU", (B, n, n)), b.produced("piv", (B, n), I32)
        rhs = b.inp("b", np.random.RandomState(60 + n + k).randn(B, n, k))
        return ([("dmpc_batch_lu_factor", [B, n, A, LU, piv, None, None])],
                ("dmpc_batch_lu_solve", [B, n, k, LU, piv, rhs, b.out("x", (B, n, k)), None]))
    return make


for _n in (3, 12):
    add("lu:factor_n%d" % _n, "dmpc_batch_lu_factor", _lu_factor(_n))
    for _k in (1, 2):
        add("lu:solve_n%d_k%d" % (_n, _k), "dmpc_batch_lu_solve", _lu_solve(_n, _k))


# ---- MPCstep: the whole step, its two halves, the helpers around them.  `kernel`: the one the call launches last, which is
# what tells the families of csrc/mpc_api.hip apart ((5,3), like every shape with at most four controls and fifteen elements of
# tau, runs padded inside a 16-lane container, not on the runtime-dimension kernels) ----
LS_DECAY, MAX_LS, N_QP = 0.2, 5, 10


def _step_outputs(b, T, B, nx, nu, gains=True, nqp=True):
    out = [b.out("x_out", (T, B, nx)), b.out("u_out", (T, B, nu))]
    if gains:
        out += [b.out("Ks", (T, B, nu, nx)), b.out("ks", (T, B, nu))]
    out += [b.out("costs", (B,)), b.out("old_costs", (B,)), b.out("alphas", (B,)), b.out("objs", (T, B)), b.out("u_first", (T, B, nu))]
    if nqp:
        out.append(b.out("n_qp_iter", (B,), I32))
    return out + [b.out("n_ls_iter", (B,), I32)]


def _step_forward(nx, nu, B, need_expand=1, coupled=0, T=3, bound=0.25):
    def make(b, lib):
        p, lo, hi, u0, x0 = mpc_problem(B, T, nx, nu, bound, 11)
        C, c, F, f = (b.inp(k, p[k]) for k in ("C", "c", "F", "f"))
        u, xs, lo_, hi_ = b.inp("controls", u0), b.inp("states", x0), b.inp("u_lower", lo), b.inp("u_upper", hi)
        need = lib.dmpc_mpc_step_workspace_bytes(T, B, nx, nu)
        return None, ("dmpc_mpc_step_forward", [T, B, nx, nu, C, c, F, f, u, xs, lo_, hi_, C, c, F, f, need_expand, LS_DECAY, MAX_LS, N_QP,
                                                coupled] + _step_outputs(b, T, B, nx, nu) + [b.ws("ws", need), need, b.info("info", B), None])
    return make


add("mpc:step_forward(8,2)B4_fused_stream", "dmpc_mpc_step_forward", _step_forward(8, 2, 4), kernel="mpc_step_fused_asm_kernel<8, 2, false, true>")
add("mpc:step_forward(8,2)B4_with_f", "dmpc_mpc_step_forward", _step_forward(8, 2, 4, need_expand=0), kernel="mpc_step_fused_asm_kernel<8, 2, true, false>")
add("mpc:step_forward(8,2)B5_two_launches", "dmpc_mpc_step_forward", _step_forward(8, 2, 5), kernel="mpc_forward_rec_kernel<8, 2, 16, false, false>")
add("mpc:step_forward(4,4)B4_dma_ring", "dmpc_mpc_step_forward", _step_forward(4, 4, 4, bound=0.375), kernel="mpc_forward_rec_kernel<4, 4, 16, true, false>")
add("mpc:step_forward(5,3)B5_container", "dmpc_mpc_step_forward", _step_forward(5, 3, 5), kernel="mpc_forward_rec_kernel<8, 4, 16, false, true>")
add("mpc:step_forward(5,3)B4_container", "dmpc_mpc_step_forward", _step_forward(5, 3, 4), kernel="mpc_forward_rec_kernel<8, 4, 16, false, true>")
add("mpc:step_forward(4,10)B4_tiled", "dmpc_mpc_step_forward", _step_forward(4, 10, 4), kernel="mpc_tiled_forward_kernel")
add("mpc:step_forward(8,2)B4_coupled", "dmpc_mpc_step_forward", _step_forward(8, 2, 4, coupled=1), kernel="mpc_forward_asm_kernel<8, 2>")
add("mpc:step_forward(4,10)B3_tiled_coupled", "dmpc_mpc_step_forward", _step_forward(4, 10, 3, coupled=1), kernel="mpc_tiled_forward_kernel")


def _backward_rec(nx, nu, B, coupled=0, T=3, bound=0.25):
    def make(b, lib):
        p, lo, hi, u0, x0 = mpc_problem(B, T, nx, nu, bound, 12)
        ins = [b.inp(k, p[k]) for k in ("C", "c", "F", "f")] + [b.inp("controls", u0), b.inp("u_lower", lo), b.inp("u_upper", hi)]
        need = lib.dmpc_mpc_backward_rec_workspace_bytes(T, B, nx, nu, N_QP, coupled)
        ws = b.ws("ws", need) if need else None
        return None, ("dmpc_mpc_backward_rec", [T, B, nx, nu] + ins + [N_QP, coupled, b.out("Ks", (T, B, nu, nx)), b.out("ks", (T, B, nu)),
                                                                       b.out("n_qp_iter", (B,), I32), ws, need, b.info("info", B), None])
    return make


add("mpc:backward_rec(8,2)B4", "dmpc_mpc_backward_rec", _backward_rec(8, 2, 4), kernel="mpc_backward_asm_kernel<8, 2, true, false>")
add("mpc:backward_rec(8,2)B5", "dmpc_mpc_backward_rec", _backward_rec(8, 2, 5), kernel="mpc_backward_rec_kernel<8, 2, 16, false>")
add("mpc:backward_rec(4,10)B4_tiled", "dmpc_mpc_backward_rec", _backward_rec(4, 10, 4), kernel="mpc_tiled_backward_kernel")
add("mpc:backward_rec(8,2)B4_coupled", "dmpc_mpc_backward_rec", _backward_rec(8, 2, 4, coupled=1), kernel="mpc_backward_rec_kernel<8, 2, 16, false>")
add("mpc:backward_rec(4,10)B3_tiled_coupled", "dmpc_mpc_backward_rec", _backward_rec(4, 10, 3, coupled=1), kernel="mpc_coupled_backward_kernel")


def _gains(T, B, nx, nu, seed):
    rng = np.random.RandomState(seed)
    return 0.1 * rng.randn(T, B, nu, nx), 0.2 * rng.randn(T, B, nu)


def _forward_rec(nx, nu, B, T=3, bound=0.25):
    def make(b, lib):
        p, lo, hi, u0, x0 = mpc_problem(B, T, nx, nu, bound, 13)
        Ks, ks = _gains(T, B, nx, nu, 14)
        ins = [b.inp("Ks", Ks), b.inp("ks", ks), b.inp("controls", u0), b.inp("states", x0), b.inp("u_lower", lo), b.inp("u_upper", hi)]
        ins += [b.inp(k, p[k]) for k in ("C", "c", "F", "f")]
        return None, ("dmpc_mpc_forward_rec", [T, B, nx, nu] + ins + [LS_DECAY, MAX_LS] + _step_outputs(b, T, B, nx, nu, False, False)
                      + [b.info("info", B), None])
    return make


add("mpc:forward_rec(8,2)B4", "dmpc_mpc_forward_rec", _forward_rec(8, 2, 4), kernel="mpc_forward_asm_kernel<8, 2>")
add("mpc:forward_rec(8,2)B5", "dmpc_mpc_forward_rec", _forward_rec(8, 2, 5), kernel="mpc_forward_rec_kernel<8, 2, 16, false, false>")
add("mpc:forward_rec(5,3)B5", "dmpc_mpc_forward_rec", _forward_rec(5, 3, 5), kernel="mpc_forward_rec_kernel<8, 4, 16, false, true>")
add("mpc:forward_rec(4,10)B4", "dmpc_mpc_forward_rec", _forward_rec(4, 10, 4), kernel="mpc_tiled_forward_kernel")


def pendulum_start(B, seed):
    rng = np.random.RandomState(seed)
    th, w = rng.uniform(-np.pi, np.pi, B), rng.uniform(-1.0, 1.0, B)
    return f32(np.stack((np.cos(th), np.sin(th), w), axis=1))


def _forward_rec_pendulum(B, T=4):
    def make(b, lib):
        p = lqr_problem(B, T, 3, 1, 15)
        Ks, ks = _gains(T, B, 3, 1, 16)
        states = np.stack([pendulum_start(B, 17 + t) for t in range(T)])
        ins = [b.inp("Ks", Ks), b.inp("ks", ks), b.inp("controls", np.zeros((T, B, 1))), b.inp("states", states),
               b.inp("u_lower", -2.0 * np.ones((T, B, 1))), b.inp("u_upper", 2.0 * np.ones((T, B, 1))), b.inp("C", p["C"]), b.inp("c", p["c"])]
        return None, ("dmpc_mpc_forward_rec_pendulum", [T, B] + ins + list(PENDULUM) + [LS_DECAY, MAX_LS]
                      + _step_outputs(b, T, B, 3, 1, False, False) + [b.info("info", B), None])
    return make


add("mpc:forward_rec_pendulum_B4", "dmpc_mpc_forward_rec_pendulum", _forward_rec_pendulum(4))
add("mpc:forward_rec_pendulum_B5", "dmpc_mpc_forward_rec_pendulum", _forward_rec_pendulum(5))


def _pendulum_rollout(B, T, with_F=True):
    def make(b, lib):
        u = np.random.RandomState(18).uniform(-2.5, 2.5, (T, B, 1))
        F, f = (b.out("F_out", (T - 1, B, 3, 4)), b.out("f_out", (T - 1, B, 3))) if with_F else (None, None)
        return None, ("dmpc_pendulum_rollout_linearize", [T, B, b.inp("x_init", pendulum_start(B, 19)), b.inp("u", u)] + list(PENDULUM)
                      + [1, b.out("x_out", (T, B, 3)), F, f, None])
    return make


add("pendulum:rollout_linearize_B5_T4", "dmpc_pendulum_rollout_linearize", _pendulum_rollout(5, 4))
add("pendulum:rollout_B5_T4", "dmpc_pendulum_rollout_linearize", _pendulum_rollout(5, 4, with_F=False))
add("pendulum:rollout_linearize_B3_T1", "dmpc_pendulum_rollout_linearize", _pendulum_rollout(3, 1))


def _lin_rollout(nx, nu, B, T, with_f=True):
    def make(b, lib):
        p = lqr_problem(B, T, nx, nu, 20, with_f=with_f)
        u = np.random.RandomState(21).randn(T, B, nu)
        F = b.inp("F", p["F"]) if T > 1 else None
        f = b.inp("f", p["f"]) if with_f and T > 1 else None
        return None, ("dmpc_lin_rollout", [T, B, nx, nu, b.inp("x_init", p["x_init"]), b.inp("u", u), F, f, b.out("x_out", (T, B, nx)), None])
    return make


add("mpc:lin_rollout(8,2)B5_T3", "dmpc_lin_rollout", _lin_rollout(8, 2, 5, 3))
add("mpc:lin_rollout(5,3)B1_T3-f", "dmpc_lin_rollout", _lin_rollout(5, 3, 1, 3, with_f=False))
add("mpc:lin_rollout(3,1)B3_T1", "dmpc_lin_rollout", _lin_rollout(3, 1, 3, 1))


def _step_status(B, full=True):
    def make(b, lib):
        rng = np.random.RandomState(22)
        info = b.inp("info", rng.randint(0, 16, B), I32) if full else None
        nqp = b.inp("n_qp_iter", rng.randint(1, 40, B), I32) if full else None
        return None, ("dmpc_mpc_step_status", [B, info, nqp, b.inp("alphas", 0.2 ** rng.randint(0, 4, B)), b.out("status", (8,), I32), None])
    return make


add("mpc:step_status_B5", "dmpc_mpc_step_status", _step_status(5))
add("mpc:step_status_B1_alphas_only", "dmpc_mpc_step_status", _step_status(1, full=False))


def step_backward_inputs(b, T, B, nx, nu, seed):
    """C_hat, c_hat, F_hat, x, u, u_lower, u_upper, grad_x, grad_u: some controls on the box (tests/test_kkt_gpu.py's problem)"""
    p = lqr_problem(B, T, nx, nu, seed, with_f=False)
    rng = np.random.RandomState(seed + 1)
    x, u = rng.randn(T, B, nx), np.clip(0.5 * rng.rand(T, B, nu) - 0.25, -0.2, 0.2)
    return [b.inp("C", p["C"]), b.inp("c", p["c"]), b.inp("F", p["F"]), b.inp("x", x), b.inp("u", u), b.inp("u_lower", np.full((T, B, nu), -0.2)),
            b.inp("u_upper", np.full((T, B, nu), 0.2)), b.inp("gx", rng.randn(T, B, nx)), b.inp("gu", rng.randn(T, B, nu))]


def _step_backward(nx, nu, B, T=3, sums=False, dense=True, detach=False):
    def make(b, lib):
        ns = nx + nu
        ins = step_backward_inputs(b, T, B, nx, nu, 910)
        outs = [b.out("dx0", (B, nx))]
        outs += [b.out("dC", (T, B, ns, ns)), b.out("dc", (T, B, ns)), b.out("dF", (T - 1, B, nx, ns)), b.out("df", (T - 1, B, nx))] if dense \
            else [None, None, None, None]
        # (sums formed with float atomics: compared between the layouts at the contract's tolerance, not bit for bit)
        outs += [b.out("dC_sum", (ns, ns), tol=TOL_PRIMAL), b.out("dc_sum", (ns,), tol=TOL_PRIMAL)] if sums else [None, None]
        det = [b.inp("detach_norm", np.array([0.0, 1.0] * B)[:B]), b.inp("detach_flag", [1], I32), 0.5] if detach else [None, None, 0.0]
        need = lib.dmpc_mpc_step_workspace_bytes(T, B, nx, nu)
        return None, ("dmpc_mpc_step_backward", [T, B, nx, nu] + ins + outs + det + [b.ws("ws", need), need, b.info("info", B), None])
    return make


add("mpc:step_backward(3,1)B5_dense", "dmpc_mpc_step_backward", _step_backward(3, 1, 5))
add("mpc:step_backward(5,3)B5_dense", "dmpc_mpc_step_backward", _step_backward(5, 3, 5))
add("mpc:step_backward(3,1)B4_dense+sums", "dmpc_mpc_step_backward", _step_backward(3, 1, 4, sums=True))
add("mpc:step_backward(3,1)B4_sums_only", "dmpc_mpc_step_backward", _step_backward(3, 1, 4, sums=True, dense=False))
add("mpc:step_backward(3,1)B5_sums_refused", "dmpc_mpc_step_backward", _step_backward(3, 1, 5, sums=True))
add("mpc:step_backward(3,1)B4_detach", "dmpc_mpc_step_backward", _step_backward(3, 1, 4, detach=True))


def _step_backward_shared(nx, nu, B, layout, T=3):
    def make(b, lib):
        ns = nx + nu
        ins = step_backward_inputs(b, T, B, nx, nu, 920)
        t = lambda bit, lead, shape: ((lead,) if layout & bit else ()) + shape    # noqa: E731
        outs = [b.out("dx0", (B, nx)), b.out("dC", t(1, T, (ns, ns))), b.out("dc", t(4, T, (ns,))), b.out("dF", t(2, T - 1, (nx, ns))),
                b.out("df", t(16, T - 1, (nx,)))]
        need = lib.dmpc_mpc_step_shared_grad_workspace_bytes(T, B, nx, nu)
        return None, ("dmpc_mpc_step_backward_shared", [T, B, nx, nu, layout] + ins + outs + [None, None, 0.0, b.ws("ws", need), need,
                                                                                            b.info("info", B), None])
    return make


add("mpc:step_backward_shared(3,1)B5_layout0", "dmpc_mpc_step_backward_shared", _step_backward_shared(3, 1, 5, 0))
add("mpc:step_backward_shared(3,1)B5_time", "dmpc_mpc_step_backward_shared", _step_backward_shared(3, 1, 5, 1 | 2 | 4 | 16))
add("mpc:step_backward_shared(17,4)B3_layout0", "dmpc_mpc_step_backward_shared", _step_backward_shared(17, 4, 3, 0))


# ---- box-DDP: the whole loop as one chain ----
def _box_ddp(dyn_kind, B, nx=3, nu=2, T=4, max_iter=2, coupled=0):
    def make(b, lib):
        if dyn_kind == 0:
            p, lo, hi, u0, _ = mpc_problem(B, T, nx, nu, 0.25, 23)
            x_init, F, f, params = p["x_init"], b.inp("F", p["F"]), b.inp("f", p["f"]), None
        else:
            p = lqr_problem(B, T, 3, 1, 24)
            lo, hi, u0 = -2.0 * np.ones((T, B, 1)), 2.0 * np.ones((T, B, 1)), np.zeros((T, B, 1))
            x_init, F, f = pendulum_start(B, 25), None, None
            params = (ctypes.c_float * 6)(*(PENDULUM + (1.0,)))          # a HOST array
        n_x, n_u = (nx, nu) if dyn_kind == 0 else (3, 1)
        ins = [b.inp("x_init", x_init), b.inp("C", p["C"]), b.inp("c", p["c"]), F, f, dyn_kind, params, b.inp("u_init", u0), b.inp("u_lower", lo),
               b.inp("u_upper", hi)]
        outs = [b.out("x_best", (T, B, n_x)), b.out("u_best", (T, B, n_u)), b.out("costs_best", (B,)), b.out("du_norm_best", (B,)),
                b.out("du_norm_last", (B,)), b.out("state", (8,), I32)]
        need = lib.dmpc_box_ddp_workspace_bytes(T, B, n_x, n_u)
        # eps, not_improved_lim, ls_decay, max_ls_iter, best_cost_eps, max_iter, n_qp_iter_max, scrambled_norm, batch_coupled
        scalars = [1e-5, 5, LS_DECAY, 10, 1e-4, max_iter, N_QP, 1, coupled]
        # (info is cleared by the call: handed over prefilled)
        return None, ("dmpc_box_ddp", [T, B, n_x, n_u] + ins + scalars + outs + [b.ws("ws", need), need, b.info("info", B, written=True), None])
    return make


add("box_ddp:lin(3,2)B5", "dmpc_box_ddp", _box_ddp(0, 5))
add("box_ddp:pendulum_B4", "dmpc_box_ddp", _box_ddp(1, 4))
add("box_ddp:pendulum_B5", "dmpc_box_ddp", _box_ddp(1, 5))
# (batch-coupled: the decision slots at ddp_layout.sync are handed over prefilled and cleared by every sweep's launch)
add("box_ddp:lin(3,2)B5_coupled", "dmpc_box_ddp", _box_ddp(0, 5, coupled=1))
add("box_ddp:pendulum_B4_coupled", "dmpc_box_ddp", _box_ddp(1, 4, coupled=1))


# ---- MlpDx ----
MLP_SMALL, MLP_LARGE = mlp_dx_cases.CASES[0], mlp_dx_cases.CASES[3]      # (3,1) H=5 B=5; (16,8) H=256 B=3


def mlp_inputs(b, case):
    nx, nu, H, B, T, s = case
    net = mlp_dx_cases.NumpyMlp(nx, nu, H, s)
    return net, [b.inp(k, getattr(net, k)) for k in ("W1", "b1", "W2", "b2")]


def _mlp_rollout(case, T=None, with_F=True):
    nx, nu, H, B, T0, s = case
    T = T or T0

    def make(b, lib):
        net, w = mlp_inputs(b, case)
        p = lqr_problem(B, T, nx, nu, s)
        u = np.random.RandomState(s + 30).uniform(-0.5, 0.5, (T, B, nu))
        if T == 1:       # include/dmpc.h: "T = 1: x_out = x_init, nothing else is written" - two arrays that must stay as they are
            Fo, fo = b.out("F_out", (1, B, nx, nx + nu), unwritten=True), b.out("f_out", (1, B, nx), unwritten=True)
        else:
            Fo, fo = (b.out("F_out", (T - 1, B, nx, nx + nu)), b.out("f_out", (T - 1, B, nx))) if with_F else (None, None)
        return None, ("dmpc_mlp_rollout_linearize", [T, B, nx, nu, H, 0, 1] + w + [b.inp("x_init", p["x_init"]), b.inp("u", u),
                                                                                 b.out("x_out", (T, B, nx)), Fo, fo, None])
    return make


def _mlp_param_grad(case, T=None, with_d=True):
    nx, nu, H, B, T0, s = case
    T = T or T0

    def make(b, lib):
        net, w = mlp_inputs(b, case)
        p = lqr_problem(B, T, nx, nu, s)
        u = b.inp("u", np.random.RandomState(s + 30).uniform(-0.5, 0.5, (T, B, nu)))
        x0, x = b.inp("x_init", p["x_init"]), b.produced("x", (T, B, nx))
        gf = b.inp("grad_f", np.random.RandomState(s + 31).randn(T - 1, B, nx)) if T > 1 else None
        outs = [b.out("dW1", (H, nx + nu)), b.out("db1", (H,)), b.out("dW2", (nx, H)), b.out("db2", (nx,))]
        outs += [b.out("d_x_init", (B, nx)), b.out("d_u", (T, B, nu))] if with_d else [None, None]
        need = lib.dmpc_mlp_param_grad_workspace_bytes(B, nx, nu, H)
        ws = b.ws("ws", need) if T > 1 else None         # (T = 1 only zeroes the outputs: no workspace)
        return ([("dmpc_mlp_rollout_linearize", [T, B, nx, nu, H, 0, 1] + w + [x0, u, x, None, None, None])],
                ("dmpc_mlp_param_grad", [T, B, nx, nu, H, 0, 1] + w + [x, u, gf] + outs + [ws, need if T > 1 else 0, None]))
    return make


def _mlp_forward_rec(case):
    nx, nu, H, B, T, s = case

    def make(b, lib):
        net, w = mlp_inputs(b, case)
        P = mlp_dx_cases.problem(case)
        u0 = np.zeros((T, B, nu))
        xs = [P["x_init"]]
        for t in range(T - 1):
            xs.append(net.step(xs[t], u0[t]))
        Ks, ks = _gains(T, B, nx, nu, s + 40)
        ins = [b.inp("Ks", Ks), b.inp("ks", ks), b.inp("controls", u0), b.inp("states", np.stack(xs)), b.inp("u_lower", P["lo"]),
               b.inp("u_upper", P["hi"]), b.inp("C", P["C"]), b.inp("c", P["c"])]
        return None, ("dmpc_mpc_forward_rec_mlp", [T, B, nx, nu, H, 0, 1] + w + ins + [LS_DECAY, 10]
                      + _step_outputs(b, T, B, nx, nu, False, False) + [b.info("info", B), None])
    return make


for _name, _case in (("(3,1)H5_B5", MLP_SMALL), ("(16,8)H256_B3", MLP_LARGE)):
    add("mlp:rollout_linearize" + _name, "dmpc_mlp_rollout_linearize", _mlp_rollout(_case))
    add("mlp:rollout_linearize" + _name + "_T1", "dmpc_mlp_rollout_linearize", _mlp_rollout(_case, T=1))
    add("mlp:param_grad" + _name, "dmpc_mlp_param_grad", _mlp_param_grad(_case))
    add("mlp:param_grad" + _name + "_T1", "dmpc_mlp_param_grad", _mlp_param_grad(_case, T=1))
    add("mlp:forward_rec" + _name, "dmpc_mpc_forward_rec_mlp", _mlp_forward_rec(_case))
add("mlp:rollout(3,1)H5_B5_states_only", "dmpc_mlp_rollout_linearize", _mlp_rollout(MLP_SMALL, with_F=False))
add("mlp:param_grad(3,1)H5_B5_weights_only", "dmpc_mlp_param_grad", _mlp_param_grad(MLP_SMALL, with_d=False))


# ---- LQR with batch-shared C and F: the solve, then its gradient on the front of the solve's workspace ----
SHARED_LAYOUTS = {"shared": (0, dict()),
                  "time+batch": (63, dict(C_time=True, F_time=True, c_kind="batch", f_kind="batch"))}


def _shared(nx, nu, name, grad, B=5, T=3):
    layout, kw = SHARED_LAYOUTS[name]

    def make(b, lib):
        p = shared_lqr_problems.make(nx, nu, T, B, seed=70 + nx, **kw)
        C, c, F, x0 = b.inp("C", p["C"]), b.inp("c", p["c"]), b.inp("F", p["F"]), b.inp("x_init", p["x_init"])
        f = None if p["f"] is None else b.inp("f", p["f"])
        need = lib.dmpc_lqr_shared_workspace_bytes(T, B, nx, nu)
        if not grad:
            return None, ("dmpc_lqr_shared_solve", [T, B, nx, nu, layout, C, c, F, f, x0, b.out("x", (T, B, nx)), b.out("u", (T, B, nu)),
                                                    b.ws("ws", need), need, b.info("info", B, written=True), None])
        x, u, sws = b.produced("x", (T, B, nx)), b.produced("u", (T, B, nu)), b.produced("ws_saved", (need,), U8)
        rng = np.random.RandomState(71)
        gx, gu = b.inp("gx", rng.randn(T, B, nx)), b.inp("gu", rng.randn(T, B, nu))
        outs = [b.out("dx0", (B, nx)), b.out("dC", p["C"].shape), b.out("dc", p["c"].shape), b.out("dF", p["F"].shape),
                None if p["f"] is None else b.out("df", p["f"].shape)]
        gneed = lib.dmpc_lqr_shared_grad_workspace_bytes(T, B, nx, nu)
        return ([("dmpc_lqr_shared_solve", [T, B, nx, nu, layout, C, c, F, f, x0, x, u, sws, need, None, None])],
                ("dmpc_lqr_shared_kkt_grad", [T, B, nx, nu, layout, C, c, F, x, u, sws, gx, gu, 0] + outs
                 + [b.ws("ws", gneed), gneed, b.info("info", B, written=True), None]))
    return make


for _nx, _nu in ((3, 1), (17, 4)):
    for _name in SHARED_LAYOUTS:
        add("shared:solve(%d,%d)%s" % (_nx, _nu, _name), "dmpc_lqr_shared_solve", _shared(_nx, _nu, _name, False))
        add("shared:kkt_grad(%d,%d)%s" % (_nx, _nu, _name), "dmpc_lqr_shared_kkt_grad", _shared(_nx, _nu, _name, True))


# ---- the imitation-learning update ----
IL_KINDS = [(0, 1), (0, 3), (0, 8), (1, 1), (1, 3), (1, 8), (2, 4), (3, 4)]       # (kind, n_sc)


def il_n_params(kind, n):
    return 2 * n + (n * (n - 1) // 2 if kind in (1, 3) else 0)


def il_params(kind, n, seed=80):
    return f32(0.7 * np.random.RandomState(seed + 10 * kind + n).randn(il_n_params(kind, n)))


def il_batch(kind, nx, nu, B=5, T=3, N=7, warm=True, u_init=True):
    ns = nx + nu
    rng = np.random.RandomState(81 + ns)
    idx = np.array([3, -1, 0, N, N - 1, 2])[:B]        # an index on either side of the split: reads zeros, writes nothing
    return dict(kind=kind, N=N, T=T, B=B, nx=nx, nu=nu, tau=f32(rng.randn(N, T, ns)), warm=f32(rng.randn(N, T, nu)) if warm else None,
                idx=idx.astype(I32), params=il_params(kind, ns), u_init=u_init)


def _il_batch_begin(kind, nx, nu, **kw):
    def make(b, lib):
        d = il_batch(kind, nx, nu, **kw)
        T, B, ns = d["T"], d["B"], nx + nu
        warm = None if d["warm"] is None else b.inp("warm", d["warm"])
        outs = [b.out("x_init", (B, nx)), b.out("us", (T, B, nu)), b.out("u_init", (T, B, nu)) if d["u_init"] else None, b.out("Q", (ns, ns)),
                b.out("p", (ns,)), b.out("C", (T, B, ns, ns)), b.out("c", (T, B, ns))]
        return None, ("dmpc_il_batch_begin", [kind, d["N"], T, B, nx, nu, b.inp("tau", d["tau"]), warm, b.inp("idx", d["idx"], I32),
                                              b.inp("params", d["params"])] + outs + [None])
    return make


# (the cost map at n_sc = 1 cannot be reached here: nx and nu are both at least 1 - that row is a refused call)
IL_BEGIN = [(0, 1, 1), (0, 2, 1), (0, 6, 2), (1, 1, 1), (1, 2, 1), (1, 6, 2), (2, 3, 1), (3, 3, 1)]     # (kind, nx, nu)
for _k, _nx, _nu in IL_BEGIN:
    add("il:batch_begin_kind%d_nsc%d" % (_k, _nx + _nu), "dmpc_il_batch_begin", _il_batch_begin(_k, _nx, _nu), il=(_k, _nx, _nu, {}))
add("il:batch_begin_kind0_nsc4-warm", "dmpc_il_batch_begin", _il_batch_begin(0, 3, 1, warm=False), il=(0, 3, 1, dict(warm=False)))
add("il:batch_begin_kind1_nsc4-u_init_B1", "dmpc_il_batch_begin", _il_batch_begin(1, 3, 1, u_init=False, B=1),
    il=(1, 3, 1, dict(u_init=False, B=1)))
add("il:batch_begin_kind0_nsc1_refused", "dmpc_il_batch_begin", _il_batch_begin(0, 1, 0))
add("il:batch_begin_kind2_nsc3_refused", "dmpc_il_batch_begin", _il_batch_begin(2, 2, 1))

IL_LOSS = [(1, 1, 1), (31, 3, 11), (41, 5, 5), (100, 5, 10)]       # (T, B, nu): T*B*nu = 1, 1023, 1025, 5000


def il_loss_data(T, B, nu, N=7):
    rng = np.random.RandomState(90 + T)
    idx = np.array([3, -1, 0, N, N - 1])[:B] if B > 1 else np.array([2])
    return dict(N=N, u=f32(rng.randn(T, B, nu)), us=f32(rng.randn(T, B, nu)), idx=idx.astype(I32), warm=f32(rng.randn(N, T, nu)))


def _il_loss(T, B, nu, full=True):
    def make(b, lib):
        d = il_loss_data(T, B, nu)
        untouched = np.ones((d["N"], T, nu), dtype=bool)
        untouched[[r for r in d["idx"] if 0 <= r < d["N"]]] = False
        gu = b.out("grad_u", (T, B, nu)) if full else None
        warm = b.inout("warm", d["warm"], unwritten=untouched) if full else None
        return None, ("dmpc_il_loss", [d["N"], T, B, nu, b.inp("u", d["u"]), b.inp("us", d["us"]), b.inp("idx", d["idx"], I32), b.out("loss", (1,)),
                                       gu, warm, None])
    return make


for _T, _B, _nu in IL_LOSS:
    add("il:loss_n%d" % (_T * _B * _nu), "dmpc_il_loss", _il_loss(_T, _B, _nu), il=(_T, _B, _nu))
add("il:loss_n1025_loss_only", "dmpc_il_loss", _il_loss(41, 5, 5, full=False))

IL_LR, IL_ALPHA, IL_EPS = 1e-2, 0.99, 1e-8


def il_step_data(kind, n):
    rng = np.random.RandomState(95 + 10 * kind + n)
    return dict(dQ=f32(rng.randn(n, n)), dp=f32(rng.randn(n)), params=il_params(kind, n), ms=f32(0.1 * rng.rand(il_n_params(kind, n))))


def _il_param_step(kind, n, enable=7):
    def make(b, lib):
        d = il_step_data(kind, n)
        group = np.array([1] * n + [2] * n + [4] * (il_n_params(kind, n) - 2 * n))
        off = (group & enable) == 0        # a disabled group's params and ms are left untouched
        return None, ("dmpc_il_param_step", [kind, n, b.inp("dQ", d["dQ"]), b.inp("dp", d["dp"]), b.inout("params", d["params"], unwritten=off),
                                             b.inout("ms", d["ms"], unwritten=off), b.out("grad", (il_n_params(kind, n),)), enable,
                                             IL_LR, IL_ALPHA, IL_EPS, None])
    return make


for _k, _n in IL_KINDS:
    add("il:param_step_kind%d_nsc%d" % (_k, _n), "dmpc_il_param_step", _il_param_step(_k, _n), il=(_k, _n))
add("il:param_step_kind1_nsc8_only_q_and_lower", "dmpc_il_param_step", _il_param_step(1, 8, enable=5))
add("il:param_step_kind0_nsc9_refused", "dmpc_il_param_step", _il_param_step(0, 9))



# ---- the float64 (and float32) reference of dmpc_il_param_step: torch on the CPU ----
def cost_net(kind, n, params):
    """the float64 net of pendulum_net.py at the parameter vector"""
    net = pendulum_net.NETS[kind](n, device="cpu", dtype=torch.float64)
    with torch.no_grad():
        net.learn_q_logit.copy_(torch.as_tensor(params[:n], dtype=torch.float64))
        net.learn_p.copy_(torch.as_tensor(params[n:2 * n], dtype=torch.float64))
        if kind in (1, 3):
            net.lower_without_diag.copy_(torch.as_tensor(params[2 * n:], dtype=torch.float64))
    return net


def param_step_reference(kind, n, d, dtype):
    """autograd through net.cost_map() and one RMSprop step in `dtype` -> (grad, params, ms) as float64 arrays"""
    net = cost_net(kind, n, d["params"]).to(dtype)
    Q, p = net.cost_map()
    loss = (torch.as_tensor(d["dQ"], dtype=dtype) * Q).sum() + (torch.as_tensor(d["dp"], dtype=dtype) * p).sum()
    groups = [net.learn_q_logit, net.learn_p] + ([net.lower_without_diag] if kind in (1, 3) else [])
    g = torch.cat([t.reshape(-1) for t in torch.autograd.grad(loss, groups)])
    lr, alpha, eps = (torch.tensor(v, dtype=dtype) for v in (IL_LR, IL_ALPHA, IL_EPS))
    ms = alpha * torch.as_tensor(d["ms"], dtype=dtype) + (1 - alpha) * g * g
    prm = torch.as_tensor(d["params"], dtype=dtype) - lr * g / (torch.sqrt(ms) + eps)
    return tuple(t.detach().to(torch.float64).numpy() for t in (g, prm, ms))


def distance(got, ref):
    """max |delta| / max(1, |ref|) over (grad, params, ms)"""
    return max(float((np.abs(np.asarray(g, np.float64) - r) / np.maximum(1.0, np.abs(r))).max()) for g, r in zip(got, ref))


assert len(set(c.id for c in CASES)) == len(CASES)
BY_ID = {c.id: c for c in CASES}
