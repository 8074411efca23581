"""Problems and the float64 reference of the closed-loop episode tests (tests/test_episode_cpu.py, tests/test_episode_gpu.py):
the cases (model -> plant), a numpy restatement of one episode over `oracle.box_ddp` - solve, apply the first control to the
plant, shift the plan - and the linear plant of the oracle case: spectral radius 0.8, so that a difference between two
episodes' states is damped from step to step rather than compounded."""
import functools

import numpy as np

from chainer_differentiable_mpc_amd import synthetic
from oracle import box_ddp as obox
from oracle import mpc as ompc
from tests import mlp2_cases, mlp_dx_cases

N_STEPS, MAX_ITER, EPS = 4, 5, 1e-3
LS_DECAY, MAX_LS_ITER = 0.2, 10
PENDULUM = (10.0, 1.0, 1.0, 0.05, 2.0)       # g, m, l, dt, max_torque (env_dx/pendulum.py's defaults)

# LinDx (4,2) -> linear: B = 5, T = 6.  The seed is chosen so that the oracle's own episode applies at least one control on a
# bound and at least one strictly inside (tests/test_episode_cpu.py asserts it); with seed 2 every solve of that episode also
# converges before MAX_ITER (3, 4, 4, 3 iterations) and no applied control is nearer to a bound than 0.02 without being on it.
LIN = dict(nx=4, nu=2, B=5, T=6, seed=2, bound=0.3, rho=0.8)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def shift_plan(u):
    """u[t] <- u[t+1] for t < T-1, the last control held"""
    return np.concatenate((u[1:], u[-1:]), axis=0)


@functools.lru_cache(maxsize=None)
def lin_problem():
    """the controller's model is the synthetic problem's time-varying LinDx; the plant is time-invariant: the model's first
    block with its state matrix scaled to spectral radius LIN['rho'], in float32-representable numbers"""
    k = LIN
    nx, nu, B, T = k["nx"], k["nu"], k["B"], k["T"]
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=k["seed"])
    A, Bm = p["F"][0][:, :, :nx], p["F"][0][:, :, nx:]
    rho = np.array([np.abs(np.linalg.eigvals(A[b])).max() for b in range(B)])
    plant_F = f32(np.concatenate((A * (k["rho"] / rho)[:, None, None], Bm), axis=2))
    plant_f = f32(p["f"][0])
    lo, hi = np.full((T, B, nu), -k["bound"]), np.full((T, B, nu), k["bound"])
    return dict(C=p["C"], c=p["c"], F=p["F"], f=p["f"], x_init=p["x_init"], plant_F=plant_F, plant_f=plant_f, lo=lo, hi=hi)


def lin_plant_step(P, x, u):
    return np.einsum("bij,bj->bi", P["plant_F"], np.concatenate((x, u), axis=1)) + P["plant_f"]


def stage_cost(C0, c0, x, u):
    """1/2 tau^T C0 tau + c0^T tau per trajectory, tau = [x;u], in float64"""
    tau = np.concatenate((np.asarray(x, np.float64), np.asarray(u, np.float64)), axis=1)
    return 0.5 * np.einsum("bi,bij,bj->b", tau, np.asarray(C0, np.float64), tau) + (np.asarray(c0, np.float64) * tau).sum(axis=1)


def oracle_lin_episode(bounds=None):
    """-> dict(x [n+1,B,nx], u [n,B,nu], n_iter [n], warm [n,T,B,nu]) of the float64 episode; `bounds` = (lower, upper) [T,B,nu]
    in place of the problem's own (`warm`: the plan every solve started from, zeros at the first)"""
    return _lin_episode(None) if bounds is None else _run_lin_episode(dict(lin_problem(), lo=bounds[0], hi=bounds[1]))


@functools.lru_cache(maxsize=None)
def _lin_episode(_):
    return _run_lin_episode(lin_problem())


def _run_lin_episode(P):
    k = LIN
    nx, nu, T = k["nx"], k["nu"], k["T"]
    cost, dyn = ompc.QuadCost(P["C"], P["c"]), ompc.LinDx(P["F"], P["f"])
    x, warm = P["x_init"], None
    xs, us, iters, warms = [x], [], [], []
    for _ in range(N_STEPS):
        warms.append(np.zeros_like(P["lo"]) if warm is None else warm)
        _, u_plan, _, _, n_iter, *_ = obox.box_ddp(x, cost, dyn, T, P["lo"], P["hi"], nx, nu, u_init=warm, eps=EPS, max_iter=MAX_ITER,
                                                   batch_coupled=False, line_search_decay=LS_DECAY, max_line_search_iter=MAX_LS_ITER)
        x = lin_plant_step(P, x, u_plan[0])
        xs.append(x), us.append(u_plan[0]), iters.append(n_iter)
        warm = shift_plan(u_plan)
    return dict(x=np.stack(xs), u=np.stack(us), n_iter=np.array(iters), warm=np.stack(warms))


def mlp_packed(net):
    """the weights of a tests/mlp_dx_cases.NumpyMlp or tests/mlp2_cases.NumpyMlp2 as `MlpDx.packed_weights` lays them out"""
    names = ("W1", "b1", "W2", "W3", "b2", "b3") if hasattr(net, "W3") else ("W1", "b1", "W2", "b2")
    return np.concatenate([getattr(net, n).reshape(-1) for n in names])


# the network cases: (model case of tests/mlp_dx_cases, plant) - plant "pendulum", "same", or a two-layer case of tests/mlp2_cases
MLP_SMALL = mlp_dx_cases.CASES[0]        # (3,1) H = 5, B = 5, T = 7: ragged workgroup
MLP_WIDE = mlp_dx_cases.CASES[1]         # (8,2) H = 64, B = 6, T = 8
MLP_LIMIT = mlp_dx_cases.CASES[3]        # (16,8) H = 256, B = 3, T = 5: every limit
MLP_ONE = mlp_dx_cases.CASES[4]          # (3,1) H = 5, B = 1, T = 2
MLP2_PLANT = (8, 2, 100, 70, 6, 8, 7)    # a two-layer (8,2) plant with other weights: more than one unit per lane


def mlp2_plant_net(activation="tanh"):
    nx, nu, H1, H2, B, T, s = MLP2_PLANT
    return mlp2_cases.NumpyMlp2(nx, nu, H1, H2, s, activation)
