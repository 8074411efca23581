"""Problems and the float64 reference of the MlpDx tests (CPU and GPU): the cost and x_init of the synthetic LQR generator,
network weights from a fixed stream, and a numpy restatement of the network with its analytic Jacobian that the oracle's
get_traj / mpc_forward / box_ddp take as callables."""
import functools

import numpy as np
import torch

from chainer_differentiable_mpc_amd import MlpDx, synthetic
from oracle import box_ddp as obox
from oracle import mpc as ompc

# (nx, nu, H, B, T, seed)
CASES = [
    (3, 1, 5, 5, 7, 1),        # H < 64 and odd; ragged workgroup
    (8, 2, 64, 6, 8, 2),       # one unit per lane
    (4, 2, 100, 5, 6, 3),      # more than one unit per lane; ragged last group
    (16, 8, 256, 3, 5, 4),     # every limit
    (3, 1, 5, 1, 2, 5),        # B = 1; a single dynamics step
]
BOUND, LS_DECAY, MAX_LS_ITER = 0.5, 0.2, 10


class NumpyMlp:
    """next = W2 tanh(W1 [x;u] + b1) + b2 + x in float64, and its analytic linearisation along the re-rolled trajectory"""

    def __init__(self, nx, nu, H, seed):
        ns = nx + nu
        rng = np.random.RandomState(seed + 10)
        f32 = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
        self.W1 = f32(0.5 * rng.randn(H, ns) / np.sqrt(ns))
        self.b1 = f32(0.1 * rng.randn(H))
        self.W2 = f32(0.5 * rng.randn(nx, H) / np.sqrt(H))
        self.b2 = f32(0.1 * rng.randn(nx))
        self.nx, self.nu, self.H = nx, nu, H

    def hidden(self, x, u):
        return np.tanh(np.concatenate((x, u), axis=1) @ self.W1.T + self.b1)

    def step(self, x, u):
        return self.hidden(x, u) @ self.W2.T + self.b2 + x

    def jacobian(self, x, u):
        a = self.hidden(x, u)
        F = np.einsum("ih,bh,hj->bij", self.W2, 1.0 - a * a, self.W1)
        F[:, :, :self.nx] += np.eye(self.nx)
        return F

    def linearize(self, x, u):
        T = x.shape[0]
        xs, Fs, fs = [x[0]], [], []
        for t in range(T - 1):
            Ft = self.jacobian(xs[t], u[t])
            nxt = self.step(xs[t], u[t])
            Fs.append(Ft)
            fs.append(nxt - np.einsum("bij,bj->bi", Ft, np.concatenate((xs[t], u[t]), axis=1)))
            xs.append(nxt)
        return np.stack(Fs), np.stack(fs)

    def module(self, device="cpu", dtype=torch.float32):
        m = MlpDx(self.nx, self.nu, self.H, residual=True)
        with torch.no_grad():
            for name in ("W1", "b1", "W2", "b2"):
                getattr(m, name).copy_(torch.as_tensor(getattr(self, name)))
        return m.to(device=device, dtype=dtype)


@functools.lru_cache(maxsize=None)
def problem(case):
    nx, nu, H, B, T, s = case
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=s)
    net = NumpyMlp(nx, nu, H, s)
    lo, hi = np.full((T, B, nu), -BOUND), np.full((T, B, nu), BOUND)
    return dict(C=p["C"], c=p["c"], x_init=p["x_init"], net=net, lo=lo, hi=hi, cost=ompc.QuadCost(p["C"], p["c"]))


def oracle_step(case, u_nom):
    """one MPC step of the float64 reference from the nominal controls u_nom -> dict"""
    nx, nu, H, B, T, s = case
    P = problem(case)
    net = P["net"]
    x_nom = obox.get_traj(T, u_nom, P["x_init"], net.step)
    Fm, fm = net.linearize(x_nom, u_nom)
    x, u, _, fo, Ks, ks = ompc.mpc_forward(P["C"], P["c"], Fm, fm, u_nom, x_nom, P["lo"], P["hi"], P["cost"], net.step,
                                           LS_DECAY, MAX_LS_ITER, T, nx, nu, need_expand=True, batch_coupled=False)
    alphas, n_ls = np.zeros(B), np.zeros(B, dtype=np.int64)
    for b in range(B):       # the reference's loop on a batch of one: this trajectory's own step size and pass count
        sl = slice(b, b + 1)
        _, _, _, al, n_it = ompc.mpc_forward_rec(Ks[:, sl], ks[:, sl], u_nom[:, sl], x_nom[:, sl], P["lo"][:, sl], P["hi"][:, sl],
                                                 ompc.QuadCost(P["C"][:, sl], P["c"][:, sl]), net.step, LS_DECAY, MAX_LS_ITER, T)
        alphas[b], n_ls[b] = al[0], n_it
    old = ompc.get_cost(T, u_nom, P["cost"], x_nom)
    return dict(x_nom=x_nom, u_nom=u_nom, F=Fm, f=fm, x=x, u=u, costs=fo.costs, old_costs=old, alphas=alphas, n_ls=n_ls,
                Ks=Ks, ks=ks)


@functools.lru_cache(maxsize=None)
def oracle_two_steps(case):
    """step 1 from u = 0; step 2 from the float32-rounded result of step 1 (so that both sides start from equal values)"""
    nx, nu, H, B, T, s = case
    first = oracle_step(case, np.zeros((T, B, nu)))
    second = oracle_step(case, first["u"].astype(np.float32).astype(np.float64))
    return first, second


@functools.lru_cache(maxsize=None)
def oracle_loop(case):
    nx, nu, H, B, T, s = case
    P = problem(case)
    x, u, costs, status, n_iter, *_ = obox.box_ddp(P["x_init"], P["cost"], P["net"].step, T, -BOUND, BOUND, nx, nu, eps=1e-3,
                                                   max_iter=10, linearize=P["net"].linearize, batch_coupled=False,
                                                   line_search_decay=LS_DECAY, max_line_search_iter=MAX_LS_ITER)
    return dict(x=x, u=u, costs=costs, status=status, n_iter=n_iter)


OVERSHOOT = 4.0      # feed-forward gains scaled, bounds widened to +-4: the first candidate overshoots on most trajectories


@functools.lru_cache(maxsize=None)
def oracle_overshoot(case):
    """`forward_rec` alone from the gains of step 1 with ks scaled by OVERSHOOT inside bounds 8 times as wide, one trajectory
    at a time: a search of one or two passes (both occur within a batch), every candidate's margin above 5e-3 (measured in
    float64), so no row is a tie"""
    nx, nu, H, B, T, s = case
    P = problem(case)
    first, _ = oracle_two_steps(case)
    Ks, ks, lo, hi = first["Ks"], OVERSHOOT * first["ks"], 8.0 * P["lo"], 8.0 * P["hi"]
    xs, us, costs, alphas, n_ls = [], [], [], [], []
    for b in range(B):
        sl = slice(b, b + 1)
        x, u, fo, al, n_it = ompc.mpc_forward_rec(Ks[:, sl], ks[:, sl], first["u_nom"][:, sl], first["x_nom"][:, sl], lo[:, sl],
                                                  hi[:, sl], ompc.QuadCost(P["C"][:, sl], P["c"][:, sl]), P["net"].step,
                                                  LS_DECAY, MAX_LS_ITER, T)
        xs.append(x), us.append(u), costs.append(fo.costs[0]), alphas.append(al[0]), n_ls.append(n_it)
    return dict(Ks=Ks, ks=ks, lo=lo, hi=hi, x=np.concatenate(xs, 1), u=np.concatenate(us, 1), costs=np.array(costs),
                alphas=np.array(alphas), n_ls=np.array(n_ls), old_costs=first["old_costs"])
