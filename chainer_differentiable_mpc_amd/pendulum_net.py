"""The four learnable pendulum costs of env_dx/pendulum_net.py as `torch.nn.Module`s, with the reference's class names
(its spelling `..._obervation` included).  Each has `cost_map() -> (Q [n_sc, n_sc], p [n_sc])` and the reference's
`forward(xinit, env, warm)`, which solves the MPC problem under that cost (`IL_Env.mpc` / `IL_Env.mpc_Q`).

    Pendulum_Net_cost_logit                             Q = diag(q),         p = sqrt(q) * learn_p       (:12-39)
    Pendulum_Net_cost_lower_triangle                    Q = L L^T,           p = learn_p                 (:41-89)
    Pendulum_Net_cost_logit_strange_obervation          Q = O^T diag(q) O,   p = (sqrt(q) * learn_p) O   (:92-140)
    Pendulum_Net_cost_lower_triangle_strange_obervation Q = O^T L L^T O,     p = learn_p O               (:143-186)

q = sigmoid(learn_q_logit); L is lower triangular with q on its diagonal and `lower_without_diag` below it in
`np.tril_indices(n_sc, -1)` order; O = OBSERVATION_MATRIX.  `isrand=True` draws learn_q_logit and learn_p from
`np.random.rand` (after `np.random.seed(0)` for the two observation nets, without a seed for the lower-triangle net, as
in the reference).  The reference's driver passes the answer string of an `input()` prompt to `isrand`, so any answer
randomises; here it is a bool.  `kind` is the net's code in the C-ABI's `dmpc_il_*` entry points."""
import numpy as np
import torch

from .il_env import Pendulum_Net_cost_logit  # noqa: F401  (re-exported: the fourth net of the module)

OBSERVATION_MATRIX = np.array([[0., 4., 1., 0.], [1., 0., 4., 0.], [0., 4., 0., 0.], [0., 0., 0., 1.]])


def _param(a, device, dtype):
    return torch.nn.Parameter(torch.as_tensor(np.asarray(a), dtype=dtype, device=device))


def _init(n_sc, isrand, seed):
    if isrand:
        if seed:
            np.random.seed(0)
        return np.random.rand(n_sc), np.random.rand(n_sc)
    return np.zeros(n_sc), np.zeros(n_sc)


def _gram(L):
    """L L^T as the sum over k of the outer products of L's columns, added left to right (the order of the kernels'
    cost map, dmpc_il_batch_begin: both routes of IL_Exp then solve with the same Q bit for bit)"""
    M = L[:, 0:1] * L[:, 0:1].T
    for k in range(1, L.shape[1]):
        M = M + L[:, k:k + 1] * L[:, k:k + 1].T
    return M


def lower_factor(q_logit, lower_without_diag):
    """L [n,n]: sigmoid(q_logit) on the diagonal, lower_without_diag scattered into np.tril_indices(n, -1)"""
    n = q_logit.shape[0]
    rows, cols = np.tril_indices(n, -1)
    L = torch.diag(torch.sigmoid(q_logit))
    return L.index_put((torch.as_tensor(rows, device=L.device), torch.as_tensor(cols, device=L.device)), lower_without_diag)


def _observe(M, p):
    """(O^T M O, p O), summed over k left to right as the kernels do"""
    O = torch.as_tensor(OBSERVATION_MATRIX, dtype=M.dtype, device=M.device)
    n = O.shape[0]
    MO = M[:, 0:1] * O[0:1, :]
    po = p[0] * O[0, :]
    for k in range(1, n):
        MO = MO + M[:, k:k + 1] * O[k:k + 1, :]
        po = po + p[k] * O[k, :]
    Q = O[0:1, :].T * MO[0:1, :]
    for k in range(1, n):
        Q = Q + O[k:k + 1, :].T * MO[k:k + 1, :]
    return Q, po


class _CostNet(torch.nn.Module):
    def forward(self, xinit, env, train_warm_start_idxs=None):
        Q, p = self.cost_map()
        u_init = None
        if train_warm_start_idxs is not None:     # [B,T,nu] warm-start controls -> time-major
            u_init = torch.as_tensor(train_warm_start_idxs).transpose(0, 1)
        return env.mpc_Q(env.true_dx, xinit, Q, p, u_init=u_init)


class Pendulum_Net_cost_lower_triangle(_CostNet):
    """Q = L L^T, p = learn_p  (pendulum_net.py:41-89)"""
    kind = 1

    def __init__(self, n_sc, isrand=False, device="cuda", dtype=torch.float32):
        super().__init__()
        self.n_sc = n_sc
        q0, p0 = _init(n_sc, isrand, seed=False)
        self.learn_q_logit = _param(q0, device, dtype)
        self.learn_p = _param(p0, device, dtype)
        self.lower_without_diag = _param(np.zeros(n_sc * (n_sc - 1) // 2), device, dtype)

    def cost_map(self):
        L = lower_factor(self.learn_q_logit, self.lower_without_diag)
        return _gram(L), self.learn_p


class Pendulum_Net_cost_logit_strange_obervation(_CostNet):
    """Q = O^T diag(q) O, p = (sqrt(q) * learn_p) O  (pendulum_net.py:92-140)"""
    kind = 2

    def __init__(self, n_sc, isrand=False, device="cuda", dtype=torch.float32):
        super().__init__()
        assert n_sc == OBSERVATION_MATRIX.shape[0]
        self.n_sc = n_sc
        q0, p0 = _init(n_sc, isrand, seed=True)
        self.learn_q_logit = _param(q0, device, dtype)
        self.learn_p = _param(p0, device, dtype)

    def cost_map(self):
        q = torch.sigmoid(self.learn_q_logit)
        return _observe(torch.diag(q), torch.sqrt(q) * self.learn_p)


class Pendulum_Net_cost_lower_triangle_strange_obervation(_CostNet):
    """Q = O^T L L^T O, p = learn_p O  (pendulum_net.py:143-186)"""
    kind = 3

    def __init__(self, n_sc, isrand=False, device="cuda", dtype=torch.float32):
        super().__init__()
        assert n_sc == OBSERVATION_MATRIX.shape[0]
        self.n_sc = n_sc
        q0, p0 = _init(n_sc, isrand, seed=True)
        self.learn_q_logit = _param(q0, device, dtype)
        self.learn_p = _param(p0, device, dtype)
        self.lower_without_diag = _param(np.zeros(n_sc * (n_sc - 1) // 2), device, dtype)

    def cost_map(self):
        L = lower_factor(self.learn_q_logit, self.lower_without_diag)
        return _observe(_gram(L), self.learn_p)


NETS = (Pendulum_Net_cost_logit, Pendulum_Net_cost_lower_triangle, Pendulum_Net_cost_logit_strange_obervation,
        Pendulum_Net_cost_lower_triangle_strange_obervation)


def make_net(n_sc, is_lower_triangle=False, is_strange_observation=False, rand_init=False, device="cuda",
             dtype=torch.float32):
    """the net il_exp.py:61-73 picks from its two switches (the logit net has no random initialisation there)"""
    if is_lower_triangle and not is_strange_observation:
        return Pendulum_Net_cost_lower_triangle(n_sc, isrand=rand_init, device=device, dtype=dtype)
    if not is_strange_observation:
        return Pendulum_Net_cost_logit(n_sc, device=device, dtype=dtype)
    if not is_lower_triangle:
        return Pendulum_Net_cost_logit_strange_obervation(n_sc, isrand=rand_init, device=device, dtype=dtype)
    return Pendulum_Net_cost_lower_triangle_strange_obervation(n_sc, isrand=rand_init, device=device, dtype=dtype)
