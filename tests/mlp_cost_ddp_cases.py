"""The cases of the `BoxDDP` chain with an `MlpCost` (`dmpc_box_ddp_mlp_cost`): the problems of tests/mlp_cost_cases.py, the float64
loop of `oracle_box_ddp` once per case, and the same loop restated with its best-so-far decisions recorded, so that the CPU test
can assert what the GPU tests rest on: no decision of the selection `costs <= best + best_cost_eps` lies within a float32
solve's error of the threshold."""
import functools

import numpy as np

from oracle import box_ddp as obox
from oracle import mpc as ompc
from tests import mlp_cost_cases as cases
from tests.mlp_cost_cases import LS_DECAY, MAX_LS_ITER

EPS = 1e-3
BEST_COST_EPS = 1e-4
NOT_IMPROVED_LIM = 5
MAX_ITER = 10
CHAIN_END = "box_ddp_summary_kernel"
SEARCH_KERNEL = "mpc_forward_rec_mlp_cost_kernel"

SOFT_BOX = ("softplus", "soft_box")
# (act, name): the loop cases of the GPU tests, and the two more (A-tanh, D-softplus) that only the C-ABI tests run to a stop
LOOP = (("softplus", "A"), ("softplus", "B"), ("silu", "B"), ("softplus", "C"), SOFT_BOX)
LOOP_CONDITIONS = LOOP + (("tanh", "A"), ("softplus", "D"))
ONE_ITERATION = tuple((act, "A") for act in cases.ACTS) + (("softplus", "B"), ("softplus", "C"), ("softplus", "D"))
SAME_BITS = tuple((act, "A") for act in cases.ACTS) + (("softplus", "B"), ("softplus", "C"))


def name(key):
    return "%s-%s" % (key[1], key[0])


def problem(key):
    act, which = key
    return cases.soft_box_problem() if which == "soft_box" else cases.problem(act, which)


@functools.lru_cache(maxsize=None)
def oracle_loop(key):
    """(x, u, costs, n_iter) of `oracle_box_ddp` at the tests' settings"""
    P = problem(key)
    nx, nu, H, B, T = P["dims"]
    return cases.oracle_box_ddp(P["cost"], P["dyn"], P["x_init"], P["lo"], P["hi"], T, nx, nu, MAX_ITER, eps=EPS,
                                not_improved_lim=NOT_IMPROVED_LIM, best_cost_eps=BEST_COST_EPS)


@functools.lru_cache(maxsize=None)
def oracle_decisions(key):
    """`oracle_box_ddp`'s loop once more with what it decides on: -> dict(n_iter, costs (best), margins: every
    `costs - (best + best_cost_eps)` of iterations >= 1, min_eig of every Taylor Hessian, first_ties: tie rows of iterate 0)"""
    from tests.helpers import tie_rows
    P = problem(key)
    nx, nu, H, B, T = P["dims"]
    cost, dyn = P["cost"], P["dyn"]
    u = np.zeros((T, B, nu))
    best, n_not_improved, n_iter = None, 0, 0
    margins, min_eig, first_ties = [], np.inf, None
    for i in range(MAX_ITER):
        x = obox.get_traj(T, u, P["x_init"], dyn)
        C, c, _ = cases.taylor_along(cost, x, u)
        min_eig = min(min_eig, float(np.linalg.eigvalsh(C).min()))
        old = ompc.get_cost(T, u, cost, x)
        x, u, _, for_out, _, _ = ompc.mpc_forward(C, c, dyn.F, dyn.f, u, x, P["lo"], P["hi"], cost, dyn, LS_DECAY, MAX_LS_ITER, T, nx, nu,
                                                  need_expand=True, batch_coupled=False)
        if i == 0:
            first_ties = tie_rows(old, for_out.costs)
        n_not_improved += 1
        if best is None:
            best = for_out.costs.copy()
        else:
            for j in range(B):
                margins.append(float(for_out.costs[j] - (best[j] + BEST_COST_EPS)))
                if for_out.costs[j] <= best[j] + BEST_COST_EPS:
                    n_not_improved = 0
                    best[j] = for_out.costs[j]
        n_iter = i + 1
        if max(for_out.full_du_norm) < EPS or n_not_improved > NOT_IMPROVED_LIM:
            break
    return dict(n_iter=n_iter, costs=best, margins=np.array(margins), min_eig=min_eig, first_ties=first_ties)
