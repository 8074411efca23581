"""The cases of the tests of BoxDDP's device chain with an MlpDx (dmpc_box_ddp, dyn_kind 2), keyed (activation, case): the
tanh problems of tests/mlp_dx_cases.py and one relu problem of tests/mlp_act_cases.py, with the float64 oracle's loop
stopped after one iteration."""
import functools

import numpy as np

from oracle import box_ddp as obox
from oracle import mpc as ompc
from tests import mlp_act_cases, mlp_dx_cases
from tests.mlp_act_cases import KINK_MARGIN      # noqa: F401
from tests.mlp_dx_cases import BOUND, CASES, LS_DECAY, MAX_LS_ITER

# relu: the (3,1) case at the seed tests/mlp_act_cases.py scanned for (LOOP_GRAD_RESEEDED) - all ten iterations of the float64
# loop run and the pair it ends at stays 6.5e-4 away from every kink, where CASES' own seed ends 4.0e-8 from one
RELU = ("relu", mlp_act_cases.loop_grad_case("relu", CASES[0]))
ONE_ITERATION = [("tanh", c) for c in CASES] + [RELU]
LOOP = [("tanh", c) for c in CASES[:2]] + [RELU]


def name(key):
    return "%s-%s" % (key[0], "_".join(str(v) for v in key[1]))


def problem(key):
    activation, case = key
    return mlp_dx_cases.problem(case) if activation == "tanh" else mlp_act_cases.problem(activation, case)


def module(key, device="cuda", **kw):
    """the MlpDx of the case with the oracle's weights; kw: device_loop, device_grad"""
    m = problem(key)["net"].module(device)
    for k, v in kw.items():
        assert k in ("device_loop", "device_grad")
        setattr(m, k, bool(v))
    return m


@functools.lru_cache(maxsize=None)
def oracle_one_iteration(key):
    """the reference's loop from u = 0 stopped after one iteration; old_costs: the cost of the nominal trajectory"""
    nx, nu, H, B, T, s = key[1]
    P = problem(key)
    net = P["net"]
    if key[0] != "tanh":
        net.reset_margin()
    x, u, costs, *_ = obox.box_ddp(P["x_init"], P["cost"], net.step, T, -BOUND, BOUND, nx, nu, eps=1e-3, max_iter=1,
                                   linearize=net.linearize, batch_coupled=False, line_search_decay=LS_DECAY,
                                   max_line_search_iter=MAX_LS_ITER)
    u0 = np.zeros((T, B, nu))
    old = ompc.get_cost(T, u0, P["cost"], obox.get_traj(T, u0, P["x_init"], net.step))
    return dict(x=x, u=u, costs=costs, old_costs=old, min_abs_z=getattr(net, "min_abs_z", np.inf))


def oracle_loop(key):
    return mlp_dx_cases.oracle_loop(key[1]) if key[0] == "tanh" else mlp_act_cases.oracle_loop(*key)
