"""GPU: the C ABI's memory contract (tests/test_abi_memory_gpu.py) for the MlpDx entry points with a TWO-layer `n_hidden` code -
`dmpc_mlp_rollout_linearize`, `dmpc_mpc_forward_rec_mlp` and `dmpc_box_ddp` with dyn_kind 2 - inside a guarded arena, in both
layouts, the chain with a workspace of exactly the queried size.  The packed `W2` = [W2 | W3] and `b2` = [b2 | b3] are inputs
like every other: read-only.  Cases A (odd widths below 64) and D (every limit: the largest LDS image).  The rows live here,
not in tests/abi_calls.CASES."""
import ctypes

import numpy as np
import pytest

from tests import abi_calls, mlp2_cases
from tests.abi_calls import I32, LS_DECAY, N_QP, _gains, _step_outputs
from tests.test_abi_memory_gpu import both

pytestmark = pytest.mark.gpu

SMALL, LARGE = mlp2_cases.CASE["A"], mlp2_cases.CASE["D"]
SILU = 3


def code(case):
    return case[2] | (case[3] << 16)         # DMPC_MLP_HIDDEN2(H1, H2)


def net_of(case):
    return mlp2_cases.problem("silu", case)["net"]


def weights(b, case):
    """W1, b1, [W2 | W3], [b2 | b3] as the entry points take them"""
    net = net_of(case)
    return [b.inp("W1", net.W1), b.inp("b1", net.b1),
            b.inp("W2|W3", np.concatenate((net.W2.reshape(-1), net.W3.reshape(-1)))), b.inp("b2|b3", np.concatenate((net.b2, net.b3)))]


def _rollout(case, T=None, with_F=True):
    nx, nu, H1, H2, B, T0, s = case
    T = T or T0

    def make(b, lib):
        P = mlp2_cases.problem("silu", case)
        u = np.random.RandomState(s + 30).uniform(-0.5, 0.5, (T, B, nu))
        if T == 1:       # "T = 1: x_out = x_init, nothing else is written"
            Fo, fo = b.out("F_out", (1, B, nx, nx + nu), unwritten=True), b.out("f_out", (1, B, nx), unwritten=True)
        else:
            Fo, fo = (b.out("F_out", (T - 1, B, nx, nx + nu)), b.out("f_out", (T - 1, B, nx))) if with_F else (None, None)
        return None, ("dmpc_mlp_rollout_linearize", [T, B, nx, nu, code(case), SILU, 1] + weights(b, case)
                      + [b.inp("x_init", P["x_init"]), b.inp("u", u), b.out("x_out", (T, B, nx)), Fo, fo, None])
    return make


def _forward_rec(case):
    nx, nu, H1, H2, B, T, s = case

    def make(b, lib):
        P, net = mlp2_cases.problem("silu", case), net_of(case)
        u0 = np.zeros((T, B, nu))
        xs = [P["x_init"]]
        for t in range(T - 1):
            xs.append(net.step(xs[t], u0[t]))
        Ks, ks = _gains(T, B, nx, nu, s + 40)
        ins = [b.inp("Ks", Ks), b.inp("ks", ks), b.inp("controls", u0), b.inp("states", np.stack(xs)), b.inp("u_lower", P["lo"]),
               b.inp("u_upper", P["hi"]), b.inp("C", P["C"]), b.inp("c", P["c"])]
        return None, ("dmpc_mpc_forward_rec_mlp", [T, B, nx, nu, code(case), SILU, 1] + weights(b, case) + ins + [LS_DECAY, 10]
                      + _step_outputs(b, T, B, nx, nu, False, False) + [b.info("info", B), None])
    return make


def _box_ddp(case, search_linearizes, max_iter=2):
    nx, nu, H1, H2, B, T, s = case

    def make(b, lib):
        P, net = mlp2_cases.problem("silu", case), net_of(case)
        packed = np.concatenate([getattr(net, k).reshape(-1) for k in ("W1", "b1", "W2", "W3", "b2", "b3")])
        params = (ctypes.c_float * 4)(float(code(case)), float(SILU), 1.0, float(search_linearizes))      # a HOST array
        ins = [b.inp("x_init", P["x_init"]), b.inp("C", P["C"]), b.inp("c", P["c"]), b.inp("weights", packed), None, 2, params,
               b.inp("u_init", np.zeros((T, B, nu))), b.inp("u_lower", P["lo"]), b.inp("u_upper", P["hi"])]
        outs = [b.out("x_best", (T, B, nx)), b.out("u_best", (T, B, nu)), b.out("costs_best", (B,)), b.out("du_norm_best", (B,)),
                b.out("du_norm_last", (B,)), b.out("state", (8,), I32)]
        need = lib.dmpc_box_ddp_workspace_bytes(T, B, nx, nu)
        # eps, not_improved_lim, ls_decay, max_ls_iter, best_cost_eps, max_iter, n_qp_iter_max, scrambled_norm, batch_coupled
        scalars = [1e-5, 5, LS_DECAY, 10, 1e-4, max_iter, N_QP, 1, 0]
        return None, ("dmpc_box_ddp", [T, B, nx, nu] + ins + scalars + outs + [b.ws("ws", need), need, b.info("info", B, written=True), None])
    return make


ROWS = []
for _name, _case in (("A(3,1)H5x7_B5", SMALL), ("D(16,8)H128x128_B3", LARGE)):
    ROWS.append(abi_calls.Case("mlp2:rollout_linearize" + _name, "dmpc_mlp_rollout_linearize", _rollout(_case)))
    ROWS.append(abi_calls.Case("mlp2:forward_rec" + _name, "dmpc_mpc_forward_rec_mlp", _forward_rec(_case)))
    for _sl in (0, 1):
        ROWS.append(abi_calls.Case("mlp2:box_ddp%s_search_linearizes%d" % (_name, _sl), "dmpc_box_ddp", _box_ddp(_case, _sl)))
ROWS.append(abi_calls.Case("mlp2:rolloutA_T1", "dmpc_mlp_rollout_linearize", _rollout(SMALL, T=1)))
ROWS.append(abi_calls.Case("mlp2:rolloutA_states_only", "dmpc_mlp_rollout_linearize", _rollout(SMALL, with_F=False)))

KERNEL = {"dmpc_mlp_rollout_linearize": "mlp_rollout_linearize_kernel", "dmpc_mpc_forward_rec_mlp": "mpc_forward_rec_mlp_kernel",
          "dmpc_box_ddp": "box_ddp_summary_kernel"}


def test_the_rows_are_not_in_the_shared_table():
    assert not set(r.id for r in ROWS) & set(abi_calls.BY_ID)


@pytest.mark.parametrize("case", ROWS, ids=[c.id for c in ROWS])
def test_memory_contract_with_two_hidden_layers(case):
    """inputs unchanged (the packed weights too), nothing written outside the outputs, outputs equal between the layouts"""
    r = both(case)
    assert r["rc"] == 0
    assert r["findings"] == [], "\n".join(r["findings"])
    assert KERNEL[case.entry] in r["kernel"], r["kernel"]
