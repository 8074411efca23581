"""GPU: the C ABI's memory contract (tests/test_abi_memory_gpu.py) on `dmpc_box_ddp` with dyn_kind 2 - the MlpDx network
inside the box-DDP chain: inside a guarded arena, in both layouts, with a workspace of exactly the queried size, both
`search_linearizes` settings.  The packed weights are an input like every other: read-only.  The rows live here, not in
tests/abi_calls.CASES."""
import ctypes

import numpy as np
import pytest

from tests import abi_calls, mlp_dx_cases
from tests.abi_calls import I32, LS_DECAY, MLP_LARGE, MLP_SMALL, N_QP
from tests.test_abi_memory_gpu import both

pytestmark = pytest.mark.gpu


def _box_ddp_mlp(case, search_linearizes, max_iter=2):
    nx, nu, H, B, T, s = case

    def make(b, lib):
        P = mlp_dx_cases.problem(case)
        net = P["net"]
        packed = np.concatenate([getattr(net, k).reshape(-1) for k in ("W1", "b1", "W2", "b2")])
        params = (ctypes.c_float * 4)(float(H), 0.0, 1.0, float(search_linearizes))      # a HOST array
        ins = [b.inp("x_init", P["x_init"]), b.inp("C", P["C"]), b.inp("c", P["c"]), b.inp("weights", packed), None, 2, params,
               b.inp("u_init", np.zeros((T, B, nu))), b.inp("u_lower", P["lo"]), b.inp("u_upper", P["hi"])]
        outs = [b.out("x_best", (T, B, nx)), b.out("u_best", (T, B, nu)), b.out("costs_best", (B,)), b.out("du_norm_best", (B,)),
                b.out("du_norm_last", (B,)), b.out("state", (8,), I32)]
        need = lib.dmpc_box_ddp_workspace_bytes(T, B, nx, nu)
        # eps, not_improved_lim, ls_decay, max_ls_iter, best_cost_eps, max_iter, n_qp_iter_max, scrambled_norm, batch_coupled
        scalars = [1e-5, 5, LS_DECAY, 10, 1e-4, max_iter, N_QP, 1, 0]
        return None, ("dmpc_box_ddp", [T, B, nx, nu] + ins + scalars + outs + [b.ws("ws", need), need, b.info("info", B, written=True), None])
    return make


ROWS = [abi_calls.Case("box_ddp:mlp%s_search_linearizes%d" % (name, sl), "dmpc_box_ddp", _box_ddp_mlp(case, sl))
        for name, case in (("(3,1)H5_B5", MLP_SMALL), ("(16,8)H256_B3", MLP_LARGE)) for sl in (0, 1)]


def test_the_rows_are_not_in_the_shared_table():
    assert MLP_SMALL[3] == 5 and MLP_LARGE[3] == 3
    assert not set(r.id for r in ROWS) & set(abi_calls.BY_ID)


@pytest.mark.parametrize("case", ROWS, ids=[c.id for c in ROWS])
def test_memory_contract_of_the_network_chain(case):
    r = both(case)
    assert r["rc"] == 0
    assert r["findings"] == [], "\n".join(r["findings"])        # (an input modified - the packed weights too - is a finding)
    assert "box_ddp_summary_kernel" in r["kernel"], r["kernel"]
