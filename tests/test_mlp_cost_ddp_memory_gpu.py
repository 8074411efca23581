"""The memory contract of `dmpc_box_ddp_mlp_cost` (include/dmpc_mlp_cost.h), as tests/test_abi_memory_gpu.py checks every other
device call: the call inside a guarded arena (tests/arena.py) in both layouts, the workspace at exactly the queried size - no
guard word overwritten, no input modified (the packed weights among them), every output word written, outputs bit-equal
between the layouts.  The rows live here, not in the shared table of tests/abi_calls.py."""
import numpy as np
import pytest

from tests import abi_calls
from tests import mlp_cost_cases as mc
from tests.mlp_cost_ddp_cases import BEST_COST_EPS, CHAIN_END, EPS, NOT_IMPROVED_LIM
from tests.test_abi_memory_gpu import both

pytestmark = pytest.mark.gpu

I32 = np.int32


def _row(act, name, mode, with_f=True, with_info=True, max_iter=2):
    def make(b, lib):
        P = mc.problem(act, name)
        nx, nu, H, B, T = P["dims"]
        c = P["cost"]
        packed = np.concatenate([np.asarray(w, dtype=np.float64).reshape(-1) for w in (c.Q, c.p, c.W1, c.b1, c.w2)])
        ins = [b.inp("x_init", P["x_init"]), b.inp("cost_packed", packed), H, mc.ACT_CODE[act], mode, b.inp("F", P["F"]),
               b.inp("f", P["f"]) if with_f else None, 0, None, b.inp("u_init", np.zeros((T, B, nu))), b.inp("u_lower", P["lo"]),
               b.inp("u_upper", P["hi"])]
        outs = [b.out("x_best", (T, B, nx)), b.out("u_best", (T, B, nu)), b.out("costs_best", (B,)), b.out("du_norm_best", (B,)),
                b.out("du_norm_last", (B,)), b.out("state", (8,), I32)]
        need = lib.dmpc_box_ddp_mlp_cost_workspace_bytes(T, B, nx, nu)
        assert need > 0
        # eps, not_improved_lim, ls_decay, max_ls_iter, best_cost_eps, max_iter, n_qp_iter_max, scrambled_norm, batch_coupled
        scalars = [EPS, NOT_IMPROVED_LIM, mc.LS_DECAY, mc.MAX_LS_ITER, BEST_COST_EPS, max_iter, 20, 1, 0]
        info = b.info("info", B, written=True) if with_info else None      # (cleared by the call: handed over prefilled)
        return None, ("dmpc_box_ddp_mlp_cost", [T, B, nx, nu] + ins + scalars + outs + [b.ws("ws", need), need, info, None])
    return make


ROWS = [abi_calls.Case("box_ddp_mlp_cost:%s_%s_mode%d%s%s" % (name, act, mode, "" if with_f else "_no_f", "" if with_info else "_no_info"),
                       "dmpc_box_ddp_mlp_cost", _row(act, name, mode, with_f, with_info))
        for act, name, mode, with_f, with_info in (("softplus", "A", 0, True, True), ("softplus", "A", 1, True, True),
                                                   ("tanh", "A", 1, False, True), ("silu", "A", 0, True, False),
                                                   ("softplus", "C", 0, True, True), ("softplus", "C", 1, True, True))]


@pytest.mark.parametrize("case", ROWS, ids=[c.id for c in ROWS])
def test_memory_contract_of_the_chain(case):
    r = both(case)
    assert r["rc"] == 0, r["rc"]
    assert r["findings"] == [], "\n".join(r["findings"])
    assert CHAIN_END in r["kernel"], r["kernel"]
    state = r["A"].host("state")
    assert 1 <= state[1] <= 2 and state[4] == 0 and state[5] == 0 and state[6] == 0
    assert np.isfinite(r["A"].host("x_best")).all() and np.isfinite(r["A"].host("costs_best")).all()
