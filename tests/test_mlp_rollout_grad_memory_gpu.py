"""GPU: the C ABI's memory contract (tests/test_abi_memory_gpu.py) for `dmpc_mlp_rollout_grad` (include/dmpc_mlp_rollout_grad.h)
inside a guarded arena, in both layouts, with a workspace of exactly the queried size: the weights, the states, the controls and
grad_x are read-only, the gradients and the optional d_x_init, d_u are written in every word, nothing else is touched.  Rows:
one hidden layer small ((3,1) H = 5, a ragged workgroup) and at every limit ((16,8) H = 256), two hidden layers A and D, T = 1
(no sweep, no workspace) and the call without d_x_init and d_u.  The rows live here, not in tests/abi_calls.CASES;
tests/test_mlp_rollout_grad_cpu.py checks that every pointer-taking symbol of the new header has one."""
import numpy as np
import pytest

from tests import abi_calls, mlp2_cases
from tests.abi_calls import MLP_LARGE, MLP_SMALL, lqr_problem, mlp_inputs
from tests.test_abi_memory_gpu import both
from tests.test_mlp2_memory_gpu import code, weights

pytestmark = pytest.mark.gpu

ENTRY = "dmpc_mlp_rollout_grad"
TWO_SMALL, TWO_LARGE = mlp2_cases.CASE["A"], mlp2_cases.CASE["D"]
SILU = 3


def _rollout_grad(case, T=None, with_d=True):
    """a row for a case of one hidden layer (nx, nu, H, B, T, seed; tanh) or two (nx, nu, H1, H2, B, T, seed; silu)"""
    two = len(case) == 7
    nx, nu, B, T0, s = case[0], case[1], case[-3], case[-2], case[-1]
    T = T or T0

    def make(b, lib):
        if two:
            H1, H2 = case[2], case[3]
            hidden, act, w = code(case), SILU, weights(b, case)
            x_init = mlp2_cases.problem("silu", case)["x_init"]
            shapes = [("dW1", (H1, nx + nu)), ("db1", (H1,)), ("dW2|dW3", (H2 * H1 + nx * H2,)), ("db2|db3", (H2 + nx,))]
            P, G = H1 * (nx + nu) + H1 + H2 * H1 + nx * H2 + H2 + nx, lib.dmpc_mlp2_param_grad_partials(B)
        else:
            H = case[2]
            hidden, act, w = H, 0, mlp_inputs(b, case)[1]
            x_init = lqr_problem(B, T, nx, nu, s)["x_init"]
            shapes = [("dW1", (H, nx + nu)), ("db1", (H,)), ("dW2", (nx, H)), ("db2", (nx,))]
            P, G = H * (nx + nu) + H + nx * H + nx, lib.dmpc_mlp_param_grad_partials(B)
        u = b.inp("u", np.random.RandomState(s + 30).uniform(-0.5, 0.5, (T, B, nu)))
        x0, x = b.inp("x_init", x_init), b.produced("x", (T, B, nx))
        gx = b.inp("grad_x", np.random.RandomState(s + 31).randn(T, B, nx))
        outs = [b.out(name, shape) for name, shape in shapes]
        outs += [b.out("d_x_init", (B, nx)), b.out("d_u", (T, B, nu))] if with_d else [None, None]
        need = lib.dmpc_mlp_rollout_grad_workspace_bytes(B, nx, nu, hidden)
        assert lib.dmpc_mlp_rollout_grad_partials(B, hidden) == G and need == G * P * 4
        ws = b.ws("ws", need) if T > 1 else None         # (T = 1: no sweep, no workspace)
        return ([("dmpc_mlp_rollout_linearize", [T, B, nx, nu, hidden, act, 1] + w + [x0, u, x, None, None, None])],
                (ENTRY, [T, B, nx, nu, hidden, act, 1] + w + [x, u, gx] + outs + [ws, need if T > 1 else 0, None]))
    return make


ROWS = []
for _name, _case in (("one(3,1)H5_B5", MLP_SMALL), ("one(16,8)H256_B3", MLP_LARGE), ("twoA(3,1)H5x7_B5", TWO_SMALL),
                     ("twoD(16,8)H128x128_B3", TWO_LARGE)):
    ROWS.append(abi_calls.Case("mlp:rollout_grad_" + _name, ENTRY, _rollout_grad(_case)))
for _name, _case in (("one(3,1)H5_B5", MLP_SMALL), ("twoA(3,1)H5x7_B5", TWO_SMALL)):
    ROWS.append(abi_calls.Case("mlp:rollout_grad_" + _name + "_T1", ENTRY, _rollout_grad(_case, T=1)))
    ROWS.append(abi_calls.Case("mlp:rollout_grad_" + _name + "_weights_only", ENTRY, _rollout_grad(_case, with_d=False)))


def test_the_rows_are_not_in_the_shared_table():
    assert not set(r.id for r in ROWS) & set(abi_calls.BY_ID)


@pytest.mark.parametrize("case", ROWS, ids=[c.id for c in ROWS])
def test_memory_contract_of_the_rollout_gradient(case):
    """inputs unchanged, every output word written, nothing written outside the outputs, outputs equal between the layouts;
    the kernel launched last is the fixed-order reduction of the row's depth"""
    r = both(case)
    assert r["rc"] == 0
    assert r["findings"] == [], "\n".join(r["findings"])
    assert ("mlp2_param_grad_reduce_kernel" if "_two" in case.id else "mlp_param_grad_reduce_kernel") in r["kernel"], r["kernel"]
    a = r["A"]
    weights_out = [n for n in a.by_name if n.startswith(("dW", "db"))]
    assert len(weights_out) == 4
    if case.id.endswith("_T1"):
        for name in weights_out + ["d_u"]:
            assert not a.host(name).any(), name
        assert np.array_equal(a.host("d_x_init"), a.host("grad_x")[0])
    else:
        assert all(np.abs(a.host(name)).max() > 0 for name in weights_out)
        if "d_u" in a.by_name:
            assert np.abs(a.host("d_x_init")).max() > 0 and np.abs(a.host("d_u")[:-1]).max() > 0 and not a.host("d_u")[-1].any()
