"""GPU: the C ABI's memory contract (tests/test_abi_memory_gpu.py) for `dmpc_mlp2_param_grad` (include/dmpc_mlp_grad.h) inside a
guarded arena, in both layouts, with a workspace of exactly the queried size: the packed weights, the states, the controls and
grad_f are read-only, the packed gradients [dW2 | dW3] and [db2 | db3] and the optional d_x_init, d_u are written in every word,
nothing else is touched.  Cases A (odd widths below 64, a workgroup with one live wavefront in its second group) and D (every
limit: the largest LDS image and every accumulator in use), T = 1 (zeros, no sweep, no workspace) and the call without d_x_init
and d_u.  The rows live here, not in tests/abi_calls.CASES; tests/test_mlp2_grad_cpu.py checks that every pointer-taking symbol
of the new header has one."""
import numpy as np
import pytest

from tests import abi_calls, mlp2_cases
from tests.test_abi_memory_gpu import both
from tests.test_mlp2_memory_gpu import code, weights

pytestmark = pytest.mark.gpu

SMALL, LARGE = mlp2_cases.CASE["A"], mlp2_cases.CASE["D"]
SILU = 3


def _param_grad(case, T=None, with_d=True):
    nx, nu, H1, H2, B, T0, s = case
    T = T or T0

    def make(b, lib):
        P = mlp2_cases.problem("silu", case)
        w = weights(b, case)
        u = b.inp("u", np.random.RandomState(s + 30).uniform(-0.5, 0.5, (T, B, nu)))
        x0, x = b.inp("x_init", P["x_init"]), b.produced("x", (T, B, nx))
        gf = b.inp("grad_f", np.random.RandomState(s + 31).randn(T - 1, B, nx)) if T > 1 else None
        outs = [b.out("dW1", (H1, nx + nu)), b.out("db1", (H1,)), b.out("dW2|dW3", (H2 * H1 + nx * H2,)), b.out("db2|db3", (H2 + nx,))]
        outs += [b.out("d_x_init", (B, nx)), b.out("d_u", (T, B, nu))] if with_d else [None, None]
        need = lib.dmpc_mlp2_param_grad_workspace_bytes(B, nx, nu, code(case))
        assert need == lib.dmpc_mlp2_param_grad_partials(B) * (H1 * (nx + nu) + H1 + H2 * H1 + nx * H2 + H2 + nx) * 4
        ws = b.ws("ws", need) if T > 1 else None         # (T = 1 only zeroes the outputs: no workspace)
        return ([("dmpc_mlp_rollout_linearize", [T, B, nx, nu, code(case), SILU, 1] + w + [x0, u, x, None, None, None])],
                ("dmpc_mlp2_param_grad", [T, B, nx, nu, code(case), SILU, 1] + w + [x, u, gf] + outs + [ws, need if T > 1 else 0, None]))
    return make


ROWS = []
for _name, _case in (("A(3,1)H5x7_B5", SMALL), ("D(16,8)H128x128_B3", LARGE)):
    ROWS.append(abi_calls.Case("mlp2:param_grad" + _name, "dmpc_mlp2_param_grad", _param_grad(_case)))
    ROWS.append(abi_calls.Case("mlp2:param_grad" + _name + "_T1", "dmpc_mlp2_param_grad", _param_grad(_case, T=1)))
ROWS.append(abi_calls.Case("mlp2:param_gradA_weights_only", "dmpc_mlp2_param_grad", _param_grad(SMALL, with_d=False)))


def test_the_rows_are_not_in_the_shared_table():
    assert not set(r.id for r in ROWS) & set(abi_calls.BY_ID)


@pytest.mark.parametrize("case", ROWS, ids=[c.id for c in ROWS])
def test_memory_contract_of_the_two_layer_weight_gradient(case):
    """inputs unchanged (the packed weights too), every output word written, nothing written outside the outputs, outputs equal
    between the layouts; the kernel launched last is the fixed-order reduction"""
    r = both(case)
    assert r["rc"] == 0
    assert r["findings"] == [], "\n".join(r["findings"])
    assert "mlp2_param_grad_reduce_kernel" in r["kernel"], r["kernel"]
    a = r["A"]
    if case.id.endswith("_T1"):
        for name in ("dW1", "db1", "dW2|dW3", "db2|db3", "d_x_init", "d_u"):
            assert not a.host(name).any(), name
    else:
        assert all(np.abs(a.host(name)).max() > 0 for name in ("dW1", "db1", "dW2|dW3", "db2|db3"))
        if "d_u" in a.by_name:
            assert not a.host("d_x_init").any() and not a.host("d_u").any()
