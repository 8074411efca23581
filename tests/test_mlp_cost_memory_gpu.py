"""GPU: the C ABI's memory contract (tests/test_abi_memory_gpu.py) for the three launching entry points of
include/dmpc_mlp_cost.h - `dmpc_mlp_cost_approx`, `dmpc_mpc_forward_rec_mlp_cost`, `dmpc_mlp_cost_param_grad` - inside a guarded
arena, in both layouts: the five parameters, the trajectories, the gains, the dynamics and the upstream gradients are read-only,
every output word is written, nothing else is touched, and the gradient runs with a workspace of exactly the queried size.
Cases A (odd widths, a ragged last workgroup) and C (every limit: the largest LDS image, every accumulator in use), and the
calls with their optional outputs and inputs left out.  The rows live here, not in tests/abi_calls.CASES."""
import numpy as np
import pytest

from tests import abi_calls
from tests import mlp_cost_cases as mc
from tests.abi_calls import LS_DECAY, _step_outputs
from tests.test_abi_memory_gpu import both

pytestmark = pytest.mark.gpu

ACT = "softplus"


def weights(b, P, with_quad=True):
    c = P["cost"]
    quad = [b.inp("Q", c.Q), b.inp("p", c.p)] if with_quad else []
    return quad + [b.inp("W1", c.W1), b.inp("b1", c.b1), b.inp("w2", c.w2)]


def _approx(name, model=True, costs=True):
    def make(b, lib):
        P = mc.problem(ACT, name)
        nx, nu, H, B, T = P["dims"]
        x, u, _, _ = mc.grad_points(P)
        outs = [b.out("H_out", (T, B, nx + nu, nx + nu)), b.out("g_out", (T, B, nx + nu))] if model else [None, None]
        outs.append(b.out("costs_out", (T, B)) if costs else None)
        return None, ("dmpc_mlp_cost_approx", [T, B, nx, nu, H, mc.ACT_CODE[ACT]] + weights(b, P) + [b.inp("x", x), b.inp("u", u)]
                      + outs + [None])
    return make


def _search(name, optional=True):
    def make(b, lib):
        P = mc.problem(ACT, name)
        nx, nu, H, B, T = P["dims"]
        it = mc.oracle_iterates(ACT, name)[0]
        ins = [b.inp("Ks", it["Ks"]), b.inp("ks", it["ks"]), b.inp("controls", it["controls"]), b.inp("states", it["states"]),
               b.inp("u_lower", P["lo"]), b.inp("u_upper", P["hi"]), b.inp("F", P["F"]), b.inp("f", P["f"]) if optional else None]
        if optional:
            outs = _step_outputs(b, T, B, nx, nu, False, False) + [b.info("info", B)]
        else:       # old_costs, objs, u_first and info left out
            outs = [b.out("x_out", (T, B, nx)), b.out("u_out", (T, B, nu)), b.out("costs", (B,)), None, b.out("alphas", (B,)), None, None,
                    b.out("n_ls_iter", (B,), abi_calls.I32), None]
        return None, ("dmpc_mpc_forward_rec_mlp_cost", [T, B, nx, nu, H, mc.ACT_CODE[ACT]] + weights(b, P) + ins + [LS_DECAY, 10] + outs
                      + [None])
    return make


def _param_grad(name, with_g=True, with_c=True):
    def make(b, lib):
        P = mc.problem(ACT, name)
        nx, nu, H, B, T = P["dims"]
        ns = nx + nu
        x, u, v, r = mc.grad_points(P)
        ups = [b.inp("grad_g", v) if with_g else None, b.inp("grad_costs", r) if with_c else None]
        outs = [b.out("dQ", (ns, ns)), b.out("dp", (ns,)), b.out("dW1", (H, ns)), b.out("db1", (H,)), b.out("dw2", (H,))]
        need = lib.dmpc_mlp_cost_param_grad_workspace_bytes(T, B, nx, nu, H)
        assert need == min(T * B, 256) * (ns * ns + ns + H * ns + 2 * H) * 4
        return None, ("dmpc_mlp_cost_param_grad", [T, B, nx, nu, H, mc.ACT_CODE[ACT]] + weights(b, P, with_quad=False)
                      + [b.inp("x", x), b.inp("u", u)] + ups + outs + [b.ws("ws", need), need, None])
    return make


ROWS = []
for _name, _label in (("A", "A(3,1)H7_B5"), ("C", "C(16,8)H256_B2")):
    ROWS.append(abi_calls.Case("mlp_cost:approx" + _label, "dmpc_mlp_cost_approx", _approx(_name)))
    ROWS.append(abi_calls.Case("mlp_cost:forward_rec" + _label, "dmpc_mpc_forward_rec_mlp_cost", _search(_name)))
    ROWS.append(abi_calls.Case("mlp_cost:param_grad" + _label, "dmpc_mlp_cost_param_grad", _param_grad(_name)))
ROWS.append(abi_calls.Case("mlp_cost:approxA_values_only", "dmpc_mlp_cost_approx", _approx("A", model=False)))
ROWS.append(abi_calls.Case("mlp_cost:approxA_model_only", "dmpc_mlp_cost_approx", _approx("A", costs=False)))
ROWS.append(abi_calls.Case("mlp_cost:forward_recA_no_optional", "dmpc_mpc_forward_rec_mlp_cost", _search("A", optional=False)))
ROWS.append(abi_calls.Case("mlp_cost:param_gradA_grad_g_only", "dmpc_mlp_cost_param_grad", _param_grad("A", with_c=False)))
ROWS.append(abi_calls.Case("mlp_cost:param_gradA_grad_costs_only", "dmpc_mlp_cost_param_grad", _param_grad("A", with_g=False)))

KERNEL = {"dmpc_mlp_cost_approx": "mlp_cost_approx_kernel", "dmpc_mpc_forward_rec_mlp_cost": "mpc_forward_rec_mlp_cost_kernel",
          "dmpc_mlp_cost_param_grad": "mlp_cost_param_grad_reduce_kernel"}


def test_the_rows_are_not_in_the_shared_table():
    assert not set(r.id for r in ROWS) & set(abi_calls.BY_ID)


@pytest.mark.parametrize("case", ROWS, ids=[c.id for c in ROWS])
def test_memory_contract_of_the_learned_cost(case):
    """inputs unchanged, every output word written, nothing written outside the outputs, outputs equal between the layouts"""
    r = both(case)
    assert r["rc"] == 0
    assert r["findings"] == [], "\n".join(r["findings"])
    assert KERNEL[case.entry] in r["kernel"], r["kernel"]
    if case.entry == "dmpc_mlp_cost_param_grad":
        assert all(np.abs(r["A"].host(name)).max() > 0 for name in ("dQ", "dp", "dW1", "db1", "dw2"))


def test_values_only_costs_are_the_full_call_s_bits():
    full, values = both(ROWS[0]), both(ROWS[6])
    assert ROWS[6].id.endswith("values_only")
    assert np.array_equal(full["A"].host("costs_out").view(np.int32), values["A"].host("costs_out").view(np.int32))
