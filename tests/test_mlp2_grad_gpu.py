"""GPU: `MlpDx(..., (H1, H2), param_grad="device")` - the gradient of `linearize`'s f from `dmpc_mlp2_param_grad` (one sweep
kernel whose workgroups share dW2, one fixed-order reduction) against float64 torch autograd of the live route on the CPU, at
TOL_COSTATE, the tolerance of the depth-one gradient tests.  Inputs and reference: tests/mlp2_grad_cases.py.  relu: every case
here stays KINK_MARGIN away from a kink on the float64 side (asserted on the CPU, tests/test_mlp2_grad_cpu.py, and again here)."""
import warnings

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import BoxDDP, MlpDx, QuadCost, _lib
from tests import mlp2_grad_cases as gc
from tests.helpers import TOL_COSTATE, assert_close, npy
from tests.mlp2_cases import CASE, KINK_MARGIN, problem
from tests.mlp_dx_cases import BOUND, LS_DECAY, MAX_LS_ITER

pytestmark = pytest.mark.gpu

REDUCE_KERNEL = "mlp2_param_grad_reduce_kernel"
NAMES = gc.NAMES
ACT_AND_CASE = [("tanh", k) for k in gc.GRAD_CASES] + [(a, k) for a in gc.OTHER_ACTIVATIONS for k in gc.OTHER_CASES]


def dev(a, dtype=torch.float32):
    return torch.as_tensor(a, dtype=dtype, device="cuda")


def device_grads(activation, case, residual=True, wrt_inputs=False):
    m = gc.module(activation, case, "cuda", torch.float32, residual, param_grad="device")
    assert not m.fused_ok(dev(gc.inputs(case)[0]), dev(gc.inputs(case)[1]))       # a gradient is wanted
    return m, gc.run(m, case, "cuda", torch.float32, wrt_inputs)


def check_weights(got, ref):
    for name in NAMES:
        assert float(np.abs(ref[name]).max()) > 0, name
        assert tuple(got[name].shape) == ref[name].shape
        assert_close(npy(got[name]), ref[name], TOL_COSTATE, "d/d" + name)


@pytest.mark.parametrize("activation,key", ACT_AND_CASE, ids=["%s-%s" % ak for ak in ACT_AND_CASE])
def test_weight_gradients_against_float64_autograd(activation, key):
    """A: odd widths, B = 5 - a workgroup with one live wavefront; C: two units per lane, ragged, H1 != H2; D: every limit;
    E: B = 1, T = 2; F: H2 > H1"""
    case = CASE[key]
    if activation == "relu":
        assert gc.margin("relu", case) >= KINK_MARGIN, gc.margin("relu", case)
    _, got = device_grads(activation, case)
    ref = gc.reference(activation, case)
    check_weights(got, ref)
    assert_close(npy(got["f"]), ref["f"], TOL_COSTATE, "f")


def test_weight_gradients_without_the_residual():
    case = CASE["C"]
    _, got = device_grads("tanh", case, residual=False)
    ref = gc.reference("tanh", case, residual=False)
    check_weights(got, ref)
    assert_close(npy(got["f"]), ref["f"], TOL_COSTATE, "f")
    assert float(np.abs(ref["F"] - gc.reference("tanh", case)["F"]).max()) > 0.5        # another model than the residual one


@pytest.mark.parametrize("key", ["A", "C"])
def test_gradients_of_x_init_and_u(key):
    case = CASE[key]
    _, got = device_grads("tanh", case, wrt_inputs=True)
    ref = gc.reference("tanh", case)
    check_weights(got, ref)
    assert_close(npy(got["x_init"]), ref["x_init"], TOL_COSTATE, "d/dx_init")
    assert_close(npy(got["u"]), ref["u"], TOL_COSTATE, "d/du")
    assert tuple(got["u"].shape) == (case[5], case[4], case[1]) and not bool(got["u"][-1].any())


def test_a_workgroup_that_walks_more_than_one_group():
    case = gc.walk_case()
    B = case[4]
    lib = _lib.load()
    assert case[:4] == (3, 1, 5, 7) and case[5] == 3 and B == 4 * lib.dmpc_mlp2_param_grad_partials(1 << 30) + 5
    assert lib.dmpc_mlp2_param_grad_partials(B) == (B - 5) // 4 < (B + 3) // 4
    _, got = device_grads("tanh", case, wrt_inputs=True)
    ref = gc.reference("tanh", case)
    check_weights(got, ref)
    assert_close(npy(got["x_init"]), ref["x_init"], TOL_COSTATE, "d/dx_init")
    assert_close(npy(got["u"]), ref["u"], TOL_COSTATE, "d/du")


@pytest.mark.parametrize("which", ["two units per lane", "several groups per workgroup"])
def test_two_calls_give_the_same_bits(which):
    case = CASE["C"] if which == "two units per lane" else gc.walk_case()
    _, one = device_grads("tanh", case, wrt_inputs=True)
    _, two = device_grads("tanh", case, wrt_inputs=True)
    for k in one:
        assert torch.equal(one[k], two[k]), k


@pytest.mark.parametrize("key", list(gc.GRAD_CASES))
def test_forward_is_the_rollout_launch(key):
    case = CASE[key]
    m, got = device_grads("tanh", case)
    x_init, u, _ = (dev(a) for a in gc.inputs(case))
    with torch.no_grad():
        _, F, f = m.rollout_linearize(x_init, u)
    assert torch.equal(got["F"], F) and torch.equal(got["f"], f)


@pytest.mark.parametrize("device_loop", [False, True])
@pytest.mark.parametrize("key", ["A", "B"])
def test_box_ddp_gradient_through_the_device_node(key, device_loop):
    """tests/test_mlp_dx_grad_gpu.py::test_box_ddp_gradient_through_the_device_node with two hidden layers, on the host loop and
    on the device chain: `BoxDDP` picks the node up through `linearize_dynamics`.  `dmpc_last_kernel_name` is per thread and
    autograd runs a GPU node on its own thread, so the name is read from a hook on W1's gradient."""
    case = CASE[key]
    nx, nu, H1, H2, B, T, s = case
    P = problem("tanh", case)
    x0, C, c = dev(P["x_init"]), dev(P["C"]), dev(P["c"])
    rng = np.random.RandomState(s + 40)
    gx, gu = dev(rng.randn(T, B, nx)), dev(rng.randn(T, B, nu))
    grads, names = [], []
    for route in ("device", "live"):
        mlp = gc.module("tanh", case, "cuda", torch.float32, param_grad=route, device_loop=device_loop)
        mlp.W1.register_hook(lambda g: names.append(_lib.last_kernel_name()))
        solver = BoxDDP(T, -BOUND, BOUND, B, nx, nu, None, eps=1e-3, max_iter=10, line_search_decay=LS_DECAY,
                        max_line_search_iter=MAX_LS_ITER, quiet=True, detach_unconverged=False, update_dynamics=True)
        solver.__dict__.pop("_loop_flag", None)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x, u, _ = solver((x0, QuadCost(C, c), mlp))
        assert (solver.__dict__.get("_loop_flag") is not None) == device_loop       # which loop ran
        assert x.requires_grad and u.requires_grad
        grads.append(torch.autograd.grad((x * gx).sum() + (u * gu).sum(), list(mlp._weights())))
    assert len(names) == 2 and REDUCE_KERNEL in names[0] and REDUCE_KERNEL not in names[1], names
    for name, a, b in zip(NAMES, *grads):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), name
        assert float(a.abs().max()) > 0 and float(b.abs().max()) > 0, name
        assert_close(npy(a), npy(b), TOL_COSTATE, "d/d" + name)


def test_a_weight_changed_in_place_before_the_backward_is_an_autograd_error():
    case = CASE["A"]
    m = gc.module("tanh", case, "cuda", torch.float32, param_grad="device")
    x_init, u, g = (dev(a) for a in gc.inputs(case))
    _, f = m.linearize(x_init[None].expand(case[5], -1, -1), u)
    with torch.no_grad():
        m.W2.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (f * g).sum().backward()


def test_param_grad_device_with_one_hidden_layer_is_device_grad():
    """the same node, the same bits"""
    from tests import test_mlp_dx_grad_gpu as one_layer
    case = one_layer.CASES[2]
    net = one_layer.problem(case)["net"]
    out = []
    for kw in (dict(device_grad=True), dict(param_grad="device")):
        m = MlpDx(net.nx, net.nu, net.H, **kw)
        with torch.no_grad():
            for name in one_layer.NAMES:
                getattr(m, name).copy_(torch.as_tensor(getattr(net, name)))
        out.append(one_layer.run(m.cuda(), case, "cuda", torch.float32, True))
    assert sorted(out[0]) == sorted(out[1])
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
    assert float(out[0]["W1"].abs().max()) > 0
