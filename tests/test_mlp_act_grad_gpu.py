"""GPU: the weight gradients of `MlpDx` with the relu, silu and softplus activations - `dmpc_mlp_param_grad` behind
`device_grad=True`, and the live route with the kernel's F behind `device_grad=False` - against float64 torch autograd of the
live route on the CPU, at TOL_COSTATE.  The tests of tests/test_mlp_dx_grad_gpu.py per activation.

relu: the reference's points of differentiation stay KINK_MARGIN away from a kink (asserted, never skipped)."""
import functools
import warnings

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import BoxDDP, QuadCost, _lib, linearize_dynamics
from tests.helpers import TOL_COSTATE, assert_close, npy
from tests.mlp_act_cases import (ACTIVATIONS, KINK_MARGIN, WALK_SEED, grad_inputs, grad_margin, loop_grad_case,
                                 margin_along, problem)
from tests.mlp_act_cases import GRAD_NAMES as NAMES
from tests.mlp_dx_cases import BOUND, CASES, LS_DECAY, MAX_LS_ITER

pytestmark = pytest.mark.gpu

REDUCE_KERNEL = "mlp_param_grad_reduce_kernel"
activations = pytest.mark.parametrize("activation", ACTIVATIONS)


def act_cases(cases):
    return pytest.mark.parametrize("activation,case", [(a, c) for a in ACTIVATIONS for c in cases])


def walk_case():
    """a wavefront that walks more than one trajectory: B just above the number of partials, which the library names"""
    return (3, 1, 5, _lib.load().dmpc_mlp_param_grad_partials(1 << 30) + 3, 3, WALK_SEED)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(a, dtype=dtype, device="cuda")


def module(activation, case, device, dtype, residual=True, device_grad=False):
    return problem(activation, case)["net"].module(device, dtype, residual=residual, device_grad=device_grad)


def run(m, activation, case, device, dtype, wrt_inputs):
    """linearize on x = [x_init, ...] and u, then the gradient of sum(f * g) -> dict of tensors"""
    T = case[4]
    x_init, u, g = (torch.as_tensor(a, dtype=dtype, device=device) for a in grad_inputs(activation, case))
    x_init.requires_grad_(wrt_inputs), u.requires_grad_(wrt_inputs)
    x = x_init[None].expand(T, -1, -1)                # only x[0] is read
    F, f = m.linearize(x, u)
    assert not F.requires_grad and f.requires_grad
    wrt = [m.W1, m.b1, m.W2, m.b2] + ([x_init, u] if wrt_inputs else [])
    grads = torch.autograd.grad((f * g).sum(), wrt)
    out = dict(zip(NAMES + ("x_init", "u"), grads))
    out.update(F=F.detach(), f=f.detach())
    return out


@functools.lru_cache(maxsize=None)
def reference(activation, case, residual=True):
    """float64 autograd of the live route on the CPU; computed once, left unchanged"""
    if activation == "relu":
        assert grad_margin(activation, case) >= KINK_MARGIN, grad_margin(activation, case)
    m = module(activation, case, "cpu", torch.float64, residual)
    return {k: npy(v) for k, v in run(m, activation, case, "cpu", torch.float64, True).items()}


def device_grads(activation, case, residual=True, wrt_inputs=False):
    m = module(activation, case, "cuda", torch.float32, residual, device_grad=True)
    x_init, u, _ = grad_inputs(activation, case)
    assert not m.fused_ok(dev(x_init), dev(u))       # a gradient is wanted
    return m, run(m, activation, case, "cuda", torch.float32, wrt_inputs)


def check_weights(got, ref):
    for name in NAMES:
        assert float(np.abs(ref[name]).max()) > 0, name
        assert_close(npy(got[name]), ref[name], TOL_COSTATE, "d/d" + name)


@act_cases(CASES)
def test_weight_gradients_against_float64_autograd(activation, case):
    _, got = device_grads(activation, case)
    check_weights(got, reference(activation, case))
    assert_close(npy(got["f"]), reference(activation, case)["f"], TOL_COSTATE, "f")


@activations
def test_weight_gradients_without_the_residual(activation):
    case = CASES[2]
    _, got = device_grads(activation, case, residual=False)
    ref = reference(activation, case, residual=False)
    check_weights(got, ref)
    assert float(np.abs(ref["F"] - reference(activation, case)["F"]).max()) > 0.5     # another model than the residual one


@act_cases(CASES[:2])
def test_gradients_of_x_init_and_u(activation, case):
    _, got = device_grads(activation, case, wrt_inputs=True)
    ref = reference(activation, case)
    check_weights(got, ref)
    assert float(np.abs(ref["x_init"]).max()) < 1e-12 and float(np.abs(ref["u"]).max()) < 1e-12     # the cancellation
    assert_close(npy(got["x_init"]), ref["x_init"], TOL_COSTATE, "d/dx_init")
    assert_close(npy(got["u"]), ref["u"], TOL_COSTATE, "d/du")
    assert not bool(got["x_init"].any()) and not bool(got["u"].any())                  # exact zeros from the kernel
    assert tuple(got["u"].shape) == (case[4], case[3], case[1])


@activations
def test_a_wavefront_that_walks_more_than_one_trajectory(activation):
    case = walk_case()
    B = case[3]
    assert _lib.load().dmpc_mlp_param_grad_partials(B) == B - 3
    _, got = device_grads(activation, case, wrt_inputs=True)
    ref = reference(activation, case)
    check_weights(got, ref)
    assert_close(npy(got["x_init"]), ref["x_init"], TOL_COSTATE, "d/dx_init")
    assert_close(npy(got["u"]), ref["u"], TOL_COSTATE, "d/du")


@activations
@pytest.mark.parametrize("which", ["several units per lane", "several trajectories per wavefront"])
def test_two_calls_give_the_same_bits(which, activation):
    case = CASES[2] if which == "several units per lane" else walk_case()
    _, one = device_grads(activation, case, wrt_inputs=True)
    _, two = device_grads(activation, case, wrt_inputs=True)
    for k in one:
        assert torch.equal(one[k], two[k]), k


@act_cases(CASES)
def test_forward_is_the_rollout_launch(activation, case):
    m, got = device_grads(activation, case)
    x_init, u, _ = (dev(a) for a in grad_inputs(activation, case))
    with torch.no_grad():
        _, F, f = m.rollout_linearize(x_init, u)
    assert torch.equal(got["F"], F) and torch.equal(got["f"], f)


@act_cases(CASES[:2])
def test_live_route_with_the_kernels_jacobian_against_a_plain_callable(activation, case):
    """`device_grad=False` with a gradient wanted: F from the kernel, next and the re-rolled states live, against
    `linearize_dynamics` around the module as a plain callable (autograd's Jacobian) on the device, and against the float64
    reference"""
    nx, nu, H, B, T, s = case
    ref = reference(activation, case)
    mlp = module(activation, case, "cuda", torch.float32)
    x_init, u, g = (dev(a) for a in grad_inputs(activation, case))
    x = x_init[None].expand(T, -1, -1)
    params = [mlp.W1, mlp.b1, mlp.W2, mlp.b2]
    assert not mlp.fused_ok(x[0], u)
    F, f = mlp.linearize(x, u)
    assert "mlp_rollout_linearize_kernel" in _lib.last_kernel_name()
    Fa, fa = linearize_dynamics(x, u, lambda a, b: mlp(a, b))
    assert not F.requires_grad and f.requires_grad
    assert_close(npy(F), npy(Fa), TOL_COSTATE, "F")
    assert_close(npy(f), npy(fa), TOL_COSTATE, "f")
    assert_close(npy(F), ref["F"], TOL_COSTATE, "F against float64")
    own = torch.autograd.grad((f * g).sum(), params)
    auto = torch.autograd.grad((fa * g).sum(), params)
    for name, a, b in zip(NAMES, own, auto):
        assert float(b.abs().max()) > 0
        assert_close(npy(a), npy(b), TOL_COSTATE, "d/d" + name)
        assert_close(npy(a), ref[name], TOL_COSTATE, "d/d" + name + " against float64")


@act_cases(CASES[:2])
def test_box_ddp_gradient_through_the_device_node(activation, case):
    """the construction of tests/test_mlp_dx_grad_gpu.py: two modules with equal weights, the gradient node of one on the
    device.  Both differentiate at the pair their own solve returned; for relu that point must be clear of every kink (in
    float64, at the returned controls) for the two float32 evaluations of z to agree on its side: `loop_grad_case` has the
    seeds at which it is."""
    case = loop_grad_case(activation, case)
    nx, nu, H, B, T, s = case
    P = problem(activation, case)
    x0, C, c = dev(P["x_init"]), dev(P["C"]), dev(P["c"])
    rng = np.random.RandomState(s + 40)
    gx, gu = dev(rng.randn(T, B, nx)), dev(rng.randn(T, B, nu))
    grads, names, us = [], [], []
    for flag in (True, False):
        mlp = module(activation, case, "cuda", torch.float32, device_grad=flag)
        mlp.W1.register_hook(lambda g: names.append(_lib.last_kernel_name()))
        solver = BoxDDP(T, -BOUND, BOUND, B, nx, nu, None, eps=1e-3, max_iter=10, line_search_decay=LS_DECAY,
                        max_line_search_iter=MAX_LS_ITER, quiet=True, detach_unconverged=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x, u, _ = solver((x0, QuadCost(C, c), mlp))
        assert x.requires_grad and u.requires_grad
        us.append(u.detach())
        grads.append(torch.autograd.grad((x * gx).sum() + (u * gu).sum(), [mlp.W1, mlp.b1, mlp.W2, mlp.b2]))
    assert len(names) == 2 and REDUCE_KERNEL in names[0] and REDUCE_KERNEL not in names[1], names
    if activation == "relu":
        margin = min(margin_along(P["net"], P["x_init"], npy(u)) for u in us)
        print("relu min |z| at the returned pairs: %.3e" % margin)
        assert margin >= KINK_MARGIN, margin
    for name, a, b in zip(NAMES, *grads):
        assert bool(torch.isfinite(a).all()) and float(b.abs().max()) > 0, name
        assert_close(npy(a), npy(b), TOL_COSTATE, "d/d" + name)
