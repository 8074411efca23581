"""GPU: `MlpDx(device_grad=True)` - the gradient of `linearize`'s f from `dmpc_mlp_param_grad` (one sweep kernel, one
fixed-order reduction) against float64 torch autograd of the live route on the CPU (`device_grad=False`, the code from before
the switch existed), at TOL_COSTATE.  In float32 on the CPU the same sums are 1.2e-6 from that reference."""
import functools
import warnings

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import BoxDDP, MlpDx, QuadCost, _lib
from tests.helpers import TOL_COSTATE, assert_close, npy
from tests.mlp_dx_cases import BOUND, CASES, LS_DECAY, MAX_LS_ITER, problem

pytestmark = pytest.mark.gpu

REDUCE_KERNEL = "mlp_param_grad_reduce_kernel"
NAMES = ("W1", "b1", "W2", "b2")


def walk_case():
    """a wavefront that walks more than one trajectory: B just above the number of partials, which the library names"""
    return (3, 1, 5, _lib.load().dmpc_mlp_param_grad_partials(1 << 30) + 3, 3, 7)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(a, dtype=dtype, device="cuda")


def module(case, device, dtype, residual=True, device_grad=False):
    """the case's network (the weights of `NumpyMlp.module`) with or without the residual and the device gradient"""
    net = problem(case)["net"]
    m = MlpDx(net.nx, net.nu, net.H, residual=residual, device_grad=device_grad)
    with torch.no_grad():
        for name in NAMES:
            getattr(m, name).copy_(torch.as_tensor(getattr(net, name)))
    return m.to(device=device, dtype=dtype)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(x_init [B,nx], u [T,B,nu], g [T-1,B,nx]) as float32-representable numpy arrays"""
    nx, nu, H, B, T, s = case
    rng = np.random.RandomState(s + 50)
    u = 0.5 * rng.randn(T, B, nu)
    g = rng.randn(T - 1, B, nx)
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)   # noqa: E731
    return f32(problem(case)["x_init"]), f32(u), f32(g)


def run(m, case, device, dtype, wrt_inputs):
    """linearize on x = [x_init, ...] and u, then the gradient of sum(f * g) -> dict of tensors"""
    T = case[4]
    x_init, u, g = (torch.as_tensor(a, dtype=dtype, device=device) for a in inputs(case))
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
def reference(case, residual=True):
    """float64 autograd of the live route on the CPU; computed once, left unchanged"""
    return {k: npy(v) for k, v in run(module(case, "cpu", torch.float64, residual), case, "cpu", torch.float64, True).items()}


def device_grads(case, residual=True, wrt_inputs=False):
    m = module(case, "cuda", torch.float32, residual, device_grad=True)
    assert not m.fused_ok(dev(inputs(case)[0]), dev(inputs(case)[1]))       # a gradient is wanted
    return m, run(m, case, "cuda", torch.float32, wrt_inputs)


def check_weights(got, ref):
    for name in NAMES:
        assert float(np.abs(ref[name]).max()) > 0, name
        assert_close(npy(got[name]), ref[name], TOL_COSTATE, "d/d" + name)


@pytest.mark.parametrize("case", CASES)
def test_weight_gradients_against_float64_autograd(case):
    _, got = device_grads(case)
    check_weights(got, reference(case))
    assert_close(npy(got["f"]), reference(case)["f"], TOL_COSTATE, "f")


def test_weight_gradients_without_the_residual():
    case = CASES[2]
    _, got = device_grads(case, residual=False)
    ref = reference(case, residual=False)
    check_weights(got, ref)
    assert float(np.abs(ref["F"] - reference(case)["F"]).max()) > 0.5        # another model than the residual one


@pytest.mark.parametrize("case", CASES[:2])
def test_gradients_of_x_init_and_u(case):
    _, got = device_grads(case, wrt_inputs=True)
    ref = reference(case)
    check_weights(got, ref)
    assert_close(npy(got["x_init"]), ref["x_init"], TOL_COSTATE, "d/dx_init")
    assert_close(npy(got["u"]), ref["u"], TOL_COSTATE, "d/du")
    assert tuple(got["u"].shape) == (case[4], case[3], case[1]) and not bool(got["u"][-1].any())


def test_a_wavefront_that_walks_more_than_one_trajectory():
    case = walk_case()
    B = case[3]
    assert _lib.load().dmpc_mlp_param_grad_partials(B) == B - 3
    _, got = device_grads(case, wrt_inputs=True)
    ref = reference(case)
    check_weights(got, ref)
    assert_close(npy(got["x_init"]), ref["x_init"], TOL_COSTATE, "d/dx_init")
    assert_close(npy(got["u"]), ref["u"], TOL_COSTATE, "d/du")


@pytest.mark.parametrize("which", ["several units per lane", "several trajectories per wavefront"])
def test_two_calls_give_the_same_bits(which):
    case = CASES[2] if which == "several units per lane" else walk_case()
    _, one = device_grads(case, wrt_inputs=True)
    _, two = device_grads(case, wrt_inputs=True)
    for k in one:
        assert torch.equal(one[k], two[k]), k


@pytest.mark.parametrize("case", CASES[:2])
def test_a_trajectory_does_not_depend_on_its_batch(case):
    """d_u[:, b] and d_x_init[b] of the batch equal the same trajectory run alone, bit for bit"""
    nx, nu, H, B, T, s = case
    m, got = device_grads(case, wrt_inputs=True)
    x_init, u, g = (dev(a) for a in inputs(case))
    for b in range(B):
        xb, ub = x_init[b:b + 1].clone().requires_grad_(True), u[:, b:b + 1].clone().requires_grad_(True)
        _, f = m.linearize(xb[None].expand(T, -1, -1), ub)
        dx, du = torch.autograd.grad((f * g[:, b:b + 1]).sum(), [xb, ub])
        assert torch.equal(f[:, 0], got["f"][:, b]), b
        assert torch.equal(dx[0], got["x_init"][b]) and torch.equal(du[:, 0], got["u"][:, b]), b


@pytest.mark.parametrize("case", CASES)
def test_forward_is_the_rollout_launch(case):
    m, got = device_grads(case)
    x_init, u, _ = (dev(a) for a in inputs(case))
    with torch.no_grad():
        _, F, f = m.rollout_linearize(x_init, u)
    assert torch.equal(got["F"], F) and torch.equal(got["f"], f)


@pytest.mark.parametrize("case", CASES[:2])
def test_box_ddp_gradient_through_the_device_node(case):
    """the construction of test_mlp_dx_gpu.py::test_box_ddp_gradient_reaches_the_weights on two modules with equal weights.
    `dmpc_last_kernel_name` is per thread and autograd runs a GPU node on its own thread, so the name is read from a
    hook on W1's gradient: on the thread of the backward, right after the node that produced it."""
    nx, nu, H, B, T, s = case
    P = problem(case)
    x0, C, c = dev(P["x_init"]), dev(P["C"]), dev(P["c"])
    rng = np.random.RandomState(s + 40)
    gx, gu = dev(rng.randn(T, B, nx)), dev(rng.randn(T, B, nu))
    grads, names = [], []
    for flag in (True, False):
        mlp = module(case, "cuda", torch.float32, device_grad=flag)
        mlp.W1.register_hook(lambda g: names.append(_lib.last_kernel_name()))
        solver = BoxDDP(T, -BOUND, BOUND, B, nx, nu, None, eps=1e-3, max_iter=10, line_search_decay=LS_DECAY,
                        max_line_search_iter=MAX_LS_ITER, quiet=True, detach_unconverged=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x, u, _ = solver((x0, QuadCost(C, c), mlp))
        assert x.requires_grad and u.requires_grad
        grads.append(torch.autograd.grad((x * gx).sum() + (u * gu).sum(), [mlp.W1, mlp.b1, mlp.W2, mlp.b2]))
    assert len(names) == 2 and REDUCE_KERNEL in names[0] and REDUCE_KERNEL not in names[1], names
    for name, a, b in zip(NAMES, *grads):
        assert bool(torch.isfinite(a).all()) and float(b.abs().max()) > 0, name
        assert_close(npy(a), npy(b), TOL_COSTATE, "d/d" + name)


def test_a_weight_changed_in_place_before_the_backward_is_an_autograd_error():
    case = CASES[0]
    m = module(case, "cuda", torch.float32, device_grad=True)
    x_init, u, g = (dev(a) for a in inputs(case))
    _, f = m.linearize(x_init[None].expand(case[4], -1, -1), u)
    with torch.no_grad():
        m.W1.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (f * g).sum().backward()
