"""What the tests of the two-layer weight gradient share (tests/test_mlp2_grad_cpu.py, tests/test_mlp2_grad_gpu.py): the cases
of tests/mlp2_cases.py with the gradient inputs of tests/test_mlp_dx_grad_gpu.py::inputs (x_init of the case, u = 0.5 randn,
g = randn, all float32-representable), the float64 reference - autograd of the live route on the CPU, computed once and left
unchanged - and the smallest |z| over both layers along the float64 rollout of those inputs, which decides whether a relu
gradient can be compared at all."""
import functools

import numpy as np
import torch

from chainer_differentiable_mpc_amd import MlpDx, _lib
from tests.helpers import npy
from tests.mlp2_cases import CASE, problem

NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
# what the GPU tests run: tanh on these, the other activations on OTHER_CASES (relu as the margin allows: asserted on the
# CPU for every one of them, tests/test_mlp2_grad_cpu.py)
GRAD_CASES = {k: CASE[k] for k in "ACDEF"}
OTHER_CASES = {k: CASE[k] for k in "AC"}
OTHER_ACTIVATIONS = ("relu", "silu", "softplus")


def walk_case():
    """a workgroup that walks more than one trajectory group: B five above four times the number of partials, which the library
    names - the second trip of workgroup 0 is a full group, that of workgroup 1 has one live wavefront"""
    return (3, 1, 5, 7, 4 * _lib.load().dmpc_mlp2_param_grad_partials(1 << 30) + 5, 3, 7)


def module(activation, case, device="cpu", dtype=torch.float32, residual=True, **kw):
    """the case's network (the weights of `NumpyMlp2`) with or without the residual; kw: param_grad, device_loop"""
    net = problem(activation, case)["net"]
    m = MlpDx(net.nx, net.nu, (net.H1, net.H2), residual=residual, activation=activation, **kw)
    with torch.no_grad():
        for name in NAMES:
            getattr(m, name).copy_(torch.as_tensor(getattr(net, name)))
    return m.to(device=device, dtype=dtype)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(x_init [B,nx], u [T,B,nu], g [T-1,B,nx]) as float32-representable numpy arrays"""
    nx, nu, H1, H2, B, T, s = case
    rng = np.random.RandomState(s + 50)
    u = 0.5 * rng.randn(T, B, nu)
    g = rng.randn(T - 1, B, nx)
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)   # noqa: E731
    return f32(problem("tanh", case)["x_init"]), f32(u), f32(g)


def run(m, case, device, dtype, wrt_inputs):
    """linearize on x = [x_init, ...] and u, then the gradient of sum(f * g) -> dict of tensors"""
    T = case[5]
    x_init, u, g = (torch.as_tensor(a, dtype=dtype, device=device) for a in inputs(case))
    x_init.requires_grad_(wrt_inputs), u.requires_grad_(wrt_inputs)
    x = x_init[None].expand(T, -1, -1)                # only x[0] is read
    F, f = m.linearize(x, u)
    assert not F.requires_grad and f.requires_grad
    wrt = list(m._weights()) + ([x_init, u] if wrt_inputs else [])
    grads = torch.autograd.grad((f * g).sum(), wrt)
    out = dict(zip(NAMES + ("x_init", "u"), grads))
    out.update(F=F.detach(), f=f.detach())
    return out


@functools.lru_cache(maxsize=None)
def reference(activation, case, residual=True):
    """float64 autograd of the live route on the CPU"""
    m = module(activation, case, "cpu", torch.float64, residual)
    assert m.param_grad == "live"
    return {k: npy(v) for k, v in run(m, case, "cpu", torch.float64, True).items()}


@functools.lru_cache(maxsize=None)
def margin(activation, case):
    """min |z| over both layers and every step of the float64 rollout of `inputs(case)`"""
    net = problem(activation, case)["net"]
    x_init, u, _ = inputs(case)
    x, worst = x_init, np.inf
    for t in range(case[5] - 1):
        z1, z2 = net.pre(x, u[t])
        worst = min(worst, float(np.abs(z1).min()), float(np.abs(z2).min()))
        x = net.step(x, u[t])
    return worst
