"""What the tests of `MlpDx.rollout`'s gradient share (tests/test_mlp_rollout_grad_cpu.py, tests/test_mlp_rollout_grad_gpu.py):
the networks, x_init and u of the weight-gradient tests - tests/test_mlp_dx_grad_gpu.py::inputs with one hidden layer,
tests/mlp2_grad_cases.py::inputs with two - with g = randn(T,B,nx) = dL/dx rounded to float32, and the float64 reference:
torch autograd of the live torch loop on the CPU, computed once and left unchanged.

A spec is (activation, case, residual); the case's length tells the depth: (nx, nu, H, B, T, seed) or (nx, nu, H1, H2, B, T, seed).
The depth-one weights do not depend on the activation (tests/mlp_act_cases.NumpyActMlp has NumpyMlp's), so one builder serves all
four.  Pendulum records for `prediction_loss`: `PendulumDx` rollouts in float64, rounded to float32."""
import functools
import math

import numpy as np
import torch

from chainer_differentiable_mpc_amd import MlpDx, PendulumDx
from tests import mlp2_cases, mlp2_grad_cases, mlp_act_cases, mlp_dx_cases
from tests.helpers import npy
from tests.test_mlp_dx_grad_gpu import inputs as inputs_one

ONE, TWO = mlp_dx_cases.CASES, mlp2_cases.CASE
KINK_MARGIN = mlp_act_cases.KINK_MARGIN


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def depth(case):
    return 1 if len(case) == 6 else 2


def names(case):
    return ("W1", "b1", "W2", "b2") if depth(case) == 1 else mlp2_grad_cases.NAMES


def dims(case):
    """(nx, nu, B, T, seed)"""
    return case[0], case[1], case[-3], case[-2], case[-1]


def model(activation, case, device="cpu", dtype=torch.float32, residual=True, **kw):
    """the case's network; kw: param_grad"""
    if depth(case) == 2:
        return mlp2_grad_cases.module(activation, case, device, dtype, residual, **kw)
    net = mlp_dx_cases.problem(case)["net"]
    m = MlpDx(net.nx, net.nu, net.H, residual=residual, activation=activation, **kw)
    with torch.no_grad():
        for name in names(case):
            getattr(m, name).copy_(torch.as_tensor(getattr(net, name)))
    return m.to(device=device, dtype=dtype)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(x_init [B,nx], u [T,B,nu], g [T,B,nx]) as float32-representable numpy arrays"""
    nx, nu, B, T, s = dims(case)
    x_init, u, _ = inputs_one(case) if depth(case) == 1 else mlp2_grad_cases.inputs(case)
    return x_init, u, f32(np.random.RandomState(s + 60).randn(T, B, nx))


def margin(activation, case):
    """min |z| along the float64 rollout of `inputs(case)`: the existing functions of the weight-gradient tests"""
    if depth(case) == 2:
        return mlp2_grad_cases.margin(activation, case)
    return mlp_act_cases.grad_margin(activation, case)


def run(m, case, device, dtype, g=None, u_rows=None):
    """x = rollout(x_init, u), then the gradient of sum(x * g) -> dict of tensors: the weights' names, x_init, u, x"""
    nx, nu, B, T, s = dims(case)
    x_init, u, g0 = (torch.as_tensor(a, dtype=dtype, device=device) for a in inputs(case))
    g = g0 if g is None else torch.as_tensor(g, dtype=dtype, device=device)
    if u_rows is not None:
        u = u[:u_rows].clone()
    x_init.requires_grad_(True), u.requires_grad_(True)
    x = m.rollout(x_init, u, T=T)
    assert x.requires_grad and tuple(x.shape) == (T, B, nx)
    grads = torch.autograd.grad((x * g).sum(), list(m._weights()) + [x_init, u], allow_unused=True)
    out = dict(zip(names(case) + ("x_init", "u"), grads))
    out["x"] = x.detach()
    return out


@functools.lru_cache(maxsize=None)
def reference(activation, case, residual=True):
    """float64 autograd of the live torch loop on the CPU"""
    m = model(activation, case, "cpu", torch.float64, residual)
    assert m.param_grad == "live"
    return {k: npy(v) for k, v in run(m, case, "cpu", torch.float64).items()}


# ---- pendulum records
PEND_T, PEND_B = 8, 6
FIT_NETS = (16, (16, 12))         # the widths of the SGD test, (3,1), seed 0
FIT_HORIZON, FIT_LR, FIT_STEPS = 4, 0.05, 5


@functools.lru_cache(maxsize=None)
def pendulum_record():
    """(x [T,B,3], u [T-1,B,1]): `PendulumDx` rolled in float64 from random angles and velocities under u ~ U(-2, 2)"""
    rng = np.random.RandomState(0)
    th, dth = rng.uniform(-math.pi, math.pi, PEND_B), rng.uniform(-1.0, 1.0, PEND_B)
    u = torch.as_tensor(rng.uniform(-2.0, 2.0, (PEND_T - 1, PEND_B, 1)))
    dx = PendulumDx().double()
    xs = [torch.as_tensor(np.stack((np.cos(th), np.sin(th), dth), axis=1))]
    with torch.no_grad():
        for t in range(PEND_T - 1):
            xs.append(dx(xs[t], u[t]))
    return f32(torch.stack(xs, 0).numpy()), f32(u.numpy())


def fit_model(n_hidden, device="cpu", dtype=torch.float32, **kw):
    return MlpDx(3, 1, n_hidden, seed=0, **kw).to(device=device, dtype=dtype)


def sgd(m, x, u, steps=FIT_STEPS):
    """plain SGD on prediction_loss -> the losses before every step and after the last"""
    losses = []
    for _ in range(steps):
        loss = m.prediction_loss(x, u, horizon=FIT_HORIZON)
        grads = torch.autograd.grad(loss, list(m._weights()))
        with torch.no_grad():
            for p, gr in zip(m._weights(), grads):
                p.sub_(FIT_LR * gr)
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(m.prediction_loss(x, u, horizon=FIT_HORIZON)))
    return losses


@functools.lru_cache(maxsize=None)
def sgd_reference(n_hidden):
    """float64, CPU, live route -> (weights after FIT_STEPS steps, losses)"""
    x, u = (torch.as_tensor(a) for a in pendulum_record())
    m = fit_model(n_hidden, "cpu", torch.float64)
    losses = sgd(m, x, u)
    return [npy(p) for p in m._weights()], losses
