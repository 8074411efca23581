"""CPU: `MlpDx` as torch code - forward, the analytic linearisation and the gradient that reaches its parameters - against a
numpy restatement and against `linearize_dynamics` on the same module as a plain callable; the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import MlpDx, _lib, linearize_dynamics
from tests.helpers import assert_close, npy
from tests.mlp_dx_cases import BOUND, CASES, problem


def _iterate(case):
    """(module, net, x [T,B,nx], u [T,B,nu]) in float64: controls inside the box, any states (only x[0] is read)"""
    nx, nu, H, B, T, s = case
    net = problem(case)["net"]
    rng = np.random.RandomState(s + 20)
    u = BOUND * (2.0 * rng.rand(T, B, nu) - 1.0)
    x = rng.randn(T, B, nx)
    return net.module(dtype=torch.float64), net, torch.as_tensor(x), torch.as_tensor(u)


@pytest.mark.parametrize("case", CASES)
def test_forward_matches_the_numpy_network(case):
    m, net, x, u = _iterate(case)
    with torch.no_grad():
        got = m(x[0], u[0])
    assert_close(npy(got), net.step(x[0].numpy(), u[0].numpy()), 1e-12, "next")
    with torch.no_grad():
        assert_close(npy(m(x[0, 0], u[0, 0])), npy(got[0]), 1e-12, "next, unbatched input")


@pytest.mark.parametrize("case", CASES)
def test_linearize_matches_the_analytic_jacobian_and_autograd(case):
    m, net, x, u = _iterate(case)
    Fr, fr = net.linearize(x.numpy(), u.numpy())
    F, f = m.linearize(x, u)
    Fa, fa = linearize_dynamics(x, u, lambda a, b: m(a, b))
    assert not F.requires_grad and f.requires_grad            # F_t is a constant of the graph, f_t stays on it
    assert_close(npy(F), Fr, 1e-10, "F against numpy")
    assert_close(npy(f), fr, 1e-10, "f against numpy")
    assert_close(npy(F), npy(Fa), 1e-10, "F against autograd")
    assert_close(npy(f), npy(fa), 1e-10, "f against autograd")
    with torch.no_grad():
        F0, f0 = m.linearize(x, u)
    assert torch.equal(F0, F) and torch.equal(f0, f.detach())
    assert linearize_dynamics(x, u, m)[1].requires_grad       # the hook `linearize_dynamics` looks for


@pytest.mark.parametrize("case", CASES)
def test_parameter_gradients_agree_between_the_two_routes(case):
    m, net, x, u = _iterate(case)
    g = torch.as_tensor(np.random.RandomState(case[5] + 30).randn(case[4] - 1, case[3], case[0]))
    params = [m.W1, m.b1, m.W2, m.b2]
    own = torch.autograd.grad((m.linearize(x, u)[1] * g).sum(), params)
    auto = torch.autograd.grad((linearize_dynamics(x, u, lambda a, b: m(a, b))[1] * g).sum(), params)
    for name, a, b in zip(("W1", "b1", "W2", "b2"), own, auto):
        assert float(b.abs().max()) > 0
        assert_close(npy(a), npy(b), 1e-10, "d/d" + name)


def test_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.load()
    for name in ("dmpc_mlp_dx_supported", "dmpc_mlp_rollout_linearize", "dmpc_mpc_forward_rec_mlp"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)       # a non-NULL pointer: the size checks come before anything reads it

    def rollout(nx, nu, H, act, ptr=p, T=2, B=1):
        return lib.dmpc_mlp_rollout_linearize(T, B, nx, nu, H, act, 1, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, None)

    def search(nx, nu, H, act, ptr=p, T=2, B=1):
        return lib.dmpc_mpc_forward_rec_mlp(T, B, nx, nu, H, act, 1, *([ptr] * 12), 0.2, 10, *([ptr] * 9), None)

    for nx, nu, H, act in ((17, 1, 5, 0), (3, 9, 5, 0), (3, 1, 257, 0), (3, 1, 0, 0), (3, 1, 5, 1)):
        assert rollout(nx, nu, H, act) == _lib.E_UNSUPPORTED
        assert search(nx, nu, H, act) == _lib.E_UNSUPPORTED
        assert lib.dmpc_mlp_dx_supported(nx, nu, H, act) == 0
    for nx, nu, H in ((3, 1, 5), (16, 8, 256), (1, 1, 1)):
        assert lib.dmpc_mlp_dx_supported(nx, nu, H, 0) == 1
        assert rollout(nx, nu, H, 0, ptr=None) == _lib.E_BADARG
        assert search(nx, nu, H, 0, ptr=None) == _lib.E_BADARG
    assert rollout(3, 1, 5, 0, T=0) == _lib.E_BADARG and rollout(3, 1, 5, 0, B=0) == _lib.E_BADARG
    assert rollout(0, 1, 5, 0) == _lib.E_BADARG and rollout(3, 0, 5, 0) == _lib.E_BADARG
    assert search(3, 1, 5, 0, T=1) == _lib.E_BADARG          # no dynamics step to search over, as dmpc_mpc_forward_rec
    assert lib.dmpc_version() == _lib.ABI_VERSION == 411


def test_fused_ok_is_false_on_the_cpu_and_when_a_gradient_is_wanted():
    m = MlpDx(3, 1, 5, seed=0)
    x0, u = torch.zeros(2, 3), torch.zeros(4, 2, 1)
    assert not m.fused_ok(x0, u)
    with torch.no_grad():
        assert not m.fused_ok(x0, u)                          # CPU tensors, whatever the grad mode
    assert all(p.requires_grad for p in m.parameters()) and m._grad_wanted(x0, u)
    with torch.no_grad():
        assert not m._grad_wanted(x0, u)
    m.requires_grad_(False)
    assert not m._grad_wanted(x0, u) and m._grad_wanted(x0.clone().requires_grad_(True), u)
    assert m.supported() and not MlpDx(3, 1, 300).supported()


def test_seed_makes_the_initial_weights_reproducible():
    a, b = MlpDx(4, 2, 7, seed=3), MlpDx(4, 2, 7, seed=3)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert tuple(a.W1.shape) == (7, 6) and tuple(a.b1.shape) == (7,) and tuple(a.W2.shape) == (4, 7) and tuple(a.b2.shape) == (4,)
