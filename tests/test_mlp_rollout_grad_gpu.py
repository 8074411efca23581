"""GPU: `MlpDx.rollout` with `param_grad="device"` - ONE autograd node whose forward is the rollout's launch and whose backward
is `dmpc_mlp_rollout_grad` (include/dmpc_mlp_rollout_grad.h: a reverse sweep that carries the co-state, then the weight gradient's
fixed-order reduction) - and `prediction_loss` on top, against float64 torch autograd of the live torch loop on the CPU at
TOL_COSTATE.  Inputs and reference: tests/mlp_rollout_grad_cases.py.

Calibration on the CPU at exactly these cases: float32 autograd of the same loss is within 2.8e-6 of float64 for every gradient
and 4.1e-7 for the states, max |ref| up to 112.  relu: a case runs only where the float64 rollout stays KINK_MARGIN away from a
kink (the margin functions of the weight-gradient tests)."""
import warnings

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import ClosedLoop, MlpDx, _lib
from tests import mlp2_grad_cases, mlp_rollout_grad_cases as rc
from tests.helpers import TOL_COSTATE, assert_close, npy
from tests.test_mlp_dx_grad_gpu import walk_case as walk_one

pytestmark = pytest.mark.gpu

ONE, TWO = rc.ONE, rc.TWO
REDUCE = {1: "mlp_param_grad_reduce_kernel", 2: "mlp2_param_grad_reduce_kernel"}
SMOOTH = ("silu", "softplus")
ACT_ONE = [(a, c) for a in SMOOTH + ("relu",) for c in ONE[:3] if a != "relu" or rc.margin(a, c) >= rc.KINK_MARGIN]
ACT_TWO = [("tanh", k) for k in mlp2_grad_cases.GRAD_CASES] + \
    [(a, k) for a in SMOOTH + ("relu",) for k in mlp2_grad_cases.OTHER_CASES if a != "relu" or rc.margin(a, TWO[k]) >= rc.KINK_MARGIN]


def dev(a, dtype=torch.float32):
    return torch.as_tensor(a, dtype=dtype, device="cuda")


def device_run(activation, case, residual=True, **kw):
    m = rc.model(activation, case, "cuda", torch.float32, residual, param_grad="device")
    return m, rc.run(m, case, "cuda", torch.float32, **kw)


def check(got, ref, case):
    """weights, x_init and u at TOL_COSTATE; the states too; d_u[T-1] exactly zero"""
    for name in rc.names(case) + ("x_init", "u"):
        assert tuple(got[name].shape) == ref[name].shape, name
        assert_close(npy(got[name]), ref[name], TOL_COSTATE, "d/d" + name)
    for name in rc.names(case):
        assert float(np.abs(ref[name]).max()) > 0, name
    assert_close(npy(got["x"]), ref["x"], TOL_COSTATE, "x")
    assert not bool(got["u"][-1].any())


def check_states_are_the_rollouts(m, got, case):
    x_init, u, _ = (dev(a) for a in rc.inputs(case))
    with torch.no_grad():
        x, _, _ = m.rollout_linearize(x_init, u)
        assert torch.equal(m.rollout(x_init, u), x)          # the route without a gradient
    assert torch.equal(got["x"], x)


@pytest.mark.parametrize("case", ONE)
def test_depth_one_against_float64_autograd(case):
    """odd H < 64 with a ragged workgroup; one unit per lane; several units per lane; every limit; B = 1 with T = 2"""
    m, got = device_run("tanh", case)
    check(got, rc.reference("tanh", case), case)
    check_states_are_the_rollouts(m, got, case)


@pytest.mark.parametrize("activation,key", ACT_TWO, ids=["%s-%s" % ak for ak in ACT_TWO])
def test_depth_two_against_float64_autograd(activation, key):
    case = TWO[key]
    if activation == "relu":
        assert rc.margin("relu", case) >= rc.KINK_MARGIN
    m, got = device_run(activation, case)
    check(got, rc.reference(activation, case), case)
    check_states_are_the_rollouts(m, got, case)


def test_every_depth_two_case_of_the_weight_gradient_tests_runs_here():
    assert [k for a, k in ACT_TWO if a == "tanh"] == list("ACDEF")
    assert all((a, k) in ACT_TWO for a in SMOOTH for k in "AC")


@pytest.mark.parametrize("activation,case", ACT_ONE, ids=["%s-%d" % (a, ONE.index(c)) for a, c in ACT_ONE])
def test_depth_one_with_the_other_activations(activation, case):
    m, got = device_run(activation, case)
    check(got, rc.reference(activation, case), case)
    check_states_are_the_rollouts(m, got, case)


@pytest.mark.parametrize("case", [ONE[2], TWO["C"]], ids=["one", "two"])
def test_without_the_residual(case):
    _, got = device_run("tanh", case, residual=False)
    ref = rc.reference("tanh", case, residual=False)
    check(got, ref, case)
    assert float(np.abs(ref["x"] - rc.reference("tanh", case)["x"]).max()) > 0.1        # another model than the residual one


@pytest.mark.parametrize("which", ["one", "two"])
def test_a_wavefront_or_workgroup_that_walks_more_than_one(which):
    """B just above the partial caps the library names: (3,1), T = 3"""
    lib = _lib.load()
    case = walk_one() if which == "one" else mlp2_grad_cases.walk_case()
    B = rc.dims(case)[2]
    m = rc.model("tanh", case)
    if which == "one":
        assert lib.dmpc_mlp_rollout_grad_partials(B, m.hidden_code) == lib.dmpc_mlp_param_grad_partials(B) == B - 3
    else:
        assert lib.dmpc_mlp_rollout_grad_partials(B, m.hidden_code) == lib.dmpc_mlp2_param_grad_partials(B) == (B - 5) // 4
    _, got = device_run("tanh", case)
    check(got, rc.reference("tanh", case), case)


@pytest.mark.parametrize("which", ["one, several units per lane", "one, walk", "two, two units per lane", "two, walk"])
def test_two_calls_give_the_same_bits(which):
    case = {"one, several units per lane": ONE[2], "one, walk": walk_one(), "two, two units per lane": TWO["C"],
            "two, walk": mlp2_grad_cases.walk_case()}[which]
    _, one = device_run("tanh", case)
    _, two = device_run("tanh", case)
    for k in one:
        assert torch.equal(one[k], two[k]), k


@pytest.mark.parametrize("case", [ONE[0], ONE[1], TWO["A"], TWO["C"]], ids=["one-0", "one-1", "two-A", "two-C"])
def test_a_trajectory_does_not_depend_on_its_batch(case):
    """d_x_init[b] and d_u[:, b] of the batch equal the same trajectory run alone, bit for bit"""
    nx, nu, B, T, s = rc.dims(case)
    m, got = device_run("tanh", case)
    x_init, u, g = (dev(a) for a in rc.inputs(case))
    for b in range(B):
        xb, ub = x_init[b:b + 1].clone().requires_grad_(True), u[:, b:b + 1].clone().requires_grad_(True)
        x = m.rollout(xb, ub)
        dx, du = torch.autograd.grad((x * g[:, b:b + 1]).sum(), [xb, ub])
        assert torch.equal(x[:, 0], got["x"][:, b]), b
        assert torch.equal(dx[0], got["x_init"][b]) and torch.equal(du[:, 0], got["u"][:, b]), b


@pytest.mark.parametrize("case", [ONE[0], TWO["A"]], ids=["one", "two"])
def test_a_single_state(case):
    """T = 1: no sweep; zeros for the weights and u, d_x_init = grad_x[0]"""
    nx, nu, B, T, s = rc.dims(case)
    m = rc.model("tanh", case, "cuda", param_grad="device")
    x_init, u, g = (dev(a) for a in rc.inputs(case))
    x_init.requires_grad_(True)
    u1 = u[:1].clone().requires_grad_(True)
    x = m.rollout(x_init, u1)
    assert tuple(x.shape) == (1, B, nx) and torch.equal(x[0], x_init)
    grads = torch.autograd.grad((x * g[:1]).sum(), list(m._weights()) + [x_init, u1])
    assert all(not bool(gr.any()) and gr.shape == p.shape for gr, p in zip(grads, m._weights()))
    assert torch.equal(grads[-2], g[0]) and not bool(grads[-1].any()) and tuple(grads[-1].shape) == (1, B, nu)


@pytest.mark.parametrize("case", [ONE[2], TWO["C"]], ids=["one", "two"])
def test_a_loss_of_the_first_state_alone(case):
    """grad_x non-zero in row 0 only: nothing to carry - d_x_init = grad_x[0] exactly and zero weight gradients"""
    g = np.array(rc.inputs(case)[2])
    g[1:] = 0.0
    _, got = device_run("tanh", case, g=g)
    assert torch.equal(got["x_init"], dev(g[0]))
    for name in rc.names(case) + ("u",):
        assert not bool(got[name].any()), name


@pytest.mark.parametrize("case", [ONE[0], TWO["A"]], ids=["one", "two"])
def test_u_with_one_row_less(case):
    T = rc.dims(case)[3]
    _, full = device_run("tanh", case)
    _, short = device_run("tanh", case, u_rows=T - 1)
    assert tuple(short["u"].shape) == (T - 1,) + tuple(full["u"].shape[1:]) and torch.equal(short["u"], full["u"][:-1])
    for k in full:
        if k != "u":
            assert torch.equal(short[k], full[k]), k


def test_a_weight_changed_in_place_before_the_backward_is_an_autograd_error():
    case = ONE[0]
    m = rc.model("tanh", case, "cuda", param_grad="device")
    x_init, u, g = (dev(a) for a in rc.inputs(case))
    x = m.rollout(x_init, u)
    with torch.no_grad():
        m.W1.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        (x * g).sum().backward()


# ---- prediction_loss
@pytest.mark.parametrize("horizon", [1, 3, None])
@pytest.mark.parametrize("n_hidden", rc.FIT_NETS, ids=["one", "two"])
def test_prediction_loss_on_pendulum_records(n_hidden, horizon):
    """the value and its weight gradient against float64 on the CPU; the backward is the device node's (its reduction ran last)"""
    x, u = rc.pendulum_record()
    ref_m = rc.fit_model(n_hidden, "cpu", torch.float64)
    ref = ref_m.prediction_loss(torch.as_tensor(x), torch.as_tensor(u), horizon=horizon)
    ref_g = torch.autograd.grad(ref, list(ref_m._weights()))
    m = rc.fit_model(n_hidden, "cuda", param_grad="device")
    names = []
    m.W1.register_hook(lambda g: names.append(_lib.last_kernel_name()))
    loss = m.prediction_loss(dev(x), dev(u), horizon=horizon)
    got_g = torch.autograd.grad(loss, list(m._weights()))
    assert len(names) == 1 and REDUCE[m.depth] in names[0], names
    assert_close(npy(loss), npy(ref), TOL_COSTATE, "prediction_loss")
    for i, (a, b) in enumerate(zip(got_g, ref_g)):
        assert float(b.abs().max()) > 0
        assert_close(npy(a), npy(b), TOL_COSTATE, "d loss / d weight %d" % i)
    live = rc.fit_model(n_hidden, "cuda")
    assert_close(npy(live.prediction_loss(dev(x), dev(u), horizon=horizon)), npy(ref), TOL_COSTATE, "prediction_loss, live route")


@pytest.mark.parametrize("n_hidden", rc.FIT_NETS, ids=["one", "two"])
def test_five_sgd_steps_on_pendulum_records(n_hidden):
    """plain SGD, horizon 4, lr 0.05, on the device route: the weights follow the float64 CPU live route and the loss at least
    halves.  Float64 here: 0.734 -> 0.064 with one hidden layer, 1.316 -> 0.156 with two; float32 live weights within 5.3e-8."""
    x, u = rc.pendulum_record()
    ref_w, ref_losses = rc.sgd_reference(n_hidden)
    assert ref_losses[-1] <= 0.5 * ref_losses[0]
    m = rc.fit_model(n_hidden, "cuda", param_grad="device")
    losses = rc.sgd(m, dev(x), dev(u))
    print("losses", losses)
    for i, (p, w) in enumerate(zip(m._weights(), ref_w)):
        assert_close(npy(p), w, TOL_COSTATE, "weight %d after %d steps" % (i, rc.FIT_STEPS))
    assert_close(np.array(losses), np.array(ref_losses), TOL_COSTATE, "losses")
    assert losses[-1] <= 0.5 * losses[0]


def test_closed_loop_logs_go_straight_in():
    """`EpisodeOut.x` [n+1,B,nx] and `EpisodeOut.u` [n,B,nu] of a short (3,1) episode, as they are"""
    from tests.test_episode_gpu import loop_objects, run_loop
    solver, plant, x0, cost, model = loop_objects("mlp_small")
    out = run_loop(ClosedLoop(solver, plant, 2), x0, cost, model)
    assert out.x.shape[0] == 3 and out.u.shape[0] == 2 and out.x.is_cuda
    m = MlpDx(3, 1, 5, seed=0, param_grad="device").cuda()
    names = []
    m.W1.register_hook(lambda g: names.append(_lib.last_kernel_name()))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loss = m.prediction_loss(out.x, out.u)
        loss.backward()
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0
    assert len(names) == 1 and REDUCE[1] in names[0], names
    for p in m._weights():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
