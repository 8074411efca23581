"""GPU: MPC with tiled dynamics - `dmpc_mpc_step_backward_shared` through `tiled_dynamics_gradient`, one
case per co-state kernel, against the float64 oracle's MPCstep.backward summed over (t, b) on the host; the reduction's tile
and chunk edges; bit-reproducibility; `BoxDDP` + `TiledLinDx`, `MpcNet_dx(shared=True)` and `mpc_exp` against the reference's
recorded experiment (tests/golden/mpcnet_experiment.npz) and against the dense route."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import BoxDDP, LinDx, MpcNet_dx, QuadCost, TiledLinDx, synthetic
from chainer_differentiable_mpc_amd.mpc_step import tiled_dynamics_gradient
from oracle import mpc as ompc
from tests.helpers import GOLDEN, TOL_COSTATE, TOL_PRIMAL, assert_close, npy

pytestmark = pytest.mark.gpu

BOUND = 0.25


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(a, dtype=dtype, device="cuda")


@functools.lru_cache(maxsize=None)
def problem(T, B, nx, nu, f_slices=None, seeded_rows=None):
    """hand-built inputs of MPCstep.backward with F_hat the tile of one [A|B]: per-trajectory C, c (synthetic), u random in the
    box with ~30 % of its entries exactly on it, x finite, random incoming gradients (nonzero on `seeded_rows` only when given);
    float32-representable float64 arrays, and the oracle's gradient at them (computed once per case)"""
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=100 + T + 7 * B + 31 * nx + nu, with_f=False)
    rng = np.random.RandomState(1000 + B + nx)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)      # noqa: E731
    nF = (T - 1) if f_slices is None else f_slices
    F = np.ascontiguousarray(np.broadcast_to(p["F"][0, 0], (nF, B, nx, nx + nu)))
    u = r32(rng.uniform(-0.9 * BOUND, 0.9 * BOUND, size=(T, B, nu)))
    on = rng.rand(T, B, nu)
    u[on < 0.15] = -BOUND
    u[on > 0.85] = BOUND
    x = r32(rng.randn(T, B, nx))
    gx, gu = r32(rng.randn(T, B, nx)), r32(rng.randn(T, B, nu))
    if seeded_rows is not None:
        keep = np.zeros(B)
        keep[list(seeded_rows)] = 1.0
        gx, gu = gx * keep[None, :, None], gu * keep[None, :, None]
    lo, hi = np.full((T, B, nu), -BOUND), np.full((T, B, nu), BOUND)
    ref = ompc.mpc_backward(x[0], p["C"], p["c"], F, np.zeros((T - 1, B, nx)), x, u, lo, hi, gx, gu, T, nx, nu)
    return dict(C=p["C"], c=p["c"], F=F, x=x, u=u, gx=gx, gu=gu, lo=lo, hi=hi, dx0=ref[0], dF=ref[3][:T - 1], df=ref[4])


def gradient(T, B, nx, nu, q, **kw):
    r = dict(C=dev(q["C"]), c=dev(q["c"]), F=dev(q["F"]), x=dev(q["x"]), u=dev(q["u"]))
    return tiled_dynamics_gradient(T, B, nx, nu, torch.device("cuda", 0), r, dev(q["lo"]), dev(q["hi"]), dev(q["gx"]),
                                   dev(q["gu"]), **kw)


# one case per co-state kernel `launch_costate` can pick (kkt_api.hip)
KERNEL_CASES = [(4, 8, 3, 1),      # 16-lane LDS-DMA
                (4, 6, 3, 1),      # ragged: costate_kernel<3,1,16>
                (5, 8, 3, 3),      # padded 16-lane container
                (3, 8, 8, 2),      # LDS-DMA
                (3, 8, 12, 8),     # wide, exact
                (3, 8, 9, 4),      # wide, padded
                (3, 5, 14, 6),     # (16,8) three-wave instance or its ragged fallback
                (3, 3, 20, 6),     # staged
                (3, 4, 32, 8),     # 64-lane
                (2, 4, 3, 1)]      # one F only


@pytest.mark.parametrize("T,B,nx,nu", KERNEL_CASES)
def test_gradient_against_the_oracle_per_costate_kernel(T, B, nx, nu):
    q = problem(T, B, nx, nu)
    dx0, dAB, df0 = gradient(T, B, nx, nu, q, want_df=True)
    assert tuple(dAB.shape) == (nx, nx + nu) and tuple(df0.shape) == (nx,)
    assert_close(npy(dAB), q["dF"].sum(axis=(0, 1)), TOL_COSTATE, "dAB")
    assert_close(npy(df0), q["df"].sum(axis=(0, 1)), TOL_COSTATE, "df0")
    assert_close(npy(dx0), q["dx0"], TOL_COSTATE, "dx_init")


def test_gradient_keeps_the_time_axis_when_the_layout_says_so():
    T, B, nx, nu = 4, 8, 3, 1
    q = problem(T, B, nx, nu)
    dx0, dAB, df0 = gradient(T, B, nx, nu, q, time_axis=True, want_df=True, f_time_axis=True)
    assert tuple(dAB.shape) == (T - 1, nx, nx + nu) and tuple(df0.shape) == (T - 1, nx)
    assert_close(npy(dAB), q["dF"].sum(axis=1), TOL_COSTATE, "dAB [T-1,nx,ns]")
    assert_close(npy(df0), q["df"].sum(axis=1), TOL_COSTATE, "df0 [T-1,nx]")
    assert_close(npy(dx0), q["dx0"], TOL_COSTATE, "dx_init")


def test_gradient_with_T_slices_of_F():
    T, B, nx, nu = 4, 6, 3, 1
    q = problem(T, B, nx, nu, f_slices=T)
    assert q["F"].shape[0] == T
    dx0, dAB, df0 = gradient(T, B, nx, nu, q)
    assert df0 is None
    assert_close(npy(dAB), q["dF"].sum(axis=(0, 1)), TOL_COSTATE, "dAB")
    assert_close(npy(dx0), q["dx0"], TOL_COSTATE, "dx_init")


def test_unsupported_size_returns_none():
    T, B, nx, nu = 3, 4, 40, 4
    z = lambda *s: torch.zeros(s, device="cuda")      # noqa: E731
    r = dict(C=z(T, B, nx + nu, nx + nu), c=z(T, B, nx + nu), F=z(T - 1, B, nx, nx + nu), x=z(T, B, nx), u=z(T, B, nu))
    assert tiled_dynamics_gradient(T, B, nx, nu, torch.device("cuda", 0), r, z(T, B, nu) - 1, z(T, B, nu) + 1, z(T, B, nx),
                                   z(T, B, nu)) is None


EDGE_ROWS = (0, 63, 64, 1023, 1024, 1090)


def test_reduction_tile_and_chunk_edges():
    """B = 1091: the reduction tiles 64 trajectories and chunks 1,024.  Gradient seeds on the six trajectories at those edges
    only - a dropped or doubled trajectory is a sixth of the signal."""
    T, B, nx, nu = 3, 1091, 3, 1
    q = problem(T, B, nx, nu, seeded_rows=EDGE_ROWS)
    rows = list(EDGE_ROWS)
    others = np.setdiff1d(np.arange(B), rows)
    assert np.abs(q["dF"][:, others]).max() == 0.0 and np.abs(q["dF"][:, rows]).sum(axis=(0, 2, 3)).min() > 1e-2
    dx0, dAB, df0 = gradient(T, B, nx, nu, q, want_df=True)
    assert_close(npy(dAB), q["dF"][:, rows].sum(axis=(0, 1)), TOL_COSTATE, "dAB over the six edge trajectories")
    assert_close(npy(df0), q["df"][:, rows].sum(axis=(0, 1)), TOL_COSTATE, "df0 over the six edge trajectories")
    assert_close(npy(dx0), q["dx0"], TOL_COSTATE, "dx_init")


@pytest.mark.parametrize("T,B,nx,nu", [(3, 1091, 3, 1), (5, 128, 3, 3)])
def test_gradient_is_bit_reproducible(T, B, nx, nu):
    q = problem(T, B, nx, nu)
    a = gradient(T, B, nx, nu, q, want_df=True)
    a = [t.clone() for t in a]
    b = gradient(T, B, nx, nu, q, want_df=True)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


@pytest.mark.parametrize("tag", ["wide", "tight"])
def test_the_reference_mpcnet_experiment_with_shared_dynamics(tag):
    """experiment_mpc/MpcNet.py at its own sizes, as test_box_ddp_gpu.py's first-training-iteration test, with
    `MpcNet_dx(shared=True)`: solutions, loss, d loss / d(A, B) against the unmodified reference's; three forward + backward
    calls on the same tensors each leave a gradient, bit for bit the same one"""
    g = np.load(os.path.join(GOLDEN, "mpcnet_experiment.npz"))
    T, B, nx, nu = int(g["T"]), int(g["B"]), int(g["nx"]), int(g["nu"])
    ns, bound = nx + nu, float(g[tag + "_bound"])
    lo, hi = torch.full((T, B, nu), -bound, dtype=torch.float64), torch.full((T, B, nu), bound, dtype=torch.float64)
    net = MpcNet_dx(T, lo, hi, B, nx, nu, 1, u_init=None, max_iter=10, quiet=True, shared=True).cuda()
    np.testing.assert_array_equal(npy(net.A), g[tag + "_A0"])
    np.testing.assert_array_equal(npy(net.B), g[tag + "_B0"])
    C = dev(np.tile(np.eye(ns), (T, B, 1, 1)), torch.float64)
    c = dev(np.tile(g[tag + "_p"], (T, B, 1)), torch.float64)
    F_exp = dev(np.tile(np.concatenate((g[tag + "_A_exp"], g[tag + "_B_exp"]), axis=1), (T - 1, B, 1, 1)), torch.float64)
    f_exp = torch.zeros((T - 1, B, nx), dtype=torch.float64, device="cuda")
    x_init = dev(g[tag + "_x_init"], torch.float64)
    cost = QuadCost(C, c)
    grads = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.no_grad():
            expert = BoxDDP(T, lo, hi, B, nx, nu, None, quiet=True)
            x_true, u_true, _ = expert((x_init, cost, LinDx(F_exp, f_exp)))
        for call in range(3):
            net.zero_grad(set_to_none=True)
            x_pred, u_pred, _ = net((x_init, cost))
            assert x_pred.grad_fn is not None and u_pred.grad_fn is not None, "call %d came back without a graph" % call
            loss = ((u_true - u_pred) ** 2).mean() + ((x_true - x_pred) ** 2).mean()
            loss.backward()
            assert net.A.grad is not None and net.B.grad is not None
            grads.append((net.A.grad.clone(), net.B.grad.clone()))
    assert expert.status == "Converged" and net.mpc_layer.status == "Converged"
    assert_close(npy(x_true), g[tag + "_x_true"], TOL_PRIMAL, "expert x")
    assert_close(npy(u_true), g[tag + "_u_true"], TOL_PRIMAL, "expert u")
    assert_close(npy(x_pred), g[tag + "_x_pred"], TOL_PRIMAL, "learner x")
    assert_close(npy(u_pred), g[tag + "_u_pred"], TOL_PRIMAL, "learner u")
    assert_close(float(loss.detach()), float(g[tag + "_loss"]), TOL_PRIMAL, "loss")
    assert_close(npy(grads[0][0]), g[tag + "_gA"], TOL_COSTATE, "d loss / dA")
    assert_close(npy(grads[0][1]), g[tag + "_gB"], TOL_COSTATE, "d loss / dB")
    for gA, gB in grads[1:]:
        assert torch.equal(gA, grads[0][0]) and torch.equal(gB, grads[0][1])


def test_recorded_chain_replays_and_still_leaves_a_gradient():
    """float32 tensors, the same ones every call: BoxDDP records its chain at the second call and replays it from the third;
    the leaves of a `TiledLinDx` are AB / f0, so the replay shortcut must not hand back a graph-less result"""
    T, B, nx, nu = 5, 8, 3, 2
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=17)
    AB = dev(p["F"][0, 0]).requires_grad_(True)
    solver = BoxDDP(T, -BOUND, BOUND, B, nx, nu, None, max_iter=12, quiet=True)
    cost, x0 = QuadCost(dev(p["C"]), dev(p["c"])), dev(p["x_init"])
    dyn = TiledLinDx(AB, None, T, B)
    grads = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for call in range(4):
            AB.grad = None
            x, u, _ = solver((x0, cost, dyn))
            assert x.grad_fn is not None, "call %d came back without a graph" % call
            (x.sum() + (u * u).sum()).backward()
            grads.append(AB.grad.clone())
    assert any(e[0] is not None for e in solver._graphs.values()), "the chain was never recorded"
    for g_ in grads[1:]:
        assert torch.equal(g_, grads[0])
    with torch.no_grad():        # nothing to differentiate: the shortcut may serve this call
        x2, u2, _ = solver((x0, cost, dyn))
    assert torch.equal(x2, x.detach()) and torch.equal(u2, u.detach())


def _mpcnet_grads(shared, max_iter, detach_unconverged=True):
    T, B, nx, nu = 5, 6, 3, 2
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=17)
    lo, hi = torch.full((T, B, nu), -BOUND), torch.full((T, B, nu), BOUND)
    net = MpcNet_dx(T, lo, hi, B, nx, nu, seed=1, u_init=None, max_iter=max_iter, quiet=True, shared=shared).cuda()
    net.mpc_layer.detach_unconverged = detach_unconverged
    C, c, x0 = dev(p["C"], torch.float64), dev(p["c"], torch.float64), dev(p["x_init"], torch.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, u, _ = net((x0, QuadCost(C, c)))
    w_x = torch.linspace(-1, 1, x.numel(), device="cuda", dtype=x.dtype).reshape(x.shape)
    # one scalar per trajectory, so that a detached trajectory shows as a missing term of the parameter gradient
    per_b = (w_x * x).sum(dim=(0, 2)) + u.sum(dim=(0, 2))
    per_b.sum().backward()
    return net, npy(x), npy(u), npy(torch.cat((net.A.grad, net.B.grad), dim=1))


def test_shared_against_dense():
    """the setting of test_mpcnet_gradient_flows_to_dynamics_parameters: both routes' A.grad, B.grad agree; a solve cut short by
    max_iter=1 detaches the same trajectories in both (the dense route decides on the host, the shared one on the device)"""
    _, xs, us, gs = _mpcnet_grads(True, 12)
    _, xd, ud, gd = _mpcnet_grads(False, 12)
    np.testing.assert_array_equal(xs, xd)
    np.testing.assert_array_equal(us, ud)
    assert np.abs(gd).max() > 0
    assert_close(gs, gd, TOL_COSTATE, "d(A|B), shared vs dense")
    for max_iter in (1, 2):      # (both short of a fixed point; which rows the mask keeps is the loop's own norm's business)
        net_s, _, _, gs1 = _mpcnet_grads(True, max_iter)
        net_d, _, _, gd1 = _mpcnet_grads(False, max_iter)
        assert_close(gs1, gd1, TOL_COSTATE, "d(A|B) of a solve cut short by max_iter=%d, shared vs dense" % max_iter)
        if max_iter == 1:
            assert net_d.mpc_layer.status != "Converged" and net_s.mpc_layer.status != "Converged"
            _, _, _, g_all = _mpcnet_grads(True, max_iter, detach_unconverged=False)
            assert np.abs(g_all - gs1).max() > 1e-3, "nothing was unconverged: the detach mask was not exercised"


def test_solve_and_gradient_capture_in_a_graph():
    """`torch.cuda.graph` around forward + backward of BoxDDP(lazy_status=True, detach_unconverged=True) with a `TiledLinDx`:
    the detach mask is applied on the device, so nothing in the chain needs the host; the replay's gradient is the eager one.
    Half of the trajectories stay far inside the box (small c, x_init): there the model is an unconstrained LQR, which the
    second iteration leaves unchanged; the others run into the box and are still moving when max_iter = 2 cuts the solve short.
    The loop's norm is the reference's (mpc_step.py:261-263: [T,nu,B] reshaped to [B, T*nu]), so row r holds the steps of
    trajectories (r % 2) * 10 ... + 9 at B = 20, T * nu = 10: even rows see the quiet half alone and pass the gate, odd rows
    do not - the gate is live and keeps some trajectories (both checked on the eager solve's own device flags)"""
    T, B, nx, nu = 5, 20, 3, 2
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=17)
    p["c"][:, :B // 2] *= 0.02
    p["x_init"][:B // 2] *= 0.02
    AB = dev(p["F"][0, 0]).requires_grad_(True)
    cost, x0 = QuadCost(dev(p["C"]), dev(p["c"])), dev(p["x_init"])
    dyn = TiledLinDx(AB, None, T, B)
    out = torch.zeros_like(AB)
    gate = []

    def step(solver):
        x, u, _ = solver((x0, cost, dyn))
        gate.append(x.grad_fn.spec[7])       # (du_norm_last [B], the loop's flag, eps) as the gradient node holds them
        g_, = torch.autograd.grad(x.sum() + (u * u).sum(), AB)
        out.copy_(g_)

    lo, hi = torch.full((T, B, nu), -BOUND, device="cuda"), torch.full((T, B, nu), BOUND, device="cuda")

    def make():
        return BoxDDP(T, lo, hi, B, nx, nu, None, max_iter=2, quiet=True, lazy_status=True, detach_unconverged=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):       # warm-up on a side stream (allocations, library load); also the eager result
            step(make())
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        eager = out.clone()
        norms, flag, eps = gate[0]
        kept = int((norms < eps).sum())
        assert int(flag) != 0 and 0 < kept < B, "the detach gate is not exercised: %d of %d trajectories kept" % (kept, B)
        assert float(eager.abs().max()) > 0
        out.zero_()
        solver = make()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step(solver)
        assert solver._pending is None
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_mpc_exp_driver(tmp_path):
    """`mpc_exp` with the experiment's defaults: the first row is the reference's first training iteration (the golden's
    `wide_loss`), three finite rows in the CSV, and the dense route gives the same first row"""
    from chainer_differentiable_mpc_amd import mpc_exp
    g = np.load(os.path.join(GOLDEN, "mpcnet_experiment.npz"))
    rows = mpc_exp.run(iters=3, train_seed=1, save_dir=str(tmp_path / "shared"))
    assert_close(rows[0][0], float(g["wide_loss"]), TOL_PRIMAL, "im_loss of the first iteration")
    with open(str(tmp_path / "shared" / "1_new_losses.csv")) as fh:
        lines = fh.read().strip().split("\n")
    assert lines[0] == "im_loss,mse" and len(lines) == 4
    table = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert table.shape == (3, 2) and np.isfinite(table).all()
    np.testing.assert_allclose(table, np.array(rows), rtol=0, atol=0)
    dense = mpc_exp.run(iters=1, train_seed=1, dense=True, save_dir=str(tmp_path / "dense"))
    assert_close(dense[0][0], rows[0][0], TOL_PRIMAL, "im_loss, dense vs shared")
    assert_close(dense[0][1], rows[0][1], TOL_PRIMAL, "mse after the first update, dense vs shared")
