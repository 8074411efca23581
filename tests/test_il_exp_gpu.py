"""GPU: the imitation-learning driver `IL_Exp` (env_dx/il_exp.py) and its device update - `dmpc_il_param_step` through
the C-ABI against torch autograd + torch.optim.RMSprop, the device update against the reference's own three-update loop
(tests/golden/imitation_loop_16.npz) and against the torch route (`device_update=False`) for all four cost nets, the files
`run()` writes, and an update that makes no host synchronisation."""
import csv
import os
import warnings

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import IL_Env, IL_Exp, _lib, make_dataset
from chainer_differentiable_mpc_amd.il_exp import ALPHA, EPS, GROUP_BITS, LR
from chainer_differentiable_mpc_amd.pendulum_net import NETS
from tests.helpers import GOLDEN, assert_close

pytestmark = pytest.mark.gpu

NAMES = ("learn_q_logit", "learn_p", "lower_without_diag")


def npy(t):
    return t.detach().cpu().numpy().astype(np.float64)


def rel(got, ref):
    got, ref = npy(got).reshape(-1), npy(ref).reshape(-1)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


@pytest.fixture(scope="module")
def small_data(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("il") / "pendulum.pkl")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        make_dataset.main(48, 16, 16, path=path, lqr_iter=50)
    return path


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("mask", [7, 2, 5])
def test_param_step_matches_autograd_and_rmsprop(kind, mask):
    """chain rule (sigmoid, sqrt, L L^T, O^T . O) + RMSprop of one workgroup against autograd through the net and
    torch.optim.RMSprop(lr=1e-2, alpha=0.5, eps=1e-8); a disabled group keeps its parameters and state bit for bit"""
    torch.manual_seed(kind * 10 + mask)
    net = NETS[kind](4, device="cuda")
    names = [n for n in NAMES if hasattr(net, n)]
    with torch.no_grad():
        for n in names:
            getattr(net, n).copy_(torch.randn_like(getattr(net, n)))
    dQ, dp = torch.randn(4, 4, device="cuda"), torch.randn(4, device="cuda")
    ms0 = {n: torch.rand_like(getattr(net, n)) for n in names}
    theta = torch.cat([getattr(net, n).detach().reshape(-1) for n in names]).clone()
    ms = torch.cat([ms0[n].reshape(-1) for n in names]).clone()
    grad = torch.full_like(theta, float("nan"))
    before_theta, before_ms = theta.clone(), ms.clone()
    lib = _lib.load()
    assert lib.dmpc_il_n_params(kind, 4) == theta.numel()
    rc = lib.dmpc_il_param_step(kind, 4, _lib.ptr(dQ), _lib.ptr(dp), _lib.ptr(theta), _lib.ptr(ms), _lib.ptr(grad), mask,
                                LR, ALPHA, EPS, _lib.stream_ptr(theta.device))
    _lib.check(rc, "dmpc_il_param_step")
    # the yardstick: autograd + torch's RMSprop with the same state
    opt = torch.optim.RMSprop([getattr(net, n) for n in names], lr=LR, alpha=ALPHA, eps=EPS)
    for n in names:
        opt.state[getattr(net, n)] = {"step": torch.tensor(0.0), "square_avg": ms0[n].clone()}
    Q, p = net.cost_map()
    ((Q * dQ).sum() + (p * dp).sum()).backward()
    ref_grad = torch.cat([getattr(net, n).grad.reshape(-1) for n in names])
    for n in names:
        if not mask & GROUP_BITS[n]:
            getattr(net, n).grad = None
    opt.step()
    torch.cuda.synchronize()
    assert rel(grad, ref_grad) <= 1e-6, (grad, ref_grad)
    off = 0
    for n in names:
        prm = getattr(net, n)
        s = slice(off, off + prm.numel())
        off += prm.numel()
        if mask & GROUP_BITS[n]:
            assert rel(theta[s], prm.reshape(-1)) <= 1e-6, n
            assert rel(ms[s], opt.state[prm]["square_avg"].reshape(-1)) <= 1e-6, n
            assert not torch.equal(theta[s], before_theta[s])
        else:
            assert torch.equal(theta[s], before_theta[s]) and torch.equal(ms[s], before_ms[s]), n


def golden_env(g):
    B, T = int(g["B"]), int(g["T"])
    env = IL_Env('pendulum', lqr_iter=int(g["lqr_iter"]), mpc_T=T)
    tau = np.zeros((B, T, 4), dtype=np.float32)
    tau[:, :, :3] = g["xinit"][:, None, :]          # only x_init and the expert controls enter the loss
    tau[:, :, 3:] = np.transpose(g["expert_u"], (1, 0, 2))
    env.train_data = env.val_data = env.test_data = torch.as_tensor(tau, device="cuda")
    return env


def test_device_update_reproduces_the_reference_loop(tmp_path):
    """tests/golden/imitation_loop_16.npz (the reference's pieces, three updates of learn_p, each followed by an evaluation
    pass warm-started from the previous one) through IL_Exp's device update: one batch of 16 per epoch"""
    g = np.load(os.path.join(GOLDEN, "imitation_loop_16.npz"))
    B, T, K = int(g["B"]), int(g["T"]), int(g["K"])
    exp = IL_Exp(B, golden_env(g), n_epoch=K, save_dir=str(tmp_path), device_update=True)
    with torch.no_grad():
        exp.net.learn_q_logit.copy_(torch.as_tensor(g["q_logit0"]))
        exp.net.learn_p.copy_(torch.as_tensor(g["learn_p0"]))
    seen = []
    exp.run(callback=lambda e, ev: seen.append((npy(e.net.learn_p), npy(e.net.learn_q_logit), e.grads(),
                                                npy(e._state.warm["val"]))) if ev == "epoch" else None)
    assert len(seen) == K and len(exp.train_log) == K and len(exp.val_test_log) == K
    for k in range(K):
        learn_p, q_logit, grads, warm = seen[k]
        loss, ref = exp.train_log[k][1], float(g["loss_%d" % k])
        assert abs(loss - ref) <= 5e-3 * ref, (k, loss, ref)
        for got, r in ((grads["learn_q_logit"], g["g_logit_%d" % k]), (grads["learn_p"], g["g_p_%d" % k])):
            assert np.abs(npy(got) - r).max() <= 5e-2 * np.abs(r).max(), (k, npy(got), r)
        assert_close(learn_p, g["learn_p_%d" % k], 1e-4, "learn_p after update %d" % k)
        assert np.array_equal(q_logit, g["q_logit0"].astype(np.float32).astype(np.float64))
        ev, ref_ev = exp.val_test_log[k][1], float(g["eval_loss_%d" % k])
        assert abs(ev - ref_ev) <= 5e-3 * ref_ev, (k, ev, ref_ev)
        assert np.mean(np.abs(np.transpose(warm, (1, 0, 2)) - g["eval_u_%d" % k]) <= 5e-4) >= 0.95


@pytest.mark.parametrize("lower,strange", [(False, False), (True, False), (False, True), (True, True)])
def test_device_update_matches_the_torch_update(small_data, tmp_path, lower, strange):
    """12 updates of 16 out of 48 (three per epoch) with the switch every 2 epochs - epoch 2 toggles on each of its three
    iterations - on both routes: parameters, RMSprop state and loss of every update within 1e-5 of device_update=False.
    Each device update starts from the state the torch route had before it (`set_state` in the callback): two
    trajectories of training do not stay within 1e-5 of each other, whatever computes them - the solve is not smooth in
    the cost (a trajectory crossing BoxDDP's detach threshold drops its gradient), and a last-place difference of the
    parameters grows to 1e-3 of the loss within three updates of q."""
    ref = IL_Exp(16, small_data, n_epoch=10, is_lower_triangle=lower, is_strange_observation=strange, rand_init=True,
                 save_dir=str(tmp_path / "torch"), device_update=False, round_robin_interval=2)
    init = {k: v.detach().clone() for k, v in ref.net.state_dict().items()}
    after = []
    ref.run(max_updates=12, callback=lambda e, ev: after.append(
        ({n: getattr(e.net, n).detach().clone() for n in e.param_names()}, e.square_avg(), e.cost_update_q))
        if ev == "update" else None)
    dev = IL_Exp(16, small_data, n_epoch=10, is_lower_triangle=lower, is_strange_observation=strange,
                 save_dir=str(tmp_path / "device"), device_update=True, round_robin_interval=2)
    dev.set_state(init)
    worst = {"param": 0.0, "square_avg": 0.0}
    flags = []

    def check_then_align(e, ev):
        if ev != "update":
            return
        params, sq, flag = after[e.n_updates - 1]
        flags.append(e.cost_update_q)
        assert e.cost_update_q == flag
        dsq = e.square_avg()
        for n in e.param_names():
            worst["param"] = max(worst["param"], rel(getattr(e.net, n), params[n]))
            worst["square_avg"] = max(worst["square_avg"], rel(dsq[n], sq[n]) if float(sq[n].abs().max()) > 0 else
                                      float(dsq[n].abs().max()))
        e.set_state(params, sq)

    dev.run(max_updates=12, callback=check_then_align)
    assert dev.n_updates == ref.n_updates == 12
    assert flags == [False] * 6 + [True, False, True, True, True, True]
    assert worst["param"] <= 1e-5 and worst["square_avg"] <= 1e-5, worst
    assert [e for e, _ in ref.train_log] == [e for e, _ in dev.train_log]
    lr_, ld = np.array([l for _, l in ref.train_log]), np.array([l for _, l in dev.train_log])
    assert np.abs(ld - lr_).max() <= 1e-5 * np.abs(lr_).max(), (ld, lr_)
    for n in ref.param_names():                   # both groups moved
        assert not torch.equal(after[-1][0][n], init[n].to(after[-1][0][n])), n
    assert len(ref.val_test_log) == len(dev.val_test_log) == 4
    for (e_r, v_r, t_r), (e_d, v_d, t_d) in zip(ref.val_test_log, dev.val_test_log):
        assert e_r == e_d and abs(v_r - v_d) <= 1e-5 * abs(v_r) and abs(t_r - t_d) <= 1e-5 * abs(t_r)


def test_run_writes_the_reference_files(small_data, tmp_path):
    save = str(tmp_path / "run")
    exp = IL_Exp(16, small_data, n_epoch=3, save_dir=save)
    exp.run()
    rows = list(csv.reader(open(os.path.join(save, "train_losses.csv"))))
    assert rows[0] == ["epoch", "imitation_loss"] and len(rows) == 1 + 9
    assert [float(r[0]) for r in rows[1:]] == pytest.approx([1 / 3, 2 / 3, 1, 4 / 3, 5 / 3, 2, 7 / 3, 8 / 3, 3])
    assert all(np.isfinite(float(r[1])) for r in rows[1:])
    rows = list(csv.reader(open(os.path.join(save, "val_test_losses.csv"))))
    assert rows[0] == ["epoch", "im_loss_val", "im_loss_test"] and [r[0] for r in rows[1:]] == ["1", "2", "3"]
    rows = list(csv.reader(open(os.path.join(save, "cost_hist.csv"))))
    true_q, true_p = exp.env.true_dx.get_true_obj()
    assert len(rows) == 1 and np.allclose([float(v) for v in rows[0]], torch.cat((true_q, true_p)).double().numpy())
    ck = torch.load(os.path.join(save, "best.pt"))
    assert ck["epoch"] in (1, 2, 3) and set(ck["net"]) == {"learn_q_logit", "learn_p"}
    assert set(ck["optimizer"]["square_avg"]) == {"learn_q_logit", "learn_p"} and ck["optimizer"]["alpha"] == 0.5
    assert min(v for _, v, _ in exp.val_test_log) == exp.best_val_loss


def test_an_update_makes_no_host_synchronisation(small_data, tmp_path):
    """after the first epoch (the solver's hipGraphs recorded), the updates of an epoch run under
    torch.cuda.set_sync_debug_mode("error"): no device or stream synchronisation and no blocking read-back until the epoch's
    losses.  (The one wait that remains, BoxDDP's deferred status check of the previous solve, waits on that solve's event
    only - DESIGN.md section 3.7.)"""
    exp = IL_Exp(16, small_data, n_epoch=2, save_dir=str(tmp_path))
    state = {}

    def cb(e, ev):
        if ev == "epoch" and e.train_iter.epoch == 1:
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            state["on"] = True
        elif ev == "update" and state.get("on"):
            state["n"] = state.get("n", 0) + 1
            if state["n"] == 3:
                torch.cuda.set_sync_debug_mode("default")
    try:
        exp.run(callback=cb)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert state.get("n") == 3 and exp.n_updates == 6
