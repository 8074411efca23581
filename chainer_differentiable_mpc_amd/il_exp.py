"""`IL_Exp` - the imitation-learning driver of env_dx/il_exp.py: epochs over the expert data set `make_dataset` wrote,
RMSprop on a learnable pendulum cost (`pendulum_net.py`), validation and test passes, CSV logs and a best checkpoint.

    exp = IL_Exp(n_batch=32, data="data/pendulum.pkl", n_epoch=300)
    exp.run()
    python -m chainer_differentiable_mpc_amd.il_exp --epochs 300 --batch 32 [--lower-triangle] [--strange-observation]

`run()` follows il_exp.py:191-316, quirks included:
  - RMSprop(lr=1e-2, alpha=0.5) with chainer's eps=1e-8 (:213).
  - `cost_update_q` starts False and is toggled at the top of EVERY ITERATION whose `epoch > 0 and epoch % 10 == 0`
    (:231-232): an epoch of several batches toggles on each of them (`round_robin_interval` is the 10).
  - While it is False only `learn_p` is updated; while it is True `learn_q_logit` (and `lower_without_diag` for the
    lower-triangle nets) is (:268-281).  A disabled parameter gets neither an update nor an RMSprop state change (chainer's
    `update_rule.enabled = False`).
  - Training solves are cold-started: the net is handed `train_warm_start[idxs]`, which is only ever zeroed (:235-238, :248);
    the plan is written to `train_warmstart`, which nothing reads.  `restart_warmstart_every` therefore changes nothing.
  - Validation and test passes (`dataset_loss`, :97-189) warm-start from their own previous predictions, never reset (the
    reset at :235-238 names the other arrays).
  - Training batches come from a shuffled, repeating `SerialIterator`, validation / test batches from an unshuffled one: a
    short last batch is filled from the start of the next pass (`IndexIterator`).  The shuffle draws from
    `np.random.RandomState(seed)` rather than numpy's global state.
  - The loss is mean((us - nom_u)^2) over the controls only (:254-263).
  - train_losses.csv `epoch,imitation_loss` (one row `epoch_detail,loss` per update), val_test_losses.csv
    `epoch,im_loss_val,im_loss_test` (one row per epoch), cost_hist.csv (the true (q, p) row only, when cost=True).
  - A better validation loss saves `best.pt`: a `torch.save` of the net's and the optimiser's state and the epoch (the
    reference pickles the whole object, :307-316).
  - dx=True raises NotImplementedError (the reference has `assert False` there, :245-246).
  - `rand_init` is a bool (the reference passes the answer string of an `input()` prompt, so any answer randomises).
  - The lower-triangle branch of `dataset_loss` (:140-141) appends a zero to p, giving n_sc + 1 entries against a
    [n_sc, n_sc] Q: that evaluation pass cannot run in the reference.  Here every evaluation uses the net's own p.
  - The batch size may not exceed any split's size (the device update keeps batch-sized buffers).

device_update=True (default): every split is resident on the device (float32 trajectories, warm-start controls, the
epoch's batch indices as int32, uploaded once per epoch), and an update is `dmpc_il_batch_begin` (gather + cost map + tiles
into persistent buffers) -> the `BoxDDP` device loop -> `dmpc_il_loss` (loss into a device log, gradient seed) -> the tiled
cost gradient (`dmpc_mpc_step_backward`) -> `dmpc_il_param_step` (chain rule + RMSprop).  Losses are read back once an
epoch.  device_update=False: the same update with torch autograd through `net.forward` (`IL_Env.mpc_Q` -> `BoxDDP` with a
`TiledQuadCost`) and `torch.optim.RMSprop` - the route to check by eye, and the yardstick of the device route."""
import argparse
import os
import time
import warnings

import numpy as np
import torch

from . import _lib
from .box_ddp import BoxDDP
from .il_env import IL_Env
from .mpc_step import tiled_cost_gradient, tiled_gradient_inputs
from .pendulum_net import make_net
from .util import TiledQuadCost

LR, ALPHA, EPS = 1e-2, 0.5, 1e-8           # il_exp.py:213, chainer's RMSprop eps
GROUP_BITS = {"learn_q_logit": 1, "learn_p": 2, "lower_without_diag": 4}     # dmpc_il_param_step's enable_mask


class IndexIterator:
    """chainer's `SerialIterator(repeat=True)` over range(n), indices only: `next()` -> int64 [batch]; `epoch`,
    `epoch_detail`, `is_new_epoch` as chainer counts them; a batch that crosses the end of a pass is filled from the
    start of the next (reshuffled when `shuffle`)"""

    def __init__(self, n, batch_size, shuffle=False, seed=0):
        self.n, self.batch_size, self.shuffle = int(n), int(batch_size), bool(shuffle)
        self._rng = np.random.RandomState(seed)
        self.epoch, self.current_position, self.is_new_epoch = 0, 0, False
        self._order = self._rng.permutation(self.n) if self.shuffle else None

    def _take(self, a, b):
        return np.arange(a, min(b, self.n)) if self._order is None else self._order[a:b]

    def next(self):
        i, i_end = self.current_position, self.current_position + self.batch_size
        batch = self._take(i, i_end)
        if i_end >= self.n:
            rest = i_end - self.n
            if self._order is not None:
                self._order = self._rng.permutation(self.n)
            if rest > 0:
                batch = np.concatenate((batch, self._take(0, rest)))
            self.current_position = rest
            self.epoch += 1
            self.is_new_epoch = True
        else:
            self.is_new_epoch = False
            self.current_position = i_end
        return batch.astype(np.int64)

    @property
    def epoch_detail(self):
        return self.epoch + self.current_position / self.n

    def pass_batches(self):
        """the batches of one evaluation pass (il_exp.py:106-107: until the epoch counter moves on)"""
        before, out = self.epoch, []
        while self.epoch < before + 1:
            out.append(self.next())
        return out


def toggles(epoch, interval):
    """il_exp.py:231-232, asked at the top of every iteration"""
    return epoch > 0 and epoch % interval == 0


class IL_Exp:
    def __init__(self, n_batch, data, n_epoch=300, cost=True, dx=False, is_lower_triangle=False,
                 is_strange_observation=False, rand_init=False, save_dir=None, device_update=True, round_robin_interval=10,
                 restart_warmstart_every=50, seed=0, device="cuda"):
        if dx:
            raise NotImplementedError("learn_dx: the reference never implemented it (il_exp.py:245-246 asserts False)")
        self.n_batch, self.n_epoch = int(n_batch), int(n_epoch)
        self.learn_cost, self.learn_dx = cost, dx
        self.device = torch.device(device)
        if isinstance(data, IL_Env):
            self.env = data.to(self.device)
        else:
            from .make_dataset import load
            self.env = load(data, device=self.device)
        if save_dir is None:
            save_dir = os.path.join("work", time.strftime("%Y%m%d-%H%M%S") + "_epoch:%d_" % self.n_epoch +
                                    (".learn_cost" if cost else ""))
        self.save = save_dir
        self.is_lower_triangle, self.is_strange_observation = bool(is_lower_triangle), bool(is_strange_observation)
        self.n_state, self.n_ctrl = self.env.true_dx.n_state, self.env.true_dx.n_ctrl
        self.n_sc = self.n_state + self.n_ctrl
        self.T = self.env.mpc_T
        self.net = make_net(self.n_sc, self.is_lower_triangle, self.is_strange_observation, bool(rand_init), device=self.device)
        self.device_update = bool(device_update)
        self.round_robin_interval = int(round_robin_interval)
        self.restart_warmstart_every = int(restart_warmstart_every)     # (resets arrays nothing reads: see the docstring)
        self.seed = seed
        self.splits = {"train": self.env.train_data, "val": self.env.val_data, "test": self.env.test_data}
        for name, d in self.splits.items():
            if d is None or d.shape[0] < self.n_batch:
                raise ValueError("IL_Exp: the %s split has %s trajectories, fewer than the batch of %d" % (
                    name, None if d is None else d.shape[0], self.n_batch))
        self.n_train = self.splits["train"].shape[0]
        self.train_iter = IndexIterator(self.n_train, self.n_batch, shuffle=True, seed=seed)
        self.val_iter = IndexIterator(self.splits["val"].shape[0], self.n_batch)
        self.test_iter = IndexIterator(self.splits["test"].shape[0], self.n_batch)
        self.cost_update_q = False
        self.train_log = []         # (epoch_detail, loss) per update
        self.val_test_log = []      # (epoch, val loss, test loss) per epoch
        self.best_val_loss = None
        self.n_updates = 0
        self._state = None
        self._square_avg_init = None

    # -- parameters and optimiser state, the same names on both routes
    def param_names(self):
        return [n for n in ("learn_q_logit", "learn_p", "lower_without_diag") if hasattr(self.net, n)]

    def enable_mask(self):
        """il_exp.py:268-281"""
        if self.cost_update_q:
            return GROUP_BITS["learn_q_logit"] | (GROUP_BITS["lower_without_diag"] if self.is_lower_triangle else 0)
        return GROUP_BITS["learn_p"]

    def square_avg(self):
        """RMSprop's running mean of the squared gradient per parameter (zeros before a parameter's first update)"""
        if self._state is None:
            return {n: torch.zeros_like(getattr(self.net, n)) for n in self.param_names()}
        return self._state.square_avg()

    def grads(self):
        """the gradient of the last update per parameter (of every group, enabled or not)"""
        return self._state.grads() if self._state is not None else {}

    def set_state(self, params, square_avg=None):
        """overwrite the parameters and RMSprop's running means (dicts by parameter name) - before `run()` (a resume from
        `best.pt`'s ["net"] and ["optimizer"]["square_avg"]) or from a callback inside it"""
        with torch.no_grad():
            for n in self.param_names():
                getattr(self.net, n).copy_(torch.as_tensor(params[n]))
        if square_avg is not None:
            self._square_avg_init = {n: torch.as_tensor(square_avg[n]).clone() for n in self.param_names()}
            if self._state is not None:
                self._state.set_square_avg(self._square_avg_init)

    def checkpoint(self, epoch):
        return {"epoch": epoch, "kind": self.net.kind, "net": {k: v.detach().cpu().clone() for k, v in self.net.state_dict().items()},
                "optimizer": {"lr": LR, "alpha": ALPHA, "eps": EPS,
                              "square_avg": {k: v.detach().cpu().clone() for k, v in self.square_avg().items()}}}

    # -- the loop (il_exp.py:191-316)
    def run(self, max_updates=None, callback=None):
        """train for n_epoch epochs (or max_updates updates); callback(self, "update") after every update and
        callback(self, "epoch") after every evaluation"""
        os.makedirs(self.save, exist_ok=True)
        train_f = open(os.path.join(self.save, "train_losses.csv"), "w")
        train_f.write("epoch,imitation_loss\n")
        vt_f = open(os.path.join(self.save, "val_test_losses.csv"), "w")
        vt_f.write("epoch,im_loss_val,im_loss_test\n")
        if self.learn_cost:
            true_q, true_p = self.env.true_dx.get_true_obj()
            with open(os.path.join(self.save, "cost_hist.csv"), "w") as cost_f:
                cost_f.write(",".join(map(str, torch.cat((true_q, true_p)).double().tolist())) + "\n")
        self._state = (_DeviceState if self.device_update else _TorchState)(self)
        if self._square_avg_init is not None:
            self._state.set_square_avg(self._square_avg_init)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                self._loop(train_f, vt_f, max_updates, callback)
        finally:
            train_f.close()
            vt_f.close()
        return self

    def _loop(self, train_f, vt_f, max_updates, callback):
        st = self._state
        while self.train_iter.epoch < self.n_epoch:
            plan = []                   # the iterations of this epoch: (epoch before next(), batch, epoch_detail after)
            while True:
                e0 = self.train_iter.epoch
                idx = self.train_iter.next()
                plan.append((e0, idx, self.train_iter.epoch_detail))
                if self.train_iter.is_new_epoch:
                    break
            st.begin_epoch([b for _, b, _ in plan])
            done = 0
            for k, (e0, _, _) in enumerate(plan):
                if toggles(e0, self.round_robin_interval):
                    self.cost_update_q = not self.cost_update_q
                st.update(k, self.enable_mask())
                self.n_updates += 1
                done += 1
                if callback is not None:
                    callback(self, "update")
                if max_updates is not None and self.n_updates >= max_updates:
                    break
            for (_, _, detail), loss in zip(plan[:done], st.train_losses(done)):
                self.train_log.append((detail, loss))
                train_f.write("%s,%s\n" % (detail, loss))
            train_f.flush()
            if done < len(plan):
                break
            val_loss = st.dataset_loss("val", self.val_iter.pass_batches())
            test_loss = st.dataset_loss("test", self.test_iter.pass_batches())
            epoch = self.train_iter.epoch
            self.val_test_log.append((epoch, val_loss, test_loss))
            vt_f.write("%s,%s,%s\n" % (epoch, val_loss, test_loss))
            vt_f.flush()
            self.env.flush()
            st.flush()
            if self.best_val_loss is None or val_loss < self.best_val_loss:
                self.best_val_loss = val_loss
                torch.save(self.checkpoint(epoch), os.path.join(self.save, "best.pt"))
            if callback is not None:
                callback(self, "epoch")
            if max_updates is not None and self.n_updates >= max_updates:
                break


class _TorchState:
    """device_update=False: autograd through net.forward and torch.optim.RMSprop"""

    def __init__(self, exp):
        self.exp = exp
        self.net = exp.net
        nu = exp.n_ctrl
        self.data = {k: v.to(device=exp.device, dtype=torch.float32) for k, v in exp.splits.items()}
        self.warm = {k: torch.zeros((v.shape[0], exp.T, nu), dtype=torch.float32, device=exp.device)
                     for k, v in self.data.items() if k != "train"}
        self.params = {n: getattr(self.net, n) for n in exp.param_names()}
        self.opt = torch.optim.RMSprop(list(self.params.values()), lr=LR, alpha=ALPHA, eps=EPS)
        self.cold = torch.zeros((exp.n_batch, exp.T, nu), dtype=torch.float32, device=exp.device)
        self._losses = []

    def begin_epoch(self, batches):
        self.batches = [torch.as_tensor(b, device=self.exp.device) for b in batches]
        self._losses = []

    def _batch(self, split, idx):
        tau = self.data[split][idx]
        nx = self.exp.n_state
        return tau[:, 0, :nx], tau[:, :, nx:].transpose(0, 1)

    def update(self, k, mask):
        xinit, us = self._batch("train", self.batches[k])
        self.opt.zero_grad(set_to_none=True)
        _, nom_u = self.net(xinit, self.exp.env, self.cold)
        loss = ((us - nom_u) ** 2).mean()
        loss.backward()
        self._grads = {n: p.grad.detach().clone() for n, p in self.params.items()}
        for n, prm in self.params.items():
            if not (mask & GROUP_BITS[n]):
                prm.grad = None         # torch's RMSprop skips it: no step, no state change
        self.opt.step()
        self._losses.append(loss.detach())

    def train_losses(self, n):
        return [float(v) for v in self._losses[:n]]

    def dataset_loss(self, split, batches):
        env = self.exp.env
        losses = []
        with torch.no_grad():
            Q, p = self.net.cost_map()
            for idx in batches:
                idx = torch.as_tensor(idx, device=self.exp.device)
                xinit, us = self._batch(split, idx)
                _, pred_u = env.mpc_Q(env.true_dx, xinit, Q, p, u_init=self.warm[split][idx].transpose(0, 1))
                self.warm[split][idx] = pred_u.transpose(0, 1).to(torch.float32)
                losses.append(float(((us - pred_u) ** 2).mean()))
        return float(np.mean(losses))

    def square_avg(self):
        return {n: (self.opt.state[p]["square_avg"].detach().clone() if "square_avg" in self.opt.state.get(p, {})
                    else torch.zeros_like(p)) for n, p in self.params.items()}

    def grads(self):
        return getattr(self, "_grads", {})

    def set_square_avg(self, sq):
        for n, p in self.params.items():
            self.opt.state[p] = {"step": torch.tensor(0.0), "square_avg": sq[n].to(p).clone()}

    def flush(self):
        pass


class _DeviceState:
    """device_update=True: the splits resident on the device, the update on the dmpc_il_* kernels around the box-DDP chain
    and the tiled cost gradient, no host read-back inside an epoch (the losses wait in a device log)"""

    def __init__(self, exp):
        self.exp = exp
        self.lib = _lib.load()
        _lib.require_gpu()
        d = self.d = exp.device if exp.device.index is not None else torch.device("cuda", torch.cuda.current_device())
        self.T, self.B, self.nx, self.nu = exp.T, exp.n_batch, exp.n_state, exp.n_ctrl
        T, B, nx, nu, ns = self.T, self.B, self.nx, self.nu, exp.n_sc
        self.kind, self.ns = exp.net.kind, ns
        self.tau = {k: v.to(device=d, dtype=torch.float32).contiguous() for k, v in exp.splits.items()}
        self.warm = {k: torch.zeros((v.shape[0], T, nu), dtype=torch.float32, device=d) for k, v in self.tau.items()
                     if k != "train"}
        # the parameter vector [learn_q_logit, learn_p, lower_without_diag], its RMSprop state and gradient; the net's
        # parameters become views of it, so the net always shows what the kernels wrote
        names = exp.param_names()
        sizes = [getattr(exp.net, n).numel() for n in names]
        assert sum(sizes) == self.lib.dmpc_il_n_params(self.kind, ns), "dmpc_il_n_params disagrees with the net"
        self.theta = torch.cat([getattr(exp.net, n).detach().reshape(-1).to(device=d, dtype=torch.float32) for n in names])
        self.ms = torch.zeros_like(self.theta)
        self.grad = torch.zeros_like(self.theta)
        self.views = {}
        off = 0
        for n, s in zip(names, sizes):
            self.views[n] = (off, s)
            getattr(exp.net, n).data = self.theta[off:off + s]
            off += s
        # persistent batch buffers: the solver's hipGraph replay is keyed on their addresses
        f32 = dict(dtype=torch.float32, device=d)
        self.x_init = torch.empty((B, nx), **f32)
        self.us = torch.empty((T, B, nu), **f32)
        self.u_init = torch.empty((T, B, nu), **f32)
        self.gu = torch.empty((T, B, nu), **f32)
        self.Q = torch.empty((ns, ns), **f32)
        self.p = torch.empty((ns,), **f32)
        self.C = torch.empty((T, B, ns, ns), **f32)
        self.c = torch.empty((T, B, ns), **f32)
        env, dx = exp.env, exp.env.true_dx
        self.dx = dx
        kw = dict(u_lower=dx.lower, u_upper=dx.upper, n_batch=B, n_state=nx, n_ctrl=nu, eps=dx.mpc_eps, max_iter=env.lqr_iter,
                  verbose=False, exit_unconverged=False, detach_unconverged=True, line_search_decay=dx.linesearch_decay,
                  max_line_search_iter=dx.max_linesearch_iter, quiet=True, lazy_status=True)
        # cold start (il_exp.py:248) from a zero buffer of its own: with u_init=None a solve called again on the same buffers
        # would take BoxDDP's replay shortcut, which returns no gradient node
        self.u_zero = torch.zeros((T, B, nu), **f32)
        self.solver_train = BoxDDP(T, u_init=self.u_zero, update_dynamics=False, **kw)
        self.solver_eval = BoxDDP(T, u_init=self.u_init, update_dynamics=False, **kw)
        self.Q_leaf = self.Q.detach().requires_grad_(True)       # what the gradient node is asked about (never read by it)
        self.p_leaf = self.p.detach().requires_grad_(True)
        self.cost_train = TiledQuadCost.from_tiles(self.C, self.c, self.Q_leaf, self.p_leaf)
        self.cost_eval = TiledQuadCost.from_tiles(self.C, self.c, self.Q, self.p)
        self.stream = _lib.stream_ptr(d)

    def _upload(self, batches):
        host = torch.from_numpy(np.stack(batches).astype(np.int32)).pin_memory()
        return host.to(self.d, non_blocking=True)

    def begin_epoch(self, batches):
        self.idx = self._upload(batches)
        self.log = torch.zeros((len(batches),), dtype=torch.float32, device=self.d)

    def _begin(self, split, idx, warm):
        N = self.tau[split].shape[0]
        rc = self.lib.dmpc_il_batch_begin(self.kind, N, self.T, self.B, self.nx, self.nu, _lib.ptr(self.tau[split]),
                                          _lib.ptr(warm), _lib.ptr(idx), _lib.ptr(self.theta), _lib.ptr(self.x_init),
                                          _lib.ptr(self.us), _lib.ptr(self.u_init), _lib.ptr(self.Q), _lib.ptr(self.p),
                                          _lib.ptr(self.C), _lib.ptr(self.c), self.stream)
        _lib.check(rc, "dmpc_il_batch_begin")
        return N

    def update(self, k, mask):
        T, B, nx, nu = self.T, self.B, self.nx, self.nu
        idx = self.idx[k]
        N = self._begin("train", idx, None)
        with torch.enable_grad():
            _, u, _ = self.solver_train((self.x_init, self.cost_train, self.dx))
        rc = self.lib.dmpc_il_loss(N, T, B, nu, _lib.ptr(u), _lib.ptr(self.us), _lib.ptr(idx), _lib.ptr(self.log[k:k + 1]),
                                   _lib.ptr(self.gu), None, self.stream)
        _lib.check(rc, "dmpc_il_loss")
        node = tiled_gradient_inputs(u)
        if node is None:
            raise _lib.DmpcError("IL_Exp: the solve carries no tiled-cost gradient node (device loop refused?)")
        (_, _, _, _, _, lo, hi, detach), retained = node
        got = tiled_cost_gradient(T, B, nx, nu, self.d, retained, lo, hi, None, self.gu, detach)
        if got is None:
            raise _lib.DmpcError("IL_Exp: dmpc_mpc_step_backward does not serve T=%d B=%d (needs B %% 4 == 0)" % (T, B))
        _, dQ, dp = got
        rc = self.lib.dmpc_il_param_step(self.kind, self.ns, _lib.ptr(dQ), _lib.ptr(dp), _lib.ptr(self.theta),
                                         _lib.ptr(self.ms), _lib.ptr(self.grad), int(mask), LR, ALPHA, EPS, self.stream)
        _lib.check(rc, "dmpc_il_param_step")

    def train_losses(self, n):
        return [float(v) for v in self.log[:n].double().cpu().tolist()]       # the epoch's one read-back

    def dataset_loss(self, split, batches):
        idx_all = self._upload(batches)
        log = torch.empty((len(batches),), dtype=torch.float32, device=self.d)
        warm = self.warm[split]
        with torch.no_grad():
            for k in range(len(batches)):
                idx = idx_all[k]
                N = self._begin(split, idx, warm)
                _, u, _ = self.solver_eval((self.x_init, self.cost_eval, self.dx))
                rc = self.lib.dmpc_il_loss(N, self.T, self.B, self.nu, _lib.ptr(u), _lib.ptr(self.us), _lib.ptr(idx),
                                           _lib.ptr(log[k:k + 1]), None, _lib.ptr(warm), self.stream)
                _lib.check(rc, "dmpc_il_loss")
        return float(np.mean(log.double().cpu().numpy()))

    def _split(self, t):
        return {n: t[o:o + s].view_as(getattr(self.exp.net, n)).detach().clone() for n, (o, s) in self.views.items()}

    def square_avg(self):
        return self._split(self.ms)

    def grads(self):
        return self._split(self.grad)

    def set_square_avg(self, sq):
        for n, (o, s) in self.views.items():
            self.ms[o:o + s].copy_(sq[n].reshape(-1).to(self.ms))

    def flush(self):
        for s in (self.solver_train, self.solver_eval):
            s._resolve()


def parse_args(argv=None):
    """the non-interactive replacement of il_exp.py's `input()` prompts"""
    ap = argparse.ArgumentParser(prog="python -m chainer_differentiable_mpc_amd.il_exp", description=__doc__.split("\n")[0])
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lower-triangle", action="store_true")
    ap.add_argument("--strange-observation", action="store_true")
    ap.add_argument("--random-init", action="store_true")
    ap.add_argument("--data", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "pendulum.pkl"))
    ap.add_argument("--save", default=None)
    ap.add_argument("--torch-update", action="store_true", help="torch autograd + torch.optim.RMSprop instead of the device update")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    exp = IL_Exp(a.batch, a.data, n_epoch=a.epochs, is_lower_triangle=a.lower_triangle,
                 is_strange_observation=a.strange_observation, rand_init=a.random_init, save_dir=a.save,
                 device_update=not a.torch_update)
    exp.run()
    print("best validation loss %s; logs in %s" % (exp.best_val_loss, exp.save))


if __name__ == "__main__":
    main()
