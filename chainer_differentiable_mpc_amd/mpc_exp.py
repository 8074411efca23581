"""`MpcExp` - the reference's MPC imitation experiment, experiment_mpc/MpcNet.py:42-112: learn the dynamics [A|B] of a
box-constrained linear MPC from an expert's trajectories.

    loss = mean((u_true - u_pred)^2) + mean((x_true - x_pred)^2)                                    (:80-89)

with (x_true, u_true) the expert's `BoxDDP` solve under the true (A, B) and (x_pred, u_pred) the learner's `MpcNet_dx`
solve under its own, both from the same random x_init and the same known cost (Q = I, p).  The draws come in the reference's
order: `np.random.seed(expert_seed)`, then p, A, B (:49-56); the learner's constructor reseeds with `train_seed` and draws
its (A, B) (mpc_net.py:59-64); then one `randn(n_batch, n_state)` per iteration (:105).  The optimiser is RMSprop
(lr 1e-2, alpha 0.5, :92), the log `<train_seed>_new_losses.csv` with the header `im_loss,mse` (:95-97, 109-110), mse the
distance of the learnt (A, B) from the expert's.  No prompts, no plots.

The learner is `MpcNet_dx(shared=True)`: [A|B] reaches `BoxDDP` as a `TiledLinDx` and its gradient is summed over time and
batch on the device.  `dense=True` is the reference's own route - `expand_time_batch` on the autograd graph,
the dense dF [T-1,B,nx,ns] reduced by autograd - and the yardstick of the shared one.

    python -m chainer_differentiable_mpc_amd.mpc_exp --iters 10 --train-seed 1 [--bound 10] [--dense] [--save DIR]"""
import argparse
import os
import warnings

import numpy as np
import torch

from .box_ddp import BoxDDP
from .mpc_net import MpcNet_dx
from .util import LinDx, QuadCost, expand_time_batch


class MpcExp:
    def __init__(self, train_seed=1, T=5, n_state=3, n_ctrl=3, n_batch=128, expert_seed=42, bound=10.0, max_iter=10,
                 dense=False, save_dir=None, device="cuda", dtype=torch.float64, quiet=True):
        self.train_seed, self.T, self.n_state, self.n_ctrl, self.n_batch = train_seed, T, n_state, n_ctrl, n_batch
        self.n_sc = n_state + n_ctrl
        self.device, self.dtype, self.quiet = torch.device(device), dtype, quiet
        self.save = save_dir if save_dir is not None else os.getcwd()
        np.random.seed(expert_seed)                                                          # MpcNet.py:49-57
        alpha = 0.2
        p = np.random.randn(self.n_sc)
        A = np.eye(n_state) + alpha * np.random.randn(n_state, n_state)
        B = np.random.randn(n_state, n_ctrl)
        t = lambda a: torch.as_tensor(a, dtype=dtype, device=self.device)      # noqa: E731
        self.A_exp, self.B_exp = t(A), t(B)
        self.cost = QuadCost(expand_time_batch(t(np.eye(self.n_sc)), T, n_batch).contiguous(),
                             expand_time_batch(t(p), T, n_batch).contiguous())              # :64-66
        self.dynamics = LinDx(expand_time_batch(torch.cat((self.A_exp, self.B_exp), dim=1), T - 1, n_batch).contiguous(),
                              torch.zeros((T - 1, n_batch, n_state), dtype=dtype, device=self.device))     # :59-63
        self.u_lower = torch.full((T, n_batch, n_ctrl), -float(bound), dtype=dtype)         # :69-74
        self.u_upper = torch.full((T, n_batch, n_ctrl), float(bound), dtype=dtype)
        self.expert = BoxDDP(T, self.u_lower, self.u_upper, n_batch, n_state, n_ctrl, None, quiet=quiet)        # :81
        self.net = MpcNet_dx(T, self.u_lower, self.u_upper, n_batch, n_state, n_ctrl, train_seed, u_init=None,
                             max_iter=max_iter, dtype=dtype, quiet=quiet, shared=not dense).to(self.device)      # :93
        self.opt = torch.optim.RMSprop(self.net.parameters(), lr=1e-2, alpha=0.5)           # :92
        self.rows = []

    def get_loss(self, x_init):
        """MpcNet.py:80-89"""
        with torch.no_grad():
            x_true, u_true, _ = self.expert((x_init, self.cost, self.dynamics))
        x_pred, u_pred, _ = self.net((x_init, self.cost))
        return ((u_true - u_pred) ** 2).mean() + ((x_true - x_pred) ** 2).mean()

    def model_loss(self):
        with torch.no_grad():
            return ((self.net.A - self.A_exp) ** 2).mean() + ((self.net.B - self.B_exp) ** 2).mean()

    def run(self, iters=10):
        """MpcNet.py:95-112 -> the rows [(im_loss, mse)] written to `<train_seed>_new_losses.csv`"""
        os.makedirs(self.save, exist_ok=True)
        path = os.path.join(self.save, str(self.train_seed) + "_new_losses.csv")
        with open(path, "w") as loss_f, warnings.catch_warnings():
            if self.quiet:
                warnings.simplefilter("ignore")
            loss_f.write("im_loss,mse\n")
            loss_f.flush()
            for i in range(iters):
                self.opt.zero_grad(set_to_none=True)
                x_init = torch.as_tensor(np.random.randn(self.n_batch, self.n_state), dtype=self.dtype, device=self.device)
                loss = self.get_loss(x_init)
                loss.backward()
                self.opt.step()
                row = (float(loss.detach()), float(self.model_loss()))
                self.rows.append(row)
                loss_f.write("{},{}\n".format(*row))
                loss_f.flush()
                if not self.quiet:
                    print("iteration", i, "{0:04f}".format(row[0]), "dyanmics loss ", "{0:04f}".format(row[1]))
        self.path = path
        return self.rows


def run(iters=10, train_seed=1, **kw):
    """the experiment with the reference's settings -> its rows [(im_loss, mse)]"""
    return MpcExp(train_seed=train_seed, **kw).run(iters)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m chainer_differentiable_mpc_amd.mpc_exp", description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--train-seed", type=int, default=1)
    ap.add_argument("--bound", type=float, default=10.0)
    ap.add_argument("--dense", action="store_true", help="the reference's route: [A|B] expanded on the autograd graph")
    ap.add_argument("--save", default=None, help="directory of the CSV (default: the current one)")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    exp = MpcExp(train_seed=a.train_seed, bound=a.bound, dense=a.dense, save_dir=a.save, quiet=False)
    rows = exp.run(a.iters)
    print("last row: im_loss %.6f, mse %.6f; log in %s" % (rows[-1][0], rows[-1][1], exp.path))


if __name__ == "__main__":
    main()
