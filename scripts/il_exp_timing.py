"""IL_Exp update time at config 4's shape (B = 1,024, T = 20, the logit net, BoxDDP max_iter 10): the device update
(dmpc_il_batch_begin -> BoxDDP device loop -> dmpc_il_loss -> tiled cost gradient -> dmpc_il_param_step, losses read back
once an epoch) against device_update=False (torch autograd through net.forward + torch.optim.RMSprop), ms per update over
50 updates after 10 of warm-up, plus one epoch's validation and test passes (one batch each).

    python scripts/il_exp_timing.py [--updates 50] [--warmup 10] [--json out.json]"""
import argparse
import json
import os
import sys
import tempfile
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from chainer_differentiable_mpc_amd import IL_Env, IL_Exp  # noqa: E402
from chainer_differentiable_mpc_amd.il_exp import GROUP_BITS, _DeviceState, _TorchState  # noqa: E402


def make_env(B, T, lqr_iter):
    env = IL_Env('pendulum', lqr_iter=lqr_iter, mpc_T=T)
    env.populate_data(n_train=B, n_val=B, n_test=B, seed=0)
    return env


def time_route(env, B, device_update, updates, warmup):
    exp = IL_Exp(B, env, n_epoch=1, save_dir=tempfile.mkdtemp(prefix="il_timing_"), device_update=device_update)
    st = (_DeviceState if device_update else _TorchState)(exp)
    batches = [exp.train_iter.next() for _ in range(warmup + updates)]
    st.begin_epoch(batches)
    mask = GROUP_BITS["learn_p"]
    for k in range(warmup):
        st.update(k, mask)
    exp.env.flush()
    st.flush()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(warmup, warmup + updates):
        st.update(k, mask)
    losses = st.train_losses(warmup + updates)       # (the epoch's read-back: included)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    exp.env.flush()
    st.flush()
    ev = []
    for _ in range(3):
        torch.cuda.synchronize()
        e0 = time.perf_counter()
        v = st.dataset_loss("val", exp.val_iter.pass_batches())
        t = st.dataset_loss("test", exp.test_iter.pass_batches())
        torch.cuda.synchronize()
        ev.append((time.perf_counter() - e0) * 1e3)
    return dict(ms_per_update=(t1 - t0) * 1e3 / updates, eval_epoch_ms=float(np.median(ev)), last_loss=losses[-1],
                val_loss=v, test_loss=t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--lqr-iter", type=int, default=10)
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = make_env(a.batch, a.T, a.lqr_iter)
        out = {"B": a.batch, "T": a.T, "lqr_iter": a.lqr_iter, "updates": a.updates, "warmup": a.warmup,
               "device": torch.cuda.get_device_name(0)}
        for name, dev in (("device_update", True), ("torch_update", False)):
            out[name] = time_route(env, a.batch, dev, a.updates, a.warmup)
    out["target_ms"] = 0.45
    out["device_update_meets_target"] = out["device_update"]["ms_per_update"] <= 0.45
    for name in ("device_update", "torch_update"):
        r = out[name]
        print("%-14s %.3f ms / update   validation + test pass %.2f ms   (loss %.4g, val %.4g, test %.4g)" % (
            name, r["ms_per_update"], r["eval_epoch_ms"], r["last_loss"], r["val_loss"], r["test_loss"]))
    print("target <= 0.45 ms / update (device update): %s" % ("met" if out["device_update_meets_target"] else "NOT met"))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
