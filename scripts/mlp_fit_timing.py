"""One `MlpDx.prediction_loss` plus `backward`, two ways on equal weights in the same run:
  device - `param_grad="device"`: `rollout` is one autograd node, forward the rollout's launch, backward `dmpc_mlp_rollout_grad`
           (one reverse sweep that carries the co-state, one fixed-order reduction);
  live   - `param_grad="live"`, the default: a Python loop of T - 1 torch steps and autograd through every one of them - the only
           way to this gradient before the node existed (the baseline).
The two routes alternate call by call.  Per case one line: the median and the range of `--iters` calls (at least 7) after warm-up,
device events around loss + backward with the host time in between included, the kernel launches of one call of each route, and
how far the two routes' gradients are apart.  The records are rollouts of a teacher network of the same shape under random
controls, `--horizon` steps per window (default: one window over the whole record).

The run fails if the device route's median is above the live route's at any case.

    python scripts/mlp_fit_timing.py [--iters 15] [--warmup 3] [--cases 3x1x32,8x2x64,8x2x64x64] [--batch 128] [--steps 20]
                                     [--horizon H] [--out file]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from chainer_differentiable_mpc_amd import MlpDx  # noqa: E402
from scripts.mlp_dx_timing import count_launches  # noqa: E402


def record(nx, nu, hidden, B, T):
    """(x [T,B,nx], u [T-1,B,nu]) on the device: a teacher of the same shape rolled under u ~ U(-1, 1)"""
    gen = torch.Generator().manual_seed(1)
    teacher = MlpDx(nx, nu, hidden, seed=7).cuda()
    x0 = torch.randn(B, nx, generator=gen).cuda()
    u = (2.0 * torch.rand(T - 1, B, nu, generator=gen) - 1.0).cuda()
    with torch.no_grad():
        return teacher.rollout(x0, u, T=T), u


def run_case(nx, nu, hidden, B, T, horizon, iters, warmup):
    x, u = record(nx, nu, hidden, B, T)
    routes = {tag: (MlpDx(nx, nu, hidden, seed=0, param_grad=tag).cuda(), []) for tag in ("device", "live")}

    def once(tag, keep=True):
        m, ts = routes[tag]
        m.zero_grad(set_to_none=True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        m.prediction_loss(x, u, horizon=horizon).backward()
        b.record()
        b.synchronize()
        if keep:
            ts.append(a.elapsed_time(b))

    for _ in range(warmup):
        for tag in routes:
            once(tag, keep=False)
    for _ in range(iters):
        for tag in routes:
            once(tag)
    out = dict(nx=nx, nu=nu, n_hidden=hidden, B=B, T=T, horizon=horizon, iters=iters)
    for tag, (m, ts) in routes.items():
        ts.sort()
        out[tag] = dict(median_ms=ts[len(ts) // 2], min_ms=ts[0], max_ms=ts[-1], launches=count_launches(lambda: once(tag, keep=False)))
    out["grads_max_rel_diff"] = max(float(((a.grad - b.grad).abs() / b.grad.abs().clamp(min=1.0)).max())
                                    for a, b in zip(routes["device"][0].parameters(), routes["live"][0].parameters()))
    return out


def line(r):
    d, v = r["device"], r["live"]
    return ("(%d,%d) H=%s B=%d T=%d horizon=%s, %d calls each, alternating: device %.3f ms [%.3f .. %.3f] %s launches | "
            "live %.3f ms [%.3f .. %.3f] %s launches | live/device %.1fx | gradients apart %.1e"
            % (r["nx"], r["nu"], r["n_hidden"], r["B"], r["T"], r["horizon"], r["iters"], d["median_ms"], d["min_ms"], d["max_ms"],
               d["launches"], v["median_ms"], v["min_ms"], v["max_ms"], v["launches"], v["median_ms"] / d["median_ms"],
               r["grads_max_rel_diff"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="3x1x32,8x2x64,8x2x64x64")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines, slower = [], []
    for c in a.cases.split(","):
        nx, nu, *h = (int(v) for v in c.split("x"))
        hidden = h[0] if len(h) == 1 else tuple(h)
        r = run_case(nx, nu, hidden, a.batch, a.steps, a.horizon, max(a.iters, 7), a.warmup)
        lines.append(line(r))
        print(lines[-1], flush=True)
        if r["device"]["median_ms"] > r["live"]["median_ms"]:
            slower.append(c)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    assert not slower, "the device route is slower than the live route at " + ", ".join(slower)


if __name__ == "__main__":
    main()
