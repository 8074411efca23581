"""A closed-loop MPC episode two ways in the same run, on equal problems:
  baseline - a Python loop of `BoxDDP.forward`, the plant's own one-launch rollout at T = 2 and a torch shift of the plan, the
             solver's `u_init` replaced by the shifted plan at each step: what a user wrote before `ClosedLoop` existed;
  chain    - `ClosedLoop(solver, plant, n_steps)`: the whole episode as one chain of launches (`dmpc_mpc_episode`), one read-back.
Two cases on the pendulum plant: the pendulum itself as the controller's model, and an `MlpDx` (3,1), H = 32
(`device_loop=True`, untrained weights: the timing does not depend on what they are).  Medians, with the smallest and the largest,
over `--iters` episodes after warm-up, the two routes alternating episode by episode (device events around the whole episode,
host time included), the kernel launches of one episode of each route, and
how far the two routes' logged states are apart.  The run fails if the chain is slower than the baseline measured beside it.

    python scripts/episode_timing.py [--iters 7] [--warmup 2] [--steps 50] [--batch 128] [--horizon 20] [--hidden 32] [--json out]"""
import argparse
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from chainer_differentiable_mpc_amd import BoxDDP, ClosedLoop, MlpDx, PendulumDx, QuadCost  # noqa: E402
from chainer_differentiable_mpc_amd.pendulum import sample_xinit  # noqa: E402
from scripts.mlp_dx_timing import count_launches, median_ms  # noqa: E402


def baseline_episode(solver, plant, n_steps, x0, cost, model):
    """the loop every user wrote: solve, read back, plant step, shift"""
    x, xs, us = x0, [x0], []
    keep = solver.u_init
    try:
        for _ in range(n_steps):
            _, u_plan, _ = solver((x, cost, model))
            u0 = u_plan[0]
            x = plant.rollout_linearize(x, torch.stack((u0, u0)), want_model=False)[0][1]
            xs.append(x), us.append(u0)
            solver.u_init = torch.cat((u_plan[1:], u_plan[-1:]), dim=0)
    finally:
        solver.u_init = keep
    return torch.stack(xs), torch.stack(us)


def run_case(tag, model, B, T, n_steps, iters, warmup):
    plant = PendulumDx()
    q, p = plant.get_true_obj()
    C = torch.diag(q)[None, None].repeat(T, B, 1, 1).cuda().contiguous()
    c = p[None, None].repeat(T, B, 1).cuda().contiguous()
    x0, cost = torch.as_tensor(sample_xinit(B, seed=0), dtype=torch.float32).cuda(), QuadCost(C, c)
    lo, hi = torch.full((T, B, 1), plant.lower, device="cuda"), torch.full((T, B, 1), plant.upper, device="cuda")
    out = dict(case=tag, B=B, T=T, n_steps=n_steps)
    logs = {}

    def make_solver():
        return BoxDDP(T, lo, hi, B, 3, 1, None, eps=plant.mpc_eps, max_iter=10, line_search_decay=plant.linesearch_decay,
                      max_line_search_iter=plant.max_linesearch_iter, quiet=True)
    base_solver, chain_solver = make_solver(), make_solver()
    loop = ClosedLoop(chain_solver, plant, n_steps)

    def baseline():
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            logs["baseline"] = baseline_episode(base_solver, plant, n_steps, x0, cost, model)

    def chain():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = loop(x0, cost, model)
            logs["chain"] = (r.x, r.u)
    routes = (("baseline", baseline), ("chain", chain))
    for _, fn in routes:
        median_ms(fn, 1, warmup)
    times = {name: [] for name, _ in routes}
    for _ in range(iters):                      # the two routes alternate episode by episode: both see the same machine
        for name, fn in routes:
            times[name].append(median_ms(fn, 1, 0))
    for name, fn in routes:
        out[name + "_ms"], out[name + "_min_ms"], out[name + "_max_ms"] = sorted(times[name])[iters // 2], min(times[name]), max(times[name])
        out[name + "_launches"] = count_launches(fn)
    out["route"] = loop.route
    out["speedup"] = out["baseline_ms"] / out["chain_ms"]
    out["x_max_abs_diff"] = float((logs["baseline"][0] - logs["chain"][0]).abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = []
    for tag, model in (("pendulum->pendulum", PendulumDx()),
                       ("mlp(3,1)H%d->pendulum" % a.hidden, MlpDx(3, 1, a.hidden, seed=0, device_loop=True).cuda())):
        r = run_case(tag, model, a.batch, a.horizon, a.steps, a.iters, a.warmup)
        print(json.dumps(r), flush=True)
        res.append(r)
        assert r["route"] == "chain", "the episode did not run on the device chain"
        assert r["chain_ms"] <= r["baseline_ms"], "the episode chain is slower than the Python loop measured beside it"
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
