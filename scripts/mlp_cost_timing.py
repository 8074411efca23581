"""One `BoxDDP` solve, and one solve plus gradient, under a learned stage cost (`MlpCost`) with a dense `LinDx`,
four ways on equal weights in the same run:
  live    - the `MlpCost` module as it is (param_grad="live"): the Taylor model of one launch and the line search inside its
            kernel wherever no gradient is wanted; the final gradient model through `approximate_cost`'s autograd route;
  device  - `MlpCost(param_grad="device")`: the final gradient model too is one launch, its backward `dmpc_mlp_cost_param_grad`;
  chain   - `MlpCost(device_loop=True, param_grad="device")`: the iLQR loop itself as one chain of launches with one read-back
            (`dmpc_box_ddp_mlp_cost`, replayed from the solver's hipGraph from the third call on); the gradient as "device".
            Its yardstick is "device" - the host loop over the same kernels - not the lambda (`chain_over_device`);
  lambda  - the same module behind `lambda tau: cost(tau)`: T (1 + ns) autograd calls per iLQR iteration and the line search as a
            Python loop - the only route a cost that is not quadratic had before `MlpCost` (the baseline).
The variants take turns solve by solve (one round = one solve of each), after `--warmup` rounds; reported per variant: the
median and the minimum over `--iters` rounds of device events around the whole call (host time included), the iterations the
solve ran, and how far its costs (and, with the gradient, its gradients) are from the baseline's.

    python scripts/mlp_cost_timing.py [--iters 10] [--warmup 2] [--cases 3x1x32,8x2x64] [--batch 128] [--horizon 20] [--json out]"""
import argparse
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from chainer_differentiable_mpc_amd import BoxDDP, LinDx, MlpCost, synthetic  # noqa: E402

VARIANTS = ("live", "device", "chain", "lambda")


def run_case(nx, nu, H, B, T, iters, warmup, grad):
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=1)
    dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")   # noqa: E731
    x0, dyn = dev(p["x_init"]), LinDx(dev(p["F"]), dev(p["f"]))
    gen = torch.Generator().manual_seed(2)
    lin = 0.3 * torch.randn(nx + nu, generator=gen)
    routes = {}
    for tag in VARIANTS:
        m = MlpCost(nx, nu, H, seed=0, p=lin, param_grad="device" if tag in ("device", "chain") else "live",
                    device_loop=tag == "chain").cuda()
        cost = (lambda tau, m=m: m(tau)) if tag == "lambda" else m
        solver = BoxDDP(T, -0.5, 0.5, B, nx, nu, None, max_iter=10, quiet=True, detach_unconverged=False,
                        update_dynamics=False)      # the gradient goes to the cost
        routes[tag] = dict(m=m, cost=cost, solver=solver, ms=[])

    def once(tag, record=True):
        r = routes[tag]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        r["m"].zero_grad(set_to_none=True)
        a.record()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if grad:
                x, u, costs = r["solver"]((x0, r["cost"], dyn))
                (x.sum() + u.sum()).backward()
            else:
                with torch.no_grad():
                    x, u, costs = r["solver"]((x0, r["cost"], dyn))
        b.record()
        b.synchronize()
        r["costs"] = costs.detach()
        if record:
            r["ms"].append(a.elapsed_time(b))

    for _ in range(warmup):
        for tag in VARIANTS:
            once(tag, record=False)
    for _ in range(iters):
        for tag in VARIANTS:
            once(tag)
    out = dict(nx=nx, nu=nu, n_hidden=H, B=B, T=T, leg="solve+grad" if grad else "solve", rounds=iters)
    base = routes["lambda"]
    for tag, r in routes.items():
        ms = sorted(r["ms"])
        out[tag + "_ms"], out[tag + "_min_ms"], out[tag + "_n_iter"] = ms[len(ms) // 2], ms[0], r["solver"].n_iter
        out[tag + "_costs_max_rel_diff"] = float(((r["costs"] - base["costs"]).abs() / base["costs"].abs().clamp(min=1.0)).max())
        if grad:
            out[tag + "_grads_max_rel_diff"] = max(float(((a.grad - b.grad).abs() / b.grad.abs().clamp(min=1.0)).max())
                                                   for a, b in zip(r["m"].parameters(), base["m"].parameters()))
        out[tag + "_speedup"] = None
    for tag in VARIANTS:
        out[tag + "_speedup"] = out["lambda_ms"] / out[tag + "_ms"]
    out["chain_over_device"] = out["device_ms"] / out["chain_ms"]          # the chain against the host loop over the same kernels
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="3x1x32,8x2x64")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = []
    for c in a.cases.split(","):
        nx, nu, H = (int(v) for v in c.split("x"))
        for grad in (False, True):
            r = run_case(nx, nu, H, a.batch, a.horizon, a.iters, a.warmup, grad)
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
