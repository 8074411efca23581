"""One `BoxDDP` solve under a learned dynamics model with one or two hidden layers, two ways in the same run:
  device   - the `MlpDx` module itself: rollout + linearisation in one launch, the line search inside its kernel;
  callable - the same module behind `lambda x, u: m(x, u)`: `linearize_dynamics` through torch.autograd and the line search
             as torch ops around the callable - the route every non-linear dynamics took before `MlpDx` (the baseline).
Medians over `--iters` solves after warm-up (device events around the whole solve, host time included), the number of
kernel launches of one solve of each, and how far the two solutions' costs are apart.

`--grad` times learning instead: one `BoxDDP(update_dynamics=True, detach_unconverged=False)` solve with grad enabled plus
`backward` of sum(x) + sum(u), for `MlpDx(param_grad="device")` (the gradient node's backward is `dmpc_mlp_param_grad`, with
`--hidden2` `dmpc_mlp2_param_grad`; the output keys keep the name `device_grad`) and `param_grad="live"` (a live torch rollout
and autograd through it: the baseline) on equal weights in the same run.

`--chain` times the iLQR loop itself: the host loop (`MlpDx(device_loop=False)`, the default route) against `dmpc_box_ddp`'s
chain with the network inside it (`device_loop=True`: `search_linearizes` 0 and 1 launched directly, and the hipGraph replay).

`--sweeps LIB[,LIB...]` times the gradient sweeps themselves (csrc/mlp_grad_kernels.hpp): `dmpc_mlp_param_grad`,
`dmpc_mlp2_param_grad` and `dmpc_mlp_rollout_grad` called directly through the C ABI of each named library (`tree`: the one in
the tree) - device events around a burst of back-to-back calls on one stream, long enough that the kernel is resolved, the
median and the range over `--iters` bursts, in ms per call.  The libraries take turns, the whole round twice, so a parent and
a head library are measured alternately in one run; with two libraries the two-run rule of DESIGN.md 3.4 is applied to the
second against the first (its worse run no further above the first's mean than the first's two runs are apart).  Sizes:
`--batch`, `--horizon` with (3,1) H 32, (8,2) H 64, (8,2) H (64,64) and each depth's largest model.

`--activation` picks the network (tanh, relu, silu, softplus; default tanh, whose output lines are what they were before
the flag existed - another activation adds an "activation" key).

`--hidden2 H2` makes every case a two-layer network: the H of `--cases` is its first width, H2 its second ("n_hidden" is then
the pair).  The run fails if the device route is not faster than the plain callable measured beside it; with `--grad`, if
solve + backward on the device route is slower than on the live route of the same run.

    python scripts/mlp_dx_timing.py [--grad | --chain | --sweeps parent.so,tree] [--iters 20] [--warmup 3] [--cases 3x1x32,8x2x64] [--batch 128] [--horizon 20]
                                    [--activation tanh] [--hidden2 H2] [--json out]"""
import argparse
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from chainer_differentiable_mpc_amd import BoxDDP, MlpDx, QuadCost, synthetic  # noqa: E402


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def count_launches(fn):
    """kernel launches of one call, as the profiler sees them (None where it records no device activity)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:       # a build without the device tracer
        return None


def run_case(nx, nu, H, B, T, iters, warmup, activation="tanh"):
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=1)
    dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")   # noqa: E731
    x0, cost = dev(p["x_init"]), QuadCost(dev(p["C"]), dev(p["c"]))
    m = MlpDx(nx, nu, H, seed=0, activation=activation).cuda()
    out = dict(nx=nx, nu=nu, n_hidden=H, B=B, T=T)
    if activation != "tanh":
        out["activation"] = activation
    sols = {}
    for tag, dyn in (("device", m), ("callable", lambda x, u: m(x, u))):
        solver = BoxDDP(T, -0.5, 0.5, B, nx, nu, None, max_iter=10, quiet=True)

        def solve():
            with torch.no_grad(), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sols[tag] = solver((x0, cost, dyn))
        out[tag + "_ms"] = median_ms(solve, iters, warmup)
        out[tag + "_launches"] = count_launches(solve)
        out[tag + "_n_iter"], out[tag + "_status"] = solver.n_iter, solver.status
    out["speedup"] = out["callable_ms"] / out["device_ms"]
    cd, cc = sols["device"][2], sols["callable"][2]
    out["costs_max_rel_diff"] = float(((cd - cc).abs() / cc.abs().clamp(min=1.0)).max())
    return out


def run_chain_case(nx, nu, H, B, T, iters, warmup, activation="tanh"):
    """the iLQR loop four ways on equal weights in ONE run: the host loop over MPCstep objects (`device_loop=False`, the
    default route), `dmpc_box_ddp`'s chain (dyn_kind 2) launched directly with `search_linearizes` 0 and 1, and the chain
    replayed from the solver's hipGraph at the setting `MlpDx` passes.  Medians of device events around the whole solve
    (host time included), the launches of one solve, and each route's costs against the host loop's."""
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=1)
    dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")   # noqa: E731
    x0, cost = dev(p["x_init"]), QuadCost(dev(p["C"]), dev(p["c"]))
    out = dict(nx=nx, nu=nu, n_hidden=H, B=B, T=T, leg="chain", passed_search_linearizes=int(MlpDx.SEARCH_LINEARIZES))
    if activation != "tanh":
        out["activation"] = activation
    sols = {}
    # (tag, device_loop, search_linearizes or None for the class's own, graph)
    for tag, loop, lin, graph in (("host_loop", False, None, False), ("chain_lin0", True, False, False),
                                  ("chain_lin1", True, True, False), ("chain_graph", True, None, True)):
        m = MlpDx(nx, nu, H, seed=0, activation=activation, device_loop=loop).cuda()
        if lin is not None:
            m.SEARCH_LINEARIZES = lin
        solver = BoxDDP(T, -0.5, 0.5, B, nx, nu, None, max_iter=10, quiet=True, graph=graph)

        def solve():
            with torch.no_grad(), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sols[tag] = solver((x0, cost, m))
        out[tag + "_ms"] = median_ms(solve, iters, warmup)
        out[tag + "_launches"] = count_launches(solve)
        out[tag + "_n_iter"], out[tag + "_status"] = solver.n_iter, solver.status
        if graph:
            out[tag + "_recorded"] = any(e[0] is not None for e in solver._graphs.values())
    ch = sols["host_loop"][2]
    for tag in ("chain_lin0", "chain_lin1", "chain_graph"):
        out[tag + "_speedup"] = out["host_loop_ms"] / out[tag + "_ms"]
        out[tag + "_costs_max_rel_diff"] = float(((sols[tag][2] - ch).abs() / ch.abs().clamp(min=1.0)).max())
    out["lin1_equals_lin0"] = all(bool(torch.equal(a, b)) for a, b in zip(sols["chain_lin0"], sols["chain_lin1"]))
    return out


def run_grad_case(nx, nu, H, B, T, iters, warmup, activation="tanh"):
    """both routes on equal weights, alternating solve by solve; per route the median of solve + backward and of the
    backward alone (device events, host time included), the launches of one solve + backward, the sampled clocks"""
    from bench import ClockSampler
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=1)
    dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")   # noqa: E731
    x0, cost = dev(p["x_init"]), QuadCost(dev(p["C"]), dev(p["c"]))
    out = dict(nx=nx, nu=nu, n_hidden=H, B=B, T=T, leg="grad", rounds=iters)
    if activation != "tanh":
        out["activation"] = activation
    routes = {}
    for tag, flag in (("device_grad", True), ("live", False)):
        m = MlpDx(nx, nu, H, seed=0, param_grad="device" if flag else "live", activation=activation).cuda()
        solver = BoxDDP(T, -0.5, 0.5, B, nx, nu, None, max_iter=10, quiet=True, update_dynamics=True, detach_unconverged=False)
        routes[tag] = (m, solver, [], [])

    def once(tag, record=True):
        m, solver, total, back = routes[tag]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        m.zero_grad(set_to_none=True)
        ev[0].record()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x, u, _ = solver((x0, cost, m))
        ev[1].record()
        (x.sum() + u.sum()).backward()
        ev[2].record()
        ev[2].synchronize()
        if record:
            total.append(ev[0].elapsed_time(ev[2]))
            back.append(ev[1].elapsed_time(ev[2]))

    for _ in range(warmup):
        for tag in routes:
            once(tag, record=False)
    with ClockSampler() as clocks:
        for _ in range(iters):
            for tag in routes:
                once(tag)
    summary = clocks.summary() or {}          # hwmon sclk / mclk / power during the timed rounds; null where not shown
    out["clocks"] = {k: summary.get(k) for k in ("sclk_mhz", "mclk_mhz", "power_w")}
    for tag, (m, solver, total, back) in routes.items():
        out[tag + "_ms"], out[tag + "_backward_ms"] = sorted(total)[len(total) // 2], sorted(back)[len(back) // 2]
        out[tag + "_min_ms"] = min(total)
        out[tag + "_launches"] = count_launches(lambda: once(tag, record=False))
        out[tag + "_n_iter"] = solver.n_iter
    out["speedup"] = out["live_ms"] / out["device_grad_ms"]
    out["backward_speedup"] = out["live_backward_ms"] / out["device_grad_backward_ms"]
    out["grads_max_rel_diff"] = max(float(((a.grad - b.grad).abs() / b.grad.abs().clamp(min=1.0)).max())
                                    for a, b in zip(routes["device_grad"][0].parameters(), routes["live"][0].parameters()))
    return out


SWEEP_CASES = ((3, 1, (32,)), (8, 2, (64,)), (8, 2, (64, 64)), (16, 8, (256,)), (16, 8, (128, 128)))


def run_sweeps(libs, B, T, iters, burst=20):
    """-> one dict per (model, entry point): per library its two runs' (median, min, max) ms per call, and the rule"""
    import numpy as np

    from chainer_differentiable_mpc_amd import _lib
    loaded = [(name, _lib.load() if name == "tree" else _lib.load(name)) for name in libs]
    ptr = lambda t: t.data_ptr()   # noqa: E731
    res = []
    for nx, nu, hidden in SWEEP_CASES:
        m = MlpDx(nx, nu, hidden[0] if len(hidden) == 1 else hidden, seed=0).cuda()
        w = [p.detach().contiguous() for p in m._weights()]
        if len(hidden) == 2:          # the C ABI's [W2 | W3], [b2 | b3]
            w = [w[0], w[1], torch.cat((w[2].reshape(-1), w[4].reshape(-1))), torch.cat((w[3], w[5]))]
        code = hidden[0] if len(hidden) == 1 else _lib.mlp_hidden2(*hidden)
        rng = np.random.RandomState(1)
        dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device="cuda")   # noqa: E731
        x_init, u, g = dev(rng.randn(B, nx)), dev(0.5 * rng.randn(T, B, nu)), dev(rng.randn(T, B, nx))
        x = torch.zeros(T, B, nx, device="cuda")
        head = [T, B, nx, nu, code, 0, 1] + [ptr(a) for a in w]
        assert loaded[0][1].dmpc_mlp_rollout_linearize(*head, ptr(x_init), ptr(u), ptr(x), None, None, None) == 0
        outs = [torch.zeros_like(a) for a in w] + [torch.zeros(B, nx, device="cuda"), torch.zeros(T, B, nu, device="cuda")]
        weight_grad = "dmpc_mlp_param_grad" if len(hidden) == 1 else "dmpc_mlp2_param_grad"
        for entry in (weight_grad, "dmpc_mlp_rollout_grad"):
            row = dict(leg="sweeps", nx=nx, nu=nu, n_hidden=list(hidden), B=B, T=T, entry=entry, burst=burst, runs={n: [] for n, _ in loaded})
            for _ in range(2):
                for name, lib in loaded:
                    need = getattr(lib, entry + "_workspace_bytes")(B, nx, nu, code)
                    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
                    args = head + [ptr(x), ptr(u), ptr(g)] + [ptr(o) for o in outs] + [ptr(ws), need, None]

                    def calls():
                        for _ in range(burst):
                            assert getattr(lib, entry)(*args) == 0
                    for _ in range(3):
                        calls()
                    torch.cuda.synchronize()
                    ts = []
                    for _ in range(iters):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        calls()
                        b.record()
                        b.synchronize()
                        ts.append(a.elapsed_time(b) / burst)
                    ts.sort()
                    row["runs"][name].append((ts[len(ts) // 2], ts[0], ts[-1]))
            if len(loaded) == 2:
                first, second = ([r[0] for r in row["runs"][n]] for n, _ in loaded)
                row["above_first_mean"] = max(second) - sum(first) / 2
                row["first_apart"] = abs(first[0] - first[1])
                row["inside_rule"] = row["above_first_mean"] <= row["first_apart"]
            res.append(row)
    return res


def print_sweeps_table(res):
    """the rows once more as a table: per library the medians of its two runs; with two libraries the rule's columns"""
    names = list(res[0]["runs"])
    print("# libraries, in column order: " + ", ".join("%d = %s" % (i + 1, n) for i, n in enumerate(names)))
    rule = "  %8s %7s  rule" % ("excess", "spread") if len(names) == 2 else ""
    print("%-18s %-22s " % ("model", "entry") + " ".join("%8s %8s" % ("%d a" % (i + 1), "%d b" % (i + 1)) for i in range(len(names))) + rule)
    for r in res:
        line = "%-18s %-22s " % ("(%d,%d) H=%s" % (r["nx"], r["nu"], ",".join(str(h) for h in r["n_hidden"])), r["entry"])
        line += " ".join("%8.4f %8.4f" % (r["runs"][n][0][0], r["runs"][n][1][0]) for n in names)
        if len(names) == 2:
            line += "  %+8.4f %7.4f  %s" % (r["above_first_mean"], r["first_apart"], "ok" if r["inside_rule"] else "ABOVE")
        print(line)
    if len(names) == 2:
        print("rows above the rule: %s" % ([(r["n_hidden"], r["entry"]) for r in res if not r["inside_rule"]] or "none"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grad", action="store_true")
    ap.add_argument("--sweeps", default=None, help="libraries whose gradient entry points are timed in turn: paths, or `tree`")
    ap.add_argument("--chain", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="3x1x32,8x2x64")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--activation", default="tanh", choices=["tanh", "relu", "silu", "softplus"])
    ap.add_argument("--hidden2", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = []
    if a.sweeps:
        res = run_sweeps(a.sweeps.split(","), a.batch, a.horizon, max(a.iters, 20))
        for r in res:
            print(json.dumps(r), flush=True)
        print_sweeps_table(res)
    for c in ([] if a.sweeps else a.cases.split(",")):
        nx, nu, H = (int(v) for v in c.split("x"))
        if a.hidden2 > 0:
            H = (H, a.hidden2)
        r = (run_chain_case if a.chain else run_grad_case if a.grad else run_case)(nx, nu, H, a.batch, a.horizon, max(a.iters, 20), a.warmup, a.activation)
        print(json.dumps(r), flush=True)
        res.append(r)
        if a.hidden2 > 0 and not (a.chain or a.grad):
            assert r["device_ms"] < r["callable_ms"], "the device route is not faster than the plain callable"
        if a.hidden2 > 0 and a.grad:
            assert r["device_grad_ms"] <= r["live_ms"], "the device gradient route is slower than the live route"
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
