#!/usr/bin/env python
"""Recording of what the line-search kernels compute (csrc/line_search.hpp and the kernels that include it).

    DMPC_LIB=/path/to/the/parent/libdmpc_hip.so python tests/golden/make_search_values.py      # needs a GPU

search_values.npz holds the raw outputs of a table of direct C-ABI calls to dmpc_mpc_forward_rec, _pendulum and _mlp - the
smallest call that reaches each search kernel - recorded from the library of the commit BEFORE a change to those kernels;
tests/test_search_values_gpu.py replays the table and compares bit for bit.  Built on make_mpc_routes.py's machinery: rows
that need a latched DMPC_NO_* switch run in a fresh child process per switch, one after another.

Every row's batch mixes the three kinds of trajectory the search tells apart: [0] accepted at the first pass, [B-1] always
worse up to the cap of 64 passes (x = 0, u = 0, C = I, c = 0, K = 0, k = 1, bounds +-0.25: every candidate costs
0.5 |u|^2 more than the nominal 0, and 0.97^63 = 0.15 still moves u), the others accepted after several passes - the
table's random K and k, k scaled until the numpy oracle says so.  The scales are part of the recording."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
NPZ = os.path.join(HERE, "search_values.npz")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def load_routes():
    spec = importlib.util.spec_from_file_location("make_mpc_routes", os.path.join(HERE, "make_mpc_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ROUTES = load_routes()
LS_DECAY, MAX_LS, CAP = 0.97, 5, 64
BOUND = 0.25
PENDULUM = ROUTES.PENDULUM
OUTPUTS = ("x", "u", "costs", "old_costs", "alphas", "objs", "u_first", "n_ls", "info")
ACTS = {0: "tanh", 2: "relu", 3: "silu", 4: "softplus"}


def rows():
    """(id, entry point, nx, nu, B, T, switch or None, the kernel the row is there for)"""
    out = []

    def add(fn, nx, nu, B, T, kernel, switch=None, **kw):
        rid = "%s(%d,%d)B%dT%d%s%s" % (fn, nx, nu, B, T, "".join(",%s=%s" % kv for kv in sorted(kw.items())), "|" + switch if switch else "")
        out.append(dict(id=rid, fn=fn, nx=nx, nu=nu, B=B, T=T, switch=switch, kernel=kernel, **kw))

    add("fwd", 8, 2, 4, 3, "mpc_forward_asm_kernel<8, 2>")                                             # stream
    add("fwd", 8, 2, 4, 3, "mpc_forward_rec_kernel<8, 2, 16, true, false>", "DMPC_NO_MPC_ASM")         # DMA ring
    add("fwd", 8, 2, 5, 3, "mpc_forward_rec_kernel<8, 2, 16, false, false>")                           # register banks
    add("fwd", 5, 3, 4, 3, "mpc_forward_rec_kernel<8, 4, 16, false, true>")                            # PAD container
    add("fwd", 12, 4, 4, 3, "mpc_wide_forward_kernel<12, 4, 2, false>")                                # wide
    add("fwd", 5, 5, 4, 3, "mpc_wide_forward_kernel<12, 8, 2, true>")                                  # wide, padded
    add("fwd", 17, 1, 4, 3, "mpc_staged_forward_kernel")
    add("fwd", 17, 1, 4, 3, "mpc_generic_forward_kernel", "DMPC_NO_MPC_STAGED_FWD")
    add("fwd", 4, 10, 3, 3, "mpc_tiled_forward_kernel")
    add("pend", 3, 1, 4, 3, "mpc_forward_rec_pendulum_spec4_kernel")
    add("pend", 3, 1, 4, 33, "mpc_forward_rec_pendulum_spec_kernel<true>")                             # speculative, DMA
    add("pend", 3, 1, 5, 33, "mpc_forward_rec_pendulum_spec_kernel<false>")                            # speculative, no DMA
    add("pend", 3, 1, 4, 3, "mpc_forward_rec_kernel<3, 1, 16, false, false>", "DMPC_NO_SPEC_LS")       # row kernel, dyn_kind 1
    for act in sorted(ACTS):
        add("mlp", 3, 1, 3, 3, "mpc_forward_rec_mlp_kernel<%d>" % act, act=act, hidden=8)
    assert len(set(r["id"] for r in out)) == len(out)
    return out


SWITCHES = sorted(set(r["switch"] for r in rows() if r["switch"]))


def base_inputs(r):
    """the row's arrays before the (i) / (ii) scaling of k: float64, [T,B,...]; trajectory B-1 is the always-worse one"""
    T, B, nx, nu, fn = r["T"], r["B"], r["nx"], r["nu"], r["fn"]
    ns = nx + nu
    from chainer_differentiable_mpc_amd import synthetic
    d = {}
    if fn == "fwd":
        p, xs = ROUTES.mpc_problem(B, T, nx, nu)
        rng = np.random.RandomState(14)
        d.update(C=p["C"].copy(), c=p["c"].copy(), F=p["F"].copy(), f=p["f"].copy(), states=np.array(xs, dtype=np.float64))
    elif fn == "pend":
        from oracle import box_ddp
        p = synthetic.make_lqr_problem(B, T, 3, 1, seed=15)
        rng = np.random.RandomState(16)
        th = rng.uniform(-np.pi, np.pi, B)
        xs = [np.stack((np.cos(th), np.sin(th), rng.uniform(-1.0, 1.0, B)), axis=1)]
        for t in range(T - 1):       # the nominal trajectory: the pendulum's own rollout under u = 0
            xs.append(box_ddp.pendulum_step(xs[t], np.zeros((B, 1)), *PENDULUM))
        d.update(C=p["C"].copy(), c=p["c"].copy(), states=np.stack(xs).astype(np.float32).astype(np.float64))
    else:
        p = synthetic.make_lqr_problem(B, T, nx, nu, seed=17)
        rng = np.random.RandomState(18)
        H = r["hidden"]
        # W2 = 0, b2 = 0, not residual: next(x, u) = 0 whatever the activation; the nominal trajectory is its rollout
        d.update(W1=0.5 * rng.randn(H, ns), b1=0.1 * rng.randn(H), W2=np.zeros((nx, H)), b2=np.zeros(nx))
        xs = np.zeros((T, B, nx))
        xs[0] = p["x_init"]
        d.update(C=p["C"].copy(), c=p["c"].copy(), states=xs)
    d["Ks"], d["ks"] = 0.1 * rng.randn(T, B, nu, nx), 0.2 * rng.randn(T, B, nu)
    d["controls"] = np.zeros((T, B, nu))
    bound = BOUND if fn != "pend" else PENDULUM[4]
    d["lower"], d["upper"] = -bound * np.ones((T, B, nu)), bound * np.ones((T, B, nu))
    w = B - 1                                                   # (iii)
    d["C"][:, w], d["c"][:, w] = np.eye(ns), 0.0
    d["Ks"][:, w], d["ks"][:, w] = 0.0, 1.0
    d["lower"][:, w], d["upper"][:, w] = -BOUND, BOUND
    if fn == "pend":
        d["states"][:, w] = (1.0, 0.0, 0.0)                     # the equilibrium
    else:
        d["states"][:, w] = 0.0
    if fn == "fwd":
        d["f"][:, w] = 0.0
    return {k: np.asarray(v, dtype=np.float32).astype(np.float64) for k, v in d.items()}


def inputs(r, ks_scale):
    """ks_scale [T,B]: what the table's random k is multiplied by"""
    d = base_inputs(r)
    d["ks"] = (d["ks"] * np.asarray(ks_scale, dtype=np.float64)[:, :, None]).astype(np.float32).astype(np.float64)
    return d


def oracle_passes(r, d, b):
    """trajectory b alone through the numpy oracle -> (passes, still worse at the cap)"""
    from oracle import box_ddp, mpc
    s = {k: v[:, b:b + 1] for k, v in d.items() if k not in ("W1", "b1", "W2", "b2")}
    if r["fn"] == "fwd":
        dyn = mpc.LinDx(s["F"], s["f"])
    elif r["fn"] == "pend":
        def dyn(x, u):
            return box_ddp.pendulum_step(x, u, *PENDULUM)
    else:
        def dyn(x, u):
            return np.zeros_like(x)
    old = mpc.get_cost(r["T"], s["controls"], mpc.QuadCost(s["C"], s["c"]), x=s["states"])
    _, _, res, _, n = mpc.mpc_forward_rec(s["Ks"], s["ks"], s["controls"], s["states"], s["lower"], s["upper"],
                                          mpc.QuadCost(s["C"], s["c"]), dyn, LS_DECAY, MAX_LS, r["T"], max_total_iter=CAP)
    return n, bool(res.costs[0] > old[0])


def choose_scales(r):
    """k's scale per timestep and trajectory, decided on the CPU: trajectory 0 accepted at once, the middle ones after
    3..40 passes (else 2..63).  One factor for the trajectory where that does it; where a clamped descent direction never
    overshoots (one control), a factor of their own for the timesteps from some timestep on."""
    T, B = r["T"], r["B"]
    scale = np.ones((T, B))
    mags = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 0.5, 0.25, 0.1, 0.05, 0.02)
    for b in range(B - 1):
        found = False
        for want in (((1, 1),) if b == 0 else ((3, 40), (2, CAP - 1))):
            signed = [sg * m for m in (mags[::-1] if b == 0 else mags) for sg in (1, -1)]
            for split, s1, s2 in [(T, s, s) for s in signed] + [(t, s1, s2) for t in range(1, min(T, 4)) for s1 in signed for s2 in signed]:
                scale[:split, b], scale[split:, b] = s1, s2
                n, worse = oracle_passes(r, inputs(r, scale), b)
                found = want[0] <= n <= want[1] and not worse
                if found:
                    break
            if found:
                break
        assert found, "no scale of k gives trajectory %d of %s the pass count wanted" % (b, r["id"])
    n, worse = oracle_passes(r, inputs(r, scale), B - 1)
    assert n == CAP and worse, (r["id"], n, worse)
    counts = [oracle_passes(r, inputs(r, scale), b)[0] for b in range(B - 1)]
    assert len(set(counts)) >= 2, (r["id"], counts)
    return scale


def call(r, d, lib, al):
    """the row's call on the allocator's arrays -> (fn(ptr) -> return code, the output arrays in OUTPUTS' order)"""
    T, B, nx, nu = r["T"], r["B"], r["nx"], r["nu"]
    i32 = np.int32
    gains = [al.inp(k, d[k]) for k in ("Ks", "ks", "controls", "states", "lower", "upper", "C", "c")]
    o = dict(x=al.out("x", (T, B, nx)), u=al.out("u", (T, B, nu)), costs=al.out("costs", (B,)), old_costs=al.out("old_costs", (B,)),
             alphas=al.out("alphas", (B,)), objs=al.out("objs", (T, B)), u_first=al.out("u_first", (T, B, nu)),
             n_ls=al.out("n_ls", (B,), i32), info=al.out("info", (B,), i32))
    order = ("x", "u", "costs", "old_costs", "alphas", "objs", "u_first", "n_ls", "info")     # the C ABI's
    if r["fn"] == "fwd":
        Ff = [al.inp("F", d["F"]), al.inp("f", d["f"])]
        return (lambda ptr: lib.dmpc_mpc_forward_rec(T, B, nx, nu, *[ptr(a) for a in gains + Ff], LS_DECAY, MAX_LS,
                                                     *[ptr(o[k]) for k in order], None)), o
    if r["fn"] == "pend":
        return (lambda ptr: lib.dmpc_mpc_forward_rec_pendulum(T, B, *[ptr(a) for a in gains], *PENDULUM, LS_DECAY, MAX_LS,
                                                              *[ptr(o[k]) for k in order], None)), o
    net = [al.inp(k, d[k]) for k in ("W1", "b1", "W2", "b2")]
    return (lambda ptr: lib.dmpc_mpc_forward_rec_mlp(T, B, nx, nu, r["hidden"], r["act"], 0, *[ptr(a) for a in net],
                                                     *[ptr(a) for a in gains], LS_DECAY, MAX_LS, *[ptr(o[k]) for k in order],
                                                     None)), o


def run_rows(switch, scales):
    """the rows of `switch` (None: those that need none) with this process's library -> {id: {output: array, "kernel": name}}"""
    import torch

    sys.path.insert(0, ROOT)
    from chainer_differentiable_mpc_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda:0")
    got = {}
    for r in rows():
        if r["switch"] != switch:
            continue
        al = ROUTES.TorchArrays(dev)
        fn, o = call(r, inputs(r, scales[r["id"]]), lib, al)
        rc = fn(al.ptr)
        name = _lib.last_kernel_name()
        torch.cuda.synchronize()
        assert rc == 0, (r["id"], rc)
        got[r["id"]] = dict({k: o[k].cpu().numpy() for k in OUTPUTS}, kernel=name)
    return got


def flat(got):
    return {"%s/%s" % (rid, k): np.asarray(v) for rid, res in got.items() for k, v in res.items()}


def run_child(switch, scales_path, out_path):
    """the switch's rows in a fresh process -> {id: {...}}"""
    subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", switch, scales_path, out_path],
                   env=ROUTES.switch_env(switch), check=True, timeout=ROUTES.CHILD_TIMEOUT)
    with np.load(out_path) as z:
        got = {}
        for key in z.files:
            rid, k = key.rsplit("/", 1)
            got.setdefault(rid, {})[k] = z[key] if k != "kernel" else str(z[key])
    return got


def record(tmp, scales):
    """every row, each process one after another -> the flat recording"""
    scales_path = os.path.join(tmp, "scales.json")
    with open(scales_path, "w") as fh:
        json.dump({k: v.tolist() for k, v in scales.items()}, fh)
    got = {}
    for switch in ["none"] + SWITCHES:
        got.update(run_child(switch, scales_path, os.path.join(tmp, switch + ".npz")))
    for r in rows():
        res = got[r["id"]]
        assert r["kernel"] in res["kernel"], (r["id"], res["kernel"])
        assert res["n_ls"][-1] == CAP and res["info"][-1] & 8, (r["id"], res["n_ls"], res["info"])
        assert len(set(res["n_ls"][:-1].tolist())) >= 2 and not (res["info"][:-1] & 8).any(), (r["id"], res["n_ls"])
    rec = flat(got)
    rec.update({"%s/ks_scale" % rid: s for rid, s in scales.items()})
    return rec


def main():
    import tempfile
    if len(sys.argv) == 5 and sys.argv[1] == "--rows":
        with open(sys.argv[3]) as fh:
            scales = json.load(fh)
        np.savez(sys.argv[4], **flat(run_rows(None if sys.argv[2] == "none" else sys.argv[2], scales)))
        return
    with tempfile.TemporaryDirectory() as tmp:
        scales = {r["id"]: choose_scales(r) for r in rows()}
        first = record(tmp, scales)
        second = record(tmp, scales)
    assert sorted(first) == sorted(second)
    for k in first:     # recorded twice: a table that is not deterministic records nothing
        assert first[k].dtype == second[k].dtype and first[k].tobytes() == second[k].tobytes(), "two recordings differ in " + k
    np.savez_compressed(NPZ, **first)
    print("wrote", NPZ, "-", len(rows()), "rows,", os.path.getsize(NPZ), "bytes; passes per row:",
          {r["id"]: first[r["id"] + "/n_ls"].tolist() for r in rows()})


if __name__ == "__main__":
    main()
