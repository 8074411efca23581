#!/usr/bin/env python
"""Recording of the MPC step dispatch (csrc/mpc_api.hip): which kernel takes a call.

    python tests/golden/make_mpc_routes.py            # mpc_routes.json: return code and last kernel of a case table (needs a GPU)

Recorded from the library in the tree (or `DMPC_LIB`) at the commit BEFORE a change to the dispatch;
tests/test_mpc_routes_gpu.py replays it.  Regenerating at an unchanged dispatch gives a byte-identical file.  The table runs
once with no switch set and once per latched DMPC_NO_* switch, each in a child process of its own (`--rows OUT`), one after
another; of a switch's run the file keeps the rows that differ from the run with none set."""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
JSON = os.path.join(HERE, "mpc_routes.json")

SWITCHES = ["DMPC_NO_MPC_ASM", "DMPC_NO_MPC_DMA", "DMPC_NO_WIDE", "DMPC_NO_CONTAINER", "DMPC_NO_MPC_WAVE", "DMPC_NO_MPC_FUSED",
            "DMPC_NO_MPC_STAGED_FWD", "DMPC_NO_SPEC_LS", "DMPC_NO_SPEC4"]
CHILD_TIMEOUT = 120      # seconds, per child: a few seconds of work behind the start of the runtime
LS_DECAY, MAX_LS, N_QP = 0.2, 5, 10
PENDULUM = (10.0, 1.0, 1.0, 0.05, 2.0)       # g, m, l, dt, max_torque

STREAM = [(8, 2), (3, 1), (4, 2), (6, 2), (2, 2), (1, 1), (2, 1), (3, 2)]     # the generated streams' shapes
RING = [(4, 4), (8, 4), (12, 3)]                                              # LDS-DMA ring only
CONTAINED = [(2, 3), (5, 3), (9, 1), (9, 2)]                                  # -> (4,4), (8,4), (14,1), (13,2)
WIDE = [(12, 4), (16, 4), (12, 8), (16, 8)]
WIDE_PADDED = [(5, 5), (9, 4), (14, 2)]
WAVE_CONTAINED = [(10, 6), (24, 8), (32, 4), (24, 2), (21, 3), (20, 2)]       # ((20,2) stays on the runtime-dimension kernel)
# ((62,1): the largest staged search there is, 68 KB of LDS - no shape with nx + nu + 1 <= 64 passes the 150 KB bound)
RUNTIME = [(17, 1), (40, 5), (62, 1)]
TILED = [(4, 10), (70, 3)]


# ---- the case table: (entry point, nx, nu, B, T, options) ----
def cases():
    out = []

    def add(fn, nx, nu, B, T, **kw):
        tag = "".join("+" + k if v is True else "-" + k if v is False else ",%s=%s" % (k, v) for k, v in sorted(kw.items()))
        out.append(dict(id="%s(%d,%d)B%dT%d%s" % (fn, nx, nu, B, T, tag), fn=fn, nx=nx, nu=nu, B=B, T=T, **kw))

    def forms(nx, nu, B, T=3):
        """the sweep with f_hat and without, the search, the step re-centring and not"""
        add("back", nx, nu, B, T, has_f=True)
        add("back", nx, nu, B, T, has_f=False)
        add("fwd", nx, nu, B, T)
        add("step", nx, nu, B, T, expand=0)
        add("step", nx, nu, B, T, expand=1)

    def coupled(nx, nu, B, T=3):
        """batch-coupled: cooperative on the whole batch, and with DMPC_NO_COOP_REGISTER=1 (read per call) the fixed grid"""
        for mode in ("coop", "fixed"):
            add("back", nx, nu, B, T, coupled=mode)
            add("step", nx, nu, B, T, coupled=mode, expand=1)

    for nx, nu in STREAM:
        for B in ((3, 4, 5, 8) if (nx, nu) in ((8, 2), (3, 1)) else (4, 5)):
            forms(nx, nu, B)
    forms(8, 2, 4, T=2)
    forms(3, 1, 8, T=2)
    for nx, nu in RING:
        for B in (4, 5):
            forms(nx, nu, B)
    for nx, nu in CONTAINED:
        for B in (4, 5):
            forms(nx, nu, B)
    forms(9, 3, 5)
    forms(10, 4, 5)
    for nx, nu in WIDE:
        for B in (3, 4, 5):
            forms(nx, nu, B)
    forms(12, 4, 4, T=2)
    for nx, nu in WIDE_PADDED:
        for B in (4, 5):        # (B = 5: no whole wavefronts, refused by the wide instances)
            forms(nx, nu, B)
    forms(32, 8, 4)
    forms(32, 8, 3, T=2)
    for nx, nu in WAVE_CONTAINED + RUNTIME:
        forms(nx, nu, 4)
    for nx, nu in TILED:
        for B in (3, 4):
            forms(nx, nu, B)
    # batch-coupled, one shape or two per family
    for nx, nu, B in ((8, 2, 4), (8, 2, 5), (3, 1, 8), (4, 4, 4), (5, 3, 4), (9, 2, 5), (12, 4, 4), (5, 5, 4), (16, 8, 3), (32, 8, 4),
                      (24, 8, 4), (17, 1, 4), (40, 5, 3), (4, 10, 3), (70, 3, 4)):
        coupled(nx, nu, B)
    # a misaligned `controls` per ring family: stream, ring, wide exact, wide padded (and the pendulum's below)
    for nx, nu in ((8, 2), (3, 1), (4, 4), (12, 4), (5, 5)):
        add("back", nx, nu, 4, 3, has_f=True, unaligned=True)
        add("fwd", nx, nu, 4, 3, unaligned=True)
        add("step", nx, nu, 4, 3, expand=1, unaligned=True)
    # workspaces: one byte short, and absent where one is needed
    for nx, nu, B in ((8, 2, 4), (4, 10, 4), (70, 3, 3)):
        add("step", nx, nu, B, 3, expand=1, ws="short")
        add("step", nx, nu, B, 3, expand=1, ws="none")
    for nx, nu, B in ((4, 10, 4), (70, 3, 3)):
        add("back", nx, nu, B, 3, has_f=True, ws="short")
        add("back", nx, nu, B, 3, has_f=True, ws="none")
    for nx, nu, B in ((8, 2, 4), (5, 3, 4), (4, 10, 3)):
        add("back", nx, nu, B, 3, coupled="coop", ws="short")
        add("back", nx, nu, B, 3, coupled="coop", ws="none")
        add("step", nx, nu, B, 3, coupled="coop", expand=1, ws="short")
    # the pendulum's search: a wavefront per trajectory up to kSpec4MaxT = 32 steps, sixteen candidates per trajectory above
    for B in (3, 4, 5, 8):
        for T in (2, 3):
            add("pend", 3, 1, B, T)
    add("pend", 3, 1, 4, 33)
    add("pend", 3, 1, 5, 33)
    add("pend", 3, 1, 4, 33, unaligned=True)
    add("pend", 3, 1, 4, 3, unaligned=True)
    # PNQP: register kernels up to eight unknowns, the tiled kernel beyond
    for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 13):
        add("pnqp", n, n, 5, 1)
    for n, B in ((4, 5), (8, 3), (9, 5), (13, 4)):
        add("pnqp", n, n, B, 1, coupled="coop")
        add("pnqp", n, n, B, 1, coupled="fixed")
    for n in (4, 9):
        add("pnqp", n, n, 5, 1, coupled="coop", ws="short")
        add("pnqp", n, n, 5, 1, coupled="coop", ws="none")
        add("pnqp", n, n, 5, 1, coupled="fixed", ws="coupled_only")     # the decision slots without the fixed grid's rows
    assert len(set(c["id"] for c in out)) == len(out)
    return out


class TorchArrays:
    """the arrays of a case: one torch tensor each (tests/golden/make_lqr_routes.py's allocator, with an offset view)"""

    def __init__(self, device):
        import torch
        self.torch, self.device = torch, device

    def inp(self, name, array, dtype=np.float32, offset_words=0):
        flat = np.asarray(array, dtype=dtype)
        if offset_words:       # a view `offset_words` elements into a longer allocation
            t = self.torch.as_tensor(np.concatenate((np.zeros(offset_words, dtype), flat.reshape(-1))), device=self.device)
            return t[offset_words:].view(flat.shape)
        return self.torch.as_tensor(flat, device=self.device)

    def out(self, name, shape, dtype=np.float32):
        return self.torch.zeros(tuple(shape), dtype=getattr(self.torch, np.dtype(dtype).name), device=self.device)

    def ws(self, name, nbytes):
        return self.torch.zeros(max(nbytes, 16), dtype=self.torch.uint8, device=self.device)

    @staticmethod
    def ptr(t):
        return None if t is None else t.data_ptr()


_PROBLEMS = {}


def mpc_problem(B, T, nx, nu):
    """an MPC step from u = 0 and its nominal rollout (tests/abi_calls.py's)"""
    key = (B, T, nx, nu)
    if key not in _PROBLEMS:
        from chainer_differentiable_mpc_amd import synthetic
        p = synthetic.make_lqr_problem(B, T, nx, nu, seed=11)
        xs = [p["x_init"]]
        for t in range(T - 1):
            xs.append(np.einsum("bij,bj->bi", p["F"][t], np.concatenate((xs[t], np.zeros((B, nu))), axis=1)) + p["f"][t])
        _PROBLEMS[key] = (p, np.stack(xs))
    return _PROBLEMS[key]


def call(c, lib, al):
    """the arrays of case c from the allocator `al` -> fn: `fn(ptr)` makes the case's call and returns its code"""
    T, B, nx, nu, fn = c["T"], c["B"], c["nx"], c["nu"], c["fn"]
    is_coupled = 1 if c.get("coupled") else 0
    off = 1 if c.get("unaligned") else 0       # `controls` 4 bytes into its allocation
    i32 = np.int32

    def workspace(need, coupled_only=0):
        kind = c.get("ws", "ok")
        if kind == "none":
            return None, need
        given = {"ok": need, "short": need - 1, "coupled_only": coupled_only}[kind]
        return al.ws("ws", given), given

    if fn == "pnqp":
        from chainer_differentiable_mpc_amd import synthetic
        n, n_iter = nx, 20
        q = synthetic.make_box_qp(B, n, seed=3 + n)
        H, qq, lo, hi = (al.inp(k, q[k]) for k in ("H", "q", "lower", "upper"))
        ws, given = workspace(lib.dmpc_pnqp_workspace_bytes(B, n, n_iter, is_coupled), lib.dmpc_coupled_workspace_bytes(1, n_iter))
        outs = [al.out("x", (B, n)), al.out("fac", (B, n, n)), al.out("piv", (B, n), i32), al.out("index_f", (B, n)),
                al.out("n_iter_out", (B,), i32)]
        info = al.out("info", (B,), i32)
        return lambda ptr: lib.dmpc_pnqp(B, n, ptr(H), ptr(qq), ptr(lo), ptr(hi), None, n_iter, is_coupled, *[ptr(o) for o in outs],
                                         ptr(ws), given, ptr(info), None)

    def search_outputs():
        return [al.out("x_out", (T, B, nx)), al.out("u_out", (T, B, nu)), al.out("costs", (B,)), al.out("old_costs", (B,)),
                al.out("alphas", (B,)), al.out("objs", (T, B)), al.out("u_first", (T, B, nu)), al.out("n_ls_iter", (B,), i32)]

    info = al.out("info", (B,), i32)
    if fn == "pend":
        from chainer_differentiable_mpc_amd import synthetic
        p = synthetic.make_lqr_problem(B, T, 3, 1, seed=15)
        rng = np.random.RandomState(16)
        th = rng.uniform(-np.pi, np.pi, (T, B))
        states = np.stack((np.cos(th), np.sin(th), rng.uniform(-1.0, 1.0, (T, B))), axis=2)
        ins = [al.inp("Ks", 0.1 * rng.randn(T, B, 1, 3)), al.inp("ks", 0.2 * rng.randn(T, B, 1)),
               al.inp("controls", np.zeros((T, B, 1)), offset_words=off), al.inp("states", states),
               al.inp("u_lower", -2.0 * np.ones((T, B, 1))), al.inp("u_upper", 2.0 * np.ones((T, B, 1))), al.inp("C", p["C"]),
               al.inp("c", p["c"])]
        outs = search_outputs()
        return lambda ptr: lib.dmpc_mpc_forward_rec_pendulum(T, B, *[ptr(a) for a in ins], *PENDULUM, LS_DECAY, MAX_LS,
                                                             *[ptr(o) for o in outs], ptr(info), None)

    p, xs = mpc_problem(B, T, nx, nu)
    bound = 0.25
    C, cc, F = al.inp("C", p["C"]), al.inp("c", p["c"]), al.inp("F", p["F"])
    f = al.inp("f", p["f"]) if c.get("has_f", True) else None
    u = al.inp("controls", np.zeros((T, B, nu)), offset_words=off)
    lo, hi = al.inp("u_lower", -bound * np.ones((T, B, nu))), al.inp("u_upper", bound * np.ones((T, B, nu)))
    if fn == "back":
        ws, given = workspace(lib.dmpc_mpc_backward_rec_workspace_bytes(T, B, nx, nu, N_QP, is_coupled))
        Ks, ks, nqp = al.out("Ks", (T, B, nu, nx)), al.out("ks", (T, B, nu)), al.out("n_qp_iter", (B,), i32)
        return lambda ptr: lib.dmpc_mpc_backward_rec(T, B, nx, nu, ptr(C), ptr(cc), ptr(F), ptr(f), ptr(u), ptr(lo), ptr(hi), N_QP,
                                                     is_coupled, ptr(Ks), ptr(ks), ptr(nqp), ptr(ws), given, ptr(info), None)
    states = al.inp("states", xs)
    if fn == "fwd":
        rng = np.random.RandomState(14)
        Ks, ks = al.inp("Ks", 0.1 * rng.randn(T, B, nu, nx)), al.inp("ks", 0.2 * rng.randn(T, B, nu))
        outs = search_outputs()
        return lambda ptr: lib.dmpc_mpc_forward_rec(T, B, nx, nu, ptr(Ks), ptr(ks), ptr(u), ptr(states), ptr(lo), ptr(hi), ptr(C), ptr(cc),
                                                    ptr(F), ptr(f), LS_DECAY, MAX_LS, *[ptr(o) for o in outs], ptr(info), None)
    assert fn == "step"
    ws, given = workspace(lib.dmpc_mpc_step_workspace_bytes(T, B, nx, nu))
    so = search_outputs()
    Ks, ks, nqp = al.out("Ks", (T, B, nu, nx)), al.out("ks", (T, B, nu)), al.out("n_qp_iter", (B,), i32)
    outs = so[:2] + [Ks, ks] + so[2:7] + [nqp, so[7]]
    return lambda ptr: lib.dmpc_mpc_step_forward(T, B, nx, nu, ptr(C), ptr(cc), ptr(F), ptr(f), ptr(u), ptr(states), ptr(lo), ptr(hi),
                                                 ptr(C), ptr(cc), ptr(F), ptr(f), c["expand"], LS_DECAY, MAX_LS, N_QP, is_coupled,
                                                 *[ptr(o) for o in outs], ptr(ws), given, ptr(info), None)


def run_cases():
    """-> [{id, rc, kernel}] with this process's switches; kernel None: the call launched nothing"""
    import torch

    sys.path.insert(0, ROOT)
    from chainer_differentiable_mpc_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda:0")
    ptr = _lib.ptr
    s_in = [torch.zeros(shape, dtype=torch.float32, device=dev) for shape in ((1, 1, 1, 2), (1, 1, 1), (1, 2))]
    s_out = [torch.zeros(shape, dtype=torch.float32, device=dev) for shape in ((1, 1, 2), (1, 1, 1))]

    def sentinel():
        # a launch no case of the table makes: a call that leaves its name behind launched nothing
        rc = lib.dmpc_lqr_forward_sweep(1, 1, 2, 1, ptr(s_in[0]), ptr(s_in[1]), None, None, ptr(s_in[2]), None, ptr(s_out[0]),
                                        ptr(s_out[1]), None, None)
        assert rc == 0
        return _lib.last_kernel_name()

    rows = []
    for c in cases():
        al = TorchArrays(dev)
        fn = call(c, lib, al)
        idle = sentinel()
        if c.get("coupled") == "fixed":
            os.environ["DMPC_NO_COOP_REGISTER"] = "1"
        try:
            rc = fn(al.ptr)
        finally:
            os.environ.pop("DMPC_NO_COOP_REGISTER", None)
        name = _lib.last_kernel_name()
        torch.cuda.synchronize()
        del al, fn
        rows.append(dict(id=c["id"], rc=int(rc), kernel=None if name == idle else name))
    return rows


def switch_env(label):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DMPC_NO_")}
    if label != "none":
        env[label] = "1"
    return env


def run_child(label, out_path):
    """the table in a fresh process with one switch set (or none) -> its rows"""
    subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", out_path], env=switch_env(label), check=True,
                   timeout=CHILD_TIMEOUT)
    with open(out_path) as fh:
        return json.load(fh)


def changed(rows, base):
    """what a switch's run is recorded as: its rows that differ from the run with none set"""
    return [row for row, b in zip(rows, base) if row != b]


def main():
    import tempfile
    if len(sys.argv) == 3 and sys.argv[1] == "--rows":
        with open(sys.argv[2], "w") as fh:
            json.dump(run_cases(), fh)
        return
    with tempfile.TemporaryDirectory() as tmp:
        base = run_child("none", os.path.join(tmp, "none.json"))
        rec = dict(none=base)
        for label in SWITCHES:
            rec[label] = changed(run_child(label, os.path.join(tmp, label + ".json")), base)
            print(label, "changes", len(rec[label]), "rows", flush=True)
    with open(JSON, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print("wrote", JSON, "-", len(base), "rows;", {k: len(v) for k, v in rec.items() if k != "none"})


if __name__ == "__main__":
    main()
