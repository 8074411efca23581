#!/usr/bin/env python
"""Recordings of the LQR solve dispatch (csrc/lqr_api.hip): what a caller is told, and which kernel runs.

    python tests/golden/make_lqr_routes.py            # told_lqr_routes.npz: the told paths over a grid of sizes (no GPU needed)
    python tests/golden/make_lqr_routes.py --gpu      # lqr_routes.json: return code and last kernel of a case table

Both files are recorded from the library in the tree (or `DMPC_LIB`) at the commit BEFORE a change to the dispatch;
tests/test_lqr_routes_cpu.py and tests/test_lqr_routes_gpu.py replay them.  Regenerating at an unchanged dispatch gives
byte-identical files.  The DMPC_NO_* switches are latched per process: every switch is queried in a child process of its own
(`--query OUT`)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
NPZ = os.path.join(HERE, "told_lqr_routes.npz")
JSON = os.path.join(HERE, "lqr_routes.json")

NX = list(range(0, 71))
NU = list(range(0, 13))
TS = [1, 2, 3, 20, 50, 51, 52, 74, 75, 76, 200, 400]
BS = [1, 3, 4, 5, 7, 8, 16, 4096, 65536, 2 ** 20]
KNOBS = ["DMPC_NO_ASM", "DMPC_NO_STASH", "DMPC_NO_DMA", "DMPC_NO_WAVE_MFMA", "DMPC_NO_WIDE", "DMPC_NO_CONTAINER"]
LABELS = ["none"] + KNOBS
FIELDS = ("family", "path", "saving", "workspace")


def _library():
    lib = ctypes.CDLL(os.environ.get("DMPC_LIB", os.path.join(ROOT, "chainer_differentiable_mpc_amd", "libdmpc_hip.so")))
    i4 = [ctypes.c_int] * 4
    lib.dmpc_lqr_kernel_family.restype, lib.dmpc_lqr_kernel_family.argtypes = ctypes.c_int, i4[:2]
    lib.dmpc_lqr_solve_path.restype, lib.dmpc_lqr_solve_path.argtypes = ctypes.c_int, i4
    lib.dmpc_lqr_saving_available.restype, lib.dmpc_lqr_saving_available.argtypes = ctypes.c_int, i4
    lib.dmpc_lqr_workspace_bytes.restype, lib.dmpc_lqr_workspace_bytes.argtypes = ctypes.c_size_t, i4
    return lib


def query():
    """the four queries over the whole grid, with this process's switches -> {field: array}"""
    lib = _library()
    shape = (len(NX), len(NU), len(TS), len(BS))
    out = dict(family=np.zeros(shape[:2], np.int8), path=np.zeros(shape, np.int8), saving=np.zeros(shape, np.int8),
               workspace=np.zeros(shape, np.uint64))
    for i, nx in enumerate(NX):
        for j, nu in enumerate(NU):
            out["family"][i, j] = lib.dmpc_lqr_kernel_family(nx, nu)
            for k, T in enumerate(TS):
                for m, B in enumerate(BS):
                    out["path"][i, j, k, m] = lib.dmpc_lqr_solve_path(T, B, nx, nu)
                    out["saving"][i, j, k, m] = lib.dmpc_lqr_saving_available(T, B, nx, nu)
                    out["workspace"][i, j, k, m] = lib.dmpc_lqr_workspace_bytes(T, B, nx, nu)
    return out


def knob_env(label):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DMPC_NO_")}
    if label != "none":
        env[label] = "1"
    return env


def query_children(tmp_dir):
    """one child per switch (and one with none set), side by side -> {label: {field: array}}"""
    procs = [(label, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--query",
                                       os.path.join(tmp_dir, label + ".npz")], env=knob_env(label))) for label in LABELS]
    got = {}
    for label, p in procs:
        assert p.wait() == 0, label
        with np.load(os.path.join(tmp_dir, label + ".npz")) as z:
            got[label] = {f: z[f] for f in FIELDS}
    return got


def load_recorded():
    with np.load(NPZ) as z:
        # (an array equal to the one recorded with no switch set is stored once, under "none")
        return {label: {f: z[label + "/" + f if label + "/" + f in z.files else "none/" + f] for f in FIELDS} for label in LABELS}


# ---- the case table of the GPU recording: (entry point, nx, nu, B, T, options) ----
def cases():
    out = []

    def add(fn, nx, nu, B, T, **kw):
        tag = "".join(("+" if kw[k] else "-") + k for k in sorted(kw))
        out.append(dict(id="%s(%d,%d)B%dT%d%s" % (fn, nx, nu, B, T, tag), fn=fn, nx=nx, nu=nu, B=B, T=T, **kw))

    # dmpc_lqr_solve at (8,2)
    for has_f in (True, False):
        for gains in (False, True):
            add("solve", 8, 2, 4, 2, has_f=has_f, gains=gains)
    add("solve", 8, 2, 4, 2, mask=True)
    add("solve", 8, 2, 5, 2, mask=True)
    add("solve", 8, 2, 3, 2)
    add("solve", 8, 2, 4, 1)
    for T in (51, 52, 74, 75):
        add("solve", 8, 2, 4, T)
    add("solve", 8, 2, 4, 75, gains=True)
    add("solve", 8, 2, 4, 75, has_ws=False)
    # other 16-lane shapes
    add("solve", 3, 1, 4, 3)
    add("solve", 3, 1, 6, 3, mask=True)
    add("solve", 4, 4, 4, 2)
    add("solve", 6, 2, 4, 2)
    add("solve", 8, 4, 4, 2)
    add("solve", 8, 4, 3, 2)
    add("solve", 8, 4, 4, 2, mask=True)
    add("solve", 8, 4, 4, 200)
    add("solve", 8, 4, 4, 200, gains=True)
    add("solve", 12, 3, 4, 2)
    # the wave shapes
    add("solve", 32, 8, 1, 2)
    add("solve", 32, 8, 1, 2, mask=True)
    add("solve", 32, 8, 1, 2, gains=True)
    add("solve", 32, 8, 1, 2, has_ws=False)
    add("solve", 24, 8, 1, 2)
    add("solve", 16, 8, 5, 2)
    # the wide shapes
    add("solve", 16, 4, 4, 2)
    add("solve", 16, 4, 4, 2, has_ws=False)
    add("solve", 16, 4, 4, 2, mask=True)
    add("solve", 16, 4, 3, 2)
    add("solve", 13, 3, 4, 2)
    add("solve", 13, 3, 5, 2)
    # containers and beyond
    add("solve", 20, 6, 2, 2)
    add("solve", 20, 6, 2, 2, mask=True)
    for nx, nu in ((5, 3), (5, 5), (7, 8), (14, 1)):
        add("solve", nx, nu, 4, 2)
    add("solve", 5, 3, 1, 300, has_ws=False)
    add("solve", 40, 4, 2, 2)
    add("solve", 10, 9, 2, 2)
    add("solve", 60, 10, 2, 2)
    add("solve", 60, 10, 2, 2, has_ws=False)
    # the sweeps on their own
    for nx, nu in ((8, 2), (8, 4), (32, 8), (5, 3), (20, 6), (40, 4), (60, 10)):
        for mask in (False, True):
            kw = dict(mask=True) if mask else {}
            add("backward_ws", nx, nu, 4, 3, **kw)
            add("backward", nx, nu, 4, 3, **kw)
            add("forward", nx, nu, 4, 3, **kw)
    # saving and saved gains
    add("solve_saving", 8, 2, 4, 2)
    add("solve_saving", 8, 2, 5, 2)
    add("solve_saving", 3, 1, 4, 2)
    add("solve_saving", 8, 4, 4, 2)
    add("saved_solve", 8, 2, 4, 2)
    add("saved_solve", 8, 2, 5, 2)
    add("saved_solve", 2, 1, 4, 2)
    add("kkt_grad_saved", 8, 2, 4, 2)
    add("kkt_grad_saved", 8, 2, 4, 2, has_vv=False)
    add("kkt_grad_saved", 8, 2, 5, 2)
    add("kkt_grad", 8, 2, 4, 2)       # (its second solve takes c as two arrays)
    add("kkt_grad", 5, 3, 4, 2)
    assert len(set(c["id"] for c in out)) == len(out)
    return out


class TorchArrays:
    """the arrays of a case as the recording makes them: one zero-filled torch tensor each.  `call` below asks for its arrays
    through these methods; tests/arena.py's Builder has the same ones and puts them into one guarded allocation instead."""

    def __init__(self, device):
        import torch
        self.torch, self.device = torch, device

    def inp(self, name, array, dtype=np.float32):
        return self.torch.as_tensor(np.asarray(array, dtype=dtype), device=self.device)

    def out(self, name, shape, dtype=np.float32):
        return self.torch.zeros(tuple(shape), dtype=getattr(self.torch, np.dtype(dtype).name), device=self.device)

    produced = out      # an input of the call that a preparing call writes
    pre = out           # an output of a preparing call that the call itself does not see

    def info(self, name, n, written=False):
        return self.torch.zeros(n, dtype=self.torch.int32, device=self.device)

    def ws(self, name, nbytes):
        return self.torch.zeros(max(nbytes, 16), dtype=self.torch.uint8, device=self.device)

    @staticmethod
    def ptr(t):
        return None if t is None else t.data_ptr()


def call(c, lib, al):
    """the arrays of case c from the allocator `al` -> (prepare, fn): `fn(ptr)` makes the case's call and returns its code,
    `prepare(ptr)` - or None - the saving solve whose blocks it reads; `ptr` turns an array of `al` into its device pointer"""
    T, B, nx, nu, ns = c["T"], c["B"], c["nx"], c["nu"], c["nx"] + c["nu"]
    from chainer_differentiable_mpc_amd import synthetic
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=5, with_f=c.get("has_f", True))
    fn = c["fn"]
    d = {k: (None if v is None or v.size == 0 else al.inp(k, v)) for k, v in p.items()}
    mask = None
    if c.get("mask"):
        mask = al.inp("mask", (np.arange(T * B * nu).reshape(T, B, nu) % 3 == 0), dtype=np.uint8)
    need = lib.dmpc_lqr_workspace_bytes(T, B, nx, nu)
    head = (T, B, nx, nu)
    if fn in ("solve", "backward_ws", "backward", "forward"):
        info = al.info("info", B)
        if fn == "solve":
            g = c.get("gains", False)
            Ks, ks = (al.out("Ks", (T, B, nu, nx)), al.out("ks", (T, B, nu))) if g else (None, None)
            x, u = al.out("x", (T, B, nx)), al.out("u", (T, B, nu))
            ws = al.ws("ws", need) if c.get("has_ws", True) else None
            return None, lambda ptr: lib.dmpc_lqr_solve(*head, ptr(d["C"]), ptr(d["c"]), ptr(d["F"]), ptr(d["f"]), ptr(d["x_init"]),
                                                        ptr(mask), ptr(Ks), ptr(ks), ptr(x), ptr(u), ptr(ws),
                                                        need if ws is not None else 0, ptr(info), None)
        if fn == "forward":
            Ks, ks = al.inp("Ks", np.zeros((T, B, nu, nx))), al.inp("ks", np.zeros((T, B, nu)))
            x, u = al.out("x", (T, B, nx)), al.out("u", (T, B, nu))
            return None, lambda ptr: lib.dmpc_lqr_forward_sweep(*head, ptr(Ks), ptr(ks), ptr(d["F"]), ptr(d["f"]), ptr(d["x_init"]),
                                                                ptr(mask), ptr(x), ptr(u), ptr(info), None)
        Ks, ks = al.out("Ks", (T, B, nu, nx)), al.out("ks", (T, B, nu))
        if fn == "backward_ws":
            ws = al.ws("ws", need)
            return None, lambda ptr: lib.dmpc_lqr_backward_sweep_ws(*head, ptr(d["C"]), ptr(d["c"]), ptr(d["F"]), ptr(d["f"]), ptr(mask),
                                                                    ptr(Ks), ptr(ks), ptr(ws), need, ptr(info), None)
        return None, lambda ptr: lib.dmpc_lqr_backward_sweep(*head, ptr(d["C"]), ptr(d["c"]), ptr(d["F"]), ptr(d["f"]), ptr(mask),
                                                             ptr(Ks), ptr(ks), ptr(info), None)
    # the saving solve, as the call itself or as the one that leaves the blocks the call reads (zeros where it does not serve
    # the size)
    last = fn == "solve_saving"
    made = al.out if last else al.produced
    Ks, ks = made("Ks", (T, B, nu, nx)), (al.out if last else al.pre)("ks", (T, B, nu))
    Quu, Qxu = made("Quu", (T, B, nu, nu)), made("Qxu", (T, B, nx, nu))
    Vv = (al.pre if fn == "saved_solve" else made)("Vv", (T, B, nx, nx + 1))
    x, u = ((al.pre, al.pre) if fn == "saved_solve" else (made, made))
    x, u = x("x", (T, B, nx)), u("u", (T, B, nu))
    info = al.info("info", B, written=last)

    def saving(ptr):
        return lib.dmpc_lqr_solve_saving(*head, ptr(d["C"]), ptr(d["c"]), ptr(d["F"]), ptr(d["f"]), ptr(d["x_init"]), ptr(Ks), ptr(ks),
                                         ptr(Quu), ptr(Qxu), ptr(Vv), ptr(x), ptr(u), ptr(info), None)
    if last:
        return None, saving
    if fn == "saved_solve":
        c2 = al.inp("c2", np.random.RandomState(7).randn(T, B, ns))
        x2, u2 = al.out("x2", (T, B, nx)), al.out("u2", (T, B, nu))
        return saving, lambda ptr: lib.dmpc_lqr_saved_solve(*head, ptr(c2), ptr(d["F"]), ptr(Ks), ptr(Quu), ptr(Qxu), ptr(d["x_init"]),
                                                            ptr(x2), ptr(u2), ptr(info), None)
    rng = np.random.RandomState(9)
    gx, gu = al.inp("gx", rng.randn(T, B, nx)), al.inp("gu", rng.randn(T, B, nu))
    dx0, dC, dc = al.out("dx0", (B, nx)), al.out("dC", (T, B, ns, ns)), al.out("dc", (T, B, ns))
    dF, df = al.out("dF", (T - 1, B, nx, ns)), al.out("df", (T - 1, B, nx))
    kneed = lib.dmpc_lqr_kkt_workspace_bytes(T, B, nx, nu)
    kws = al.ws("kws", kneed)
    tail = lambda ptr: (0, ptr(dx0), ptr(dC), ptr(dc), ptr(dF), ptr(df), ptr(kws), kneed, ptr(info), None)   # noqa: E731
    if fn == "kkt_grad_saved":
        vv = Vv if c.get("has_vv", True) else None
        return saving, lambda ptr: lib.dmpc_lqr_kkt_grad_saved(*head, ptr(d["C"]), ptr(d["c"]), ptr(d["F"]), ptr(x), ptr(u), ptr(Ks),
                                                               ptr(Quu), ptr(Qxu), ptr(vv), ptr(gx), ptr(gu), *tail(ptr))
    assert fn == "kkt_grad"
    return saving, lambda ptr: lib.dmpc_lqr_kkt_grad(*head, ptr(d["C"]), ptr(d["c"]), ptr(d["F"]), ptr(x), ptr(u), ptr(gx), ptr(gu),
                                                     *tail(ptr))


def run_cases():
    """-> [{id, rc, kernel}]; kernel None: the call launched nothing"""
    import torch

    sys.path.insert(0, ROOT)
    from chainer_differentiable_mpc_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda:0")
    f32 = dict(dtype=torch.float32, device=dev)
    ptr = _lib.ptr

    def empty(*shape):
        return torch.zeros(shape, **f32)

    def sentinel():
        # a launch no case of the table makes: a call that leaves its name behind launched nothing
        Ks, ks, x0, x, u = empty(1, 1, 1, 2), empty(1, 1, 1), empty(1, 2), empty(1, 1, 2), empty(1, 1, 1)
        rc = lib.dmpc_lqr_forward_sweep(1, 1, 2, 1, ptr(Ks), ptr(ks), None, None, ptr(x0), None, ptr(x), ptr(u), None, None)
        assert rc == 0
        return _lib.last_kernel_name()

    rows = []
    for c in cases():
        al = TorchArrays(dev)
        prepare, fn = call(c, lib, al)
        if prepare is not None:
            prepare(al.ptr)          # (the saved blocks the call reads)
            torch.cuda.synchronize()
        idle = sentinel()
        rc = fn(al.ptr)
        name = _lib.last_kernel_name()
        torch.cuda.synchronize()
        del al, prepare, fn
        rows.append(dict(id=c["id"], rc=int(rc), kernel=None if name == idle else name))
    return rows


def main():
    import tempfile
    if len(sys.argv) == 3 and sys.argv[1] == "--query":
        np.savez(sys.argv[2], **query())
    elif len(sys.argv) == 2 and sys.argv[1] == "--gpu":
        with open(JSON, "w") as fh:
            json.dump(run_cases(), fh, indent=1)
            fh.write("\n")
        print("wrote", JSON)
    else:
        with tempfile.TemporaryDirectory() as tmp:
            got = query_children(tmp)
        np.savez_compressed(NPZ, **{label + "/" + f: got[label][f] for label in LABELS for f in FIELDS
                                    if label == "none" or not np.array_equal(got[label][f], got["none"][f])})
        paths, counts = np.unique(got["none"]["path"], return_counts=True)
        print("wrote", NPZ, "- paths with no switch set:", dict(zip(paths.tolist(), counts.tolist())))


if __name__ == "__main__":
    main()
