#!/usr/bin/env python
"""Recording of what the MlpDx kernels compute (csrc/mlp_dx_kernels.hpp), bit for bit.

    DMPC_LIB=/path/to/the/parent/libdmpc_hip.so python tests/golden/make_mlp_values.py [out.npz]      # needs a GPU

mlp_values.npz holds the raw outputs of a table of direct C-ABI calls - dmpc_mlp_rollout_linearize, dmpc_mpc_forward_rec_mlp,
dmpc_box_ddp with dyn_kind 2 and dmpc_mlp_param_grad - and per row the name of the kernel launched last, recorded from the
library of the commit BEFORE a change to those kernels; tests/test_mlp_values_gpu.py replays the table and compares bit for
bit.  This recording: commit 37e51b3 ("MlpDx: two-hidden-layer networks on the device kernels and DDP chain"), before the
network was rewritten by layers.

Every input comes from a seed.  The weights are those of the tests' numpy restatements (NumpyMlp, NumpyActMlp, NumpyMlp2:
float32 roundings of a seeded RandomState, every matrix and bias non-zero).  Two inputs come from the FILE, not from the
library under test: a search row's `states` and a gradient row's `x` are the `x` its rollout row recorded, so a rollout
regression cannot hide behind them.  A search row's `ks` is scaled per trajectory until the numpy restatement of the search
says trajectory 0 is accepted at the first pass and trajectory 1 after several; the scales are part of the recording.

    DMPC_LIB=/path/to/the/parent/libdmpc_hip.so python tests/golden/make_mlp_values.py --grads [out.npz]

A second table, mlp_grad_values.npz, for the gradient sweeps the first one does not reach (csrc/mlp_grad_kernels.hpp):
dmpc_mlp2_param_grad and dmpc_mlp_rollout_grad at both depths, replayed by tests/test_mlp_grad_values_gpu.py.  This recording:
commit a66dcb6 ("Test every MPC kernel with per-element, asymmetric control bounds"), before the four sweeps moved into one
header under one host entry point.  A gradient output of DIGEST_FROM elements or more is kept as the SHA-256 of its bytes (a
comparison of digests is a comparison bit for bit; the arrays themselves would not fit into 256 KB): `main` checks the
conditions on the arrays before it replaces them."""
import argparse
import ctypes
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
NPZ = os.path.join(HERE, "mlp_values.npz")
NPZ_GRADS = os.path.join(HERE, "mlp_grad_values.npz")
DIGEST_FROM = 4096
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ACTS = {0: "tanh", 2: "relu", 3: "silu", 4: "softplus"}
BOUND, LS_DECAY, MAX_LS, CAP = 0.5, 0.5, 5, 64
OUTPUTS = {"rollout": ("x", "F", "f"),
           "search": ("x", "u", "costs", "old_costs", "alphas", "objs", "u_first", "n_ls", "info"),      # make_search_values.OUTPUTS
           "chain": ("x_best", "u_best", "costs_best", "du_norm_best", "du_norm_last", "state"),
           "grad": ("dW1", "db1", "dW2", "db2", "d_x_init", "d_u")}
OUTPUTS["grad2"] = OUTPUTS["rgrad"] = OUTPUTS["grad"]
# kind -> (entry point, its workspace query, its cotangent in `problem`)
GRAD_CALLS = {"grad": ("dmpc_mlp_param_grad", "dmpc_mlp_param_grad_workspace_bytes", "grad_f"),
              "grad2": ("dmpc_mlp2_param_grad", "dmpc_mlp2_param_grad_workspace_bytes", "grad_f"),
              "rgrad": ("dmpc_mlp_rollout_grad", "dmpc_mlp_rollout_grad_workspace_bytes", "grad_x")}
# (nx, nu, hidden widths, seed of the weights and the problem)
MODELS = {"(3,1)H5": (3, 1, (5,), 1), "(8,2)H64": (8, 2, (64,), 2), "(4,2)H100": (4, 2, (100,), 3), "(5,3)H150": (5, 3, (150,), 6),
          "(16,8)H256": (16, 8, (256,), 4), "(3,1)(5,7)": (3, 1, (5, 7), 1), "(5,3)(100,70)": (5, 3, (100, 70), 3),
          "(4,2)(20,128)": (4, 2, (20, 128), 6), "(16,8)(128,128)": (16, 8, (128, 128), 4),
          # the second table's: cases C and E of tests/mlp2_cases.py, the walk case of tests/mlp2_grad_cases.py
          "(4,2)(100,70)": (4, 2, (100, 70), 3), "(3,1)(5,3)": (3, 1, (5, 3), 5), "(3,1)(5,7)w": (3, 1, (5, 7), 7)}
MLP2_GRAD_CAP = 256      # dmpc_mlp2_param_grad_partials at a large B (asserted when a walk row runs)


def rows(table="values"):
    """the table: a rollout row before the rows that read its `x` from the recording.  "values": mlp_values.npz, "grads":
    mlp_grad_values.npz"""
    out = []

    def add(kind, model, act=0, B=5, T=3, **kw):
        nx, nu, hidden, seed = MODELS[model]
        if table == "grads":
            kw = dict(kw, T=T)                       # (the first table's ids are the recording's keys: they stay as they are)
        rid = "%s:%s,%s,B%d%s" % (kind, model, ACTS[act], B, "".join(",%s=%s" % kv for kv in sorted(kw.items())))
        depth = ", 2>" if len(hidden) == 2 else ">"
        reduce = "mlp_param_grad_reduce_kernel" if len(hidden) == 1 else "mlp2_param_grad_reduce_kernel"
        kernel = {"rollout": "mlp_rollout_linearize_kernel<%d%s" % (act, depth), "search": "mpc_forward_rec_mlp_kernel<%d%s" % (act, depth),
                  "chain": "box_ddp_summary_kernel", "grad": reduce, "grad2": reduce, "rgrad": reduce}[kind]
        r = dict(id=rid, kind=kind, model=model, act=act, B=B, T=T, nx=nx, nu=nu, hidden=hidden, seed=seed, kernel=kernel,
                 residual=1, F=1, f=1, lin=0, null=0, walk=0)
        r.update(kw)
        if kind in ("search",) + tuple(GRAD_CALLS):  # the rollout row whose x this row reads
            r["src"] = [q["id"] for q in out if q["kind"] == "rollout" and all(q[k] == r[k] for k in ("model", "act", "B", "T", "residual"))][0]
        out.append(r)

    if table == "grads":
        grad_rows(add, out)
        assert len(set(r["id"] for r in out)) == len(out)
        return out
    for a in sorted(ACTS):
        add("rollout", "(3,1)H5", a)
    add("rollout", "(8,2)H64")
    add("rollout", "(4,2)H100", residual=0)
    add("rollout", "(5,3)H150", 3)                   # three units per lane
    add("rollout", "(16,8)H256", B=3)                # four units per lane, a lane owns six entries of F
    add("rollout", "(3,1)H5", F=0, f=0)
    add("rollout", "(3,1)H5", f=0)
    add("rollout", "(3,1)H5", B=515, F=0, f=0)       # (the states of the gradient row past the 512 partials)
    for a in sorted(ACTS):
        add("rollout", "(3,1)(5,7)", a)
    add("rollout", "(5,3)(100,70)")                  # N's last row group is ragged, H1 != H2
    add("rollout", "(4,2)(20,128)", 2, residual=0)   # H2 > H1
    add("rollout", "(16,8)(128,128)", B=3)           # the 131,456-byte launch
    add("rollout", "(3,1)(5,7)", F=0, f=0)           # the launch without wavefront slices
    for m in ("(3,1)H5", "(3,1)(5,7)"):
        for a in sorted(ACTS):
            add("search", m, a)
    add("search", "(5,3)H150", 3)
    add("search", "(16,8)H256", B=3)
    add("search", "(5,3)(100,70)")
    add("search", "(16,8)(128,128)", B=3)
    for m in ("(3,1)H5", "(5,3)(100,70)"):
        for lin in (0, 1):
            add("chain", m, lin=lin)                 # lin = 1: the only way to the search's F_next epilogue
    for a in sorted(ACTS):
        add("grad", "(3,1)H5", a)
    add("grad", "(4,2)H100", residual=0)
    add("grad", "(5,3)H150", 3)
    add("grad", "(16,8)H256", B=3)
    add("grad", "(3,1)H5", B=515)                    # a wavefront serves two trajectories
    assert len(set(r["id"] for r in out)) == len(out)
    return out


def grad_rows(add, out):
    """the second table: the smallest shapes at which the sweeps can still go wrong; all four activations on the smallest case
    of each kernel, tanh on the rest"""
    def both(kinds, model, act=0, B=5, T=3, residual=1, **kw):
        if not any(q["kind"] == "rollout" and (q["model"], q["act"], q["B"], q["T"], q["residual"]) == (model, act, B, T, residual) for q in out):
            add("rollout", model, act, B, T, residual=residual, F=0, f=0)
        for kind in kinds:
            add(kind, model, act, B, T, residual=residual, **kw)

    one, two = ("rgrad",), ("grad2", "rgrad")
    for a in sorted(ACTS):
        both(one, "(3,1)H5", a, 5, 7)
    both(one, "(4,2)H100", 0, 5, 6)
    both(one, "(4,2)H100", 0, 5, 6, residual=0)
    both(one, "(5,3)H150", 0, 3, 5)                  # three units per lane
    both(one, "(16,8)H256", 0, 3, 5)                 # four units per lane, every limit
    both(one, "(3,1)H5", 0, 515, 3, walk=1)          # a wavefront serves two trajectories, past the 512 partials
    both(one, "(3,1)H5", 0, 5, 2)                    # a single step
    both(one, "(3,1)H5", 0, 5, 1)                    # no sweep: d_x_init is a copy of grad_x[0]
    both(one, "(3,1)H5", 0, 5, 7, null=1)            # d_x_init and d_u both NULL
    for a in sorted(ACTS):
        both(two, "(3,1)(5,7)", a, 5, 7)             # case A: a ragged workgroup
    both(two, "(4,2)(100,70)", 0, 5, 6)              # C: two units per lane, H1 != H2, H2 no multiple of 8: rows past H2 in a block of eight
    both(two, "(16,8)(128,128)", 0, 3, 5)            # D: every limit
    both(two, "(3,1)(5,3)", 0, 1, 2)                 # E: B = 1, a single step
    both(two, "(4,2)(20,128)", 0, 4, 6)              # F: H2 > H1
    both(two, "(3,1)(5,7)w", 0, 4 * MLP2_GRAD_CAP + 5, 3, walk=1)   # a workgroup walks two groups, one trip has a single live wavefront
    both(two, "(3,1)(5,7)", 0, 5, 1)
    both(two, "(3,1)(5,7)", 0, 5, 7, null=1)


def net_of(r):
    """the numpy restatement that owns the row's weights (its `step` is the residual network)"""
    from tests import mlp2_cases, mlp_act_cases, mlp_dx_cases
    nx, nu, hidden, seed = r["nx"], r["nu"], r["hidden"], r["seed"]
    if len(hidden) == 2:
        return mlp2_cases.NumpyMlp2(nx, nu, hidden[0], hidden[1], seed, ACTS[r["act"]])
    if r["act"] == 0:
        return mlp_dx_cases.NumpyMlp(nx, nu, hidden[0], seed)
    return mlp_act_cases.NumpyActMlp(nx, nu, hidden[0], seed, ACTS[r["act"]])


def weights(r):
    """(the `n_hidden` code, [W1, b1, W2, b2] as the entry points take them: for two layers [W2 | W3] and [b2 | b3])"""
    net, hidden = net_of(r), r["hidden"]
    if len(hidden) == 1:
        return hidden[0], [net.W1, net.b1, net.W2, net.b2]
    return hidden[0] | (hidden[1] << 16), [net.W1, net.b1, np.concatenate((net.W2.reshape(-1), net.W3.reshape(-1))),
                                           np.concatenate((net.b2, net.b3))]


def problem(r):
    """x_init, C, c, the rollout's u (the search's `controls`), the search's gains, the gradients' grad_f and grad_x: float64, from seeds"""
    from chainer_differentiable_mpc_amd import synthetic
    T, B, nx, nu, s = r["T"], r["B"], r["nx"], r["nu"], r["seed"]
    p = synthetic.make_lqr_problem(B, T, nx, nu, seed=s)
    rng = np.random.RandomState(s + 40)
    d = dict(x_init=p["x_init"], C=p["C"], c=p["c"], u=np.random.RandomState(s + 30).uniform(-BOUND, BOUND, (T, B, nu)),
             Ks=0.1 * rng.randn(T, B, nu, nx), ks=0.2 * rng.randn(T, B, nu), grad_f=np.random.RandomState(s + 31).randn(T - 1, B, nx),
             grad_x=np.random.RandomState(s + 32).randn(T, B, nx),
             lower=np.full((T, B, nu), -BOUND), upper=np.full((T, B, nu), BOUND))
    return {k: np.asarray(v, dtype=np.float32).astype(np.float64) for k, v in d.items()}


def scaled_ks(d, scale):
    return (d["ks"] * np.asarray(scale, dtype=np.float64)[None, :, None]).astype(np.float32).astype(np.float64)


def choose_scale(r, states):
    """k's scale per trajectory, decided on the CPU: trajectory 0 accepted at once, and the first later trajectory for which a
    scale does it accepted after 3..40 passes"""
    from oracle import mpc
    d, net, T = problem(r), net_of(r), r["T"]
    scale = np.ones(r["B"])
    mags = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 0.5, 0.25, 0.1, 0.05, 0.02)

    def found(b, lo, hi):
        sl = slice(b, b + 1)
        cost = mpc.QuadCost(d["C"][:, sl], d["c"][:, sl])
        old = mpc.get_cost(T, d["u"][:, sl], cost, x=states[:, sl])
        for s in [sg * m for m in (mags[::-1] if b == 0 else mags) for sg in (1, -1)]:
            scale[b] = s
            _, _, res, _, n = mpc.mpc_forward_rec(d["Ks"][:, sl], scaled_ks(d, scale)[:, sl], d["u"][:, sl], states[:, sl], d["lower"][:, sl],
                                                  d["upper"][:, sl], cost, net.step, LS_DECAY, MAX_LS, T, max_total_iter=CAP)
            if lo <= n <= hi and not res.costs[0] > old[0]:
                return True
        scale[b] = 1.0
        return False

    assert found(0, 1, 1), "no scale of k lets trajectory 0 of %s be accepted at once" % r["id"]
    assert any(found(b, 3, 40) for b in range(1, r["B"])), "no scale of k gives a trajectory of %s several passes" % r["id"]
    return scale


class Arrays:
    def __init__(self, device):
        import torch
        self.torch, self.device = torch, device

    def inp(self, array, dtype=np.float32):
        return self.torch.as_tensor(np.ascontiguousarray(array, dtype=dtype), device=self.device)

    def out(self, shape, dtype="float32"):
        return self.torch.zeros(tuple(shape), dtype=getattr(self.torch, dtype), device=self.device)


def ptr(t):
    return None if t is None else t.data_ptr()


def run_row(r, lib, al, recorded, scale=None):
    """the row's call -> (return code, {output: tensor}); `recorded`: the flat recording (a rollout row's x), `scale`: ks'"""
    T, B, nx, nu, ns = r["T"], r["B"], r["nx"], r["nu"], r["nx"] + r["nu"]
    d = problem(r)
    code, w = weights(r)
    w = [al.inp(a) for a in w]
    head = [T, B, nx, nu, code, r["act"], r["residual"]] + [ptr(a) for a in w]
    if r["kind"] == "rollout":
        o = dict(x=al.out((T, B, nx)), F=al.out((T - 1, B, nx, ns)) if r["F"] else None, f=al.out((T - 1, B, nx)) if r["f"] else None)
        ins = [al.inp(d["x_init"]), al.inp(d["u"])]
        rc = lib.dmpc_mlp_rollout_linearize(*head, *[ptr(a) for a in ins], ptr(o["x"]), ptr(o["F"]), ptr(o["f"]), None)
        return rc, {k: v for k, v in o.items() if v is not None}
    x_src = recorded[r["src"] + "/x"] if "src" in r else None
    if r["kind"] == "search":
        ins = [al.inp(a) for a in (d["Ks"], scaled_ks(d, scale), d["u"], x_src, d["lower"], d["upper"], d["C"], d["c"])]
        o = dict(x=al.out((T, B, nx)), u=al.out((T, B, nu)), costs=al.out((B,)), old_costs=al.out((B,)), alphas=al.out((B,)),
                 objs=al.out((T, B)), u_first=al.out((T, B, nu)), n_ls=al.out((B,), "int32"), info=al.out((B,), "int32"))
        rc = lib.dmpc_mpc_forward_rec_mlp(*head, *[ptr(a) for a in ins], LS_DECAY, MAX_LS, *[ptr(o[k]) for k in OUTPUTS["search"]], None)
        return rc, o
    if r["kind"] in GRAD_CALLS:
        call, query, cotangent = GRAD_CALLS[r["kind"]]
        H, H2 = r["hidden"][0], (r["hidden"] + (0,))[1]
        if r["walk"] and H2:
            assert B == 4 * lib.dmpc_mlp2_param_grad_partials(1 << 30) + 5, r["id"]
        ins = [al.inp(x_src), al.inp(d["u"]), al.inp(d[cotangent])]
        o = dict(dW1=al.out((H, ns)), db1=al.out((H,)), dW2=al.out((H2 * H + nx * H2,) if H2 else (nx, H)), db2=al.out((H2 + nx,)),
                 d_x_init=None if r["null"] else al.out((B, nx)), d_u=None if r["null"] else al.out((T, B, nu)))
        need = getattr(lib, query)(B, nx, nu, code)
        ws = al.out((need,), "uint8")               # exactly the queried size
        rc = getattr(lib, call)(*head, *[ptr(a) for a in ins], *[ptr(o[k]) for k in OUTPUTS["grad"]], ptr(ws), need, None)
        return rc, {k: v for k, v in o.items() if v is not None}
    net = net_of(r)
    names = ("W1", "b1", "W2", "b2") if len(r["hidden"]) == 1 else ("W1", "b1", "W2", "W3", "b2", "b3")
    packed = al.inp(np.concatenate([getattr(net, k).reshape(-1) for k in names]))
    params = (ctypes.c_float * 4)(float(code), float(r["act"]), 1.0, float(r["lin"]))
    ins = [al.inp(d["x_init"]), al.inp(d["C"]), al.inp(d["c"]), packed, al.inp(np.zeros((T, B, nu))), al.inp(d["lower"]), al.inp(d["upper"])]
    o = dict(x_best=al.out((T, B, nx)), u_best=al.out((T, B, nu)), costs_best=al.out((B,)), du_norm_best=al.out((B,)),
             du_norm_last=al.out((B,)), state=al.out((8,), "int32"))
    need = lib.dmpc_box_ddp_workspace_bytes(T, B, nx, nu)
    ws, info = al.out((need,), "uint8"), al.out((B,), "int32")
    # eps, not_improved_lim, ls_decay, max_ls_iter, best_cost_eps, max_iter, n_qp_iter_max, scrambled_norm, batch_coupled
    rc = lib.dmpc_box_ddp(T, B, nx, nu, *[ptr(a) for a in ins[:4]], None, 2, ctypes.cast(params, ctypes.c_void_p), *[ptr(a) for a in ins[4:]],
                          1e-5, 5, 0.2, 10, 1e-4, 2, 10, 1, 0, *[ptr(o[k]) for k in OUTPUTS["chain"]], ptr(ws), need, ptr(info), None)
    return rc, o


def run_rows(recorded=None, table="values"):
    """the table with this process's library -> the flat recording {"id/output": array, "id/kernel": name, "id/ks_scale"}.
    `recorded`: a recording whose rollout `x` and ks scales are used (the test); None: the rows' own, the scales chosen here"""
    import torch

    from chainer_differentiable_mpc_amd import _lib
    lib, al = _lib.load(), Arrays(torch.device("cuda:0"))
    got = {}
    for r in rows(table):
        src = got if recorded is None else recorded
        scale = None
        if r["kind"] == "search":
            scale = choose_scale(r, src[r["src"] + "/x"].astype(np.float64)) if recorded is None else recorded[r["id"] + "/ks_scale"]
            got[r["id"] + "/ks_scale"] = np.asarray(scale, dtype=np.float64)
        rc, o = run_row(r, lib, al, src, scale)
        name = _lib.last_kernel_name()
        torch.cuda.synchronize()
        assert rc == 0, (r["id"], rc)
        got.update({"%s/%s" % (r["id"], k): v.cpu().numpy() for k, v in o.items()})
        got[r["id"] + "/kernel"] = np.asarray(name)
    return got


def keys(r):
    """the keys of a row in the recording"""
    outs = [k for k in OUTPUTS[r["kind"]] if (r["kind"] != "rollout" or k == "x" or r[k]) and not (r["null"] and k in ("d_x_init", "d_u"))]
    return ["%s/%s" % (r["id"], k) for k in outs + ["kernel"] + (["ks_scale"] if r["kind"] == "search" else [])]


def compact(rec, table="grads"):
    """the recording as the file keeps it: a gradient output of DIGEST_FROM elements or more as the SHA-256 of its bytes"""
    big = set(k for r in rows(table) if r["kind"] in GRAD_CALLS for k in keys(r) if rec[k].dtype.kind == "f" and rec[k].size >= DIGEST_FROM)
    return {k: np.frombuffer(hashlib.sha256(v.tobytes()).digest(), dtype=np.uint8) if k in big else v for k, v in rec.items()}


def check_conditions(rec, table="values"):
    """what a recording must satisfy to be worth keeping (conditions, not measurements); of an array the file keeps as a
    digest `main` has checked them before it was replaced"""
    assert sorted(rec) == sorted(k for r in rows(table) for k in keys(r))
    for r in rows(table):
        assert r["kernel"] in str(rec[r["id"] + "/kernel"]), (r["id"], str(rec[r["id"] + "/kernel"]))
        for k in keys(r):
            if rec[k].dtype.kind == "f":
                assert np.isfinite(rec[k]).all(), k
        if r["kind"] == "rollout" and r["F"]:
            F = rec[r["id"] + "/F"].copy()
            F[..., np.arange(r["nx"]), np.arange(r["nx"])] -= float(r["residual"])
            assert (F != 0).any(axis=(2, 3)).all(), (r["id"], "a Jacobian that is [I|0]")
        if r["kind"] == "search":
            n_ls = rec[r["id"] + "/n_ls"]
            assert (n_ls == 1).any() and ((n_ls > 1) & (n_ls < CAP)).any(), (r["id"], n_ls)
        if r["kind"] in GRAD_CALLS and r["T"] > 1:
            for k in ("dW1", "db1", "dW2", "db2"):
                a = rec["%s/%s" % (r["id"], k)]
                assert a.dtype.kind != "f" or (a != 0).any(), (r["id"], k, "a weight gradient of zeros")
        if r["kind"] == "rgrad" and not r["null"]:
            d_u, d_x = rec[r["id"] + "/d_u"], rec[r["id"] + "/d_x_init"]
            assert (d_u[r["T"] - 1] == 0).all() and (r["T"] == 1 or (d_u[0] != 0).any()), (r["id"], "d_u")
            if r["T"] == 1:      # no sweep: the state IS x_init
                assert d_x.tobytes() == problem(r)["grad_x"][0].astype(np.float32).tobytes(), (r["id"], "d_x_init is not grad_x[0]")
            if r["walk"]:        # the trajectory of a later trip is not a copy of the first's
                assert (d_x[-1] != d_x[0]).any() and (d_u[0, -1] != d_u[0, 0]).any(), (r["id"], "the last trajectory's gradient is the first's")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grads", action="store_true", help="the second table, mlp_grad_values.npz")
    ap.add_argument("out", nargs="?")
    args = ap.parse_args()
    table = "grads" if args.grads else "values"
    first = run_rows(table=table)
    second = run_rows(table=table)
    assert sorted(first) == sorted(second)
    for k in first:     # recorded twice: a table that is not deterministic records nothing
        assert first[k].dtype == second[k].dtype and first[k].tobytes() == second[k].tobytes(), "two recordings differ in " + k
    check_conditions(first, table)
    out = args.out or (NPZ_GRADS if args.grads else NPZ)
    if args.grads:
        first = compact(first)
        check_conditions(first, table)
    np.savez_compressed(out, **first)
    print("wrote", out, "-", len(rows(table)), "rows,", os.path.getsize(out), "bytes; passes per search row:",
          {r["id"]: first[r["id"] + "/n_ls"].tolist() for r in rows(table) if r["kind"] == "search"})


if __name__ == "__main__":
    main()
