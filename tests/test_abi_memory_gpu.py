"""The C ABI's memory contract (include/dmpc.h: "the caller owns every buffer; the library allocates nothing, inputs are
read-only"; every `*_workspace_bytes` query is enough) on every entry point that takes a device pointer: each row of
tests/abi_calls.py runs inside a guarded arena (tests/arena.py) in two layouts - 256-byte bands with a NaN prefill, and
272-byte bands with base pointers 16 modulo 256, the arrays in reverse order and another prefill - with a workspace of exactly
the queried size.  Reported: a guard word overwritten, an input modified, an output word never written, an output that differs
between the layouts (something read that the call did not write), a refused call that wrote.

And, because the arrays are there: the served rows of the LQR route table against the oracle, and the three entry points of
the imitation-learning update against numpy / float64 autograd."""
import json
import math

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import _lib, pendulum_net
from oracle import kkt as okkt
from oracle import lqr as olqr
from oracle import mpc as ompc
from tests import abi_calls
from tests.helpers import TOL_COSTATE, TOL_PRIMAL, assert_close

pytestmark = pytest.mark.gpu

_RUNS = {}
with open(abi_calls.ROUTES.JSON) as _fh:
    RECORDED_RC = {row["id"]: row["rc"] for row in json.load(_fh)}


def both(case):
    """the row in both layouts (once per session) -> dict(A=arena, B=arena, rc=, findings=[...])"""
    if case.id not in _RUNS:
        lib = _lib.load()
        dev = torch.device("cuda", 0)
        found, arenas = [], {}
        for layout in "AB":
            try:
                a, rc = abi_calls.run(case, layout, lib, dev, torch.cuda.synchronize)
            except RuntimeError as e:      # a HIP error at the synchronisation: nothing that follows on this device means anything
                pytest.exit("%s, layout %s: %s" % (case.id, layout, e), returncode=3)
            if rc > 0:
                pytest.exit("%s, layout %s: HIP error %d" % (case.id, layout, rc), returncode=3)
            found += ["layout %s: %s" % (layout, f) for f in a.check(rc)]
            a.buf = None              # (the host images stay)
            arenas[layout] = a
        found += ["A against B: " + f for f in arenas["A"].compare(arenas["B"])]
        _RUNS[case.id] = dict(A=arenas["A"], B=arenas["B"], rc=arenas["A"].rc, findings=found,
                             kernel=arenas["A"].kernel if arenas["A"].kernel == arenas["B"].kernel else "A: %s; B: %s" % (
                                 arenas["A"].kernel, arenas["B"].kernel))
    return _RUNS[case.id]


@pytest.mark.parametrize("case", abi_calls.CASES, ids=[c.id for c in abi_calls.CASES])
def test_memory_contract(case):
    r = both(case)
    assert r["rc"] <= 0, "HIP error %d" % r["rc"]
    assert r["findings"] == [], "\n".join(r["findings"])
    if case.id.endswith("_refused"):
        assert r["rc"] < 0
    elif "lqr" in case.meta:           # (which rows of the LQR table are served: as tests/golden/lqr_routes.json recorded)
        assert r["rc"] == RECORDED_RC[case.meta["lqr"]["id"]]
    else:
        assert r["rc"] == 0
    print("%s | rc %d | %s" % (case.id, r["rc"], r["kernel"]))
    if "kernel" in case.meta:          # the family the row is there for, by the kernel launched last
        assert case.meta["kernel"] in r["kernel"], r["kernel"]


def test_the_arena_sees_what_a_kernel_leaves_unwritten():
    """the device path of the checks, on a real launch that breaks nothing: dmpc_lin_rollout into an x_out declared one
    time step longer than the call knows - the step it does not write is reported, in layout A by its guard words and between
    the layouts by the two prefills, and nothing else is"""
    T, B, nx, nu = 3, 5, 8, 2
    p = abi_calls.lqr_problem(B, T, nx, nu, 20)

    def make(b, lib):
        u = np.random.RandomState(21).randn(T, B, nu)
        return None, ("dmpc_lin_rollout", [T, B, nx, nu, b.inp("x_init", p["x_init"]), b.inp("u", u), b.inp("F", p["F"]), b.inp("f", p["f"]),
                                           b.out("x_out", (T + 1, B, nx)), None])
    r = both(abi_calls.Case("planted:lin_rollout_longer_x_out", "dmpc_lin_rollout", make))
    assert r["rc"] == 0
    at = T * B * nx * 4
    assert r["findings"] == ["layout A: x_out: not written at byte %d (%d words left)" % (at, B * nx),
                             "A against B: x_out: layouts differ at element %d (byte %d): %r against %r" % (
                                 at // 4, at, r["A"].host("x_out").reshape(-1)[at // 4], np.float32(12345678.0))]


# ---- the served rows of the LQR route table carry numbers, not only names ----
LQR_ROWS = [c for c in abi_calls.CASES if "lqr" in c.meta]
GRAD_TOLS = dict(dx0=TOL_COSTATE, dC=TOL_PRIMAL, dc=TOL_PRIMAL, dF=TOL_COSTATE, df=TOL_COSTATE)     # (tests/test_kkt_gpu.py's)


@pytest.mark.parametrize("case", LQR_ROWS, ids=[c.id for c in LQR_ROWS])
def test_served_lqr_rows_match_the_oracle(case):
    """x, u, the gains and the saved blocks at TOL_PRIMAL against olqr.lqr_solve / olqr.lqr_backward / ompc.lqr_active_solve on
    the values the call read; the gradient rows against okkt.difflqr_backward at the tolerances of tests/test_kkt_gpu.py"""
    r = both(case)
    if r["rc"] != 0:
        assert r["rc"] < 0
        return
    c, a = case.meta["lqr"], r["A"]
    T, nx, nu, fn = c["T"], c["nx"], c["nu"], c["fn"]
    have = a.by_name
    inp = lambda k: a.host(k, a.before).astype(np.float64) if k in have else None      # noqa: E731
    got = lambda k: a.host(k).astype(np.float64)                                       # noqa: E731
    C, cc, F, f, x0 = inp("C"), inp("c"), inp("F"), inp("f"), inp("x_init")
    mask = None if "mask" not in have else a.host("mask", a.before).astype(bool)
    if fn in ("solve", "backward", "backward_ws"):
        if mask is None:
            Ks, ks = olqr.lqr_backward(C, cc, F, f, T, nx, nu)
        else:
            Ks, ks = ompc.lqr_active_backward(C, cc, F, f, mask, T, nx, nu)
        if "Ks" in have:
            assert_close(got("Ks"), Ks, TOL_PRIMAL, "Ks")
            assert_close(got("ks"), ks, TOL_PRIMAL, "ks")
        if fn == "solve":
            xr, ur = (olqr.lqr_solve(x0, C, cc, F, f, T, nx, nu) if mask is None
                      else ompc.lqr_active_solve(x0, C, cc, F, f, mask, T, nx, nu))
            assert_close(got("x"), xr, TOL_PRIMAL, "x")
            assert_close(got("u"), ur, TOL_PRIMAL, "u")
    elif fn == "forward":
        xr, ur = olqr.lqr_forward(inp("Ks"), inp("ks"), x0, F, f, T, nx, nu, u_zero_index=mask)
        assert_close(got("x"), xr, TOL_PRIMAL, "x")
        assert_close(got("u"), ur, TOL_PRIMAL, "u")
    elif fn == "solve_saving":
        blocks = {}
        Ks, ks = olqr.lqr_backward(C, cc, F, f, T, nx, nu, blocks=blocks)
        xr, ur = olqr.lqr_forward(Ks, ks, x0, F, f, T, nx, nu)
        Vv = np.concatenate((blocks["V"], blocks["v"][..., None]), axis=3)
        for k, ref in (("x", xr), ("u", ur), ("Ks", Ks), ("ks", ks), ("Quu", blocks["Quu"]), ("Qxu", blocks["Qxu"]), ("Vv", Vv)):
            assert_close(got(k), ref, TOL_PRIMAL, k)
    elif fn == "saved_solve":
        xr, ur = olqr.lqr_solve(x0, C, inp("c2"), F, None, T, nx, nu)
        assert_close(got("x2"), xr, TOL_PRIMAL, "x2")
        assert_close(got("u2"), ur, TOL_PRIMAL, "u2")
    else:
        ref = okkt.difflqr_backward(x0, C, cc, F, inp("x"), inp("u"), inp("gx"), inp("gu"), T, nx, nu)
        for k, want in zip(("dx0", "dC", "dc", "dF", "df"), ref):
            assert_close(got(k), want, GRAD_TOLS[k], k)


# ---- dmpc_il_batch_begin ----
def cost_map_bound(kind, n, params):
    """-> (bound_Q, bound_p): R 2^-24 times the cost map evaluated on absolute values, R the roundings on the longest path
    of the float32 evaluation: 4 for a sigmoid (exp, add, divide and the exp's own ulp), 1 for sqrt, 1 per product, K for a
    sum of K terms.  Q = diag(q): 4; p = sqrt(q) learn_p: 4/2 + 1 + 1 <= 6.  L L^T: two entries of L (4 each), a product, n
    adds: 9 + n.  Each of the two products with the 4 x 4 observation matrix: 5 more."""
    p = np.asarray(params, dtype=np.float64)
    q = 1.0 / (1.0 + np.exp(-p[:n]))
    if kind in (0, 2):
        M, pt, R = np.diag(q), np.abs(np.sqrt(q) * p[n:2 * n]), 6
    else:
        L = np.diag(q)
        L[np.tril_indices(n, -1)] = np.abs(p[2 * n:])
        M, pt, R = L @ L.T, np.abs(p[n:2 * n]), 9 + n
    if kind in (2, 3):
        O = pendulum_net.OBSERVATION_MATRIX
        M, pt, R = O.T @ M @ O, pt @ O, R + 10
    return R * 2.0 ** -24 * M, R * 2.0 ** -24 * pt


IL_BEGIN_ROWS = [c for c in abi_calls.CASES if c.entry == "dmpc_il_batch_begin" and "il" in c.meta]


@pytest.mark.parametrize("case", IL_BEGIN_ROWS, ids=[c.id for c in IL_BEGIN_ROWS])
def test_il_batch_begin_against_numpy(case):
    """the gathers and the tiles are copies: equal to the bit (indices -1 and N read zeros; warm = NULL gives zeros; u_init =
    NULL is skipped); (Q, p) against net.cost_map() in float64 within cost_map_bound"""
    kind, nx, nu, kw = case.meta["il"]
    r = both(case)
    assert r["rc"] == 0
    a, d = r["A"], abi_calls.il_batch(kind, nx, nu, **kw)
    T, B, N, ns = d["T"], d["B"], d["N"], nx + nu
    ok = (d["idx"] >= 0) & (d["idx"] < N)
    rows = np.where(ok, d["idx"], 0)
    gathered = np.where(ok[:, None, None], d["tau"][rows], np.float32(0))                    # [B,T,ns]
    np.testing.assert_array_equal(a.host("x_init"), gathered[:, 0, :nx])
    np.testing.assert_array_equal(a.host("us"), gathered[:, :, nx:].transpose(1, 0, 2))
    if d["u_init"]:
        warm = np.zeros((B, T, nu), np.float32) if d["warm"] is None else np.where(ok[:, None, None], d["warm"][rows], np.float32(0))
        np.testing.assert_array_equal(a.host("u_init"), warm.transpose(1, 0, 2))
    Q, p = a.host("Q"), a.host("p")
    np.testing.assert_array_equal(a.host("C"), np.broadcast_to(Q, (T, B, ns, ns)))
    np.testing.assert_array_equal(a.host("c"), np.broadcast_to(p, (T, B, ns)))
    Qr, pr = (t.detach().numpy() for t in abi_calls.cost_net(kind, ns, d["params"]).cost_map())
    bQ, bp = cost_map_bound(kind, ns, d["params"])
    assert (np.abs(Q - Qr) <= bQ).all(), (np.abs(Q - Qr).max(), bQ.max())
    assert (np.abs(p - pr) <= bp).all(), (np.abs(p - pr).max(), bp.max())
    assert np.abs(Qr).max() > 0.1


# ---- dmpc_il_loss ----
IL_LOSS_ROWS = [c for c in abi_calls.CASES if c.entry == "dmpc_il_loss" and "il" in c.meta]


@pytest.mark.parametrize("case", IL_LOSS_ROWS, ids=[c.id for c in IL_LOSS_ROWS])
def test_il_loss_against_float64_numpy(case):
    """loss = mean((u - us)^2) within (ceil(n / 1024) + 16) 2^-24 relative (every term is non-negative: one rounding per add
    of a thread's strided sum, ten tree levels, the square, the difference and the divide); grad_u = 2 (u - us) / n within
    4 roundings (difference, the scale 2 / n, the product, the float32 n); the warm-start scatter is a copy"""
    T, B, nu = case.meta["il"]
    r = both(case)
    assert r["rc"] == 0
    a, d = r["A"], abi_calls.il_loss_data(T, B, nu)
    n = T * B * nu
    diff = d["u"].astype(np.float64) - d["us"].astype(np.float64)
    want = float(np.mean(diff ** 2))
    got = float(a.host("loss")[0])
    bound = (math.ceil(n / 1024) + 16) * 2.0 ** -24
    print("il_loss n=%d: relative error %.3e, bound %.3e" % (n, abs(got - want) / want, bound))
    assert abs(got - want) <= bound * want
    gref = 2.0 * diff / n
    assert (np.abs(a.host("grad_u") - gref) <= 4 * 2.0 ** -24 * np.abs(gref)).all()
    warm = d["warm"].copy()
    for b_, row in enumerate(d["idx"]):
        if 0 <= row < d["N"]:
            warm[row] = d["u"][:, b_]
    np.testing.assert_array_equal(a.host("warm"), warm)


# ---- dmpc_il_param_step ----
IL_STEP_ROWS = [c for c in abi_calls.CASES if c.entry == "dmpc_il_param_step" and "il" in c.meta]


@pytest.mark.parametrize("case", IL_STEP_ROWS, ids=[c.id for c in IL_STEP_ROWS])
def test_il_param_step_against_float64_autograd(case):
    """grad, params and ms against float64 autograd + RMSprop (abi_calls.param_step_reference), max |delta| / max(1, |ref|):
    within 4 times the distance of torch's own float32 route from it on the same inputs (the kernel sums in another order
    than torch).  That yardstick is a CPU computation with an assertion of its own,
    tests/test_arena_cpu.py::test_float32_autograd_is_within_float32_of_float64_on_the_param_step_inputs (1.6e-8 to 1.07e-6).
    Measured on an MI355X, kernel / yardstick: kind 0 n_sc 1, 3, 8: 2.16e-8 / 2.16e-8, 3.66e-8 / 3.66e-8, 4.13e-8 / 4.13e-8;
    kind 1 n_sc 1, 3, 8: 1.65e-8 / 1.65e-8, 1.06e-7 / 1.06e-7, 3.28e-7 / 2.35e-7; kind 2: 3.81e-7 / 4.10e-7; kind 3:
    9.52e-7 / 1.07e-6."""
    kind, n = case.meta["il"]
    r = both(case)
    assert r["rc"] == 0
    a, d = r["A"], abi_calls.il_step_data(kind, n)
    ref = abi_calls.param_step_reference(kind, n, d, torch.float64)
    yard = abi_calls.distance(abi_calls.param_step_reference(kind, n, d, torch.float32), ref)
    dist = abi_calls.distance((a.host("grad"), a.host("params"), a.host("ms")), ref)
    print("param_step kind %d n_sc %d: kernel %.3e, float32 autograd %.3e" % (kind, n, dist, yard))
    assert dist <= 4 * yard
    assert np.abs(ref[0]).max() > 1e-3 and not np.array_equal(a.host("params"), d["params"])
