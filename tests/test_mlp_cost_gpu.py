"""GPU: `MlpCost` on the device kernels (include/dmpc_mlp_cost.h) against the float64 restatement and oracle of
tests/mlp_cost_cases.py: the Taylor model of one launch, `MPCstep` with the cost inside its line-search kernel against two
iterates of the reference's loop, the `stage_costs` route under other dynamics, `BoxDDP`'s host loop over the new kernels, the
parameter gradient of one kernel and a fixed-order reduction, and a hipGraph capture of the launches.  The tolerances are the
project's own (tests/helpers.py); every assertion logs its margin through DMPC_PARITY_LOG."""
import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import BoxDDP, LinDx, MlpCost, MlpDx, MPCstep, _lib, approximate_cost
from chainer_differentiable_mpc_amd.lqr_recursion import _workspace
from tests import mlp_cost_cases as mc
from tests.helpers import TOL_COSTATE, TOL_PRIMAL, TOL_STEP, assert_close, assert_step_close, npy

pytestmark = pytest.mark.gpu

# every activation on A, every other case once
ROWS = [(act, "A") for act in mc.ACTS] + [("tanh", "B"), ("softplus", "C"), ("silu", "D"), ("relu", "E")]
IDS = ["%s-%s" % (name, act) for act, name in ROWS]
SEARCH_KERNEL = "mpc_forward_rec_mlp_cost_kernel"


def dev(a):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.float32, device="cuda")


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def lin_dx(P):
    return LinDx(dev(P["F"]), dev(P["f"]))


# ---------------------------------------------------------------------- the Taylor model
@pytest.mark.parametrize("act,name", ROWS, ids=IDS)
def test_taylor_model_against_the_oracle(act, name):
    P = mc.problem(act, name)
    x, u, _, _ = mc.grad_points(P)
    H_ref, g_ref, c_ref = mc.taylor_along(P["cost"], x, u)
    m = mc.module(P)
    xd, ud = dev(x), dev(u)
    with torch.no_grad():
        assert m.approx_ok(xd, ud)
        H, g0, costs = m.approximate(xd, ud)
        assert "mlp_cost_approx_kernel" in _lib.last_kernel_name()
        hooked = approximate_cost(xd, ud, m)
        values = m.stage_costs(xd, ud)
    assert_close(npy(H), H_ref, TOL_PRIMAL, "mlp_cost H")
    assert_close(npy(costs), c_ref, TOL_PRIMAL, "mlp_cost costs")
    assert_close(npy(g0), g_ref, TOL_COSTATE, "mlp_cost g0")
    assert torch.equal(H, H.transpose(2, 3))
    for got, want in zip(hooked, (H, g0, costs)):
        assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(values), bits(costs))
    assert not m.approx_ok(xd, ud)                # "live": a call that wants a gradient keeps the autograd route
    m.param_grad = "device"
    assert m.approx_ok(xd, ud) and not m.approx_ok(xd.clone().requires_grad_(True), ud)
    node = approximate_cost(xd, ud, m)
    assert not node[0].requires_grad and node[1].requires_grad and node[2].requires_grad
    for got, want in zip(node, (H, g0, costs)):
        assert np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------------- MPCstep
def make_step(P, it, m, **kw):
    nx, nu, H, B, T = P["dims"]
    return MPCstep(controls=dev(it["controls"]), T=T, u_upper=dev(P["hi"]), u_lower=dev(P["lo"]), n_batch=B, n_state=nx, n_ctrl=nu,
                   current_states=dev(it["states"]), true_cost=m, true_dynamics=lin_dx(P), ls_decay=mc.LS_DECAY,
                   max_ls_iter=mc.MAX_LS_ITER, need_expand=True, **kw)


@pytest.mark.parametrize("k", [0, 1], ids=["first", "second"])
@pytest.mark.parametrize("act,name", ROWS, ids=IDS)
def test_mpc_step_against_the_oracle_iterates(act, name, k):
    """T > 1: the whole step (`forward`: re-centring, backward_rec, the new search).  T = 1 (no dynamics step, which
    dmpc_mpc_backward_rec does not serve): the search alone, `forward_rec` on the oracle's gains."""
    P = mc.problem(act, name)
    nx, nu, H, B, T = P["dims"]
    it = mc.oracle_iterates(act, name)[k]
    m = mc.module(P)
    step = make_step(P, it, m)
    with torch.no_grad():
        if T > 1:
            x, u = step.forward((dev(P["x_init"]), dev(it["C"]), dev(it["c"]), dev(P["F"]), dev(P["f"])))
            costs = step.for_out.costs
        else:
            x, u, res = step.forward_rec(dev(it["Ks"]), dev(it["ks"]), m, lin_dx(P), mc.LS_DECAY, mc.MAX_LS_ITER)
            costs = res.costs
    assert SEARCH_KERNEL in _lib.last_kernel_name()
    strict = ~it["ties"]
    assert strict.any() or name not in mc.NO_TIE_IN_SECOND
    what = "mlp_cost step %d" % k
    assert_step_close(npy(u), npy(x), it["u"], it["x"], it["old_costs"], it["costs"], mc.candidates_of(P, it), TOL_STEP, what)
    if strict.any():
        assert_close(npy(costs)[strict], it["costs"][strict], TOL_STEP, what + " costs")
        assert np.array_equal(step.n_ls_iter.cpu().numpy()[strict], it["n_ls"][strict])
        assert np.abs(npy(step.alphas)[strict] - it["alphas"][strict]).max() <= 1e-6


@pytest.mark.parametrize("act,name", ROWS, ids=IDS)
def test_zero_gains_reproduce_the_iterate(act, name):
    """a candidate equal to the nominal trajectory: cost difference exactly 0, one pass at alpha = 1, the same bits.  The total
    the search reports against the sum of `stage_costs` over t: the same float32 stage values added in another order - at most
    T + log2(64) roundings of 6e-8 apart, 1e-6 at these T <= 6."""
    P = mc.problem(act, name)
    nx, nu, H, B, T = P["dims"]
    it = mc.oracle_iterates(act, name)[1]
    m = mc.module(P)
    u0, x0, dyn = dev(it["controls"]), dev(P["x_init"]), lin_dx(P)
    xs = BoxDDP._nominal(T, u0, x0, dyn) if T > 1 else x0[None].clone()
    step = make_step(P, dict(controls=it["controls"], states=npy(xs)), m)
    with torch.no_grad():
        x, u, res = step.forward_rec(torch.zeros(T, B, nu, nx, device="cuda"), torch.zeros(T, B, nu, device="cuda"), m, dyn,
                                     mc.LS_DECAY, mc.MAX_LS_ITER)
    assert SEARCH_KERNEL in _lib.last_kernel_name()
    assert np.array_equal(bits(x), bits(xs)) and np.array_equal(bits(u), bits(u0))
    assert (step.n_ls_iter == 1).all() and (step.alphas == 1.0).all()
    with torch.no_grad():
        assert_close(npy(res.costs), npy(m.stage_costs(xs, u0).sum(dim=0)), 1e-6, "mlp_cost search total against stage_costs")


def test_stage_costs_route_under_other_dynamics():
    """an `MlpDx` as dynamics: no in-kernel search for that pair - the host search evaluates the cost by one launch per pass"""
    P = mc.problem("softplus", "A")
    nx, nu, H, B, T = P["dims"]
    m = mc.module(P)
    dyn = MlpDx(nx, nu, 6, seed=4).to("cuda")
    u0, x0 = torch.zeros(T, B, nu, device="cuda"), dev(P["x_init"])
    out = {}
    with torch.no_grad():
        xs, F, f = dyn.rollout_linearize(x0, u0)
        C, c, _ = m.approximate(xs, u0)
        for route, cost in (("device", m), ("lambda", lambda tau: m(tau))):
            step = MPCstep(controls=u0, T=T, u_upper=dev(P["hi"]), u_lower=dev(P["lo"]), n_batch=B, n_state=nx, n_ctrl=nu,
                           current_states=xs, true_cost=cost, true_dynamics=dyn, ls_decay=mc.LS_DECAY, max_ls_iter=mc.MAX_LS_ITER,
                           need_expand=True)
            x, u = step.forward((x0, C, c, F, f))
            out[route] = (npy(x), npy(u), npy(step.for_out.costs), step.n_ls_iter.cpu().numpy(), _lib.last_kernel_name())
    assert "mlp_cost_approx_kernel" in out["device"][4] and "mlp_cost" not in out["lambda"][4]
    for got, want, what in zip(out["device"][:3], out["lambda"][:3], ("x", "u", "costs")):
        assert_close(got, want, TOL_STEP, "mlp_cost stage_costs route " + what)
    assert np.array_equal(out["device"][3], out["lambda"][3])
    assert np.abs(out["device"][1]).max() > 0.05


# ---------------------------------------------------------------------- BoxDDP
def box_ddp(P, m, max_iter=4, **kw):
    nx, nu, H, B, T = P["dims"]
    return BoxDDP(T, dev(P["lo"]), dev(P["hi"]), B, nx, nu, None, max_iter=max_iter, line_search_decay=mc.LS_DECAY,
                  max_line_search_iter=mc.MAX_LS_ITER, quiet=True, exit_unconverged=False, **kw)


@pytest.mark.parametrize("which", ["B-softplus", "soft_box"])
def test_box_ddp_host_loop_against_the_restated_oracle_loop(which):
    if which == "soft_box":
        P = mc.soft_box_problem()
        m = MlpCost.soft_box(2, 1, P["x_lower"], P["x_upper"], weight=P["weight"], sharpness=P["sharpness"], Q=P["Q"], p=P["p"]).to("cuda")
    else:
        P = mc.problem("softplus", "B")
        m = mc.module(P)
    nx, nu, H, B, T = P["dims"]
    x_ref, u_ref, c_ref, n_ref = mc.oracle_box_ddp(P["cost"], P["dyn"], P["x_init"], P["lo"], P["hi"], T, nx, nu, max_iter=4)
    solver = box_ddp(P, m, detach_unconverged=False)
    with torch.no_grad():
        x, u, costs = solver.forward((dev(P["x_init"]), m, lin_dx(P)))
    assert SEARCH_KERNEL in _lib.last_kernel_name()            # the host loop's last launch: the last step's search
    assert_close(npy(costs), c_ref, 1e-4, "mlp_cost BoxDDP %s costs" % which)
    assert n_ref >= 2 and solver.n_iter >= 2
    if which == "soft_box":       # the limit is felt: the second trajectory ends at it, not at the linear cost's pull
        assert 0.9 < x_ref[:, 1, 0].max() < 1.1 and npy(x)[:, 1, 0].max() < 1.1


# ---------------------------------------------------------------------- the parameter gradient
@pytest.mark.parametrize("upstream", ["grad_g", "grad_costs", "both"])
@pytest.mark.parametrize("act,name", ROWS, ids=IDS)
def test_parameter_gradient_against_the_float64_sums(act, name, upstream):
    P = mc.problem(act, name)
    x, u, v, r = mc.grad_points(P)
    v = v if upstream != "grad_costs" else None
    r = r if upstream != "grad_g" else None
    m = mc.module(P, param_grad="device")
    H, g0, costs = m.approximate(dev(x), dev(u))
    assert g0.grad_fn is not None and g0.grad_fn is costs.grad_fn and not H.requires_grad
    loss = 0.0
    if v is not None:
        loss = loss + (dev(v) * g0).sum()
    if r is not None:
        loss = loss + (dev(r) * costs).sum()
    params = [m.Q, m.p, m.W1, m.b1, m.w2]
    first = torch.autograd.grad(loss, params, retain_graph=True)
    again = torch.autograd.grad(loss, params)
    ref = P["cost"].grad_sums(np.concatenate((x, u), axis=2), v, r)
    for got, rep, want, what in zip(first, again, ref, ("dQ", "dp", "dW1", "db1", "dw2")):
        assert_close(npy(got), want, TOL_COSTATE, "mlp_cost %s (%s)" % (what, upstream))
        assert np.array_equal(bits(got), bits(rep)), what                  # no atomics: bit-equal from call to call


@pytest.mark.parametrize("act", ["softplus", "relu"])
def test_box_ddp_gradient_device_against_live(act):
    """d sum(u*) / d(Q, p, W1, b1, w2) of a solve: the one-node device route against the autograd route"""
    P = mc.problem(act, "A")
    grads = {}
    for mode in ("device", "live"):
        m = mc.module(P, param_grad=mode)
        solver = box_ddp(P, m, max_iter=6, detach_unconverged=False, update_dynamics=False)     # the cost is what is learnt
        x, u, _ = solver.forward((dev(P["x_init"]), m, lin_dx(P)))
        assert u.requires_grad
        u.sum().backward()
        grads[mode] = [npy(w.grad) for w in (m.Q, m.p, m.W1, m.b1, m.w2)]
    for got, want, what in zip(grads["device"], grads["live"], ("Q", "p", "W1", "b1", "w2")):
        assert_close(got, want, TOL_COSTATE, "mlp_cost BoxDDP gradient %s, device against live" % what)
        if act == "relu" and what == "b1":
            assert not got.any()        # db1 = w2 act''(z) q + r w2 act'(z): relu has act'' = 0, and sum(u*) does not read the costs (r = 0)
        else:
            assert np.abs(got).max() > 0, what


# ---------------------------------------------------------------------- graph capture
def test_the_launches_capture_in_a_graph():
    """The Taylor model through `approximate`, then what one `MPCstep.forward` enqueues for this cost - the re-centring,
    `dmpc_mpc_backward_rec` and the new search - and the parameter gradient, captured by `torch.cuda.graph` and replayed: the
    same bits as the eager run.  (`MPCstep.forward` itself reads the step's flags back, as the reference asserts on them; the
    launches are captured at the C ABI.)"""
    P = mc.problem("softplus", "B")
    nx, nu, H, B, T = P["dims"]
    ns = nx + nu
    it = mc.oracle_iterates("softplus", "B")[1]
    m = mc.module(P)
    lib = _lib.load()
    d = torch.device("cuda", torch.cuda.current_device())
    xs, u0, lo, hi, F, f = (dev(a) for a in (it["states"], it["controls"], P["lo"], P["hi"], P["F"], P["f"]))
    v, r = dev(mc.grad_points(P)[2]), dev(mc.grad_points(P)[3])
    p = _lib.ptr

    def run():
        with torch.no_grad():
            Hm, g0, costs = m.approximate(xs, u0)
            c = torch.einsum("tbij,tbj->tbi", Hm, torch.cat((xs, u0), dim=2)) + g0            # need_expand, mpc_step.py:305-317
            f32 = dict(dtype=torch.float32, device=d)
            Ks, ks, nqp = torch.empty(T, B, nu, nx, **f32), torch.empty(T, B, nu, **f32), torch.empty(B, dtype=torch.int32, device=d)
            info = torch.zeros(B, dtype=torch.int32, device=d)
            stream = _lib.stream_ptr(d)
            assert lib.dmpc_mpc_backward_rec(T, B, nx, nu, p(Hm), p(c), p(F), None, p(u0), p(lo), p(hi), 20, 0, p(Ks), p(ks), p(nqp),
                                             None, 0, p(info), stream) == 0
            x, u = torch.empty(T, B, nx, **f32), torch.empty(T, B, nu, **f32)
            cs, al, nls = torch.empty(B, **f32), torch.empty(B, **f32), torch.empty(B, dtype=torch.int32, device=d)
            w = m.device_weights(d)
            assert lib.dmpc_mpc_forward_rec_mlp_cost(T, B, nx, nu, H, m.act_code, *(p(t) for t in w), p(Ks), p(ks), p(u0), p(xs), p(lo),
                                                     p(hi), p(F), p(f), mc.LS_DECAY, mc.MAX_LS_ITER, p(x), p(u), p(cs), None, p(al),
                                                     None, None, p(nls), p(info), stream) == 0
            outs = [torch.empty_like(t) for t in w]
            need = lib.dmpc_mlp_cost_param_grad_workspace_bytes(T, B, nx, nu, H)
            ws = _workspace(need, d)
            assert lib.dmpc_mlp_cost_param_grad(T, B, nx, nu, H, m.act_code, p(w[2]), p(w[3]), p(w[4]), p(x), p(u), p(v), p(r),
                                                *(p(o) for o in outs), p(ws), need, stream) == 0
        return [Hm, g0, costs, x, u, cs, al] + outs

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # warm-up on a side stream (allocations, library load); also the eager result
        eager = [t.clone() for t in run()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert_close(npy(eager[4]), it["u"], TOL_STEP, "mlp_cost captured chain u (eager)")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(got, eager):
            assert np.array_equal(bits(a), bits(b))
