"""The conditions that keep tests/test_varying_bounds_gpu.py from passing vacuously, checked on the numpy oracle alone: the
bounds of every row of the route table really vary and pin some controls; the oracle's step puts controls on both kinds of
bound, leaves others strictly inside and touches a bound in every trajectory, at every time step and for every control index;
every way of misreading the bounds (tests/varying_bounds_cases.mutations) moves the oracle's controls by at least a hundred
times the tolerance the kernels are held to, so a kernel that reads them that way fails its comparison; and no row is a
line-search tie, so the plain tolerance applies to all of them.  The same for the linear episode and the pinned box QPs."""
import numpy as np
import pytest

from oracle import pnqp as opnqp
from tests import episode_cases as ec
from tests import varying_bounds_cases as vb
from tests.helpers import TOL_STEP, tie_rows

IDS = [r.id for r in vb.ROUTES]


def test_the_table_has_one_row_per_id_and_two_switch_rows():
    assert len(set(IDS)) == len(IDS)
    assert sorted(tuple(r.env) for r in vb.ROUTES if r.env) == [("DMPC_NO_MPC_ASM",), ("DMPC_NO_MPC_STAGED_FWD",)]
    assert all(r.T in (4, 5) for r in vb.ROUTES)


def test_the_recipe_of_the_bounds():
    lo, hi = vb.bounds(5, 8, 3, 0.25, 7, pin=False)
    assert (lo < 0).all() and (hi > 0).all() and lo.min() >= -0.25 * 1.7 and hi.max() <= 0.25 * 1.7
    assert np.array_equal(lo, lo.astype(np.float32)) and np.array_equal(hi, hi.astype(np.float32))
    plo, phi = vb.bounds(5, 8, 3, 0.25, 7, pin=True)
    pinned = plo == phi
    assert pinned.any() and np.array_equal(plo[~pinned], lo[~pinned]) and np.array_equal(phi[~pinned], hi[~pinned])
    half = (np.abs(plo[pinned] - vb.f32(0.5 * lo[pinned])) == 0) | (np.abs(plo[pinned] - vb.f32(0.5 * hi[pinned])) == 0)
    assert half.all()


@pytest.mark.parametrize("need_expand", [True, False], ids=["recentring", "with_f"])
@pytest.mark.parametrize("row_id", IDS)
def test_a_row_can_fail_its_gpu_comparison(row_id, need_expand):
    f = vb.figures(row_id, need_expand)
    print(row_id, need_expand, f)
    assert f["finite"]
    assert f["ordered"] and f["strict"] and f["distinct"]
    assert 0.0 < f["pinned_share"] <= 0.15
    assert f["lower_share"] >= 0.05 and f["upper_share"] >= 0.05 and f["inside_share"] >= 0.20
    assert f["every_b"] and f["every_t"] and f["every_m"]
    for name, moved in f["sensitivity"].items():
        assert moved >= 100 * TOL_STEP, "bounds %s move u by %.3e only" % (name, moved)
    assert f["ties"] == 0


def test_the_step_case_starts_on_some_bounds_and_away_from_zero():
    p, lo, hi, u_nom, x_nom = vb.route_problem(IDS[0])
    free = lo < hi
    assert ((u_nom == lo) & free).any() and ((u_nom == hi) & free).any() and np.abs(u_nom).max() > 0
    assert (u_nom >= lo).all() and (u_nom <= hi).all()
    assert np.array_equal(x_nom[0], p["x_init"])


@pytest.mark.parametrize("c", vb.COUPLED, ids=[c.id for c in vb.COUPLED])
def test_the_batch_coupled_cases_are_finite_and_active(c):
    for need_expand in (True, False):
        (p, lo, hi, u_nom, x_nom), ref = vb.coupled_case(c.B, c.T, c.nx, c.nu, c.bound, c.seed, need_expand)
        free = lo < hi
        assert np.isfinite(ref["u"]).all() and np.isfinite(ref["Ks"]).all()
        on = (vb.on_lower(ref["u"], lo) | vb.on_upper(ref["u"], hi)) & free
        assert on.any() and (free & ~on).any()


def test_the_linear_episode_with_varying_bounds():
    ep = vb.lin_episode()
    lo, hi = vb.lin_episode_bounds()
    assert (lo < 0).all() and (hi > 0).all()                         # no pins: u_init = None is feasible
    assert (ep["n_iter"] < ec.MAX_ITER).all()                        # every solve converges
    u, l0, h0 = ep["u"], lo[0][None], hi[0][None]                    # the applied control is the plan's first: bounds of t = 0
    on = (u == l0) | (u == h0)
    near = np.minimum(np.abs(u - l0), np.abs(u - h0)) < 0.02
    assert not (near & ~on).any()
    assert on.any() and (~on).any()
    assert ep["warm_outside"] >= 10                                  # the shifted plan leaves the box that did not shift
    assert np.isfinite(ep["x"]).all()


def test_the_box_ddp_cases_are_active_and_no_line_search_ties():
    refs = [vb.ddp_lin_case(*c)[1:] for c in vb.DDP_LIN] + [vb.ddp_mlp_case()[1:]]
    pendulums = [vb.ddp_pendulum_case(B, T) for B, T, _ in vb.DDP_PENDULUM]
    refs += [(q["lo"], q["hi"], dict(q["step"], old_costs=q["old_costs"])) for q in pendulums]
    for lo, hi, ref in refs:
        assert (lo < 0).all() and (hi > 0).all()
        u = ref["u"]
        assert (u == lo).mean() >= 0.05 and (u == hi).mean() >= 0.05 and ((u > lo) & (u < hi)).mean() >= 0.2
        assert not tie_rows(ref["old_costs"], ref["costs"]).any()
    for B, T, _ in vb.DDP_PENDULUM:
        q = vb.ddp_pendulum_case(B, T)
        assert np.abs(q["hi"]).max() < 2.0 and np.abs(q["lo"]).max() < 2.0
        assert np.array_equal(q["first"]["u"], q["step"]["u"])          # the loop's first iteration is that step


def test_the_shared_gradient_case_has_both_kinds_of_active_control():
    q = vb.shared_case()
    pinned = q["lo"] == q["hi"]
    assert pinned.any() and np.array_equal(q["u"][pinned], q["lo"][pinned])
    assert ((q["u"] == q["lo"]) & ~pinned).any() and ((q["u"] == q["hi"]) & ~pinned).any()
    assert ((q["u"] > q["lo"]) & (q["u"] < q["hi"])).mean() > 0.3
    T, B, nx, nu = vb.SHARED_SHAPE
    for axis in (0, 1):                                                  # a mask from misread bounds moves the gradient
        mlo, mhi = np.roll(q["lo"], 1, axis=axis), np.roll(q["hi"], 1, axis=axis)
        ref = vb.ompc.mpc_backward(q["x"][0], q["C"], q["c"], q["F"], np.zeros((T - 1, B, nx)), q["x"], q["u"], mlo, mhi, q["gx"],
                                   q["gu"], T, nx, nu)
        assert np.abs(ref[3][:T - 1].sum(axis=(0, 1)) - q["dF"].sum(axis=(0, 1))).max() > 1e-1


@pytest.mark.parametrize("n", [1, 2, 8, 9])
def test_the_pinned_box_qps(n):
    q = vb.pinned_qp(n)
    pinned = q["pinned"]
    assert pinned[0].all() and not pinned[1].any() and 0.15 < pinned[2:].mean() < 0.5
    assert np.array_equal(q["lower"][pinned], q["upper"][pinned]) and (q["lower"][~pinned] < q["upper"][~pinned]).all()
    for coupled in (False, True):
        x, fac, idx_f, i, info = opnqp.pnqp(q["H"], q["q"], q["lower"], q["upper"], batch_coupled=coupled, return_info=True, warn=False)
        assert np.isfinite(x).all() and np.array_equal(x[pinned], q["lower"][pinned])
        if not coupled:
            assert info["iters"][0] == 0                             # a fully pinned row has nowhere to go: stops at pass 0
