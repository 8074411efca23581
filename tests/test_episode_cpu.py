"""CPU: the C ABI of the closed-loop episode (include/dmpc_episode.h) - the two symbols exported, declared and bound in a table
of their own; every argument error reported before any launch, on pointers that are never dereferenced; the workspace query -
and what needs no GPU of `ClosedLoop`: the shift rule against numpy, `plant_step` on CPU tensors, and the condition the oracle
episode of tests/episode_cases.py is chosen by."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from chainer_differentiable_mpc_amd import BoxDDP, ClosedLoop, LinDx, MlpDx, PendulumDx, QuadCost, _lib, plant_step, shift_plan
from tests import episode_cases as ec
from tests.helpers import assert_close, npy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dmpc_mpc_episode_workspace_bytes", "dmpc_mpc_episode")
P = 4096          # a dummy device pointer: 16-byte aligned, never dereferenced by a refused call


def test_the_symbols_are_exported_declared_and_bound_in_a_table_of_their_own():
    lib = _lib.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmpc_episode.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(dmpc_[a-z0-9_]+)\s*\(", txt))) == sorted(NEW) == sorted(_lib.EPISODE_SIGNATURES)
    for name in NEW:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.EPISODE_SIGNATURES[name][1]
        assert name not in _lib.SIGNATURES and name not in _lib.GRAD_SIGNATURES
    assert len(_lib.EPISODE_SIGNATURES["dmpc_mpc_episode"][1]) == 37
    assert lib.dmpc_version() == _lib.ABI_VERSION == 411


def floats(*v):
    return ctypes.cast((ctypes.c_float * len(v))(*v), ctypes.c_void_p)


PEND = (10.0, 1.0, 1.0, 0.05, 2.0, 1.0)


def call(lib, n_steps=2, T=4, B=2, nx=3, nu=1, x_init=P, C=P, c=P, F=P, f=None, dyn_kind=0, dyn_params=None, plant_F=P, plant_f=None,
         plant_kind=0, plant_params=None, u_init=P, lo=P, hi=P, max_iter=2, n_qp=20, x_log=P, u_log=P, stage=P, state_log=P, ws=P,
         short=0):
    need = lib.dmpc_mpc_episode_workspace_bytes(T, B, nx, nu)
    dp = None if dyn_params is None else floats(*dyn_params)
    pp = None if plant_params is None else floats(*plant_params)
    return lib.dmpc_mpc_episode(n_steps, T, B, nx, nu, x_init, C, c, F, f, dyn_kind, dp, plant_F, plant_f, plant_kind, pp, u_init, lo, hi,
                                1e-3, 5, 0.2, 10, 1e-4, max_iter, n_qp, 1, x_log, u_log, stage, None, None, state_log, ws,
                                need - short, None, None)


BADARG = [dict(n_steps=0), dict(n_steps=-1), dict(T=1), dict(T=0), dict(B=0), dict(nx=0), dict(nu=-1), dict(max_iter=0), dict(n_qp=0),
          dict(x_init=None), dict(C=None), dict(c=None), dict(u_init=None), dict(lo=None), dict(hi=None), dict(x_log=None),
          dict(u_log=None), dict(stage=None), dict(state_log=None), dict(ws=None), dict(ws=P + 4),
          dict(plant_F=None),                                                           # a linear plant needs its matrix
          dict(plant_kind=1, plant_params=None), dict(plant_kind=2, plant_params=None),
          dict(plant_kind=2, plant_params=(5.0, 0.0, 1.0), plant_F=None),
          dict(plant_kind=2, plant_params=(5.0, 0.0, 1.0), plant_f=P),
          dict(plant_kind=2, plant_params=(5.5, 0.0, 1.0)), dict(plant_kind=2, plant_params=(-1.0, 0.0, 1.0)),
          dict(plant_kind=2, plant_params=(5.0, 0.5, 1.0)), dict(plant_kind=2, plant_params=(5.0, -2.0, 1.0)),
          dict(plant_kind=2, plant_params=(float("nan"), 0.0, 1.0)), dict(plant_kind=2, plant_params=(5.0, 0.0, 2.0)),
          # what dmpc_box_ddp reports for the model
          dict(F=None), dict(dyn_kind=1, dyn_params=None), dict(dyn_kind=2, dyn_params=None),
          dict(dyn_kind=2, dyn_params=(5.5, 0.0, 1.0, 0.0)), dict(dyn_kind=2, dyn_params=(5.0, 0.0, 1.0, 0.0), f=P), dict(C=P + 4)]
UNSUPPORTED = [dict(plant_kind=3), dict(plant_kind=-1),
               dict(plant_kind=1, plant_params=PEND, nx=4), dict(plant_kind=1, plant_params=PEND, nu=2),
               dict(plant_kind=2, plant_params=(300.0, 0.0, 1.0)), dict(plant_kind=2, plant_params=(0.0, 0.0, 1.0)),
               dict(plant_kind=2, plant_params=(5.0, 1.0, 1.0)),                      # act 1 is never assigned
               dict(plant_kind=2, plant_params=(5.0, 5.0, 1.0)), dict(plant_kind=2, plant_params=(5.0, 0.0, 1.0), nx=17),
               dict(plant_kind=2, plant_params=(5.0, 0.0, 1.0), nu=9),
               dict(plant_kind=2, plant_params=(float(_lib.mlp_hidden2(129, 5)), 0.0, 1.0)),
               dict(nx=60, nu=5),                                                      # a lane per element of [x;u]
               # what dmpc_box_ddp refuses for the model
               dict(dyn_kind=3), dict(dyn_kind=-1), dict(dyn_kind=2, dyn_params=(300.0, 0.0, 1.0, 0.0)),
               dict(dyn_kind=2, dyn_params=(5.0, 1.0, 1.0, 0.0))]
SERVED = [dict(), dict(plant_f=P), dict(plant_kind=1, plant_params=PEND), dict(plant_kind=1, plant_params=PEND, plant_F=None),
          dict(plant_kind=2, plant_params=(5.0, 0.0, 1.0)), dict(plant_kind=2, plant_params=(256.0, 4.0, 0.0), nx=16, nu=8),
          dict(plant_kind=2, plant_params=(float(_lib.mlp_hidden2(128, 128)), 3.0, 1.0), nx=16, nu=8),
          dict(dyn_kind=1, dyn_params=PEND, F=None, plant_kind=1, plant_params=PEND),
          dict(dyn_kind=2, dyn_params=(5.0, 0.0, 1.0, 0.0), plant_kind=1, plant_params=PEND)]


@pytest.mark.parametrize("kw", BADARG, ids=[str(i) for i in range(len(BADARG))])
def test_bad_arguments_are_reported_before_any_launch(kw):
    assert call(_lib.load(), **kw) == _lib.E_BADARG


@pytest.mark.parametrize("kw", UNSUPPORTED, ids=[str(i) for i in range(len(UNSUPPORTED))])
def test_unsupported_problems_are_reported_before_any_launch(kw):
    assert call(_lib.load(), **kw) == _lib.E_UNSUPPORTED


@pytest.mark.parametrize("kw", SERVED, ids=[str(i) for i in range(len(SERVED))])
def test_a_short_workspace_is_the_only_thing_wrong_with_a_served_call(kw):
    """every argument in order but the workspace: one byte short, and a byte count of zero"""
    lib = _lib.load()
    assert call(lib, short=1, **kw) == _lib.E_WORKSPACE
    args = dict(kw)
    T, B, nx, nu = (args.get(k, v) for k, v in (("T", 4), ("B", 2), ("nx", 3), ("nu", 1)))
    assert call(lib, short=lib.dmpc_mpc_episode_workspace_bytes(T, B, nx, nu), **kw) == _lib.E_WORKSPACE


def test_the_workspace_query_covers_the_solve_and_the_listed_arrays_and_is_monotone():
    lib = _lib.load()
    q = lib.dmpc_mpc_episode_workspace_bytes
    for T, B, nx, nu in ((2, 1, 3, 1), (6, 5, 4, 2), (7, 5, 3, 1), (8, 6, 8, 2), (5, 3, 16, 8), (20, 128, 3, 1)):
        listed = 4 * (B * nx + 2 * T * B * nu + T * B * nx + 3 * B + 8 + B)     # x_cur, u_warm, u_best, x_best, three [B], state, info
        assert q(T, B, nx, nu) >= lib.dmpc_box_ddp_workspace_bytes(T, B, nx, nu) + listed
        assert q(T, B, nx, nu) % 16 == 0
        assert q(T + 1, B, nx, nu) >= q(T, B, nx, nu) and q(T, B + 1, nx, nu) >= q(T, B, nx, nu)
    assert q(0, 1, 3, 1) == 0 and q(4, 0, 3, 1) == 0 and q(4, 2, 0, 1) == 0 and q(4, 2, 3, 0) == 0


@pytest.mark.parametrize("T", [2, 5])
def test_the_shift_rule_against_numpy(T):
    u = np.random.RandomState(T).randn(T, 3, 2)
    want = np.empty_like(u)
    for t in range(T):
        want[t] = u[min(t + 1, T - 1)]
    got = shift_plan(torch.as_tensor(u))
    assert got.shape == (T, 3, 2) and np.array_equal(got.numpy(), want)
    assert np.array_equal(ec.shift_plan(u), want)
    assert np.array_equal(got[-1].numpy(), u[-1]) and np.array_equal(got[-2].numpy(), u[-1])     # the last control is held


def test_the_oracle_episode_applies_controls_on_a_bound_and_strictly_inside():
    """what the seed of tests/episode_cases.LIN is chosen by, on the float64 oracle alone; also: the plant's spectral radius"""
    P, r = ec.lin_problem(), ec.oracle_lin_episode()
    bound, nx = ec.LIN["bound"], ec.LIN["nx"]
    u = r["u"]
    assert u.shape == (ec.N_STEPS, ec.LIN["B"], ec.LIN["nu"]) and r["x"].shape == (ec.N_STEPS + 1, ec.LIN["B"], nx)
    assert (np.abs(u) <= bound).all()
    on, inside = np.abs(u) == bound, np.abs(u) < bound - 1e-2
    assert on.sum() >= 1 and inside.sum() >= 1
    assert (on | inside).all()                       # nothing hovers next to a bound
    assert (r["n_iter"] < ec.MAX_ITER).all()         # every solve converged: the plan does not depend on the warm start
    for b in range(ec.LIN["B"]):
        assert np.abs(np.linalg.eigvals(P["plant_F"][b][:, :nx])).max() < 0.81


def lin_setup(device="cpu"):
    P, k = ec.lin_problem(), ec.LIN
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=device)      # noqa: E731
    solver = BoxDDP(k["T"], -k["bound"], k["bound"], k["B"], k["nx"], k["nu"], None, eps=ec.EPS, max_iter=ec.MAX_ITER,
                    line_search_decay=ec.LS_DECAY, max_line_search_iter=ec.MAX_LS_ITER, quiet=True)
    plant = LinDx(t(P["plant_F"])[None], t(P["plant_f"])[None])
    return solver, plant, t(P["x_init"]), QuadCost(t(P["C"]), t(P["c"])), LinDx(t(P["F"]), t(P["f"]))


def test_plant_step_on_cpu_tensors_is_torch():
    P = ec.lin_problem()
    _, plant, x0, _, _ = lin_setup()
    u = torch.as_tensor(np.random.RandomState(0).uniform(-0.3, 0.3, (ec.LIN["B"], ec.LIN["nu"])))
    assert_close(npy(plant_step(plant, x0, u)), ec.lin_plant_step(P, P["x_init"], u.numpy()), 1e-12, "linear plant")
    pend = PendulumDx()
    x = torch.tensor([[0.6, 0.8, 0.5], [1.0, 0.0, -1.0]], dtype=torch.float64)
    up = torch.tensor([[3.0], [-0.5]], dtype=torch.float64)
    assert torch.equal(plant_step(pend, x, up), pend(x, up))
    net = MlpDx(3, 1, 5, seed=1).double()
    assert torch.equal(plant_step(net, x, up), net(x, up))
    with pytest.raises(TypeError):
        plant_step(object(), x, up)


def test_closed_loop_refuses_what_it_cannot_run():
    solver, plant, *_ = lin_setup()
    with pytest.raises(TypeError):
        ClosedLoop(object(), plant, 2)
    with pytest.raises(TypeError):
        ClosedLoop(solver, PendulumDx(simple=False), 2)
    with pytest.raises(ValueError):
        ClosedLoop(solver, plant, 0)
    from chainer_differentiable_mpc_amd import closed_loop
    assert "NOT differentiable" in closed_loop.__doc__
