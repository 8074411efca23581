"""`ClosedLoop` - a receding-horizon (closed-loop) MPC episode around a `BoxDDP` controller:

    loop = ClosedLoop(solver, plant, n_steps, device_episode=True)
    out  = loop(x_init, cost, dynamics)
    # -> EpisodeOut(x [n+1,B,nx], u [n,B,nu], stage_costs [n,B], state [n,8] int32, info [B] int32, x_plan, u_plan)

Each of the `n_steps` steps solves from the current state with `solver` (its T, bounds, u_init, eps, max_iter, ...) on the
model `dynamics`, applies the plan's first control to `plant`, logs the step and shifts the plan into the next solve's warm
start (`shift_plan`: u[t] <- u[t+1], the last control held).  `cost` is the same at every step: a time-invariant stage cost over
a sliding horizon, of which `stage_costs[k]` is the t = 0 term at (x_k, u_k).  `x_plan`, `u_plan` are the last solve's best
trajectory, `state[k]` the loop state of solve k (`dmpc_box_ddp`: [1] iterations run, [2] 1 Converged / 2 Not improved lim /
3 Not Converged, ...), `info` the OR of the solves' per-trajectory flags.

`plant` is a `LinDx` (its first block F[0], f[0] is the time-invariant plant), a simple `PendulumDx` or an `MlpDx`;
`plant_step(plant, x, u)` is one step of it with no solver around it.

Where `BoxDDP._device_loop` would run the solve as one chain of launches - GPU tensors, a dense `QuadCost`, no `batch_coupled`,
and `dynamics` a `LinDx`, the simple pendulum or an `MlpDx(device_loop=True)` - the whole episode is ONE chain
(`dmpc_mpc_episode`, include/dmpc_episode.h): per step the solve's launches and one launch that does everything between two
solves, no host round trip, ONE read-back per episode (`state`), from which come the solver's input asserts and the non-finite
check, raised as `BoxDDP` raises them.  `lazy_status=True` on the solver defers that read-back to `resolve()`, at the latest
the next call.  Anything else, or `device_episode=False`, runs the host loop: `solver`, `plant_step`, a torch shift - the same
fields (of `state` the host loop fills [1] and [2]).

An `MlpDx` used as model or plant goes through `packed_weights` before every call, so an optimiser step in place is seen by the
next episode; nothing is cached.  The whole call runs under `torch.no_grad()`: an episode is NOT differentiable.  The class
records no hipGraph of its own; a caller may capture the call (no read-back happens while a capture is open)."""
import collections
import ctypes

import torch

from . import _lib
from .box_ddp import _UNRESOLVED, BoxDDP
from .lqr_recursion import _as_tensor, _workspace
from .mlp_dx import MlpDx
from .mpc_step import _is_simple_pendulum
from .util import LinDx, QuadCost

EpisodeOut = collections.namedtuple("EpisodeOut", "x u stage_costs state info x_plan u_plan")

_STATUS_CODE = {"Converged": 1, "Not improved lim": 2, "Not Converged": 3}


def shift_plan(u):
    """the next solve's warm start from a plan u [T,B,nu]: u[t] <- u[t+1] for t < T-1, the last control held"""
    return torch.cat((u[1:], u[-1:]), dim=0)


def _is_plant(plant):
    return isinstance(plant, (LinDx, MlpDx)) or _is_simple_pendulum(plant)


def plant_step(plant, x, u):
    """x [B,nx], u [B,nu] -> the plant's next state [B,nx].  GPU tensors: the rollout entry point of that kind of plant at T = 2
    (`dmpc_lin_rollout`, `dmpc_pendulum_rollout_linearize`, `MlpDx.rollout_linearize`) - the step functions the episode chain
    evaluates, so both give the same bits; otherwise torch."""
    with torch.no_grad():
        on_gpu = isinstance(x, torch.Tensor) and x.is_cuda and u.is_cuda
        u2 = torch.stack((u, u), dim=0)              # [2,B,nu]: the rollouts take a horizon of controls, step 0 is applied
        if isinstance(plant, LinDx):
            F0 = plant.F[0].detach()
            f0 = None if plant.f is None else plant.f[0].detach()
            if not on_gpu:
                nxt = torch.einsum("bij,bj->bi", F0.to(x), torch.cat((x, u), dim=1))
                return nxt if f0 is None else nxt + f0.to(x)
            lib = _lib.load()
            d = x.device
            B, nx, nu = x.shape[0], x.shape[1], u.shape[1]
            x0, ud = _lib.f32c(x.detach(), d), _lib.f32c(u2, d)
            Fd, fd = _lib.f32c(F0[None], d), (None if f0 is None else _lib.f32c(f0[None], d))
            out = torch.empty((2, B, nx), dtype=torch.float32, device=d)
            with _lib.guard(d):
                rc = lib.dmpc_lin_rollout(2, B, nx, nu, _lib.ptr(x0), _lib.ptr(ud), _lib.ptr(Fd), _lib.ptr(fd), _lib.ptr(out),
                                          _lib.stream_ptr(d))
            _lib.check(rc, "dmpc_lin_rollout")
            return out[1].to(x.dtype)
        if _is_simple_pendulum(plant):
            if on_gpu:
                return plant.rollout_linearize(x, u2, want_model=False)[0][1]
            return plant(x, u)
        if isinstance(plant, MlpDx):
            if on_gpu and plant.supported():
                return plant.rollout_linearize(x, u2, want_model=False)[0][1]
            return plant(x, u)
    raise TypeError("ClosedLoop: the plant is a LinDx, a simple PendulumDx or an MlpDx, found %r" % (plant,))


class ClosedLoop:
    def __init__(self, solver, plant, n_steps, device_episode=True):
        if not isinstance(solver, BoxDDP):
            raise TypeError("ClosedLoop: the controller is a BoxDDP, found %r" % (solver,))
        if not _is_plant(plant):
            raise TypeError("ClosedLoop: the plant is a LinDx, a simple PendulumDx or an MlpDx, found %r" % (plant,))
        if int(n_steps) < 1:
            raise ValueError("ClosedLoop: n_steps >= 1, found %r" % (n_steps,))
        self.solver, self.plant, self.n_steps = solver, plant, int(n_steps)
        self.device_episode = bool(device_episode)
        self.route = None           # "chain" / "host": what the last call ran
        self._pending = None        # the chain's state log, not read back yet: (device [n,8] | (pinned [n,8], event))
        self._host_state = None

    # ------------------------------------------------------------------ the one read-back
    def resolve(self):
        """the episode's one synchronisation: MPCstep's input asserts and the non-finite check of every solve, as BoxDDP raises them"""
        if self._pending is None:
            return
        state = self._pending
        self._pending = None
        if isinstance(state, tuple):
            state[1].synchronize()
            rows = state[0].tolist()
        else:
            rows = state.cpu().tolist()
        assert not any(r[4] for r in rows)
        assert not any(r[5] for r in rows), " lower is larger than upper"
        bad = max(r[6] for r in rows)
        if bad:
            raise AssertionError("BoxDDP: NaN/Inf in the solution of %d trajectories" % bad)

    # ------------------------------------------------------------------ the device chain
    def _model(self, dynamics, x_init, u, d):
        """(dyn_kind, F, f, host params) of the controller's model as BoxDDP._device_loop takes it, or None"""
        s = self.solver
        T, B, nx, nu = s.T, s.n_batch, s.n_state, s.n_ctrl
        if isinstance(dynamics, LinDx):
            F = _lib.f32c(_as_tensor(dynamics.F).detach(), d)
            f = None if dynamics.f is None else _lib.f32c(_as_tensor(dynamics.f).detach(), d)
            if F.shape[0] not in (T - 1, T) or list(F.shape[1:]) != [B, nx, nx + nu]:
                return None
            if f is not None and list(f.shape) != [T - 1, B, nx]:
                return None
            return 0, F, f, None
        if _is_simple_pendulum(dynamics) and dynamics.fused_ok(x_init, u) and (nx, nu) == (3, 1):
            g_, m_, l_ = dynamics.host_params()
            return 1, None, None, (ctypes.c_float * 6)(g_, m_, l_, float(dynamics.dt), float(dynamics.max_torque),
                                                       1.0 if dynamics.clamp_grad_closed else 0.0)
        if isinstance(dynamics, MlpDx) and dynamics.device_loop and (nx, nu) == (dynamics.n_state, dynamics.n_ctrl) and \
                dynamics.fused_ok(x_init, u):
            return 2, dynamics.packed_weights(d), None, (ctypes.c_float * 4)(*dynamics.host_params())
        return None

    def _plant(self, dynamics, model, x_init, d):
        """(plant_kind, plant_F, plant_f, host params) or None; a model that is also the plant packs once"""
        s, p = self.solver, self.plant
        B, nx, nu = s.n_batch, s.n_state, s.n_ctrl
        if isinstance(p, LinDx):
            F0 = _lib.f32c(_as_tensor(p.F).detach()[0], d)
            f0 = None if p.f is None else _lib.f32c(_as_tensor(p.f).detach()[0], d)
            if list(F0.shape) != [B, nx, nx + nu] or (f0 is not None and list(f0.shape) != [B, nx]):
                return None
            return 0, F0, f0, None
        if _is_simple_pendulum(p):
            if (nx, nu) != (3, 1):
                return None
            g_, m_, l_ = p.host_params()
            return 1, None, None, (ctypes.c_float * 6)(g_, m_, l_, float(p.dt), float(p.max_torque), 0.0)
        if (p.n_state, p.n_ctrl) != (nx, nu) or not p.supported():
            return None
        packed = model[1] if (p is dynamics and model[0] == 2) else p.packed_weights(d)
        return 2, packed, None, (ctypes.c_float * 3)(*p.host_params()[:3])

    def _chain(self, x_init, cost, dynamics, u, lo, hi):
        s = self.solver
        T, B, nx, nu, n = s.T, s.n_batch, s.n_state, s.n_ctrl, self.n_steps
        ns = nx + nu
        if not (isinstance(cost, QuadCost) and s.device_loop and not s.batch_coupled and not s.verbose and not s.ilqr_verbose):
            return None
        if not (isinstance(x_init, torch.Tensor) and x_init.is_cuda) or T < 2 or ns > 64:
            return None
        d = x_init.device
        u0 = _lib.f32c(u, d)
        x0 = _lib.f32c(x_init.detach(), d)
        model = self._model(dynamics, x0, u0, d)
        if model is None:
            return None
        plant = self._plant(dynamics, model, x0, d)
        if plant is None:
            return None
        C, c = _lib.f32c(_as_tensor(cost.C).detach(), d), _lib.f32c(_as_tensor(cost.c).detach(), d)
        if list(C.shape) != [T, B, ns, ns] or list(c.shape) != [T, B, ns]:
            return None
        lo_, hi_ = _lib.f32c(lo, d), _lib.f32c(hi, d)
        lib = _lib.load()
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.resolve()
            for other in list(_UNRESOLVED):       # solves whose read-back was deferred: their asserts come now
                other._resolve()
        n_xl, n_ul, n_xp, n_up = (n + 1) * B * nx, n * B * nu, T * B * nx, T * B * nu
        fl = torch.empty((n_xl + n_ul + n * B + n_xp + n_up,), dtype=torch.float32, device=d)
        ints = torch.empty((n * 8 + B,), dtype=torch.int32, device=d)
        x_log, u_log = fl[:n_xl].view(n + 1, B, nx), fl[n_xl:n_xl + n_ul].view(n, B, nu)
        off = n_xl + n_ul
        costs = fl[off:off + n * B].view(n, B)
        x_plan = fl[off + n * B:off + n * B + n_xp].view(T, B, nx)
        u_plan = fl[off + n * B + n_xp:].view(T, B, nu)
        state, info = ints[:n * 8].view(n, 8), ints[n * 8:]
        need = lib.dmpc_mpc_episode_workspace_bytes(T, B, nx, nu)
        ws = _workspace(need, d)
        cast = lambda p: None if p is None else ctypes.cast(p, ctypes.c_void_p)      # noqa: E731
        with _lib.guard(d):
            rc = lib.dmpc_mpc_episode(n, T, B, nx, nu, _lib.ptr(x0), _lib.ptr(C), _lib.ptr(c), _lib.ptr(model[1]), _lib.ptr(model[2]),
                                      model[0], cast(model[3]), _lib.ptr(plant[1]), _lib.ptr(plant[2]), plant[0], cast(plant[3]),
                                      _lib.ptr(u0), _lib.ptr(lo_), _lib.ptr(hi_), float(s.eps), int(s.not_improved_lim),
                                      float(s.ls_decay), int(s.max_ls_iter), float(s.best_cost_eps), int(s.max_iter), 20, 1,
                                      _lib.ptr(x_log), _lib.ptr(u_log), _lib.ptr(costs), _lib.ptr(x_plan), _lib.ptr(u_plan),
                                      _lib.ptr(state), _lib.ptr(ws), need, _lib.ptr(info), _lib.stream_ptr(d))
        if rc == _lib.E_UNSUPPORTED:
            return None
        _lib.check(rc, "dmpc_mpc_episode")
        if not capturing:
            if s.lazy_status:          # the state log to pinned memory behind the chain, with its event
                if self._host_state is None or self._host_state[0].shape[0] != n:
                    self._host_state = (torch.empty((n, 8), dtype=torch.int32, pin_memory=True), torch.cuda.Event())
                self._host_state[0].copy_(state, non_blocking=True)
                self._host_state[1].record()
                self._pending = self._host_state
            else:
                self._pending = state
                self.resolve()
        dt = x_init.dtype
        return EpisodeOut(x_log.to(dt), u_log.to(dt), costs.to(dt), state, info, x_plan.to(dt), u_plan.to(dt))

    # ------------------------------------------------------------------ the host loop
    def _host(self, x_init, cost, dynamics):
        s, n = self.solver, self.n_steps
        if not isinstance(cost, QuadCost):
            raise TypeError("ClosedLoop: the stage cost of an episode is a QuadCost, found %r" % (cost,))
        B = s.n_batch
        x = x_init.detach()
        xs, us, costs, rows = [x], [], [], []
        info = torch.zeros((B,), dtype=torch.int32, device=x.device)
        keep = s.u_init
        try:
            for _ in range(n):
                x_plan, u_plan, _costs = s((x, cost, dynamics))
                u0 = u_plan[0]
                tau = torch.cat((x, u0), dim=1)
                C0, c0 = _as_tensor(cost.C)[0].detach().to(tau), _as_tensor(cost.c)[0].detach().to(tau)
                costs.append(0.5 * torch.einsum("bi,bij,bj->b", tau, C0, tau) + (c0 * tau).sum(dim=1))
                x = plant_step(self.plant, x, u0)
                xs.append(x)
                us.append(u0)
                rows.append([0, int(s.n_iter), _STATUS_CODE.get((s.status or "").strip(), 0), 0, 0, 0, 0, 0])
                if isinstance(s.info, torch.Tensor):
                    info |= s.info.to(device=info.device, dtype=torch.int32)
                s.u_init = shift_plan(u_plan)
        finally:
            s.u_init = keep
        state = torch.tensor(rows, dtype=torch.int32, device=x.device)
        return EpisodeOut(torch.stack(xs, 0), torch.stack(us, 0), torch.stack(costs, 0), state, info, x_plan, u_plan)

    def __call__(self, x_init, cost, dynamics):
        with torch.no_grad():
            s = self.solver
            x_init = _as_tensor(x_init)
            T, B, nx, nu = s.T, s.n_batch, s.n_state, s.n_ctrl
            assert list(x_init.shape) == [B, nx], " x_init dim mismatch"
            if self.device_episode:
                dev, dt = x_init.device, x_init.dtype
                if s.u_init is None:
                    u = torch.zeros((T, B, nu), dtype=dt, device=dev)
                else:
                    u = _as_tensor(s.u_init).to(device=dev, dtype=dt)
                    if list(u.shape) == [T, nu]:
                        u = u.unsqueeze(1).repeat(1, B, 1)
                assert list(u.shape) == [T, B, nu], "u dim mismatch, actual" + str(tuple(u.shape))
                out = self._chain(x_init, cost, dynamics, u.detach(), s.u_lower.to(device=dev, dtype=dt),
                                  s.u_upper.to(device=dev, dtype=dt))
                if out is not None:
                    self.route = "chain"
                    return out
            self.route = "host"
            return self._host(x_init, cost, dynamics)
