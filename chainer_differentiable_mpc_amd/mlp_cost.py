"""`MlpCost` - a learned, stationary, non-quadratic stage cost for `BoxDDP` / `MPCstep`, the cost-side counterpart of `MlpDx`:

    c(tau) = 1/2 tau' Q tau + p' tau + w2' act(W1 tau + b1),      tau = [x;u]
    Q [ns,ns]   p [ns]   W1 [H,ns]   b1 [H]   w2 [H]              act = tanh, relu, silu or softplus (`MlpDx`'s codes)

The same cost at every timestep, as the reference's `Cf(tau_t)` is (mpc/box_ddp.py:133-136).  `Q` is used as given and is not
symmetrised; the quadratic part of the Hessian is Qs = (Q + Q')/2.  `forward` is torch code (CPU and GPU tensors), so the module
is a valid callable cost on every route that takes one.  On the GPU, at a size the kernels serve (nx <= 16, nu <= 8, H <= 256):

  * `approximate_cost` gets its Taylor model from ONE launch (`dmpc_mlp_cost_approx`, include/dmpc_mlp_cost.h) instead of
    T (1 + ns) autograd calls: H = Qs + W1' diag(w2 act''(z)) W1, g0 = grad - H tau, the values;
  * `MPCstep.forward_rec` with a `LinDx` evaluates the cost inside its line-search kernel (`dmpc_mpc_forward_rec_mlp_cost`); with
    any other dynamics the host search evaluates it by one launch per pass (`stage_costs`);
  * with `param_grad="device"` the Taylor model is ONE autograd node whose backward is one kernel and a fixed-order reduction
    (`dmpc_mlp_cost_param_grad`): gradients reach Q, p, W1, b1, w2; the Hessian is a constant of the graph (approximate.py:75)
    and x, u receive none.  "live" (the default) leaves a call that wants a gradient to `approximate_cost`'s autograd route.

`BoxDDP` drives those kernels from its host loop.  With `device_loop=True` (the last keyword; off by default) it runs the whole
iLQR loop as one chain of launches instead (`dmpc_box_ddp_mlp_cost`), where the chain serves the problem - GPU tensors, a
supported size, a `LinDx` with a dense F, T >= 2, no `batch_coupled` and no verbose output; anything else keeps the host loop.
The chain takes the weights as ONE flat float32 buffer, `packed_weights`:

    [Q (ns*ns) | p (ns) | W1 (H*ns) | b1 (H) | w2 (H)]

kept per device and refilled in place by one launch before every solve and every replay of a recorded one.

The weights go to the library as device pointers on every call: nothing is read back and nothing is cached, so an optimiser step
in place is seen by the next call.  CPU tensors or a size outside the limits take the autograd route whatever the keyword says.

Nothing here enforces convexity: like the reference, the solver uses the Hessian as it comes.  With softplus or relu, `w2 >= 0`
keeps H >= Qs (act'' >= 0), so a positive definite Qs is enough; tanh and silu have act'' of either sign.

`MlpCost.soft_box` builds softplus units for soft state limits - the box of `BoxDDP` covers controls only."""
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .lqr_recursion import _workspace
from .mlp_dx import ACTIVATIONS, PARAM_GRADS, _ACT_FN


class MlpCost(torch.nn.Module):
    """c(tau) = 1/2 tau' Q tau + p' tau + w2' act(W1 tau + b1) (the module's docstring has the routes).

    `device_loop` (the last keyword, default False): `BoxDDP` runs its whole iLQR loop with this cost as one chain of launches
    (`dmpc_box_ddp_mlp_cost`) where that chain serves the problem - GPU tensors, a supported size that is the solver's, a `LinDx`
    with a dense F, T >= 2, no `batch_coupled`, no verbose output; False, or any other problem: the host loop over the kernels.
    The chain reads the weights from `packed_weights(device)`, ONE flat float32 buffer per device in the order

        [Q (ns*ns) | p (ns) | W1 (H*ns) | b1 (H) | w2 (H)]

    refilled in place by one launch on every call, at the same address each time."""

    def __init__(self, n_state, n_ctrl, n_hidden, activation="softplus", Q=None, p=None, seed=None, param_grad="live",
                 device_loop=False):
        super().__init__()
        if activation not in ACTIVATIONS:
            raise ValueError("MlpCost: unknown activation %r (one of %s)" % (activation, ", ".join(ACTIVATIONS)))
        if param_grad not in PARAM_GRADS:
            raise ValueError("MlpCost: param_grad is \"live\" or \"device\", found %r" % (param_grad,))
        self.activation, self.param_grad = activation, param_grad
        self.device_loop = bool(device_loop)
        self._packed = {}           # device -> the flat weight buffer of `packed_weights` (no parameter, no buffer, not pickled)
        self.n_state, self.n_ctrl, self.n_hidden = int(n_state), int(n_ctrl), int(n_hidden)
        if self.n_hidden < 1:
            raise ValueError("MlpCost: the network needs at least one hidden unit, found %r" % (n_hidden,))
        ns, H = self.n_state + self.n_ctrl, self.n_hidden
        Q = torch.eye(ns) if Q is None else torch.as_tensor(Q).detach().clone().to(torch.get_default_dtype())
        p = torch.zeros(ns) if p is None else torch.as_tensor(p).detach().clone().to(torch.get_default_dtype())
        if list(Q.shape) != [ns, ns] or list(p.shape) != [ns]:
            raise ValueError("MlpCost: Q [%d,%d] and p [%d], found %s and %s" % (ns, ns, ns, tuple(Q.shape), tuple(p.shape)))
        gen = None if seed is None else torch.Generator().manual_seed(int(seed))
        self.Q = torch.nn.Parameter(Q)
        self.p = torch.nn.Parameter(p)
        self.W1 = torch.nn.Parameter(torch.randn(H, ns, generator=gen) / math.sqrt(ns))
        self.b1 = torch.nn.Parameter(torch.zeros(H))
        self.w2 = torch.nn.Parameter(torch.randn(H, generator=gen).abs() / math.sqrt(H))
        self._size_ok = None

    @classmethod
    def soft_box(cls, n_state, n_ctrl, x_lower, x_upper, weight=1.0, sharpness=10.0, Q=None, p=None):
        """soft state limits lo <= x <= hi as softplus units, one per FINITE bound, state by state (its upper bound's unit, then
        its lower bound's), with k = sharpness:
            upper bound on state i:  W1 row = k e_i,  b1 = -k hi_i,  w2 = weight / k     -> weight/k softplus(k (x_i - hi_i))
            lower bound on state i:  W1 row = -k e_i, b1 = k lo_i,   w2 = weight / k     -> weight/k softplus(k (lo_i - x_i))
        about weight * max(0, violation), rounded over a width of 1/k.  Infinite bounds make no unit; no finite bound at all is
        a ValueError (a network needs a unit).  Q, p: the quadratic part, as the constructor takes them."""
        n_state, n_ctrl = int(n_state), int(n_ctrl)
        lo = torch.as_tensor(x_lower, dtype=torch.float64).reshape(-1)
        hi = torch.as_tensor(x_upper, dtype=torch.float64).reshape(-1)
        if lo.numel() != n_state or hi.numel() != n_state:
            raise ValueError("MlpCost.soft_box: x_lower and x_upper have one entry per state (%d)" % n_state)
        k, rows, bias = float(sharpness), [], []
        for i in range(n_state):
            for sign, bound in ((1.0, float(hi[i])), (-1.0, float(lo[i]))):
                if math.isfinite(bound):
                    rows.append((i, sign * k))
                    bias.append(-sign * k * bound)
        if not rows:
            raise ValueError("MlpCost.soft_box: no finite bound, hence no unit")
        m = cls(n_state, n_ctrl, len(rows), activation="softplus", Q=Q, p=p)
        with torch.no_grad():
            m.W1.zero_()
            for h, (i, w) in enumerate(rows):
                m.W1[h, i] = w
            m.b1.copy_(torch.tensor(bias, dtype=m.b1.dtype))
            m.w2.fill_(float(weight) / k)
        return m

    def extra_repr(self):
        return "n_state=%d, n_ctrl=%d, n_hidden=%d, activation=%s%s%s" % (
            self.n_state, self.n_ctrl, self.n_hidden, self.activation,
            ", param_grad=%s" % self.param_grad if self.param_grad != "live" else "",
            ", device_loop=True" if self.device_loop else "")

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_packed"] = {}       # a copy or an unpickled model packs into a buffer of its own
        return state

    def __setstate__(self, state):
        state.setdefault("device_loop", False)      # (pickled before the keyword existed)
        state.setdefault("_packed", {})
        super().__setstate__(state)

    @property
    def act_code(self):
        """the `act` argument of the C ABI"""
        return ACTIVATIONS[self.activation]

    def _weights(self):
        return self.Q, self.p, self.W1, self.b1, self.w2

    def forward(self, tau):
        """tau [B,ns] (or [ns]) -> the cost [B] (or a scalar)"""
        assert tau.shape[-1] == self.n_state + self.n_ctrl
        Q, p, W1, b1, w2 = (w.to(tau) for w in self._weights())
        a = _ACT_FN[self.activation][0](tau @ W1.t() + b1)
        return 0.5 * ((tau @ Q.t()) * tau).sum(dim=-1) + tau @ p + a @ w2

    # ------------------------------------------------------------------ the device path
    def supported(self):
        """the kernels serve this size (asked of the library once; nothing is launched)"""
        if self._size_ok is None:
            self._size_ok = bool(_lib.load().dmpc_mlp_cost_supported(self.n_state, self.n_ctrl, self.n_hidden, self.act_code))
        return self._size_ok

    def _on_device(self, x, u):
        return isinstance(x, torch.Tensor) and isinstance(u, torch.Tensor) and x.is_cuda and u.is_cuda and \
            x.shape[-1] == self.n_state and u.shape[-1] == self.n_ctrl and self.supported()

    def _grad_wanted(self, *tensors):
        return torch.is_grad_enabled() and (any(w.requires_grad for w in self._weights()) or
                                            any(t.requires_grad for t in tensors))

    def approx_ok(self, x, u):
        """the one-launch Taylor model applies: GPU tensors, a supported size, and either no gradient wanted now or
        param_grad="device" with neither x nor u on the graph"""
        if not self._on_device(x, u):
            return False
        if not self._grad_wanted(x, u):
            return True
        return self.param_grad == "device" and not (x.requires_grad or u.requires_grad)

    def device_weights(self, device):
        """(Q, p, W1, b1, w2) as the kernels take them - contiguous float32 on `device`; made on every call, never kept"""
        return tuple(_lib.f32c(w.detach(), device) for w in self._weights())

    def packed_weights(self, device):
        """[Q | p | W1 | b1 | w2] as ONE flat float32 buffer on `device`, the `cost_packed` of `dmpc_box_ddp_mlp_cost`.  The buffer
        is kept per device and refilled in place by one launch on every call: its address is stable (a recorded hipGraph keeps
        reading it), its contents are the parameters' of this moment."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        parts = [w.detach().reshape(-1) for w in self._weights()]
        if any(w.dtype != torch.float32 or w.device != device for w in parts):
            parts = [w.to(device=device, dtype=torch.float32) for w in parts]
        buf = self._packed.get(device)
        if buf is None or buf.numel() != sum(w.numel() for w in parts):
            buf = self._packed[device] = torch.empty(sum(w.numel() for w in parts), dtype=torch.float32, device=device)
        torch.cat(parts, out=buf)
        return buf

    def _launch_approx(self, x, u, weights, want_model):
        T, B = x.shape[0], x.shape[1]
        nx, nu, ns = self.n_state, self.n_ctrl, self.n_state + self.n_ctrl
        d = x.device
        xd, ud = _lib.f32c(x.detach(), d), _lib.f32c(u.detach(), d)
        assert list(xd.shape) == [T, B, nx] and list(ud.shape) == [T, B, nu]
        f32 = dict(dtype=torch.float32, device=d)
        H = torch.empty((T, B, ns, ns), **f32) if want_model else None
        g = torch.empty((T, B, ns), **f32) if want_model else None
        costs = torch.empty((T, B), **f32)
        with _lib.guard(d):
            rc = _lib.load().dmpc_mlp_cost_approx(T, B, nx, nu, self.n_hidden, self.act_code, *(_lib.ptr(w) for w in weights),
                                                  _lib.ptr(xd), _lib.ptr(ud), _lib.ptr(H), _lib.ptr(g), _lib.ptr(costs),
                                                  _lib.stream_ptr(d))
        _lib.check(rc, "dmpc_mlp_cost_approx")
        return H, g, costs

    def approximate(self, x, u):
        """(H [T,B,ns,ns], g0 [T,B,ns], costs [T,B]) of `approximate_cost` at x [T,B,nx], u [T,B,nu] in one launch
        (`dmpc_mlp_cost_approx`).  With param_grad="device" and a gradient wanted: one autograd node whose backward is
        `dmpc_mlp_cost_param_grad`; H is a constant of the graph, x and u receive no gradient.  For a call `approx_ok` passes."""
        if not self._on_device(x, u):
            raise _lib.DmpcError("MlpCost.approximate: GPU tensors at a size the kernels serve (`approx_ok`); "
                                 "`approximate_cost` takes the autograd route otherwise")
        if self._grad_wanted(x, u) and self.param_grad == "device":
            return _DeviceApprox.apply(self, x, u, *self._weights())
        H, g, costs = self._launch_approx(x, u, self.device_weights(x.device), True)
        return H.to(x.dtype), g.to(x.dtype), costs.to(x.dtype)

    def stage_costs(self, x, u):
        """the costs [T,B] alone: the same launch with the model outputs left out, bit-equal to `approximate`'s"""
        if not self._on_device(x, u):
            raise _lib.DmpcError("MlpCost.stage_costs: GPU tensors at a size the kernels serve (`approx_ok`)")
        return self._launch_approx(x, u, self.device_weights(x.device), False)[2].to(x.dtype)


class _DeviceApprox(torch.autograd.Function):
    """(H, g0, costs) of `MlpCost.approximate` as ONE node over (Q, p, W1, b1, w2): forward is the Taylor model's launch, backward
    `dmpc_mlp_cost_param_grad`.  H is a constant of the graph; x and u get no gradient.  The weights are saved as autograd saves
    any input, so one changed in place before the backward is autograd's version error."""

    @staticmethod
    def forward(ctx, model, x, u, *weights):
        d = x.device
        H, g, costs = model._launch_approx(x, u, [_lib.f32c(w.detach(), d) for w in weights], True)
        ctx.model = model
        ctx.save_for_backward(x, u, *weights)
        ctx.set_materialize_grads(False)
        H, g, costs = H.to(x.dtype), g.to(x.dtype), costs.to(x.dtype)
        ctx.mark_non_differentiable(H)
        return H, g, costs

    @staticmethod
    @once_differentiable
    def backward(ctx, _grad_H, grad_g, grad_costs):
        if grad_g is None and grad_costs is None:
            return (None,) * 8
        m = ctx.model
        x, u, *weights = ctx.saved_tensors
        T, B = x.shape[0], x.shape[1]
        nx, nu = m.n_state, m.n_ctrl
        lib = _lib.load()
        d = x.device
        w = [_lib.f32c(p.detach(), d) for p in weights]
        xd, ud = _lib.f32c(x.detach(), d), _lib.f32c(u.detach(), d)
        gg = None if grad_g is None else _lib.f32c(grad_g, d)
        gc = None if grad_costs is None else _lib.f32c(grad_costs, d)
        assert gg is None or list(gg.shape) == [T, B, nx + nu]
        assert gc is None or list(gc.shape) == [T, B]
        outs = [torch.empty_like(a) for a in w]
        nbytes = lib.dmpc_mlp_cost_param_grad_workspace_bytes(T, B, nx, nu, m.n_hidden)
        ws = _workspace(nbytes, d)
        with _lib.guard(d):
            rc = lib.dmpc_mlp_cost_param_grad(T, B, nx, nu, m.n_hidden, m.act_code, _lib.ptr(w[2]), _lib.ptr(w[3]), _lib.ptr(w[4]),
                                              _lib.ptr(xd), _lib.ptr(ud), _lib.ptr(gg), _lib.ptr(gc), *(_lib.ptr(o) for o in outs),
                                              _lib.ptr(ws), nbytes, _lib.stream_ptr(d))
        _lib.check(rc, "dmpc_mlp_cost_param_grad")
        grads = [o.to(device=p.device, dtype=p.dtype) if need else None
                 for o, p, need in zip(outs, weights, ctx.needs_input_grad[3:])]
        return (None, None, None, *grads)
