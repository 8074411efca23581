"""`MlpDx` - a learned dynamics model with one or two hidden layers for `BoxDDP` / `MPCstep`:

    n_hidden = H:         next(x, u) = W2 act(W1 [x;u] + b1) + b2 (+ x when residual)
    n_hidden = (H1, H2):  next(x, u) = W3 act(W2 act(W1 [x;u] + b1) + b2) + b3 (+ x when residual)

act = tanh (the default), relu, silu or softplus, the same in both layers.  `MlpDx.from_sequential` takes the weights of a
`torch.nn.Sequential(Linear, act, Linear)` trained elsewhere; the six tensors of a two-layer network are copied into
`W1, b1, W2, b2, W3, b3` by hand.

`forward` is torch code (CPU and GPU tensors).  On the GPU, at a size the kernels serve (nx <= 16, nu <= 8, and H <= 256 or
H1, H2 <= 128), the nominal rollout with its analytic linearisation is one launch (`dmpc_mlp_rollout_linearize`) and `MPCstep`'s line search
evaluates the network inside its kernel (`dmpc_mpc_forward_rec_mlp`); the hooks are the ones `PendulumDx` has (`linearize`,
`fused_ok`, `rollout_linearize`).  The weights go to the library as device pointers on every call: nothing is read back and
nothing is cached, so an optimiser step in place is seen by the next call.

`BoxDDP` drives those kernels from its host loop.  With `device_loop=True` it runs the whole iLQR loop as one chain of launches
instead (`dmpc_box_ddp`, dyn_kind 2: the weights as one packed buffer, `packed_weights`), where the chain serves the problem -
GPU tensors, a supported size, a dense `QuadCost`, no `batch_coupled`; anything else keeps the host loop.

Learning the weights follows mpc/approximate.py:77-119: the Jacobians F_t are constants of the graph, f_t = next - F_t [x;u]
stays on it through `next` and the re-rolled states, and `MPCstep.backward`'s df reaches every weight.  `param_grad` says
where that gradient comes from: "live" (the default) is a live torch rollout on the graph - a Python loop of T - 1 steps;
"device" is ONE autograd node around the rollout's launch whose backward is one sweep kernel and one fixed-order reduction,
`dmpc_mlp_param_grad` with one hidden layer and `dmpc_mlp2_param_grad` (include/dmpc_mlp_grad.h) with two.  `device_grad=True`
is the older spelling of `param_grad="device"` and serves one hidden layer only.  CPU tensors or a size outside the kernels'
limits take the live route whatever the keyword says.

Fitting the network to recorded trajectories: `rollout(x_init, u)` is the multi-step prediction xhat_{t+1} = next(xhat_t, u_t)
and `prediction_loss(x, u, horizon, weight)` its mean squared error against the record over windows of `horizon` steps
(`ClosedLoop`'s `EpisodeOut.x`, `EpisodeOut.u` go in as they are).  In that loss the co-state is NOT zero - it back-propagates
through time.  With `param_grad="device"` `rollout` is one autograd node: forward the rollout's launch, backward
`dmpc_mlp_rollout_grad` (include/dmpc_mlp_rollout_grad.h), one reverse-sweep kernel that carries the co-state and the weight
gradient's fixed-order reduction, with gradients to every weight, x_init and u.  "live" (the default) is the torch loop."""
import math

import torch
import torch.nn.functional as F_nn
from torch.autograd.function import once_differentiable

from . import _lib
from .lqr_recursion import _workspace
from .util import bmv

ACT_TANH = 0     # the `act` argument of the C ABI (1 is never assigned)
ACT_RELU = 2
ACT_SILU = 3
ACT_SOFTPLUS = 4
ACTIVATIONS = {"tanh": ACT_TANH, "relu": ACT_RELU, "silu": ACT_SILU, "softplus": ACT_SOFTPLUS}

# name -> (a(z), da/dz(z)); relu'(0) = 0 as torch has it; softplus' = sigmoid everywhere, as the kernels (torch's own is 1
# beyond its threshold of 20, 2.1e-9 away)
_ACT_FN = {
    "tanh": (torch.tanh, lambda z: 1.0 - torch.tanh(z) ** 2),
    "relu": (torch.relu, lambda z: (z > 0).to(z.dtype)),
    "silu": (F_nn.silu, lambda z: torch.sigmoid(z) * (1.0 + z * (1.0 - torch.sigmoid(z)))),
    "softplus": (F_nn.softplus, torch.sigmoid),
}
PARAM_GRADS = ("live", "device")      # `param_grad`: where the weight gradient of `linearize`'s f comes from
_ACT_OF_MODULE = {torch.nn.Tanh: "tanh", torch.nn.ReLU: "relu", torch.nn.SiLU: "silu", torch.nn.Softplus: "softplus"}


class MlpDx(torch.nn.Module):
    # `search_linearizes` of dmpc_box_ddp's dyn_kind 2 as `BoxDDP` passes it: both settings return the same bits, and 0 measured
    # no slower at either size of DESIGN.md 3.10 (the chain is bound by its kernels, not by its launches)
    SEARCH_LINEARIZES = False

    def __init__(self, n_state, n_ctrl, n_hidden, residual=True, seed=None, device_grad=False, activation="tanh",
                 device_loop=False, param_grad="live"):
        super().__init__()
        if activation not in ACTIVATIONS:
            raise ValueError("MlpDx: unknown activation %r (one of %s)" % (activation, ", ".join(ACTIVATIONS)))
        if param_grad not in PARAM_GRADS:
            raise ValueError("MlpDx: param_grad is \"live\" or \"device\", found %r" % (param_grad,))
        self.activation = activation
        # `device_grad`: the one-layer spelling of param_grad="device" from before the keyword existed; it implies it
        self.param_grad = "device" if device_grad else param_grad
        # BoxDDP runs its iLQR loop as one chain of launches (`dmpc_box_ddp`, dyn_kind 2) where the chain serves the problem
        self.device_loop = bool(device_loop)
        self._packed = {}           # device -> the flat weight buffer of `packed_weights` (no parameter, no buffer, not pickled)
        self.n_state, self.n_ctrl = int(n_state), int(n_ctrl)
        # `hidden`: the widths as a tuple of one or two; `n_hidden` is what the caller gave - an int, or the pair
        if isinstance(n_hidden, (tuple, list)):
            if len(n_hidden) != 2:
                raise ValueError("MlpDx: n_hidden is an int or a pair (H1, H2), found %r" % (n_hidden,))
            self.hidden = (int(n_hidden[0]), int(n_hidden[1]))
            self.n_hidden = self.hidden
        else:
            self.n_hidden = int(n_hidden)
            self.hidden = (self.n_hidden,)
        if min(self.hidden) < 1:
            raise ValueError("MlpDx: every hidden layer needs at least one unit, found %r" % (n_hidden,))
        if self.depth == 2 and device_grad:
            raise ValueError("MlpDx: device_grad=True serves one hidden layer only (dmpc_mlp_param_grad); for a model with two "
                             "pass param_grad=\"device\" (dmpc_mlp2_param_grad)")
        self.residual = bool(residual)
        ns = self.n_state + self.n_ctrl
        gen = None if seed is None else torch.Generator().manual_seed(int(seed))
        H1, out = self.hidden[0], self.n_state
        self.W1 = torch.nn.Parameter(0.5 * torch.randn(H1, ns, generator=gen) / math.sqrt(ns))
        self.b1 = torch.nn.Parameter(torch.zeros(H1))
        if self.depth == 2:
            H2 = self.hidden[1]
            self.W2 = torch.nn.Parameter(torch.randn(H2, H1, generator=gen) / math.sqrt(H1))
            self.b2 = torch.nn.Parameter(torch.zeros(H2))
            self.W3 = torch.nn.Parameter(0.5 * torch.randn(out, H2, generator=gen) / math.sqrt(H2))
            self.b3 = torch.nn.Parameter(torch.zeros(out))
        else:
            self.W2 = torch.nn.Parameter(0.5 * torch.randn(out, H1, generator=gen) / math.sqrt(H1))
            self.b2 = torch.nn.Parameter(torch.zeros(out))
        self._size_ok = None

    @property
    def depth(self):
        """the number of hidden layers, 1 or 2"""
        return len(self.hidden)

    @property
    def device_grad(self):
        """`param_grad == "device"` of a model with one hidden layer, under the name it had before `param_grad` existed;
        assigning to it assigns `param_grad`"""
        return self.depth == 1 and self.param_grad == "device"

    @device_grad.setter
    def device_grad(self, value):
        if value and self.depth == 2:
            raise ValueError("MlpDx: device_grad serves one hidden layer only; for a model with two set param_grad = \"device\"")
        self.param_grad = "device" if value else "live"

    @property
    def hidden_code(self):
        """the `n_hidden` argument of the C ABI: H, or DMPC_MLP_HIDDEN2(H1, H2)"""
        return self.hidden[0] if self.depth == 1 else _lib.mlp_hidden2(*self.hidden)

    @classmethod
    def from_sequential(cls, net, n_state, n_ctrl, residual=True, device_grad=False, device_loop=False, param_grad="live"):
        """the model of a trained `torch.nn.Sequential(Linear(n_state + n_ctrl, H), act, Linear(H, n_state))` whose input is
        [x;u], act one of Tanh, ReLU, SiLU, Softplus (beta = 1, threshold = 20).  The four tensors are copied; anything else is
        a ValueError that names what was found - a deeper network too: for two hidden layers construct
        `MlpDx(n_state, n_ctrl, (H1, H2), activation=...)` and copy the six tensors into W1, b1, W2, b2, W3, b3."""
        n_state, n_ctrl = int(n_state), int(n_ctrl)
        found = "Sequential(%s)" % ", ".join(repr(m) for m in net) if isinstance(net, torch.nn.Sequential) else repr(net)
        if not isinstance(net, torch.nn.Sequential) or len(net) != 3:
            raise ValueError("MlpDx.from_sequential: want Sequential(Linear, activation, Linear), found " + found)
        l1, act, l2 = net
        if not isinstance(l1, torch.nn.Linear) or not isinstance(l2, torch.nn.Linear):
            raise ValueError("MlpDx.from_sequential: want Sequential(Linear, activation, Linear), found " + found)
        if l1.bias is None or l2.bias is None:
            raise ValueError("MlpDx.from_sequential: both Linear layers need a bias, found " + found)
        name = _ACT_OF_MODULE.get(type(act))
        if name is None:
            raise ValueError("MlpDx.from_sequential: activation must be Tanh, ReLU, SiLU or Softplus, found %r" % (act,))
        if name == "softplus" and (act.beta != 1 or act.threshold != 20):
            raise ValueError("MlpDx.from_sequential: Softplus must have beta=1, threshold=20, found %r" % (act,))
        if l1.in_features != n_state + n_ctrl or l2.out_features != n_state or l2.in_features != l1.out_features:
            raise ValueError("MlpDx.from_sequential: want Linear(%d, H) and Linear(H, %d), found %s"
                             % (n_state + n_ctrl, n_state, found))
        m = cls(n_state, n_ctrl, l1.out_features, residual=residual, device_grad=device_grad, activation=name,
                device_loop=device_loop, param_grad=param_grad)
        with torch.no_grad():
            for p, q in zip(m._weights(), (l1.weight, l1.bias, l2.weight, l2.bias)):
                p.copy_(q.detach())
        return m.to(device=l1.weight.device, dtype=l1.weight.dtype)

    def extra_repr(self):
        return "n_state=%d, n_ctrl=%d, n_hidden=%s, residual=%s, activation=%s, device_grad=%s%s%s" % (
            self.n_state, self.n_ctrl, self.n_hidden, self.residual, self.activation, self.device_grad,
            ", device_loop=True" if self.device_loop else "",
            ", param_grad=%s" % self.param_grad if self.param_grad != "live" else "")

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_packed"] = {}       # a copy or an unpickled model packs into a buffer of its own
        return state

    def __setstate__(self, state):
        if "param_grad" not in state:       # pickled before the keyword existed: `device_grad` was a plain attribute
            state["param_grad"] = "device" if state.pop("device_grad", False) else "live"
        super().__setstate__(state)

    @property
    def act_code(self):
        """the `act` argument of the C ABI"""
        return ACTIVATIONS[self.activation]

    def _weights(self):
        """the parameters layer by layer: (W1, b1, W2, b2) or (W1, b1, W2, b2, W3, b3)"""
        if self.depth == 2:
            return self.W1, self.b1, self.W2, self.b2, self.W3, self.b3
        return self.W1, self.b1, self.W2, self.b2

    def _pre(self, x, u):
        """z = W1 [x;u] + b1"""
        return torch.cat((x, u), dim=-1) @ self.W1.to(x).t() + self.b1.to(x)

    def _step(self, x, u):
        """(next state, pre-activations of every hidden layer)"""
        act = _ACT_FN[self.activation][0]
        zs = (self._pre(x, u),)
        if self.depth == 2:
            zs = zs + (act(zs[0]) @ self.W2.to(x).t() + self.b2.to(x),)
        return self._output(act(zs[-1]), x), zs

    def _output(self, a, x):
        """the last layer on the last hidden layer's activations"""
        W, b = self._weights()[-2:]
        nxt = a @ W.to(x).t() + b.to(x)
        return nxt + x if self.residual else nxt

    def forward(self, x, u):
        """x [B,nx] (or [nx]), u [B,nu] (or [nu]) -> next state"""
        assert x.shape[-1] == self.n_state and u.shape[-1] == self.n_ctrl and x.shape[:-1] == u.shape[:-1]
        return self._step(x, u)[0]

    def _jacobian(self, *zs):
        """d next / d [x;u] at the pre-activations z [B,H] of every hidden layer -> [B,nx,ns], a constant of the graph:
        W2 diag(act'(z)) W1, or W3 diag(act'(z2)) W2 diag(act'(z1)) W1, plus [I|0] when residual"""
        dact = _ACT_FN[self.activation][1]
        zs = [z.detach() for z in zs]
        z = zs[0]
        if self.depth == 2:
            F = torch.einsum("ik,bk,kh,bh,hj->bij", self.W3.detach().to(z), dact(zs[1]), self.W2.detach().to(z), dact(z),
                             self.W1.detach().to(z))
        else:
            F = torch.einsum("ih,bh,hj->bij", self.W2.detach().to(z), dact(z), self.W1.detach().to(z))
        if self.residual:
            F = F + torch.eye(self.n_state, self.n_state + self.n_ctrl, dtype=z.dtype, device=z.device)
        return F

    # ------------------------------------------------------------------ the device path
    def supported(self):
        """the kernels serve this size (asked of the library once; nothing is launched)"""
        if self._size_ok is None:
            self._size_ok = bool(_lib.load().dmpc_mlp_dx_supported(self.n_state, self.n_ctrl, self.hidden_code, self.act_code))
        return self._size_ok

    def _on_device(self, x_init, u):
        return isinstance(x_init, torch.Tensor) and isinstance(u, torch.Tensor) and x_init.is_cuda and u.is_cuda and \
            self.supported()

    def _grad_wanted(self, *tensors):
        return torch.is_grad_enabled() and (any(p.requires_grad for p in self._weights()) or
                                            any(t.requires_grad for t in tensors))

    def fused_ok(self, x_init, u):
        """the one-launch rollout + linearisation applies: GPU tensors, a supported size, no gradient wanted now"""
        return self._on_device(x_init, u) and not self._grad_wanted(x_init, u)

    def device_weights(self, device):
        """(W1, b1, W2, b2) as the kernels take them - contiguous float32 on `device`; made on every call, never kept.  Two
        hidden layers: the last two are "the layers behind the first, one after the other", [W2 | W3] and [b2 | b3], one
        `torch.cat` each."""
        w = [_lib.f32c(p.detach(), device) for p in self._weights()]
        if self.depth == 2:
            return w[0], w[1], torch.cat((w[2].reshape(-1), w[4].reshape(-1))), torch.cat((w[3], w[5]))
        return tuple(w)

    def _packed_order(self):
        """the parameters in the order of `packed_weights`"""
        if self.depth == 2:
            return self.W1, self.b1, self.W2, self.W3, self.b2, self.b3
        return self._weights()

    def packed_weights(self, device):
        """[W1 | b1 | W2 | b2] - with two hidden layers [W1 | b1 | W2 | W3 | b2 | b3], so that the tails behind b1 are what
        `device_weights` passes - as ONE flat float32 buffer on `device`, the `F` of `dmpc_box_ddp`'s dyn_kind 2.  The buffer is
        kept per device and refilled in place by one launch on every call: its address is stable (a recorded hipGraph keeps
        reading it) and an optimiser step in place is seen by the next solve - call this before every launch or replay."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        parts = [p.detach().reshape(-1) for p in self._packed_order()]
        if any(p.dtype != torch.float32 or p.device != device for p in parts):
            parts = [p.to(device=device, dtype=torch.float32) for p in parts]
        buf = self._packed.get(device)
        if buf is None or buf.numel() != sum(p.numel() for p in parts):
            buf = self._packed[device] = torch.empty(sum(p.numel() for p in parts), dtype=torch.float32, device=device)
        torch.cat(parts, out=buf)
        return buf

    def host_params(self):
        """dyn_params of `dmpc_box_ddp`'s dyn_kind 2: (n_hidden, act, residual, search_linearizes) as floats, n_hidden the
        code of `hidden_code` (exact in float32)"""
        return (float(self.hidden_code), float(self.act_code), 1.0 if self.residual else 0.0,
                1.0 if self.SEARCH_LINEARIZES else 0.0)

    def rollout_linearize(self, x_init, u, want_model=True):
        """(x [T,B,nx], F [T-1,B,nx,ns], f [T-1,B,nx]) from x_init [B,nx], u [T,B,nu] in one kernel launch
        (`dmpc_mlp_rollout_linearize`): get_traj + linearize_dynamics of the reference's BoxDDP loop.  F = f = None without
        want_model.  CPU tensors or a size outside the kernels' limits: the same results from torch."""
        T, B = u.shape[0], u.shape[1]
        nx, nu = self.n_state, self.n_ctrl
        if not self._on_device(x_init, u):
            with torch.no_grad():
                return self._rollout_linearize_torch(x_init.detach(), u.detach(), want_model)
        lib = _lib.load()
        d = x_init.device
        x0, ud = _lib.f32c(x_init.detach(), d), _lib.f32c(u.detach(), d)
        assert list(x0.shape) == [B, nx] and list(ud.shape) == [T, B, nu]
        W1, b1, W2, b2 = self.device_weights(d)
        x = torch.empty((T, B, nx), dtype=torch.float32, device=d)
        F = torch.empty((max(T - 1, 0), B, nx, nx + nu), dtype=torch.float32, device=d) if want_model else None
        f = torch.empty((max(T - 1, 0), B, nx), dtype=torch.float32, device=d) if want_model else None
        with _lib.guard(d):
            rc = lib.dmpc_mlp_rollout_linearize(T, B, nx, nu, self.hidden_code, self.act_code, int(self.residual), _lib.ptr(W1),
                                                _lib.ptr(b1), _lib.ptr(W2), _lib.ptr(b2), _lib.ptr(x0), _lib.ptr(ud),
                                                _lib.ptr(x), _lib.ptr(F), _lib.ptr(f), _lib.stream_ptr(d))
        _lib.check(rc, "dmpc_mlp_rollout_linearize")
        return x.to(x_init.dtype), (None if F is None else F.to(x_init.dtype)), (None if f is None else f.to(x_init.dtype))

    def _rollout_linearize_torch(self, x_init, u, want_model):
        T = u.shape[0]
        xs, Fs, fs = [x_init], [], []
        for t in range(T - 1):
            nxt, zs = self._step(xs[t], u[t])
            if want_model:
                Fs.append(self._jacobian(*zs))
                fs.append(nxt - bmv(Fs[t], torch.cat((xs[t], u[t]), dim=1)))
            xs.append(nxt)
        x = torch.stack(xs, 0)
        if not want_model:
            return x, None, None
        if T == 1:
            return x, x.new_zeros((0,) + tuple(x_init.shape) + (self.n_state + self.n_ctrl,)), x.new_zeros((0,) + tuple(x_init.shape))
        return x, torch.stack(Fs, 0), torch.stack(fs, 0)

    def linearize(self, x, u):
        """F_t = d next / d [x;u], f_t = next - F_t [x_t;u_t] along the trajectory re-rolled from x[0] (the contract of
        `PendulumDx.linearize`).  No gradient wanted: all of it from the kernel.  Otherwise F still comes from the kernel on
        the GPU, next and the re-rolled states from a live torch rollout - or, with `param_grad="device"`, f too comes from
        the kernel and its gradient from `dmpc_mlp_param_grad` / `dmpc_mlp2_param_grad`."""
        T = x.shape[0]
        x0 = x[0]
        if self.fused_ok(x0, u):
            _, F, f = self.rollout_linearize(x0, u)
            return F, f
        if not self._grad_wanted(x0, u):
            _, F, f = self._rollout_linearize_torch(x0, u, True)
            return F, f
        if self.param_grad == "device" and self._on_device(x0, u):
            return _DeviceLinearize.apply(self, x0, u, *self._weights())
        F_dev = None
        if self._on_device(x0, u):
            F_dev = self.rollout_linearize(x0, u)[1]
        xs, Fs, fs = [x0], [], []
        for t in range(T - 1):
            xt, ut = xs[t], u[t]
            nxt, zs = self._step(xt, ut)
            Ft = F_dev[t] if F_dev is not None else self._jacobian(*zs)
            Fs.append(Ft)
            fs.append(nxt - bmv(Ft, torch.cat((xt, ut), dim=1)))
            xs.append(nxt)
        if T == 1:
            _, F, f = self._rollout_linearize_torch(x0.detach(), u.detach(), True)
            return F, f
        return torch.stack(Fs, 0), torch.stack(fs, 0)

    # ------------------------------------------------------------------ fitting the network to trajectories
    def rollout(self, x_init, u, T=None):
        """x [T,B,nx] with x[0] = x_init [B,nx], x[t+1] = next(x[t], u[t]).  `u` [T,B,nu] or [T-1,B,nu]: its row T-1 is never
        read; T = u.shape[0] unless given (then u has T or T - 1 rows).  Three routes:
          no gradient wanted                      the one-launch rollout, `rollout_linearize(x_init, u, want_model=False)[0]`
          a gradient wanted, param_grad="device",
          GPU tensors, a supported size           ONE autograd node: forward that same launch - the states are bit-equal to what
                                                  the solver's rollout sees - backward `dmpc_mlp_rollout_grad`, one reverse sweep
                                                  that carries the co-state; gradients reach the weights, x_init and u
          otherwise                               the torch loop over `_step`, autograd through every step"""
        T = u.shape[0] if T is None else int(T)
        if T < 1 or u.shape[0] not in (T, T - 1):
            raise ValueError("MlpDx.rollout: u has %d rows, want T = %d or T - 1" % (u.shape[0], T))
        assert x_init.shape[-1] == self.n_state and u.shape[-1] == self.n_ctrl and tuple(u.shape[1:-1]) == tuple(x_init.shape[:-1])
        if not self._grad_wanted(x_init, u):
            return self.rollout_linearize(x_init, _rows(u, T), want_model=False)[0]
        if self.param_grad == "device" and self._on_device(x_init, u):
            return _DeviceRollout.apply(self, T, x_init, u, *self._weights())
        xs = [x_init]
        for t in range(T - 1):
            xs.append(self._step(xs[t], u[t])[0])
        return torch.stack(xs, 0)

    def prediction_loss(self, x, u, horizon=None, weight=None):
        """Multi-step prediction error along recorded trajectories x [T,B,nx], u [T,B,nu] or [T-1,B,nu] (`EpisodeOut.x` and
        `EpisodeOut.u` as they are): the mean of weight_i (xhat - x)_i^2 over windows, steps >= 1 and components i, xhat rolled
        from the record's state at the window's start under the record's controls.
          horizon=None   one window from x[0] over the whole record
          horizon=h      1 <= h <= T - 1: a window from every t = 0 .. T-1-h, each rolled h steps; h = 1 is one-step teacher forcing
        The windows are folded into the batch axis start-major (row start * B + b) and go through `rollout` as one batch: with
        param_grad="device" the network runs in one launch forward and two backward, whatever T and h; the rest is plain torch.
        `weight` [nx] or None."""
        T = x.shape[0]
        if x.dim() != 3 or u.dim() != 3 or u.shape[0] not in (T, T - 1):
            raise ValueError("MlpDx.prediction_loss: x [T,B,nx] and u [T,B,nu] or [T-1,B,nu], found %s and %s"
                             % (tuple(x.shape), tuple(u.shape)))
        h = T - 1 if horizon is None else int(horizon)
        if h < 1 or h > T - 1:
            raise ValueError("MlpDx.prediction_loss: horizon must be in 1 .. T - 1 = %d, found %r" % (T - 1, horizon))
        n_w, B = T - h, x.shape[1]
        x0 = x[:n_w].reshape(n_w * B, self.n_state)
        uw = torch.stack([u[s:s + n_w] for s in range(h)], 0).reshape(h, n_w * B, self.n_ctrl)
        target = torch.stack([x[s:s + n_w] for s in range(1, h + 1)], 0).reshape(h, n_w * B, self.n_state)
        err = (self.rollout(x0, uw, T=h + 1)[1:] - target) ** 2
        if weight is not None:
            err = err * torch.as_tensor(weight, dtype=err.dtype, device=err.device)
        return err.mean()


def _rows(u, T):
    """u with T rows: a zero row behind one that has T - 1 (the row is never read)"""
    return u if u.shape[0] == T else torch.cat((u, u.new_zeros((1,) + tuple(u.shape[1:]))), 0)


def _packed_grads(depth, w):
    """(args, outs, split) for the gradient entry points: the weights `w` as they take them - two hidden layers: [W2 | W3] and
    [b2 | b3] - empty outputs of those shapes, and views of the outputs in the order and shapes of `w`"""
    if depth == 2:
        args = [w[0], w[1], torch.cat((w[2].reshape(-1), w[4].reshape(-1))), torch.cat((w[3], w[5]))]
        outs = [torch.empty_like(a) for a in args]
        split = [outs[0], outs[1], outs[2][:w[2].numel()].view(w[2].shape), outs[3][:w[3].numel()],
                 outs[2][w[2].numel():].view(w[4].shape), outs[3][w[3].numel():]]
        return args, outs, split
    outs = [torch.empty_like(a) for a in w]
    return w, outs, outs


class _DeviceLinearize(torch.autograd.Function):
    """(F, f) of `MlpDx.linearize` as ONE node over (x[0], u, W1, b1, W2, b2[, W3, b3]): forward is the rollout's launch,
    backward `dmpc_mlp_param_grad` or, with two hidden layers, `dmpc_mlp2_param_grad`.  F is a constant of the graph.  The
    weights are saved as autograd saves any input, so one changed in place before the backward is autograd's version error,
    not a gradient at other weights than the forward's."""

    @staticmethod
    def forward(ctx, model, x0, u, *weights):
        x, F, f = model.rollout_linearize(x0, u)
        ctx.model = model
        ctx.save_for_backward(x, u, *weights)
        ctx.mark_non_differentiable(F)
        return F, f

    @staticmethod
    @once_differentiable
    def backward(ctx, _grad_F, grad_f):
        m = ctx.model
        x, u, *weights = ctx.saved_tensors
        T, B = u.shape[0], u.shape[1]
        nx, nu = m.n_state, m.n_ctrl
        lib = _lib.load()
        d = u.device
        w = [_lib.f32c(p.detach(), d) for p in weights]
        xs, ud, g = _lib.f32c(x, d), _lib.f32c(u.detach(), d), _lib.f32c(grad_f, d)
        assert list(xs.shape) == [T, B, nx] and list(g.shape) == [max(T - 1, 0), B, nx]
        f32 = dict(dtype=torch.float32, device=d)
        if m.depth == 2:
            entry, query = "dmpc_mlp2_param_grad", lib.dmpc_mlp2_param_grad_workspace_bytes
        else:
            entry, query = "dmpc_mlp_param_grad", lib.dmpc_mlp_param_grad_workspace_bytes
        args, outs, split = _packed_grads(m.depth, w)
        dx0 = torch.empty((B, nx), **f32) if ctx.needs_input_grad[1] else None
        du = torch.empty((T, B, nu), **f32) if ctx.needs_input_grad[2] else None
        nbytes = query(B, nx, nu, m.hidden_code)
        ws = _workspace(nbytes, d)
        with _lib.guard(d):
            rc = getattr(lib, entry)(T, B, nx, nu, m.hidden_code, m.act_code, int(m.residual), *(_lib.ptr(a) for a in args),
                                     _lib.ptr(xs), _lib.ptr(ud), _lib.ptr(g), *(_lib.ptr(o) for o in outs), _lib.ptr(dx0),
                                     _lib.ptr(du), _lib.ptr(ws), nbytes, _lib.stream_ptr(d))
        _lib.check(rc, entry)
        grads = [gr.to(p.dtype) if need else None for gr, p, need in zip(split, weights, ctx.needs_input_grad[3:])]
        return (None, None if dx0 is None else dx0.to(grad_f.dtype), None if du is None else du.to(u.dtype), *grads)


class _DeviceRollout(torch.autograd.Function):
    """x of `MlpDx.rollout` as ONE node over (x_init, u, W1, b1, W2, b2[, W3, b3]): forward is the rollout's launch without its
    Jacobians, backward `dmpc_mlp_rollout_grad` (include/dmpc_mlp_rollout_grad.h) on the states that launch stored.  The weights
    are saved as autograd saves any input, so one changed in place before the backward is autograd's version error."""

    @staticmethod
    def forward(ctx, model, T, x_init, u, *weights):
        x = model.rollout_linearize(x_init, _rows(u, T), want_model=False)[0]
        ctx.model = model
        ctx.save_for_backward(x, u, *weights)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_x):
        m = ctx.model
        x, u, *weights = ctx.saved_tensors
        T, B = x.shape[0], x.shape[1]
        nx, nu = m.n_state, m.n_ctrl
        lib = _lib.load()
        d = x.device
        w = [_lib.f32c(p.detach(), d) for p in weights]
        xs, ud, g = _lib.f32c(x, d), _lib.f32c(_rows(u.detach(), T), d), _lib.f32c(grad_x, d)
        assert list(xs.shape) == [T, B, nx] and list(ud.shape) == [T, B, nu] and list(g.shape) == [T, B, nx]
        f32 = dict(dtype=torch.float32, device=d)
        args, outs, split = _packed_grads(m.depth, w)
        dx0 = torch.empty((B, nx), **f32) if ctx.needs_input_grad[2] else None
        du = torch.empty((T, B, nu), **f32) if ctx.needs_input_grad[3] else None
        nbytes = lib.dmpc_mlp_rollout_grad_workspace_bytes(B, nx, nu, m.hidden_code)
        ws = _workspace(nbytes, d)
        with _lib.guard(d):
            rc = lib.dmpc_mlp_rollout_grad(T, B, nx, nu, m.hidden_code, m.act_code, int(m.residual), *(_lib.ptr(a) for a in args),
                                           _lib.ptr(xs), _lib.ptr(ud), _lib.ptr(g), *(_lib.ptr(o) for o in outs), _lib.ptr(dx0),
                                           _lib.ptr(du), _lib.ptr(ws), nbytes, _lib.stream_ptr(d))
        _lib.check(rc, "dmpc_mlp_rollout_grad")
        grads = [gr.to(p.dtype) if need else None for gr, p, need in zip(split, weights, ctx.needs_input_grad[4:])]
        return (None, None, None if dx0 is None else dx0.to(grad_x.dtype), None if du is None else du[:u.shape[0]].to(u.dtype), *grads)
