"""Host-side mirror of the reference's util.py on torch tensors.

Names and argument meaning follow /root/reference/util.py: QuadCost/LinDx (:25-32), clamp
(:101-123), get_cost (:126-198), get_traj (:201-277), bmv (:280-298), bger (:301-329), bquad
(:332-358), expand_time_batch / expand_batch (:361-408), bdot (:411-434), batch LU factor/solve
(:462-528).  The tiny batched helpers are plain torch ops (inside the solver kernels they are
device functions); the LU pair calls the HIP library.
"""
from collections import namedtuple

import torch

from . import _lib

QuadCost = namedtuple("QuadCost", "C c", defaults=(None, None))
LinDx = namedtuple("LinDx", "F f", defaults=(None, None))


class TiledQuadCost(QuadCost):
    """A `QuadCost` that is ONE (Q [ns,ns], p [ns]) tiled over time and batch - the imitation loop's learnable cost
    (env_dx/il_env.py:119-129 repeats Q and p to [T,B,ns,ns], [T,B,ns]).  `.C` / `.c` are those dense tensors (what the
    kernels read; constants of the graph), `.Q` / `.p` the tensors a gradient flows to: `BoxDDP` then asks
    `MPCstep.backward` for the gradient already summed over time and batch (formed in the co-state kernel) instead of
    letting autograd reduce dC [T,B,ns,ns] and dc [T,B,ns] afterwards.  Everything that takes a `QuadCost` takes it."""

    def __new__(cls, Q, p, T, n_batch):
        C = Q.detach()[None, None].expand(T, n_batch, -1, -1).contiguous()
        c = p.detach()[None, None].expand(T, n_batch, -1).contiguous()
        self = super().__new__(cls, C, c)
        self.Q, self.p = Q, p
        return self

    @classmethod
    def from_tiles(cls, C, c, Q, p):
        """around tiles the caller already holds (C [T,B,ns,ns], c [T,B,ns] equal to Q, p repeated): no copy, so a solver
        called again sees the same buffers (the imitation driver's device update writes them in place)"""
        self = super().__new__(cls, C, c)
        self.Q, self.p = Q, p
        return self


class TiledLinDx(LinDx):
    """A `LinDx` that is ONE [A|B] tiled over the batch (and over time) - the learnable dynamics of mpc/mpc_net.py, which
    builds its model with `expand_time_batch`.  `.F` / `.f` are the dense, detached, contiguous tiles the forward kernels
    read ([T-1,B,nx,ns], [T-1,B,nx] or None); `.AB` ([nx,ns] or [T-1,nx,ns]) and `.f0` ([nx], [T-1,nx] or None) the tensors
    a gradient flows to: `BoxDDP(update_dynamics=True)` then asks for the gradient already summed over the batch (and time)
    on the device (`mpc_step.tiled_dynamics_gradient`) instead of forming dF [T-1,B,nx,ns] and leaving the sum to autograd's
    backward of the tiling.  Everything that takes a `LinDx` takes it."""

    def __new__(cls, AB, f, T, n_batch):
        F = cls.tile(AB.detach(), 2, T, n_batch).contiguous()
        ft = None if f is None else cls.tile(f.detach(), 1, T, n_batch).contiguous()
        return cls.from_tiles(F, ft, AB, f)

    @classmethod
    def from_tiles(cls, F, f, AB, f0):
        """around tiles the caller already holds (F [T-1,B,nx,ns], f [T-1,B,nx] or None, equal to AB, f0 repeated): no copy,
        so a solver called again sees the same buffers (`MpcNet_dx(shared=True)` refreshes them in place)"""
        self = super().__new__(cls, F, f)
        self.AB, self.f0 = AB, f0
        return self

    @staticmethod
    def tile(m, base_dim, T, n_batch):
        """m without a time axis (m.dim() == base_dim) or with one -> the view [T-1, n_batch, ...] (on m's graph)"""
        assert m.dim() in (base_dim, base_dim + 1), "a tiled model is [...] or [T-1, ...]"
        if m.dim() == base_dim:
            return expand_time_batch(m, T - 1, n_batch)
        assert m.shape[0] == T - 1, "a tiled model with a time axis has T-1 slices"
        return m.unsqueeze(1).expand((T - 1, n_batch) + tuple(m.shape[1:]))


def bmv(a, x):
    assert a.shape[0] == x.shape[0], "batch mismatch"
    assert a.shape[2] == x.shape[1], "mat mul dim mismatch"
    assert x.dim() == 2, " x is not batch vector"
    return torch.matmul(a, x.unsqueeze(2)).squeeze(2)


def bger(x, y):
    return x.unsqueeze(2) @ y.unsqueeze(1)


def bquad(x, Q):
    assert x.shape[0] == Q.shape[0], "batch mismatch"
    assert x.shape[1] == Q.shape[1], "mat mul dim mismatch"
    assert Q.shape[2] == Q.shape[1], "Q is not square matrix"
    return (x.unsqueeze(1) @ Q @ x.unsqueeze(2)).squeeze(1).squeeze(1)


def bdot(x, y):
    assert x.shape == y.shape
    return (x.unsqueeze(1) @ y.unsqueeze(2)).squeeze(1).squeeze(1)


def clamp(x, lower, upper):
    assert x.shape == lower.shape
    assert x.shape == upper.shape
    assert bool((lower <= upper).all()), " lower is larger than upper"
    return torch.minimum(torch.maximum(x, lower), upper)


def expand_time_batch(m, time, n_batch):
    return m.unsqueeze(0).unsqueeze(0).expand((time, n_batch) + tuple(m.shape))


def expand_batch(m, n_batch):
    return m.unsqueeze(0).expand((n_batch,) + tuple(m.shape))


def get_traj(T, u, x_init, dynamics):
    """roll a control sequence out; dynamics is a LinDx or a callable (x, u) -> x'"""
    xs = [x_init]
    for t in range(T - 1):
        if isinstance(dynamics, LinDx):
            xu = torch.cat((xs[t], u[t]), dim=1)
            nx = bmv(dynamics.F[t], xu)
            if dynamics.f is not None:
                nx = nx + dynamics.f[t]
        else:
            nx = dynamics(xs[t], u[t])
        xs.append(nx)
    return torch.stack(xs, dim=0)


def get_cost(T, u, cost, dynamics=None, x_init=None, x=None):
    """sum_t 1/2 tau' C_t tau + c_t' tau (QuadCost) or sum_t cost(tau) -> [B]"""
    assert x_init is not None or x is not None
    if x is None:
        x = get_traj(T, u, x_init, dynamics)
    tau = torch.cat((x, u), dim=2)
    if isinstance(cost, QuadCost):
        quad = torch.einsum("tbi,tbij,tbj->b", tau, cost.C, tau)
        return 0.5 * quad + (tau * cost.c).sum(dim=(0, 2))
    return torch.stack([cost(tau[t]) for t in range(T)], dim=0).sum(dim=0)


def batch_lu_factor(A):
    """[B,n,n] -> (LU [B,n,n], pivots [B,n] int32, 1-based) - LAPACK getrf layout (util.py:462-482)"""
    assert A.dim() == 3 and A.shape[1] == A.shape[2], "Actual" + str(tuple(A.shape))
    _lib.require_gpu()
    lib = _lib.load()
    dev = A.device if A.is_cuda else torch.device("cuda", torch.cuda.current_device())
    a = _lib.f32c(A, dev)
    B, n, _ = a.shape
    LU = torch.empty_like(a)
    piv = torch.empty((B, n), dtype=torch.int32, device=dev)
    with _lib.guard(dev):
        _lib.check(lib.dmpc_batch_lu_factor(B, n, _lib.ptr(a), _lib.ptr(LU), _lib.ptr(piv), None,
                                            _lib.stream_ptr(dev)), "dmpc_batch_lu_factor")
    return LU.to(A.device), piv.to(A.device)


def batch_lu_solve(lu_and_piv, b):
    """float32 solve; b is [B,n] or [B,n,k] (util.py:505-528)"""
    LU, piv = lu_and_piv
    _lib.require_gpu()
    lib = _lib.load()
    dev = LU.device if LU.is_cuda else torch.device("cuda", torch.cuda.current_device())
    lu = _lib.f32c(LU, dev)
    pv = piv.to(device=dev, dtype=torch.int32).contiguous()
    vec = b.dim() == 2
    rhs = _lib.f32c(b.unsqueeze(2) if vec else b, dev)
    B, n, k = rhs.shape
    x = torch.empty_like(rhs)
    with _lib.guard(dev):
        _lib.check(lib.dmpc_batch_lu_solve(B, n, k, _lib.ptr(lu), _lib.ptr(pv), _lib.ptr(rhs), _lib.ptr(x),
                                           _lib.stream_ptr(dev)), "dmpc_batch_lu_solve")
    x = x.squeeze(2) if vec else x
    return x.to(b.device)
