"""LQR with batch-shared C and F: shape classification, and the raw device calls behind
`dmpc_lqr_shared_solve` / `dmpc_lqr_shared_kkt_grad` (include/dmpc.h).

Accepted shapes, next to today's full ones (C [T,B,ns,ns], c [T,B,ns], F [T-1 or T,B,nx,ns], f None or [T-1,B,nx]):
  C [ns,ns] or [T,ns,ns];  F [nx,ns] or [T-1 (or T),nx,ns];  c [ns] or [T,ns];  f [nx] or [T-1,nx].
`classify` decides which code runs:
  "full"   - every input has today's shape: today's code, untouched (expand views of full shape included: strides are not
             looked at, so the rounding of an existing call cannot change);
  "shared" - neither C nor F has a batch axis, float32, nx <= 32, nu <= 8: one Riccati sweep for the whole batch;
  "expand" - any other mix of reduced shapes (float64, larger sizes, a batched C with a shared F, ...): the reduced inputs are
             expanded, materialised and solved by today's dense kernels - the result of expanding them by hand.
"""
import torch

from . import _lib

SHARED_C_TIME, SHARED_F_TIME = 1, 2
SHARED_CVEC_TIME, SHARED_CVEC_BATCH, SHARED_FVEC_TIME, SHARED_FVEC_BATCH = 4, 8, 16, 32
MAX_NX, MAX_NU, MAX_T = 32, 8, 65535


def _dims(t):
    return None if t is None else len(t.shape)


def check_shapes(T, B, nx, nu, C, c, F, f):
    """assert the shape of every input against the accepted forms (full or reduced)"""
    ns = nx + nu
    sC, sc, sF = tuple(C.shape), tuple(c.shape), tuple(F.shape) if F is not None else None
    assert sC in ((T, B, ns, ns), (T, ns, ns), (ns, ns)), "C dim mismatch: %r" % (sC,)
    assert sc in ((T, B, ns), (T, ns), (ns,)), "c dim mismatch: %r" % (sc,)
    if T > 1 or F is not None:
        assert sF is not None and (sF == (nx, ns) or (len(sF) == 3 and sF[0] in (T - 1, T) and sF[1:] == (nx, ns)) or
                                   (len(sF) == 4 and sF[0] in (T - 1, T) and sF[1:] == (B, nx, ns))), \
            "F dim mismatch: %r" % (sF,)
    if f is not None:
        sf = tuple(f.shape)
        assert sf in ((T - 1, B, nx), (T - 1, nx), (nx,)), " f dim mismatch: %r" % (sf,)


def is_full(C, c, F, f):
    """every input of today's shape (a batch axis everywhere)"""
    return _dims(C) == 4 and _dims(c) == 3 and _dims(F) == 4 and _dims(f) in (None, 3)


def layout_of(C, c, F, f):
    """the `layout` bits of dmpc_lqr_shared_* for reduced inputs"""
    lay = 0
    if _dims(C) == 3:
        lay |= SHARED_C_TIME
    if _dims(F) == 3:
        lay |= SHARED_F_TIME
    if _dims(c) >= 2:
        lay |= SHARED_CVEC_TIME
    if _dims(c) == 3:
        lay |= SHARED_CVEC_BATCH
    if f is not None and _dims(f) >= 2:
        lay |= SHARED_FVEC_TIME
    if f is not None and _dims(f) == 3:
        lay |= SHARED_FVEC_BATCH
    return lay


def classify(T, nx, nu, C, c, F, f, precision="float32"):
    """-> "full", "shared" or "expand" (module docstring); shapes are assumed checked"""
    if is_full(C, c, F, f):
        return "full"
    if (_dims(C) in (2, 3) and _dims(F) in (2, 3) and precision == "float32" and nx <= MAX_NX and nu <= MAX_NU
            and T <= MAX_T):
        return "shared"
    return "expand"


def expand_full(T, B, C, c, F, f):
    """reduced inputs as (non-materialised) expand views of today's full shapes; full ones are returned as they are"""
    def ex(t, lead, batch_dims):
        if t is None or _dims(t) == batch_dims:
            return t
        if _dims(t) == batch_dims - 1:              # a time axis, no batch axis
            return t.unsqueeze(1).expand(t.shape[0], B, *t.shape[1:])
        return t.expand(lead, B, *t.shape)          # neither
    return ex(C, T, 4), ex(c, T, 3), ex(F, T - 1, 4), ex(f, T - 1, 3)


def reduce_to(g, shape):
    """the gradient of an expanded input summed back to the input's own shape (the expand path's backward)"""
    if g is None or shape is None or tuple(g.shape) == tuple(shape):
        return g
    if len(shape) == g.dim() - 1:                   # time axis kept: sum over the batch
        return g.sum(dim=1)
    return g.sum(dim=(0, 1))


def solve_device(C, c, F, f, x_init, layout, T, n_state, n_ctrl, info=None):
    """`dmpc_lqr_shared_solve` on float32 device tensors -> (x, u, ws).  `ws` holds the shared blocks of every step: keep it
    for `kkt_grad_device`."""
    lib = _lib.load()
    _lib.require_gpu()
    dev = x_init.device
    B = x_init.shape[0]
    nx, nu = n_state, n_ctrl
    x = torch.empty((T, B, nx), dtype=torch.float32, device=dev)
    u = torch.empty((T, B, nu), dtype=torch.float32, device=dev)
    need = lib.dmpc_lqr_shared_workspace_bytes(T, B, nx, nu)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)     # retained by the caller: not the shared scratch
    with _lib.guard(dev):
        rc = lib.dmpc_lqr_shared_solve(T, B, nx, nu, layout, _lib.ptr(C), _lib.ptr(c), _lib.ptr(F), _lib.ptr(f),
                                       _lib.ptr(x_init), _lib.ptr(x), _lib.ptr(u), _lib.ptr(ws), need, _lib.ptr(info),
                                       _lib.stream_ptr(dev))
    _lib.check(rc, "dmpc_lqr_shared_solve")
    return x, u, ws


def kkt_grad_device(C, c, F, f_shape, x, u, ws_saved, grad_x, grad_u, layout, T, n_state, n_ctrl, strict_math=False,
                    info=None, workspace=None):
    """`dmpc_lqr_shared_kkt_grad` -> (d_x_init [B,nx], dC, dc, dF, df): each gradient in its input's own shape, already
    reduced on the device.  f_shape: the shape of the solve's f, or None (df is then None)."""
    lib = _lib.load()
    _lib.require_gpu()
    dev = x.device
    B = x.shape[1]
    nx, nu = n_state, n_ctrl
    ns = nx + nu
    f32 = dict(dtype=torch.float32, device=dev)
    dx0 = torch.empty((B, nx), **f32)
    dC = torch.empty(tuple(C.shape), **f32)
    dc = torch.empty(tuple(c.shape), **f32)
    dF_shape = (T - 1, nx, ns) if layout & SHARED_F_TIME else (nx, ns)
    dF = torch.empty(dF_shape, **f32) if T > 1 else torch.zeros(dF_shape, **f32)    # (T = 1: F is never read)
    df = None
    if f_shape is not None:
        df = torch.empty(tuple(f_shape), **f32) if T > 1 else torch.zeros(tuple(f_shape), **f32)
    need = lib.dmpc_lqr_shared_grad_workspace_bytes(T, B, nx, nu)
    ws = workspace(need, dev)
    with _lib.guard(dev):
        rc = lib.dmpc_lqr_shared_kkt_grad(T, B, nx, nu, layout, _lib.ptr(C), _lib.ptr(c), _lib.ptr(F), _lib.ptr(x),
                                          _lib.ptr(u), _lib.ptr(ws_saved), _lib.ptr(grad_x), _lib.ptr(grad_u),
                                          1 if strict_math else 0, _lib.ptr(dx0), _lib.ptr(dC), _lib.ptr(dc),
                                          _lib.ptr(dF if T > 1 else None), _lib.ptr(df if T > 1 else None), _lib.ptr(ws),
                                          need, _lib.ptr(info), _lib.stream_ptr(dev))
    _lib.check(rc, "dmpc_lqr_shared_kkt_grad")
    return dx0, dC, dc, dF, df
