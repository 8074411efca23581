"""Problems with batch-shared C and F, and the float64 reference for their gradients: the oracle's dense
difflqr_backward on the expanded inputs, summed over the axes each reduced input lacks."""
import numpy as np

from oracle import kkt, lqr


def f32(a):
    return None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64)


def make(nx, nu, T, B, seed=0, C_time=False, F_time=False, c_kind="shared", f_kind="none", nonsym=False, illcond=False):
    """c_kind: "shared" [ns], "time" [T,ns], "batch" [T,B,ns];  f_kind: "none", "shared" [nx], "time" [T-1,nx],
    "batch" [T-1,B,nx].  Values are float32-representable float64."""
    rng = np.random.default_rng(seed)
    ns = nx + nu

    def cost():
        M = rng.standard_normal((ns, ns)) / np.sqrt(ns)
        C = M @ M.T + np.eye(ns)
        if nonsym:
            C = C + 0.3 * np.triu(rng.standard_normal((ns, ns)), 1)
        if illcond:                       # Quu with eigenvalues down to ~1e-3 of its largest
            C[nx:, :] *= 0.0
            C[:, nx:] *= 0.0
            C[nx:, nx:] = np.diag(np.logspace(0, -3, nu))
        return C

    def dyn():
        A = 0.9 * np.eye(nx) + 0.2 * rng.standard_normal((nx, nx)) / np.sqrt(nx)
        Bm = rng.standard_normal((nx, nu)) / np.sqrt(nx)
        if illcond:
            Bm[:, -1] *= 1e-2
        return np.concatenate((A, Bm), axis=1)

    C = np.stack([cost() for _ in range(T)]) if C_time else cost()
    F = np.stack([dyn() for _ in range(T - 1)]) if F_time else dyn()
    c = {"shared": lambda: rng.standard_normal(ns), "time": lambda: rng.standard_normal((T, ns)),
         "batch": lambda: rng.standard_normal((T, B, ns))}[c_kind]()
    f = {"none": lambda: None, "shared": lambda: 0.1 * rng.standard_normal(nx),
         "time": lambda: 0.1 * rng.standard_normal((T - 1, nx)),
         "batch": lambda: 0.1 * rng.standard_normal((T - 1, B, nx))}[f_kind]()
    x_init = rng.standard_normal((B, nx))
    return dict(T=T, B=B, nx=nx, nu=nu, C=f32(C), c=f32(c), F=f32(F), f=f32(f), x_init=f32(x_init))


def expand(a, lead, B, batch_dims):
    """a reduced input expanded to today's full shape (float64 copy)"""
    if a is None or a.ndim == batch_dims:
        return a
    if a.ndim == batch_dims - 1:
        return np.ascontiguousarray(np.broadcast_to(a[:, None], (a.shape[0], B) + a.shape[1:]))
    return np.ascontiguousarray(np.broadcast_to(a, (lead, B) + a.shape))


def full(p):
    T, B = p["T"], p["B"]
    return expand(p["C"], T, B, 4), expand(p["c"], T, B, 3), expand(p["F"], T - 1, B, 4), expand(p["f"], T - 1, B, 3)


def reduce(g, shape):
    """a dense gradient summed to the input's own shape"""
    if g is None or shape is None or g.shape == tuple(shape):
        return g
    if len(shape) == g.ndim - 1:
        return g.sum(axis=1)
    return g.sum(axis=(0, 1))


def solve(p):
    C, c, F, f = full(p)
    return lqr.lqr_solve(p["x_init"], C, c, F, f, p["T"], p["nx"], p["nu"])


def grads(p, x, u, gx, gu, strict_math=False):
    """-> (d_x_init, dC, dc, dF, df) in the shapes of p's inputs (df None without f)"""
    C, c, F, f = full(p)
    dx0, dC, dc, dF, df = kkt.difflqr_backward(p["x_init"], C, c, F, x, u, gx, gu, p["T"], p["nx"], p["nu"],
                                               strict_math=strict_math)
    return (dx0, reduce(dC, p["C"].shape), reduce(dc, p["c"].shape), reduce(dF, p["F"].shape),
            None if p["f"] is None else reduce(df, p["f"].shape))
