// lqr_shared.hpp - LQR with batch-shared C and F (include/dmpc.h, dmpc_lqr_shared_*).
//
// When neither C nor F has a batch axis the quadratic half of the Riccati recursion (V_t, K_t, Quu_t, Qxu_t) is the same
// for every trajectory: ONE workgroup runs it (lqr_shared_sweep_kernel) and leaves one record of padded blocks per step in
// the workspace.  What stays per trajectory is affine - the v_t / k_t recursion, the rollout, the gradient's second solve
// and its two co-state sweeps - and runs one lane per trajectory with the shared blocks read through the scalar unit
// (wave-uniform addresses in the constant address space: s_load into SGPRs, each v_fma takes its matrix operand from an
// SGPR), state vectors in VGPRs at padded compile-time sizes (NXP in {4,8,16,32}, NUP in {1,2,4,8}; the padding is zeros).
// The gradients of the shared parameters are sums over the batch: lqr_shared_reduce_kernel forms partial sums per
// (step, chunk of trajectories, thread group) in a fixed order, lqr_shared_finalize_kernel adds them in a fixed order
// (and over t where the input has no time axis).  No atomics, no grid barrier: the gradient is bit-reproducible.
// Arithmetic as the reference's (lqr_recursion.py:85-152, differentiable_lqr.py:87-134): Q = C + (F^T V) F in full, no
// symmetrisation of V, all four terms of the value update, Quu^-1 by a pivoted Gauss-Jordan elimination (1/Quu at nu = 1).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/dmpc.h"

namespace dmpc {

constexpr int kSharedMaxNx = 32, kSharedMaxNu = 8;
constexpr int kSharedSweepThreads = 1024;
constexpr int kSharedLaneThreads = 256;
constexpr int kSharedRedThreads = 256;
constexpr int kSharedRedTile = 64;       // trajectories per LDS tile of the reduction
constexpr int kSharedChunk = 1024;       // trajectories per reduction workgroup
constexpr int kSharedHeader = 64;        // floats in front of the step records: [0] = the sweep's DMPC_INFO_* flags (int)

__host__ __device__ constexpr int shared_pad_nx(int nx) { return nx <= 4 ? 4 : nx <= 8 ? 8 : nx <= 16 ? 16 : 32; }
__host__ __device__ constexpr int shared_pad_nu(int nu) { return nu <= 1 ? 1 : nu <= 2 ? 2 : nu <= 4 ? 4 : 8; }
__host__ __device__ constexpr int shared_round4(int n) { return (n + 3) / 4 * 4; }

// One step's record (offsets in floats), padded to (P, U) = (shared_pad_nx, shared_pad_nu), row-major blocks:
//   K [U][P], W = -Quu^-1 [U][U], Qxu [P][U], Quu [U][U], Fx = F_t[:, :nx] [P][P], Fu = F_t[:, nx:] [P][U],
//   Cx = C_t[:nx, :nx] [P][P], Cxu = C_t[:nx, nx:] [P][U], Gx / Gu = rows x / u of F_t^T V_{t+1} [P][P] / [U][P],
//   V_t [P][P], qb = the shared part of q_t [P + U] (c_t if c is shared, + (F_t^T V_{t+1}) f_t if f is shared),
//   fv = f_t if f is shared [P], cx = c_t[:nx] if c is shared [P].  F, G, fv are zero at t = T-1.
struct SharedRec {
  int K, W, Qxu, Quu, Fx, Fu, Cx, Cxu, Gx, Gu, V, qb, fv, cx, size;
};

__host__ __device__ constexpr SharedRec shared_rec(int P, int U) {
  SharedRec r{};
  int o = 0;
  r.K = o; o += U * P;
  r.W = o; o += U * U;
  r.Qxu = o; o += P * U;
  r.Quu = o; o += U * U;
  r.Fx = o; o += P * P;
  r.Fu = o; o += P * U;
  r.Cx = o; o += P * P;
  r.Cxu = o; o += P * U;
  r.Gx = o; o += P * P;
  r.Gu = o; o += U * P;
  r.V = o; o += P * P;
  r.qb = o; o += P + U;
  r.fv = o; o += P;
  r.cx = o; o += P;
  r.size = (o + 3) / 4 * 4;
  return r;
}

// floats of the saved region (header + T records): what the gradient reads of the solve's workspace
__host__ __device__ constexpr size_t shared_saved_floats(int T, int nx, int nu) {
  return (size_t)kSharedHeader + (size_t)T * shared_rec(shared_pad_nx(nx), shared_pad_nu(nu)).size;
}

// floats of one partial record of the reduction: dC [ns][ns], dF [nx][ns], dc [ns], df [nx]
__host__ __device__ constexpr int shared_part_floats(int nx, int nu) {
  return (nx + nu) * (nx + nu) + nx * (nx + nu) + (nx + nu) + nx;
}
__host__ __device__ constexpr int shared_red_groups(int nx, int nu) {
  return kSharedRedThreads / ((shared_round4(nx + nu) / 4) * (shared_round4(nx + nu) / 4));
}

// the shared blocks are read at wave-uniform addresses through the scalar data cache
typedef const __attribute__((address_space(4))) float *shared_cfp;

__device__ inline shared_cfp shared_record(const float *ws, int t, int size) {
  return (shared_cfp)(ws + kSharedHeader) + (size_t)t * size;
}

// ---------------------------------------------------------------------------------------------------------------------
// 1. The quadratic sweep, t = T-1 ... 0, one workgroup, matrices in LDS, runtime nx <= 32, nu <= 8.
__global__ __launch_bounds__(kSharedSweepThreads) void lqr_shared_sweep_kernel(int T, int nx, int nu, uint32_t layout,
                                                                             const float *__restrict__ C,
                                                                             const float *__restrict__ c,
                                                                             const float *__restrict__ F,
                                                                             const float *__restrict__ f,
                                                                             float *__restrict__ ws) {
  constexpr int MX = kSharedMaxNx, MU = kSharedMaxNu, MS = MX + MU;
  __shared__ float sV[MX * MX];        // V_{t+1}, then V_t
  __shared__ float sF[MX * MS];        // F_t [nx][ns]
  __shared__ float sG[MS * MX];        // F_t^T V_{t+1} [ns][nx]
  __shared__ float sQ[MS * MS];        // Q_t [ns][ns]
  __shared__ float sA[MU * 2 * MU];    // [Quu | I] -> [I | Quu^-1]
  __shared__ float sK[MU * MX];        // K_t [nu][nx]
  __shared__ float sKQ[MX * MU];       // K_t^T Quu [nx][nu]
  __shared__ float sq[MS];             // shared part of q_t
  __shared__ float sC[MS * MS];        // C_t [ns][ns]
  __shared__ float sc[MS], sf[MX];     // c_t (when shared), f_t (when shared)
  __shared__ int sPiv, sFlag;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int ns = nx + nu, P = shared_pad_nx(nx), U = shared_pad_nu(nu);
  const SharedRec R = shared_rec(P, U);
  const bool CT = layout & DMPC_SHARED_C_TIME, FT = layout & DMPC_SHARED_F_TIME;
  const bool cT = layout & DMPC_SHARED_CVEC_TIME, cB = layout & DMPC_SHARED_CVEC_BATCH;
  const bool fT = layout & DMPC_SHARED_FVEC_TIME, fB = layout & DMPC_SHARED_FVEC_BATCH;
  const bool f_shared = f != nullptr && !fB;
  if (tid == 0) sFlag = 0;
  for (int e = tid; e < MX * MX; e += nt) sV[e] = 0.f;
  __syncthreads();
  for (int t = T - 1; t >= 0; --t) {
    const bool last = t == T - 1;
    // the step's inputs into LDS (those without a time axis once): no global load latency inside the step
    const bool ft_ = f_shared && !last;
    if (CT || last) {
      const float *Ct = C + (CT ? (size_t)t * ns * ns : 0);
      for (int e = tid; e < ns * ns; e += nt) sC[(e / ns) * MS + e % ns] = Ct[e];
    }
    if (!cB && (cT || last))
      for (int e = tid; e < ns; e += nt) sc[e] = c[(cT ? (size_t)t * ns : 0) + e];
    if (!last && (FT || t == T - 2)) {
      const float *Ft = F + (FT ? (size_t)t * nx * ns : 0);
      for (int e = tid; e < nx * ns; e += nt) sF[(e / ns) * MS + e % ns] = Ft[e];
    }
    if (ft_ && (fT || t == T - 2))
      for (int e = tid; e < nx; e += nt) sf[e] = f[(fT ? (size_t)t * nx : 0) + e];
    __syncthreads();
    for (int e = tid; e < ns * ns; e += nt) sQ[(e / ns) * MS + e % ns] = sC[(e / ns) * MS + e % ns];
    __syncthreads();
    if (!last) {
      for (int e = tid; e < ns * nx; e += nt) {            // G = F^T V
        const int i = e / nx, j = e % nx;
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < nx; ++k) s += sF[k * MS + i] * sV[k * MX + j];
        sG[i * MX + j] = s;
      }
      __syncthreads();
      for (int e = tid; e < ns * ns; e += nt) {            // Q = C + G F
        const int i = e / ns, j = e % ns;
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < nx; ++k) s += sG[i * MX + k] * sF[k * MS + j];
        sQ[i * MS + j] += s;
      }
    }
    for (int e = tid; e < ns; e += nt) {                   // q_t's shared part: c_t + G f_t
      float s = cB ? 0.f : sc[e];
      if (ft_) {
        float g = 0.f;
        for (int k = 0; k < nx; ++k) g += sG[e * MX + k] * sf[k];
        s += g;
      }
      sq[e] = s;
    }
    __syncthreads();
    // Quu^-1: Gauss-Jordan with partial pivoting on [Quu | I] (nu == 1: the scalar inverse 1 / Quu)
    for (int e = tid; e < nu * 2 * nu; e += nt) {
      const int i = e / (2 * nu), j = e % (2 * nu);
      sA[i * 2 * MU + j] = j < nu ? sQ[(nx + i) * MS + nx + j] : (j - nu == i ? 1.f : 0.f);
    }
    __syncthreads();
    for (int col = 0; col < nu; ++col) {
      if (tid == 0) {
        int piv = col;
        float best = fabsf(sA[col * 2 * MU + col]);
        for (int r = col + 1; r < nu; ++r) {
          const float a = fabsf(sA[r * 2 * MU + col]);
          if (a > best) best = a, piv = r;
        }
        if (best == 0.f) sFlag |= DMPC_INFO_SINGULAR;
        sPiv = piv;
      }
      __syncthreads();
      const int piv = sPiv;
      float val = 0.f;
      int r = 0, j = 0;
      const bool mine = tid < nu * 2 * nu;
      if (mine) {
        r = tid / (2 * nu), j = tid % (2 * nu);
        const int rr = r == col ? piv : (r == piv ? col : r);     // rows col and piv swapped
        const float p = sA[piv * 2 * MU + col];
        const float prow = sA[piv * 2 * MU + j] / p;
        val = r == col ? prow : sA[rr * 2 * MU + j] - sA[rr * 2 * MU + col] * prow;
      }
      __syncthreads();
      if (mine) sA[r * 2 * MU + j] = val;
      __syncthreads();
    }
    for (int e = tid; e < nu * nx; e += nt) {              // K = -(Quu^-1 Qux)
      const int i = e / nx, j = e % nx;
      float s = 0.f;
      for (int k = 0; k < nu; ++k) s += sA[i * 2 * MU + nu + k] * sQ[(nx + k) * MS + j];
      sK[i * MX + j] = -s;
    }
    __syncthreads();
    for (int e = tid; e < nx * nu; e += nt) {              // K^T Quu
      const int i = e / nu, j = e % nu;
      float s = 0.f;
      for (int k = 0; k < nu; ++k) s += sK[k * MX + i] * sQ[(nx + k) * MS + nx + j];
      sKQ[i * MU + j] = s;
    }
    __syncthreads();
    for (int e = tid; e < nx * nx; e += nt) {              // V_t = Qxx + Qxu K + K^T Qux + (K^T Quu) K
      const int i = e / nx, j = e % nx;
      float a = 0.f, b = 0.f, d = 0.f;
      for (int k = 0; k < nu; ++k) {
        a += sQ[i * MS + nx + k] * sK[k * MX + j];
        b += sK[k * MX + i] * sQ[(nx + k) * MS + j];
        d += sKQ[i * MU + k] * sK[k * MX + j];
      }
      sV[i * MX + j] = ((sQ[i * MS + j] + a) + b) + d;
    }
    __syncthreads();
    // the step's record, zero-padded to (P, U)
    float *rec = ws + kSharedHeader + (size_t)t * R.size;
    for (int e = tid; e < R.size; e += nt) {
      float v = 0.f;
      int i, j;
      if (e < R.W) {
        i = (e - R.K) / P, j = (e - R.K) % P;
        if (i < nu && j < nx) v = sK[i * MX + j];
      } else if (e < R.Qxu) {
        i = (e - R.W) / U, j = (e - R.W) % U;
        if (i < nu && j < nu) v = -sA[i * 2 * MU + nu + j];
      } else if (e < R.Quu) {
        i = (e - R.Qxu) / U, j = (e - R.Qxu) % U;
        if (i < nx && j < nu) v = sQ[i * MS + nx + j];
      } else if (e < R.Fx) {
        i = (e - R.Quu) / U, j = (e - R.Quu) % U;
        if (i < nu && j < nu) v = sQ[(nx + i) * MS + nx + j];
      } else if (e < R.Fu) {
        i = (e - R.Fx) / P, j = (e - R.Fx) % P;
        if (!last && i < nx && j < nx) v = sF[i * MS + j];
      } else if (e < R.Cx) {
        i = (e - R.Fu) / U, j = (e - R.Fu) % U;
        if (!last && i < nx && j < nu) v = sF[i * MS + nx + j];
      } else if (e < R.Cxu) {
        i = (e - R.Cx) / P, j = (e - R.Cx) % P;
        if (i < nx && j < nx) v = sC[i * MS + j];
      } else if (e < R.Gx) {
        i = (e - R.Cxu) / U, j = (e - R.Cxu) % U;
        if (i < nx && j < nu) v = sC[i * MS + nx + j];
      } else if (e < R.Gu) {
        i = (e - R.Gx) / P, j = (e - R.Gx) % P;
        if (!last && i < nx && j < nx) v = sG[i * MX + j];
      } else if (e < R.V) {
        i = (e - R.Gu) / P, j = (e - R.Gu) % P;
        if (!last && i < nu && j < nx) v = sG[(nx + i) * MX + j];
      } else if (e < R.qb) {
        i = (e - R.V) / P, j = (e - R.V) % P;
        if (i < nx && j < nx) v = sV[i * MX + j];
      } else if (e < R.fv) {
        i = e - R.qb;
        if (i < nx) v = sq[i];
        else if (i >= P && i - P < nu) v = sq[nx + i - P];
      } else if (e < R.cx) {
        i = e - R.fv;
        if (ft_ && i < nx) v = sf[i];
      } else {
        i = e - R.cx;
        if (!cB && i < nx) v = sc[i];
      }
      rec[e] = v;
    }
    __syncthreads();
  }
  if (tid == 0) reinterpret_cast<int *>(ws)[0] = sFlag;
}

// ---------------------------------------------------------------------------------------------------------------------
// per-lane helpers (P, U compile time; n the live length)
template <int N>
__device__ inline void lane_load(float (&v)[N], const float *p, int n) {
  if (n == N && N % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
#pragma unroll
    for (int i = 0; i < N; i += 4) {
      const float4 q = *reinterpret_cast<const float4 *>(p + i);
      v[i] = q.x, v[i + 1] = q.y, v[i + 2] = q.z, v[i + 3] = q.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = i < n ? p[i] : 0.f;
  }
}
template <int N>
__device__ inline void lane_store(float *p, const float (&v)[N], int n) {
  if (n == N && N % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
#pragma unroll
    for (int i = 0; i < N; i += 4) *reinterpret_cast<float4 *>(p + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i < n) p[i] = v[i];
  }
}
template <int N>
__device__ inline bool lane_finite(const float (&v)[N]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < N; ++i) ok = ok && isfinite(v[i]);
  return ok;
}
// y = M x, M [R][Cc] row-major
template <int Rr, int Cc>
__device__ inline void mv(float (&y)[Rr], shared_cfp M, const float (&x)[Cc]) {
#pragma unroll
  for (int i = 0; i < Rr; ++i) y[i] = 0.f;
#pragma unroll
  for (int k = 0; k < Cc; ++k)
#pragma unroll
    for (int i = 0; i < Rr; ++i) y[i] += M[i * Cc + k] * x[k];
}
// y = M^T x, M [Rr][Cc] row-major, y [Cc]
template <int Rr, int Cc>
__device__ inline void mtv(float (&y)[Cc], shared_cfp M, const float (&x)[Rr]) {
#pragma unroll
  for (int j = 0; j < Cc; ++j) y[j] = 0.f;
#pragma unroll
  for (int k = 0; k < Rr; ++k)
#pragma unroll
    for (int j = 0; j < Cc; ++j) y[j] += M[k * Cc + j] * x[k];
}

// one step of the affine recursion: (q_x, q_u) -> k_t, and v_t = q_x + Qxu k + K^T q_u + K^T (Quu k)
template <int P, int U>
__device__ inline void affine_step(shared_cfp r, const SharedRec &R, const float (&qx)[P], const float (&qu)[U], float (&k)[U],
                                   float (&v)[P]) {
  mv<U, U>(k, r + R.W, qu);
  float qk[U], a[P], b[P], d[P];
  mv<U, U>(qk, r + R.Quu, k);
  mv<P, U>(a, r + R.Qxu, k);
  mtv<U, P>(b, r + R.K, qu);
  mtv<U, P>(d, r + R.K, qk);
#pragma unroll
  for (int i = 0; i < P; ++i) v[i] = ((qx[i] + a[i]) + b[i]) + d[i];
}

// q_t's per-trajectory part for t < T-1: (q_x, q_u) += F_t^T v_{t+1}
template <int P, int U>
__device__ inline void add_ftv(shared_cfp r, const SharedRec &R, const float (&v)[P], float (&qx)[P], float (&qu)[U]) {
  float a[P], b[U];
  mtv<P, P>(a, r + R.Fx, v);
  mtv<P, U>(b, r + R.Fu, v);
#pragma unroll
  for (int i = 0; i < P; ++i) qx[i] += a[i];
#pragma unroll
  for (int j = 0; j < U; ++j) qu[j] += b[j];
}

// x_{t+1} = F_t [x; u]
template <int P, int U>
__device__ inline void dyn_step(shared_cfp r, const SharedRec &R, const float (&x)[P], const float (&u)[U], float (&xn)[P]) {
  float a[P], b[P];
  mv<P, P>(a, r + R.Fx, x);
  mv<P, U>(b, r + R.Fu, u);
#pragma unroll
  for (int i = 0; i < P; ++i) xn[i] = a[i] + b[i];
}

// ---------------------------------------------------------------------------------------------------------------------
// 2. Per-trajectory affine sweep and rollout: one lane per trajectory.
template <int P, int U>
__global__ __launch_bounds__(kSharedLaneThreads) void lqr_shared_affine_kernel(
    int T, int B, int nx, int nu, uint32_t layout, const float *__restrict__ c, const float *__restrict__ f,
    const float *__restrict__ x_init, const float *__restrict__ ws, float *__restrict__ kbuf, float *__restrict__ x_out,
    float *__restrict__ u_out, int32_t *__restrict__ info) {
  constexpr SharedRec R = shared_rec(P, U);
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int ns = nx + nu;
  const bool cB = layout & DMPC_SHARED_CVEC_BATCH;
  const bool fB = f != nullptr && (layout & DMPC_SHARED_FVEC_BATCH);
  float v[P];
#pragma unroll
  for (int i = 0; i < P; ++i) v[i] = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    const shared_cfp r = shared_record(ws, t, R.size);
    float qx[P], qu[U];
#pragma unroll
    for (int i = 0; i < P; ++i) qx[i] = r[R.qb + i];
#pragma unroll
    for (int j = 0; j < U; ++j) qu[j] = r[R.qb + P + j];
    if (cB) {
      const float *ct = c + ((size_t)t * B + b) * ns;
      float cx[P], cu[U];
      lane_load(cx, ct, nx);
      lane_load(cu, ct + nx, nu);
#pragma unroll
      for (int i = 0; i < P; ++i) qx[i] += cx[i];
#pragma unroll
      for (int j = 0; j < U; ++j) qu[j] += cu[j];
    }
    if (t < T - 1) {
      if (fB) {
        float fb[P], gx[P], gu[U];
        lane_load(fb, f + ((size_t)t * B + b) * nx, nx);
        mv<P, P>(gx, r + R.Gx, fb);
        mv<U, P>(gu, r + R.Gu, fb);
#pragma unroll
        for (int i = 0; i < P; ++i) qx[i] += gx[i];
#pragma unroll
        for (int j = 0; j < U; ++j) qu[j] += gu[j];
      }
      add_ftv<P, U>(r, R, v, qx, qu);
    }
    float k[U];
    affine_step<P, U>(r, R, qx, qu, k, v);
#pragma unroll
    for (int j = 0; j < U; ++j) kbuf[((size_t)t * U + j) * B + b] = k[j];
  }
  float x[P];
  lane_load(x, x_init + (size_t)b * nx, nx);
  bool ok = true;
  for (int t = 0; t < T; ++t) {
    const shared_cfp r = shared_record(ws, t, R.size);
    float u[U];
    mv<U, P>(u, r + R.K, x);
#pragma unroll
    for (int j = 0; j < U; ++j) u[j] += kbuf[((size_t)t * U + j) * B + b];
    lane_store(x_out + ((size_t)t * B + b) * nx, x, nx);
    lane_store(u_out + ((size_t)t * B + b) * nu, u, nu);
    ok = ok && lane_finite(x) && lane_finite(u);
    if (t < T - 1) {
      float xn[P];
      dyn_step<P, U>(r, R, x, u, xn);
      if (fB) {
        float fb[P];
        lane_load(fb, f + ((size_t)t * B + b) * nx, nx);
#pragma unroll
        for (int i = 0; i < P; ++i) x[i] = xn[i] + fb[i];
      } else if (f) {
#pragma unroll
        for (int i = 0; i < P; ++i) x[i] = xn[i] + r[R.fv + i];
      } else {
#pragma unroll
        for (int i = 0; i < P; ++i) x[i] = xn[i];
      }
    }
  }
  if (info) info[b] = reinterpret_cast<const int *>(ws)[0] | (ok ? 0 : DMPC_INFO_NONFINITE);
}

// ---------------------------------------------------------------------------------------------------------------------
// 3a. Gradient, per trajectory: the affine-only second solve on c' = [grad_x; grad_u], f = 0, x_init = 0 (its tau' is
// d_tau, written to dtau [T][B][ns]), then the co-state sweeps lambda / d_lambda (lam, dlam [T][B][nx]).
template <int P, int U>
__global__ __launch_bounds__(kSharedLaneThreads) void lqr_shared_grad_lane_kernel(
    int T, int B, int nx, int nu, uint32_t layout, int strict_math, const float *__restrict__ c,
    const float *__restrict__ x, const float *__restrict__ u, const float *__restrict__ grad_x,
    const float *__restrict__ grad_u, const float *__restrict__ ws_saved, float *__restrict__ kbuf,
    float *__restrict__ dtau, float *__restrict__ lam, float *__restrict__ dlam, float *__restrict__ d_x_init,
    float *__restrict__ df, int32_t *__restrict__ info) {
  constexpr SharedRec R = shared_rec(P, U);
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int ns = nx + nu;
  const bool cB = layout & DMPC_SHARED_CVEC_BATCH;
  float v[P];
#pragma unroll
  for (int i = 0; i < P; ++i) v[i] = 0.f;
  for (int t = T - 1; t >= 0; --t) {                    // second solve, affine recursion
    const shared_cfp r = shared_record(ws_saved, t, R.size);
    float qx[P], qu[U];
    lane_load(qx, grad_x + ((size_t)t * B + b) * nx, nx);
    lane_load(qu, grad_u + ((size_t)t * B + b) * nu, nu);
    if (t < T - 1) add_ftv<P, U>(r, R, v, qx, qu);
    float k[U];
    affine_step<P, U>(r, R, qx, qu, k, v);
#pragma unroll
    for (int j = 0; j < U; ++j) kbuf[((size_t)t * U + j) * B + b] = k[j];
  }
  float dx[P];
#pragma unroll
  for (int i = 0; i < P; ++i) dx[i] = 0.f;
  for (int t = 0; t < T; ++t) {                         // its rollout: d_tau
    const shared_cfp r = shared_record(ws_saved, t, R.size);
    float du[U];
    mv<U, P>(du, r + R.K, dx);
#pragma unroll
    for (int j = 0; j < U; ++j) du[j] += kbuf[((size_t)t * U + j) * B + b];
    float *row = dtau + ((size_t)t * B + b) * ns;
    lane_store(row, dx, nx);
    lane_store(row + nx, du, nu);
    if (t < T - 1) {
      float xn[P];
      dyn_step<P, U>(r, R, dx, du, xn);
#pragma unroll
      for (int i = 0; i < P; ++i) dx[i] = xn[i];
    }
  }
  float l[P], dl[P];
  bool ok = true;
  for (int t = T - 1; t >= 0; --t) {                    // co-states (differentiable_lqr.py:92-103, 115-125)
    const shared_cfp r = shared_record(ws_saved, t, R.size);
    const size_t row = (size_t)t * B + b;
    float tx[P], tu[U], dtx[P], dtu[U], gx[P], cx[P];
    lane_load(tx, x + row * nx, nx);
    lane_load(tu, u + row * nu, nu);
    lane_load(dtx, dtau + row * ns, nx);
    lane_load(dtu, dtau + row * ns + nx, nu);
    lane_load(gx, grad_x + row * nx, nx);
    if (cB) {
      lane_load(cx, c + row * ns, nx);
    } else {
#pragma unroll
      for (int i = 0; i < P; ++i) cx[i] = r[R.cx + i];
    }
    float a[P], a2[P], d[P], d2[P];
    mv<P, P>(a, r + R.Cx, tx);
    mv<P, U>(a2, r + R.Cxu, tu);
    mv<P, P>(d, r + R.Cx, dtx);
    mv<P, U>(d2, r + R.Cxu, dtu);
    if (t < T - 1) {
      float fl[P], fdl[P];
      mtv<P, P>(fl, r + R.Fx, l);
      mtv<P, P>(fdl, r + R.Fx, dl);
#pragma unroll
      for (int i = 0; i < P; ++i) {
        l[i] = (fl[i] + (a[i] + a2[i])) + cx[i];
        dl[i] = (fdl[i] + (d[i] + d2[i])) + gx[i];
      }
    } else {
#pragma unroll
      for (int i = 0; i < P; ++i) {
        l[i] = (a[i] + a2[i]) + cx[i];
        dl[i] = (d[i] + d2[i]) + gx[i];
      }
    }
    lane_store(lam + row * nx, l, nx);
    lane_store(dlam + row * nx, dl, nx);
    ok = ok && lane_finite(l) && lane_finite(dl);
    if (df) {                                           // f per trajectory: df = d_lambda[0:T-1] (strict: [1:T])
      if (!strict_math && t < T - 1) lane_store(df + row * nx, dl, nx);
      if (strict_math && t > 0) lane_store(df + ((size_t)(t - 1) * B + b) * nx, dl, nx);
    }
  }
  lane_store(d_x_init + (size_t)b * nx, dl, nx);
  if (info) info[b] = reinterpret_cast<const int *>(ws_saved)[0] | (ok ? 0 : DMPC_INFO_NONFINITE);
}

// ---------------------------------------------------------------------------------------------------------------------
// 3b. Partial sums over a chunk of trajectories, step t = blockIdx.y, chunk blockIdx.x.  Thread (I, J, g): the 4x4 blocks
// (I, J) of dC_t and (I < nx/4) dF_t over the trajectories g, g + G, ... of each tile; J = 0 also the 4-blocks I of dc_t,
// df_t.  Record [t][chunk][g][shared_part_floats]: dC [ns][ns], dF [nx][ns], dc [ns], df [nx].
// d_tau comes as two arrays with a row stride each: (dtau, dtau + nx) at stride ns for the shared LQR's one [T][B][ns] array,
// (dx, du) at strides (nx, nu) for the MPC step's workspace (dmpc_mpc_step_backward_shared).
__global__ __launch_bounds__(kSharedRedThreads) void lqr_shared_reduce_kernel(
    int T, int B, int nx, int nu, int strict_math, const float *__restrict__ x, const float *__restrict__ u,
    const float *__restrict__ dtx, const float *__restrict__ dtu, int dtx_stride, int dtu_stride,
    const float *__restrict__ lam, const float *__restrict__ dlam, float *__restrict__ part) {
  constexpr int MS4 = shared_round4(kSharedMaxNx + kSharedMaxNu), MX4 = kSharedMaxNx, TB = kSharedRedTile;
  __shared__ __align__(16) float sTau[TB * MS4], sDtau[TB * MS4], sLam[TB * MX4], sDlam[TB * MX4], sDf[TB * MX4];
  const int ch = blockIdx.x, t = blockIdx.y, nchunk = gridDim.x;
  const int tid = threadIdx.x;
  const int ns = nx + nu, S4 = shared_round4(ns), X4 = shared_round4(nx);
  const int nbi = S4 / 4, nbx = X4 / 4, nblk = nbi * nbi;
  const int G = kSharedRedThreads / nblk;
  const int blk = tid % nblk, g = tid / nblk;
  const bool active = g < G;
  const int I = blk / nbi, J = blk % nbi;
  const bool hasF = t < T - 1;
  const bool rowF = hasF && I < nbx;
  float a1[4][4] = {}, a2[4][4] = {}, f1[4][4] = {}, f2[4][4] = {}, vc[4] = {}, vf[4] = {};
  const int b_lo = ch * kSharedChunk, b_hi = min(B, b_lo + kSharedChunk);
  for (int b0 = b_lo; b0 < b_hi; b0 += TB) {
    const int nb = min(TB, b_hi - b0);
    __syncthreads();
    for (int e = tid; e < TB * S4; e += kSharedRedThreads) {
      const int bb = e / S4, i = e % S4;
      float tv = 0.f, dv = 0.f;
      if (bb < nb && i < ns) {
        const size_t row = (size_t)t * B + b0 + bb;
        tv = i < nx ? x[row * nx + i] : u[row * nu + i - nx];
        dv = i < nx ? dtx[row * dtx_stride + i] : dtu[row * dtu_stride + i - nx];
      }
      sTau[bb * MS4 + i] = tv;
      sDtau[bb * MS4 + i] = dv;
    }
    for (int e = tid; e < TB * X4; e += kSharedRedThreads) {
      const int bb = e / X4, i = e % X4;
      float lv = 0.f, dlv = 0.f, dfv = 0.f;
      if (bb < nb && i < nx && hasF) {
        const size_t row1 = (size_t)(t + 1) * B + b0 + bb;
        lv = lam[row1 * nx + i];
        dlv = dlam[row1 * nx + i];
        dfv = strict_math ? dlv : dlam[((size_t)t * B + b0 + bb) * nx + i];
      }
      sLam[bb * MX4 + i] = lv;
      sDlam[bb * MX4 + i] = dlv;
      sDf[bb * MX4 + i] = dfv;
    }
    __syncthreads();
    if (!active) continue;
    for (int bb = g; bb < nb; bb += G) {
      const float4 ti = *reinterpret_cast<const float4 *>(&sTau[bb * MS4 + 4 * I]);
      const float4 di = *reinterpret_cast<const float4 *>(&sDtau[bb * MS4 + 4 * I]);
      const float4 tj = *reinterpret_cast<const float4 *>(&sTau[bb * MS4 + 4 * J]);
      const float4 dj = *reinterpret_cast<const float4 *>(&sDtau[bb * MS4 + 4 * J]);
      const float TI[4] = {ti.x, ti.y, ti.z, ti.w}, DI[4] = {di.x, di.y, di.z, di.w};
      const float TJ[4] = {tj.x, tj.y, tj.z, tj.w}, DJ[4] = {dj.x, dj.y, dj.z, dj.w};
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          a1[p][q] += DI[p] * TJ[q];
          a2[p][q] += TI[p] * DJ[q];
        }
      if (J == 0) {
#pragma unroll
        for (int p = 0; p < 4; ++p) vc[p] += DI[p];
      }
      if (rowF) {
        const float4 li = *reinterpret_cast<const float4 *>(&sLam[bb * MX4 + 4 * I]);
        const float4 dli = *reinterpret_cast<const float4 *>(&sDlam[bb * MX4 + 4 * I]);
        const float LI[4] = {li.x, li.y, li.z, li.w}, DLI[4] = {dli.x, dli.y, dli.z, dli.w};
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            f1[p][q] += DLI[p] * TJ[q];
            f2[p][q] += LI[p] * DJ[q];
          }
        if (J == 0) {
          const float4 dfi = *reinterpret_cast<const float4 *>(&sDf[bb * MX4 + 4 * I]);
          vf[0] += dfi.x, vf[1] += dfi.y, vf[2] += dfi.z, vf[3] += dfi.w;
        }
      }
    }
  }
  if (!active) return;
  const int PF = shared_part_floats(nx, nu);
  float *rec = part + ((size_t)(t * nchunk + ch) * G + g) * PF;
  float *rdC = rec, *rdF = rec + ns * ns, *rdc = rdF + nx * ns, *rdf = rdc + ns;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = 4 * I + p;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = 4 * J + q;
      if (i < ns && j < ns) rdC[i * ns + j] = strict_math ? 0.5f * (a1[p][q] + a2[p][q]) : 0.5f * a1[p][q] + a2[p][q];
      if (i < nx && j < ns) rdF[i * ns + j] = rowF ? f1[p][q] + f2[p][q] : 0.f;
    }
    if (J == 0 && i < ns) rdc[i] = vc[p];
    if (J == 0 && i < nx) rdf[i] = rowF ? vf[p] : 0.f;
  }
}

// 3c. The reduced gradients: one workgroup per output element; thread k adds the partial records k, k + 256, ... (over
// chunks, groups and - where the input has no time axis - steps), then a tree in LDS: a fixed order, no atomics.
// out_sign: +1 DiffLqr, -1 MPCstep (mpc/mpc_step.py:383-446 is minus the strict_math forms); times 1 changes no bit.
constexpr int kSharedFinThreads = 256;
__global__ __launch_bounds__(kSharedFinThreads) void lqr_shared_finalize_kernel(int T, int nx, int nu, uint32_t layout,
                                                                                int nchunk, int G, float out_sign,
                                                                                const float *__restrict__ part,
                                                                                float *__restrict__ dC, float *__restrict__ dc,
                                                                                float *__restrict__ dF, float *__restrict__ df) {
  __shared__ float red[kSharedFinThreads];
  const int ns = nx + nu, PF = shared_part_floats(nx, nu), tid = threadIdx.x;
  const bool CT = layout & DMPC_SHARED_C_TIME, FT = layout & DMPC_SHARED_F_TIME;
  const bool cT = layout & DMPC_SHARED_CVEC_TIME, fT = layout & DMPC_SHARED_FVEC_TIME;
  const long long nC = dC ? (long long)(CT ? T : 1) * ns * ns : 0;
  const long long nF = dF && T > 1 ? (long long)(FT ? T - 1 : 1) * nx * ns : 0;
  const long long nc = dc ? (long long)(cT ? T : 1) * ns : 0;
  const long long nf = df && T > 1 ? (long long)(fT ? T - 1 : 1) * nx : 0;
  const long long total = nC + nF + nc + nf;
  const int per_t = nchunk * G;
  for (long long e = blockIdx.x; e < total; e += gridDim.x) {
    long long r = e;
    float *out;
    int off, per, t0, t1;
    if (r < nC) {
      per = ns * ns, out = dC, off = 0;
      t0 = CT ? (int)(r / per) : 0, t1 = CT ? t0 + 1 : T;
    } else if ((r -= nC) < nF) {
      per = nx * ns, out = dF, off = ns * ns;
      t0 = FT ? (int)(r / per) : 0, t1 = FT ? t0 + 1 : T - 1;
    } else if ((r -= nF) < nc) {
      per = ns, out = dc, off = ns * ns + nx * ns;
      t0 = cT ? (int)(r / per) : 0, t1 = cT ? t0 + 1 : T;
    } else {
      r -= nc;
      per = nx, out = df, off = ns * ns + nx * ns + ns;
      t0 = fT ? (int)(r / per) : 0, t1 = fT ? t0 + 1 : T - 1;
    }
    const int w = (int)(r % per);
    const long long n = (long long)(t1 - t0) * per_t;
    const float *base = part + (size_t)t0 * per_t * PF + off + w;
    float s = 0.f;
    for (long long k = tid; k < n; k += kSharedFinThreads) s += base[(size_t)k * PF];
    red[tid] = s;
    __syncthreads();
    for (int h = kSharedFinThreads / 2; h > 0; h >>= 1) {
      if (tid < h) red[tid] += red[tid + h];
      __syncthreads();
    }
    if (tid == 0) out[r] = out_sign * red[0];
    __syncthreads();
  }
}

}  // namespace dmpc
