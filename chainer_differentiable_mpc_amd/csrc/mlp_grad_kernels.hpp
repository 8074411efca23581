// mlp_grad_kernels.hpp - the reverse sweeps over the device rollout x_{t+1} = next(x_t, u_t) of a learned dynamics model
// (mlp_dx_kernels.hpp): the gradient with respect to every weight, x_init and u of
//     a loss of the linearisation's f_t = next(x_t, u_t) - F_t [x_t;u_t], F_t a CONSTANT   (include/dmpc.h, include/dmpc_mlp_grad.h:
//                                                                         mlp_param_grad_kernel, mlp2_param_grad_kernel)
//     a loss of the rolled states x themselves, the co-state carried      (include/dmpc_mlp_rollout_grad.h:
//                                                                         mlp_rollout_grad_kernel, mlp2_rollout_grad_kernel)
// One backward step.  Depth one, per trajectory, with tau = [x_t;u_t], z = W1 tau + b1,
// a = act(z), d = act'(z), for t = T-2 .. 0:
//     dW2 += r a^T ;  db2 += r ;  delta = d * (W2^T r) ;  dW1 += delta tau^T ;  db1 += delta
// Depth two, with the forward pieces of MlpNet<2>:
//     dW3 += r a2^T ;  db3 += r ;  e2 = d2 * (W3^T r) ;  dW2 += e2 a1^T ;  db2 += e2 ;  e1 = d1 * (W2^T e2) ;  dW1 += e1 tau^T ;  db1 += e1
// What differs is where r comes from and what reaches the inputs:
//     param_grad      the loss is one of f.  With g_t = dL/df_t every term of the co-state carries a factor of the co-state of step
//                     t + 1, and that of step T - 1 is 0: next's derivative through z_t and F_t's cancel at every step, as exact zeros
//                     in any arithmetic and for every activation.  So r = g_t, the co-state's lines are not evaluated, and
//                     d_x_init, d_u are stored as the zeros they are.
//     rollout_grad    the loss is one of x, g = dL/dx [T,B,nx]:  lam = g[T-1];  r = lam;  v = W1^T delta (mlp_input_vjp: one butterfly
//                     per input j < nx + nu, W1[row_k][j] at a fixed j conflict-free at the odd row stride);  d_u[t] = v[nx:];
//                     lam = g[t] + v[:nx] (+ r when residual);  at the end d_x_init = lam, d_u[T-1] = 0.
//
// Layout.  One wavefront per trajectory, four per workgroup, the weights staged once by mlp_stage; z_t is recomputed from the
// stored states through mlp_layer_from_lanes, mlp_layer_from_units and mlp_activate alone, so it has the bits of the forward
// launch.  A lane keeps the sums for ITS hidden units (lane, lane + 64, ...) in registers - every array indexed by unrolled
// loops with wave-uniform guards, never by a runtime value.  Explicit fmaf, a fixed summation order, no atomics: a result
// depends on (T, B, nx, nu, the widths) and the data alone, and d_x_init[b], d_u[:, b] on trajectory b and the weights alone.
//     depth one   wavefront w of G serves trajectories w, w + G, ... in ascending order, t descending, and stores one partial
//                 [dW1 | db1 | dW2 | db2], laid out as the parameters are, at part + w * P.
//     depth two   workgroup g of G serves the trajectory groups g, g + G, ... (b = 4 group + slot).  A wavefront keeps rows of dW1
//                 and db1 (layer-1 units), columns of dW3 and db2 (layer-2 units), db3 (lanes < nx): 85 per lane.  dW2 [H2,H1], up
//                 to 16,384 sums, belongs to the workgroup: wavefront w keeps rows 32 w .. 32 w + 31, a lane columns lane and
//                 lane + 64 of them: 64 per lane.  Each step every wavefront publishes a1 and e2 of ITS trajectory (complete to 128
//                 entries, exact zeros beyond the widths) into a double-buffered exchange behind the staged weights, and after
//                 ONE workgroup barrier every wavefront adds the four outer products into its rows: plain fmaf, slot ascending.
//                 The barrier is workgroup-uniform: every wavefront runs the trip counts of its workgroup.  A slot without a
//                 trajectory (b >= B) walks the clamped addresses of trajectory B - 1 with every activation, derivative and
//                 co-state element replaced by 0: all it adds are exact zeros, and it stores nothing.  Two buffers suffice: a
//                 wavefront that writes buffer n & 1 at step n + 2 has passed barrier n + 1, behind which nobody reads step n's.
//                 At the end the four wavefronts' register sums are added in slot order 0, 1, 2, 3 in LDS (over the weights,
//                 which nobody reads any more) and the workgroup stores ONE partial [dW1 | db1 | dW2 | dW3 | db2 | db3] - the
//                 order of the packed weights - at part + g * P.
// The reduce kernels add the G partials per element in ascending order.
//
// What is shared and what is not, by measurement (profiles/r05/mlp_grad_refactor_ab.txt; parent and head through the C ABI, runs
// 0.0001 ms apart).  Every float sequence of the backward step exists as a __forceinline__ piece below, and every sweep uses the
// pieces that leave ITS time and registers where they were:
//     all four sweeps         mlp_grad_tau and the partial-store epilogue of their depth
//     mlp2_param_grad_kernel  every piece (2 % faster than its own text, 1 to 3 VGPRs fewer)
// The loops of the other three stay written in place: from the pieces the compiler schedules them differently - in
// mlp_param_grad_kernel mlp_output_vjp alone costs 0.5 % to 4.4 % and mlp_outer_from_lanes +2.3 % to -1.5 %; the rollout gradients
// from the pieces run 1.4 % to 2.1 % longer at one size each.  Values are bit-equal either way (tests/golden/mlp_grad_values.npz).
#pragma once
#include "mlp_dx_kernels.hpp"

namespace dmpc {

constexpr int kMlpGradCap = 512;                             // partials at most: 21.5 MB at the largest model
__host__ __device__ inline int mlp_grad_partials(int B) { return B < kMlpGradCap ? B : kMlpGradCap; }
__host__ __device__ inline int mlp_grad_partial_floats(int nx, int nu, int H) { return H * (nx + nu) + H + nx * H + nx; }

constexpr int kMlp2GradCap = 256;                            // partials at most: one resident workgroup per CU; 22.3 MB at the largest model
constexpr int kMlp2GradRows = mlp_max_hidden(2) / kMlpWaves;          // rows of dW2 a wavefront keeps
constexpr int kMlp2GradExchangeFloats = 2 * kMlpWaves * 2 * mlp_max_hidden(2);   // two buffers of [slot][a1 (128) | e2 (128)]
__host__ __device__ inline int mlp2_grad_partials(int B) {
  const int groups = B / kMlpWaves + (B % kMlpWaves != 0 ? 1 : 0);       // (no overflow at any B)
  return groups < kMlp2GradCap ? groups : kMlp2GradCap;
}
__host__ __device__ inline int mlp2_grad_partial_floats(int nx, int nu, int H1, int H2) {
  return H1 * (nx + nu) + H1 + H2 * H1 + nx * H2 + H2 + nx;
}
constexpr size_t mlp2_grad_lds_bytes(int nx, int nu, int H1, int H2) {
  return mlp_lds_bytes(nx, nu, H1, H2, false) + kMlp2GradExchangeFloats * sizeof(float);
}
static_assert(mlp2_grad_lds_bytes(16, 8, 128, 128) == 96384 && mlp2_grad_lds_bytes(16, 8, 128, 128) <= kMlpLdsLimit, "weights + exchange");

struct MlpGradArgs {
  int T, B, G;                   // T >= 2
  MlpModel m;
  const float *x, *u, *g;        // [T,B,nx] as the rollout stored them, [T,B,nu] (row T-1 is not read); dL/df [T-1,B,nx] or dL/dx [T,B,nx]
  float *part;                   // [G][P]
  float *d_x_init, *d_u;         // [B,nx], [T,B,nu], each or nullptr
};
struct MlpRolloutGradArgs : MlpGradArgs {};   // (a type of its own: the name a profiler lists for the rollout-gradient kernels)

// element `lane` of W1^T delta (0 in lanes >= ns): delta at this lane's units of layer 1, exact zeros beyond the width
template <int UNITS>
__device__ __forceinline__ float mlp_input_vjp(const float *W1s, const int ld, const MlpUnits<UNITS> &U, const int ns, const int lane,
                                               const float (&delta)[UNITS]) {
  float v = 0.f;
  for (int j = 0; j < ns; ++j) {
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      if (k < U.n) {
        const float w = W1s[U.row[k] * ld + j];
        part = fmaf(U.has[k] ? w : 0.f, delta[k], part);
      }
    }
    const float s = wave_sum64(part);
    v = lane == j ? s : v;
  }
  return v;
}

// ---- pieces of a backward step, each float sequence once.  U: the units of the layer whose sums the lane keeps

// element `lane` of tau = [x_t;u_t]: x in lanes < nx, u in nx .. ns, 0 beyond
__device__ __forceinline__ float mlp_grad_tau(const MlpGradArgs &a, const size_t tb, const int lane) {
  const int nx = a.m.nx, nu = a.m.nu;
  return lane < nx ? a.x[tb * nx + lane] : (lane < nx + nu ? a.u[tb * nu + (lane - nx)] : 0.f);
}

// the output layer: s_k += sum_i W[i][row_k] r_i at this lane's units of the last hidden layer, dW[k][i] += r_i a_k; r_i in lane i
template <int UNITS>
__device__ __forceinline__ void mlp_output_vjp(const float *Ws, const int ld, const MlpUnits<UNITS> &U, const int nx, const float r,
                                               const float (&act)[UNITS], float (&s)[UNITS], float (&dW)[UNITS][kMlpMaxNx]) {
#pragma unroll
  for (int k = 0; k < UNITS; ++k) s[k] = 0.f;
#pragma unroll
  for (int i = 0; i < kMlpMaxNx; ++i) {
    if (i < nx) {
      const float ri = lane_value(r, i);
#pragma unroll
      for (int k = 0; k < UNITS; ++k) {
        if (k < U.n) {
          const float w = Ws[i * ld + U.row[k]];
          s[k] = fmaf(U.has[k] ? w : 0.f, ri, s[k]);
          dW[k][i] = fmaf(ri, act[k], dW[k][i]);
        }
      }
    }
  }
}

// delta = d * s ;  db += delta
template <int UNITS>
__device__ __forceinline__ void mlp_delta(const float (&d)[UNITS], const float (&s)[UNITS], float (&delta)[UNITS], float (&db)[UNITS]) {
#pragma unroll
  for (int k = 0; k < UNITS; ++k) {
    delta[k] = d[k] * s[k];
    db[k] += delta[k];
  }
}

// layer 1: dW1[k][j] += delta_k tau_j, element j of tau in lane j
template <int UNITS>
__device__ __forceinline__ void mlp_outer_from_lanes(const MlpUnits<UNITS> &U, const int ns, const float (&delta)[UNITS], const float tau,
                                                     float (&dW1)[UNITS][kMlpMaxNx + kMlpMaxNu]) {
#pragma unroll
  for (int j = 0; j < kMlpMaxNx + kMlpMaxNu; ++j) {
    if (j < ns) {
      const float tj = lane_value(tau, j);
#pragma unroll
      for (int k = 0; k < UNITS; ++k)
        if (k < U.n) dW1[k][j] = fmaf(delta[k], tj, dW1[k][j]);
    }
  }
}

// s_k += sum_h W[h][row_k] e_h at this lane's units of layer 1 (U), e over the H2 units of layer 2 (unit 64 k2 + l in e[k2] of
// lane l), h ascending: column reads of the staged matrix
template <int UNITS>
__device__ __forceinline__ void mlp_hidden_vjp(const float *Ws, const int ld, const MlpUnits<UNITS> &U, const int H2, const float (&e)[UNITS],
                                               float (&s)[UNITS]) {
#pragma unroll
  for (int k = 0; k < UNITS; ++k) s[k] = 0.f;
#pragma unroll
  for (int k2 = 0; k2 < UNITS; ++k2) {
    const int left = H2 - 64 * k2, cnt = left < 64 ? left : 64;
    for (int l = 0; l < cnt; ++l) {
      const float eh = lane_value(e[k2], l);
#pragma unroll
      for (int k = 0; k < UNITS; ++k) {
        if (k < U.n) {
          const float w = Ws[(64 * k2 + l) * ld + U.row[k]];
          s[k] = fmaf(U.has[k] ? w : 0.f, eh, s[k]);
        }
      }
    }
  }
}

// slot wv's a1 and e2 into the step's exchange buffer [slot][a1 (HMAX) | e2 (HMAX)]; the workgroup's barrier is the caller's
template <int UNITS>
__device__ __forceinline__ void mlp2_grad_publish(float *exb, const int wv, const int lane, const float (&a1)[UNITS], const float (&e2)[UNITS]) {
  constexpr int HMAX = mlp_max_hidden(2);
#pragma unroll
  for (int k = 0; k < UNITS; ++k) {
    exb[wv * 2 * HMAX + lane + 64 * k] = a1[k];
    exb[wv * 2 * HMAX + HMAX + lane + 64 * k] = e2[k];
  }
}

// this wavefront's rows of dW2 (row0 ..): the four trajectories' e2[row] a1[column] from the exchange, slot ascending
template <int UNITS>
__device__ __forceinline__ void mlp2_grad_accumulate(const float *exb, const int lane, const int row0, const int H2,
                                                     float (&dW2)[kMlp2GradRows][UNITS]) {
  constexpr int HMAX = mlp_max_hidden(2), ROWS = kMlp2GradRows;
  float a1s[kMlpWaves][UNITS], e2s[kMlpWaves];
#pragma unroll
  for (int s = 0; s < kMlpWaves; ++s) {
#pragma unroll
    for (int k = 0; k < UNITS; ++k) a1s[s][k] = exb[s * 2 * HMAX + lane + 64 * k];
    e2s[s] = exb[s * 2 * HMAX + HMAX + row0 + lane % ROWS];       // row row0 + l in lane l < 32
  }
#pragma unroll
  for (int q = 0; q < ROWS; q += 8) {
    if (row0 + q < H2) {                             // wave-uniform; rows beyond H2 inside the eight add exact zeros
#pragma unroll
      for (int rr = q; rr < q + 8; ++rr) {
#pragma unroll
        for (int s = 0; s < kMlpWaves; ++s) {
          const float e = lane_value(e2s[s], rr);
#pragma unroll
          for (int k = 0; k < UNITS; ++k) dW2[rr][k] = fmaf(e, a1s[s][k], dW2[rr][k]);
        }
      }
    }
  }
}

// depth one's partial [dW1 | db1 | dW2 | db2] straight from the registers of the lanes that own the units
template <int UNITS>
__device__ __forceinline__ void mlp_grad_store_partial(float *p, const int nx, const int ns, const int H, const int lane,
                                                       const float (&dW1)[UNITS][kMlpMaxNx + kMlpMaxNu], const float (&db1)[UNITS],
                                                       const float (&dW2)[UNITS][kMlpMaxNx], const float db2) {
  float *pb1 = p + H * ns, *pW2 = pb1 + H, *pb2 = pW2 + nx * H;
#pragma unroll
  for (int k = 0; k < UNITS; ++k) {
    const int h = lane + 64 * k;
    if (h < H) {
#pragma unroll
      for (int j = 0; j < kMlpMaxNx + kMlpMaxNu; ++j)
        if (j < ns) p[h * ns + j] = dW1[k][j];
      pb1[h] = db1[k];
#pragma unroll
      for (int i = 0; i < kMlpMaxNx; ++i)
        if (i < nx) pW2[i * H + h] = dW2[k][i];
    }
  }
  if (lane < nx) pb2[lane] = db2;
}

// The workgroup's partial at p, by every thread of the workgroup (it has barriers of its own).  dW2 straight from its owners;
// the rest summed over the wavefronts in slot order, in LDS from `lds` on
template <int UNITS>
__device__ __forceinline__ void mlp2_grad_store_partial(float *p, float *lds, const MlpModel &m, const int lane, const int wv,
                                                        const float (&dW1)[UNITS][kMlpMaxNx + kMlpMaxNu], const float (&db1)[UNITS],
                                                        const float (&dW2)[kMlp2GradRows][UNITS], const float (&dW3)[UNITS][kMlpMaxNx],
                                                        const float (&db2)[UNITS], const float db3) {
  constexpr int ROWS = kMlp2GradRows;
  const int nx = m.nx, ns = m.nx + m.nu, H1 = m.H[0], H2 = m.H[1];
  const int n1 = H1 * ns, n2 = H2 * H1, n3 = nx * H2, row0 = ROWS * wv;
  float *const pW2 = p + n1 + H1;
#pragma unroll
  for (int rr = 0; rr < ROWS; ++rr) {
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      const int h2 = row0 + rr, h1 = lane + 64 * k;
      if (h2 < H2 && h1 < H1) pW2[h2 * H1 + h1] = dW2[rr][k];
    }
  }
  __syncthreads();                                       // nobody reads the weights or the exchange any more
  float *const q1 = lds, *const qb1 = q1 + n1, *const q3 = qb1 + H1, *const qb2 = q3 + n3, *const qb3 = qb2 + H2;
  for (int s = 0; s < kMlpWaves; ++s) {
    if (wv == s) {
      const bool first = s == 0;
#pragma unroll
      for (int k = 0; k < UNITS; ++k) {
        const int h = lane + 64 * k;
        if (h < H1) {
#pragma unroll
          for (int j = 0; j < kMlpMaxNx + kMlpMaxNu; ++j)
            if (j < ns) q1[h * ns + j] = first ? dW1[k][j] : q1[h * ns + j] + dW1[k][j];
          qb1[h] = first ? db1[k] : qb1[h] + db1[k];
        }
        if (h < H2) {
#pragma unroll
          for (int i = 0; i < kMlpMaxNx; ++i)
            if (i < nx) q3[i * H2 + h] = first ? dW3[k][i] : q3[i * H2 + h] + dW3[k][i];
          qb2[h] = first ? db2[k] : qb2[h] + db2[k];
        }
      }
      if (lane < nx) qb3[lane] = first ? db3 : qb3[lane] + db3;
    }
    __syncthreads();
  }
  const int Q = n1 + H1 + n3 + H2 + nx;                  // the partial without dW2, which sits behind db1
  for (int e = threadIdx.x; e < Q; e += 64 * kMlpWaves) p[e < n1 + H1 ? e : e + n2] = lds[e];
}

// ---- the four sweeps
template <int ACT>
__global__ __launch_bounds__(64 * kMlpWaves) void mlp_param_grad_kernel(const MlpGradArgs a) {
  extern __shared__ float lds[];
  constexpr int UNITS = mlp_units(1);
  const MlpLds<1> L = mlp_stage<1>(a.m, lds);
  const int lane = threadIdx.x % 64;
  const int w = blockIdx.x * kMlpWaves + threadIdx.x / 64;
  if (w >= a.G) return;      // (after the only barrier)
  const int nx = a.m.nx, nu = a.m.nu, ns = nx + nu, H = a.m.H[0];
  const int T = a.T;
  const size_t B = (size_t)a.B;
  const MlpUnits<UNITS> U(lane, H);
  float dW1[UNITS][kMlpMaxNx + kMlpMaxNu] = {}, dW2[UNITS][kMlpMaxNx] = {}, db1[UNITS] = {}, db2 = 0.f;

  for (size_t b = w; b < B; b += a.G) {
    if (a.d_x_init != nullptr && lane < nx) a.d_x_init[b * nx + lane] = 0.f;
    if (a.d_u != nullptr && lane < nu)
      for (int t = 0; t < T; ++t) a.d_u[((size_t)t * B + b) * nu + lane] = 0.f;
    for (int t = T - 2; t >= 0; --t) {
      const size_t tb = (size_t)t * B + b;
      const float tau = mlp_grad_tau(a, tb, lane);
      const float r = lane < nx ? a.g[tb * nx + lane] : 0.f;
      float z[UNITS], act[UNITS], dact[UNITS];
      mlp_layer_from_lanes(L.W[0], L.ld[0], L.b[0], U, ns, tau, z);
#pragma unroll
      for (int k = 0; k < UNITS; ++k) mlp_activate<ACT>(U.live(k), z[k], act[k], dact[k]);
      db2 += r;
      float s[UNITS] = {};                               // W2^T r at this lane's units
#pragma unroll
      for (int i = 0; i < kMlpMaxNx; ++i) {
        if (i < nx) {
          const float ri = lane_value(r, i);
#pragma unroll
          for (int k = 0; k < UNITS; ++k) {
            if (k < U.n) {
              const float w2 = L.W[1][i * L.ld[1] + U.row[k]];
              s[k] = fmaf(U.has[k] ? w2 : 0.f, ri, s[k]);
              dW2[k][i] = fmaf(ri, act[k], dW2[k][i]);
            }
          }
        }
      }
      float delta[UNITS];
#pragma unroll
      for (int k = 0; k < UNITS; ++k) {
        delta[k] = dact[k] * s[k];
        db1[k] += delta[k];
      }
#pragma unroll
      for (int j = 0; j < kMlpMaxNx + kMlpMaxNu; ++j) {
        if (j < ns) {
          const float tj = lane_value(tau, j);
#pragma unroll
          for (int k = 0; k < UNITS; ++k)
            if (k < U.n) dW1[k][j] = fmaf(delta[k], tj, dW1[k][j]);
        }
      }
    }
  }

  mlp_grad_store_partial(a.part + (size_t)w * mlp_grad_partial_floats(nx, nu, H), nx, ns, H, lane, dW1, db1, dW2, db2);
}

template <int ACT>
__global__ __launch_bounds__(64 * kMlpWaves) void mlp_rollout_grad_kernel(const MlpRolloutGradArgs a) {
  extern __shared__ float lds[];
  constexpr int UNITS = mlp_units(1);
  const MlpLds<1> L = mlp_stage<1>(a.m, lds);
  const int lane = threadIdx.x % 64;
  const int w = blockIdx.x * kMlpWaves + threadIdx.x / 64;
  if (w >= a.G) return;      // (after the only barrier)
  const int nx = a.m.nx, nu = a.m.nu, ns = nx + nu, H = a.m.H[0];
  const int T = a.T;
  const size_t B = (size_t)a.B;
  const bool is_u = lane >= nx && lane < ns;
  const MlpUnits<UNITS> U(lane, H);
  float dW1[UNITS][kMlpMaxNx + kMlpMaxNu] = {}, dW2[UNITS][kMlpMaxNx] = {}, db1[UNITS] = {}, db2 = 0.f;

  for (size_t b = w; b < B; b += a.G) {
    const size_t last = (size_t)(T - 1) * B + b;
    float lam = lane < nx ? a.g[last * nx + lane] : 0.f;           // element `lane` of the co-state, 0 in lanes >= nx
    if (a.d_u != nullptr && lane < nu) a.d_u[last * nu + lane] = 0.f;
    for (int t = T - 2; t >= 0; --t) {
      const size_t tb = (size_t)t * B + b;
      const float tau = mlp_grad_tau(a, tb, lane);
      const float r = lam;
      float z[UNITS], act[UNITS], dact[UNITS];
      mlp_layer_from_lanes(L.W[0], L.ld[0], L.b[0], U, ns, tau, z);
#pragma unroll
      for (int k = 0; k < UNITS; ++k) mlp_activate<ACT>(U.live(k), z[k], act[k], dact[k]);
      db2 += r;
      float s[UNITS] = {};                               // W2^T r at this lane's units
#pragma unroll
      for (int i = 0; i < kMlpMaxNx; ++i) {
        if (i < nx) {
          const float ri = lane_value(r, i);
#pragma unroll
          for (int k = 0; k < UNITS; ++k) {
            if (k < U.n) {
              const float w2 = L.W[1][i * L.ld[1] + U.row[k]];
              s[k] = fmaf(U.has[k] ? w2 : 0.f, ri, s[k]);
              dW2[k][i] = fmaf(ri, act[k], dW2[k][i]);
            }
          }
        }
      }
      float delta[UNITS];
#pragma unroll
      for (int k = 0; k < UNITS; ++k) {
        delta[k] = dact[k] * s[k];
        db1[k] += delta[k];
      }
#pragma unroll
      for (int j = 0; j < kMlpMaxNx + kMlpMaxNu; ++j) {
        if (j < ns) {
          const float tj = lane_value(tau, j);
#pragma unroll
          for (int k = 0; k < UNITS; ++k)
            if (k < U.n) dW1[k][j] = fmaf(delta[k], tj, dW1[k][j]);
        }
      }
      const float v = mlp_input_vjp(L.W[0], L.ld[0], U, ns, lane, delta);
      if (a.d_u != nullptr && is_u) a.d_u[tb * nu + (lane - nx)] = v;
      float nl = lane < nx ? a.g[tb * nx + lane] + v : 0.f;
      if (a.m.residual) nl += r;
      lam = nl;
    }
    if (a.d_x_init != nullptr && lane < nx) a.d_x_init[b * nx + lane] = lam;
  }

  mlp_grad_store_partial(a.part + (size_t)w * mlp_grad_partial_floats(nx, nu, H), nx, ns, H, lane, dW1, db1, dW2, db2);
}

// The depth-two weight gradient, composed of the pieces.  A body under a thin kernel, as mlp_rollout_linearize_body is: written
// straight into the __global__ function the same text holds 32 accumulation registers and loses a wave per SIMD.
template <int ACT>
__device__ __forceinline__ void mlp2_param_grad_body(const MlpGradArgs &a, float *lds) {
  constexpr int UNITS = mlp_units(2), HMAX = mlp_max_hidden(2), ROWS = kMlp2GradRows;
  static_assert(UNITS == 2 && ROWS == 32, "a lane owns two units of a layer and two columns of 32 rows of dW2");
  const MlpLds<2> L = mlp_stage<2>(a.m, lds);
  float *const ex = L.b[2] + a.m.nx;           // the exchange, behind the staged biases
  const int lane = threadIdx.x % 64, wv = threadIdx.x / 64;
  const int nx = a.m.nx, ns = nx + a.m.nu, H1 = a.m.H[0], H2 = a.m.H[1];
  const size_t B = (size_t)a.B;
  const int groups = (a.B + kMlpWaves - 1) / kMlpWaves;
  const MlpUnits<UNITS> U1(lane, H1), U2(lane, H2);
  float dW1[UNITS][kMlpMaxNx + kMlpMaxNu] = {}, db1[UNITS] = {}, dW3[UNITS][kMlpMaxNx] = {}, db2[UNITS] = {}, db3 = 0.f;
  float dW2[ROWS][UNITS] = {};
  int step = 0;

  for (int grp = blockIdx.x; grp < groups; grp += a.G) {      // workgroup-uniform
    const size_t b0 = (size_t)grp * kMlpWaves + wv;
    const bool live = b0 < B;                                  // wave-uniform
    const size_t b = live ? b0 : B - 1;
    if (live) {
      if (a.d_x_init != nullptr && lane < nx) a.d_x_init[b * nx + lane] = 0.f;
      if (a.d_u != nullptr && lane < a.m.nu)
        for (int t = 0; t < a.T; ++t) a.d_u[((size_t)t * B + b) * a.m.nu + lane] = 0.f;
    }
    for (int t = a.T - 2; t >= 0; --t, ++step) {
      const size_t tb = (size_t)t * B + b;
      const float tau = mlp_grad_tau(a, tb, lane);
      const float r = live && lane < nx ? a.g[tb * nx + lane] : 0.f;
      float z[UNITS], a1[UNITS], d1[UNITS], a2[UNITS], d2[UNITS];
      mlp_layer_from_lanes(L.W[0], L.ld[0], L.b[0], U1, ns, tau, z);
#pragma unroll
      for (int k = 0; k < UNITS; ++k) mlp_activate<ACT>(live && U1.live(k), z[k], a1[k], d1[k]);
      mlp_layer_from_units(L.W[1], L.ld[1], L.b[1], U2, H1, a1, z);
#pragma unroll
      for (int k = 0; k < UNITS; ++k) mlp_activate<ACT>(live && U2.live(k), z[k], a2[k], d2[k]);

      db3 += r;
      float s2[UNITS], e2[UNITS];                   // s2: W3^T r at this lane's layer-2 units
      mlp_output_vjp(L.W[2], L.ld[2], U2, nx, r, a2, s2, dW3);
      mlp_delta(d2, s2, e2, db2);

      // publish a1 and e2 (zeros beyond the widths and in a slot without a trajectory), then the workgroup's one barrier
      float *const exb = ex + (step & 1) * (kMlpWaves * 2 * HMAX);
      mlp2_grad_publish(exb, wv, lane, a1, e2);
      __syncthreads();

      float s1[UNITS], e1[UNITS];                   // s1: W2^T e2 at this lane's layer-1 units
      mlp_hidden_vjp(L.W[1], L.ld[1], U1, H2, e2, s1);
      mlp_delta(d1, s1, e1, db1);
      mlp_outer_from_lanes(U1, ns, e1, tau, dW1);
      mlp2_grad_accumulate(exb, lane, ROWS * wv, H2, dW2);
    }
  }
  mlp2_grad_store_partial(a.part + (size_t)blockIdx.x * mlp2_grad_partial_floats(nx, a.m.nu, H1, H2), lds, a.m, lane, wv, dW1, db1,
                          dW2, dW3, db2, db3);
}

template <int ACT>
__global__ __launch_bounds__(64 * kMlpWaves) void mlp2_param_grad_kernel(const MlpGradArgs a) {
  extern __shared__ float lds[];
  mlp2_param_grad_body<ACT>(a, lds);
}

template <int ACT>
__global__ __launch_bounds__(64 * kMlpWaves) void mlp2_rollout_grad_kernel(const MlpRolloutGradArgs a) {
  extern __shared__ float lds[];
  constexpr int UNITS = mlp_units(2), HMAX = mlp_max_hidden(2), ROWS = kMlp2GradRows;
  static_assert(UNITS == 2 && ROWS == 32, "a lane owns two units of a layer and two columns of 32 rows of dW2");
  const MlpLds<2> L = mlp_stage<2>(a.m, lds);
  float *const ex = L.b[2] + a.m.nx;           // the exchange, behind the staged biases
  const int lane = threadIdx.x % 64, wv = threadIdx.x / 64;
  const int nx = a.m.nx, nu = a.m.nu, ns = nx + nu, H1 = a.m.H[0], H2 = a.m.H[1];
  const int T = a.T;
  const size_t B = (size_t)a.B;
  const int groups = (a.B + kMlpWaves - 1) / kMlpWaves;
  const bool is_u = lane >= nx && lane < ns;
  const MlpUnits<UNITS> U1(lane, H1), U2(lane, H2);
  const int row0 = ROWS * wv;
  float dW1[UNITS][kMlpMaxNx + kMlpMaxNu] = {}, db1[UNITS] = {}, dW3[UNITS][kMlpMaxNx] = {}, db2[UNITS] = {}, db3 = 0.f;
  float dW2[ROWS][UNITS] = {};
  int step = 0;

  for (int grp = blockIdx.x; grp < groups; grp += a.G) {      // workgroup-uniform
    const size_t b0 = (size_t)grp * kMlpWaves + wv;
    const bool live = b0 < B;                                  // wave-uniform
    const size_t b = live ? b0 : B - 1;
    const size_t last = (size_t)(T - 1) * B + b;
    float lam = live && lane < nx ? a.g[last * nx + lane] : 0.f;
    if (live && a.d_u != nullptr && lane < nu) a.d_u[last * nu + lane] = 0.f;
    for (int t = T - 2; t >= 0; --t, ++step) {
      const size_t tb = (size_t)t * B + b;
      const float tau = mlp_grad_tau(a, tb, lane);
      const float r = lam;
      float z[UNITS], a1[UNITS], d1[UNITS], a2[UNITS], d2[UNITS];
      mlp_layer_from_lanes(L.W[0], L.ld[0], L.b[0], U1, ns, tau, z);
#pragma unroll
      for (int k = 0; k < UNITS; ++k) mlp_activate<ACT>(live && U1.live(k), z[k], a1[k], d1[k]);
      mlp_layer_from_units(L.W[1], L.ld[1], L.b[1], U2, H1, a1, z);
#pragma unroll
      for (int k = 0; k < UNITS; ++k) mlp_activate<ACT>(live && U2.live(k), z[k], a2[k], d2[k]);

      db3 += r;
      float s2[UNITS] = {};                              // W3^T r at this lane's layer-2 units
#pragma unroll
      for (int i = 0; i < kMlpMaxNx; ++i) {
        if (i < nx) {
          const float ri = lane_value(r, i);
#pragma unroll
          for (int k = 0; k < UNITS; ++k) {
            if (k < U2.n) {
              const float w3 = L.W[2][i * L.ld[2] + U2.row[k]];
              s2[k] = fmaf(U2.has[k] ? w3 : 0.f, ri, s2[k]);
              dW3[k][i] = fmaf(ri, a2[k], dW3[k][i]);
            }
          }
        }
      }
      float e2[UNITS];
#pragma unroll
      for (int k = 0; k < UNITS; ++k) {
        e2[k] = d2[k] * s2[k];
        db2[k] += e2[k];
      }

      // publish a1 and e2 (zeros beyond the widths and in a slot without a trajectory), then the workgroup's one barrier
      float *const exb = ex + (step & 1) * (kMlpWaves * 2 * HMAX);
#pragma unroll
      for (int k = 0; k < UNITS; ++k) {
        exb[wv * 2 * HMAX + lane + 64 * k] = a1[k];
        exb[wv * 2 * HMAX + HMAX + lane + 64 * k] = e2[k];
      }
      __syncthreads();

      float s1[UNITS] = {};                              // W2^T e2 at this lane's layer-1 units: column reads of the staged W2
#pragma unroll
      for (int k2 = 0; k2 < UNITS; ++k2) {
        const int left = H2 - 64 * k2, cnt = left < 64 ? left : 64;
        for (int l = 0; l < cnt; ++l) {
          const float eh = lane_value(e2[k2], l);
#pragma unroll
          for (int k = 0; k < UNITS; ++k) {
            if (k < U1.n) {
              const float w2 = L.W[1][(64 * k2 + l) * L.ld[1] + U1.row[k]];
              s1[k] = fmaf(U1.has[k] ? w2 : 0.f, eh, s1[k]);
            }
          }
        }
      }
      float e1[UNITS];
#pragma unroll
      for (int k = 0; k < UNITS; ++k) {
        e1[k] = d1[k] * s1[k];
        db1[k] += e1[k];
      }
#pragma unroll
      for (int j = 0; j < kMlpMaxNx + kMlpMaxNu; ++j) {
        if (j < ns) {
          const float tj = lane_value(tau, j);
#pragma unroll
          for (int k = 0; k < UNITS; ++k)
            if (k < U1.n) dW1[k][j] = fmaf(e1[k], tj, dW1[k][j]);
        }
      }

      // the co-state: through layer 1 to the step's inputs (a slot without a trajectory: e1 = 0, lam stays 0)
      const float v = mlp_input_vjp(L.W[0], L.ld[0], U1, ns, lane, e1);
      if (live && a.d_u != nullptr && is_u) a.d_u[tb * nu + (lane - nx)] = v;
      float nl = live && lane < nx ? a.g[tb * nx + lane] + v : 0.f;
      if (a.m.residual) nl += r;
      lam = nl;

      // this wavefront's rows of dW2: the four trajectories' e2[row] a1[column], slot ascending
      float a1s[kMlpWaves][UNITS], e2s[kMlpWaves];
#pragma unroll
      for (int s = 0; s < kMlpWaves; ++s) {
#pragma unroll
        for (int k = 0; k < UNITS; ++k) a1s[s][k] = exb[s * 2 * HMAX + lane + 64 * k];
        e2s[s] = exb[s * 2 * HMAX + HMAX + row0 + lane % ROWS];       // row row0 + l in lane l < 32
      }
#pragma unroll
      for (int q = 0; q < ROWS; q += 8) {
        if (row0 + q < H2) {                             // wave-uniform; rows beyond H2 inside the eight add exact zeros
#pragma unroll
          for (int rr = q; rr < q + 8; ++rr) {
#pragma unroll
            for (int s = 0; s < kMlpWaves; ++s) {
              const float e = lane_value(e2s[s], rr);
#pragma unroll
              for (int k = 0; k < UNITS; ++k) dW2[rr][k] = fmaf(e, a1s[s][k], dW2[rr][k]);
            }
          }
        }
      }
    }
    if (live && a.d_x_init != nullptr && lane < nx) a.d_x_init[b * nx + lane] = lam;
  }

  mlp2_grad_store_partial(a.part + (size_t)blockIdx.x * mlp2_grad_partial_floats(nx, nu, H1, H2), lds, a.m, lane, wv, dW1, db1,
                          dW2, dW3, db2, db3);
}

// The reduction: one thread per parameter element adds the G partials in ascending order; G = 0 stores zeros (T = 1: no
// dynamics step, no partials).  A partial is [dW1 (n1) | db1 (nb1) | second matrices (n2) | second biases (nb2)] - depth one:
// n1 = H ns, nb1 = H, n2 = nx H, nb2 = nx; depth two: [dW2 | dW3] and [db2 | db3].  Two kernels over one body: the recorded
// values name each depth's.
struct MlpGradReduceArgs {
  int G, n1, nb1, n2, nb2;
  const float *part;               // [G][P]
  float *dW1, *db1, *dW2, *db2;    // [n1], [nb1], [n2], [nb2]
};
struct Mlp2GradReduceArgs : MlpGradReduceArgs {};

__device__ __forceinline__ void mlp_grad_reduce(const MlpGradReduceArgs &a) {
  const int P = a.n1 + a.nb1 + a.n2 + a.nb2;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P) return;
  float s = 0.f;
#pragma unroll 8
  for (int g = 0; g < a.G; ++g) s += a.part[(size_t)g * P + e];
  if (e < a.n1) a.dW1[e] = s;
  else if (e < a.n1 + a.nb1) a.db1[e - a.n1] = s;
  else if (e < a.n1 + a.nb1 + a.n2) a.dW2[e - a.n1 - a.nb1] = s;
  else a.db2[e - a.n1 - a.nb1 - a.n2] = s;
}
__global__ __launch_bounds__(256) void mlp_param_grad_reduce_kernel(const MlpGradReduceArgs a) { mlp_grad_reduce(a); }
__global__ __launch_bounds__(256) void mlp2_param_grad_reduce_kernel(const Mlp2GradReduceArgs a) { mlp_grad_reduce(a); }

}  // namespace dmpc
