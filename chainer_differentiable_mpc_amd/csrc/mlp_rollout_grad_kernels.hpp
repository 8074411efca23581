// mlp_rollout_grad_kernels.hpp - the vector-Jacobian product of the device rollout x_{t+1} = next(x_t, u_t) of a learned
// dynamics model (mlp_dx_kernels.hpp; include/dmpc_mlp_rollout_grad.h): from g = dL/dx [T,B,nx] of any loss of the rolled
// states the gradient with respect to every weight, x_init and u - back-propagation through time, the co-state carried.
//
// Depth one, per trajectory, with tau = [x_t;u_t], z = W1 tau + b1, a = act(z), d = act'(z):
//     lam = g[T-1]
//     for t = T-2 .. 0:   r = lam
//         dW2 += r a^T ;  db2 += r ;  delta = d * (W2^T r) ;  dW1 += delta tau^T ;  db1 += delta
//         v = W1^T delta ;  d_u[t] = v[nx:] ;  lam = g[t] + v[:nx] (+ r when residual)
//     d_x_init = lam ;  d_u[T-1] = 0
// Depth two: e2 = d2 * (W3^T r), e1 = d1 * (W2^T e2) as in mlp2_param_grad_kernel, and v = W1^T e1.
//
// These are mlp_param_grad_kernel and mlp2_param_grad_kernel with the lines those sweeps were entitled to drop (there the
// co-state is exactly zero and r = g_t): the same layout - one wavefront per trajectory, four per workgroup, the weights
// staged once by mlp_stage, a lane owns units lane, lane + 64, ..., the sums in the registers of the lane that owns the unit,
// depth two's dW2 shared by the workgroup through the double-buffered exchange behind ONE workgroup-uniform barrier per step -
// the same partials ([dW1 | db1 | dW2 | db2], [dW1 | db1 | dW2 | dW3 | db2 | db3]) under the same caps, so
// mlp_param_grad_reduce_kernel and mlp2_param_grad_reduce_kernel add them, unchanged.  What is new per step is
// mlp_input_vjp: v_j = sum over the units of layer 1 of W1[h][j] delta_h, one butterfly per input j < nx + nu (at most 24);
// W1[row_k][j] at a fixed j across the lanes is conflict-free at the odd row stride, as it is in the forward pass.
//
// z_t is recomputed from the stored states through mlp_layer_from_lanes, mlp_layer_from_units and mlp_activate alone, so
// it has the bits of the forward launch.  Explicit fmaf, fixed summation order, no atomics: the steps of a trajectory are one
// dependent chain inside one wavefront, and d_x_init[b], d_u[:, b] depend on trajectory b and the weights alone - not on B,
// the grid, or the wavefront's slot.
#pragma once
#include "mlp_dx_kernels.hpp"

namespace dmpc {

struct MlpRolloutGradArgs {
  int T, B, G;                   // T >= 2
  MlpModel m;
  const float *x, *u, *grad_x;   // [T,B,nx] as the rollout stored them, [T,B,nu] (row T-1 is not read), [T,B,nx]
  float *part;                   // [G][P]
  float *d_x_init, *d_u;         // [B,nx], [T,B,nu], each or nullptr
};

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

// wavefront w of G serves trajectories w, w + G, ... in ascending order, t descending (mlp_param_grad_kernel's walk)
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
    float lam = lane < nx ? a.grad_x[last * nx + lane] : 0.f;           // element `lane` of the co-state, 0 in lanes >= nx
    if (a.d_u != nullptr && lane < nu) a.d_u[last * nu + lane] = 0.f;
    for (int t = T - 2; t >= 0; --t) {
      const size_t tb = (size_t)t * B + b;
      const float tau = lane < nx ? a.x[tb * nx + lane] : (lane < ns ? a.u[tb * nu + (lane - nx)] : 0.f);
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
      float nl = lane < nx ? a.grad_x[tb * nx + lane] + v : 0.f;
      if (a.m.residual) nl += r;
      lam = nl;
    }
    if (a.d_x_init != nullptr && lane < nx) a.d_x_init[b * nx + lane] = lam;
  }

  float *p = a.part + (size_t)w * mlp_grad_partial_floats(nx, nu, H);
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

// Two hidden layers: mlp2_param_grad_kernel's walk (workgroup g of G serves the trajectory groups g, g + G, ...), its registers,
// its exchange and its barrier.  A slot without a trajectory walks the clamped addresses of trajectory B - 1 with every
// activation, derivative and co-state element replaced by 0: all it adds are exact zeros, and it stores nothing.
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
    float lam = live && lane < nx ? a.grad_x[last * nx + lane] : 0.f;
    if (live && a.d_u != nullptr && lane < nu) a.d_u[last * nu + lane] = 0.f;
    for (int t = T - 2; t >= 0; --t, ++step) {
      const size_t tb = (size_t)t * B + b;
      const float tau = lane < nx ? a.x[tb * nx + lane] : (lane < ns ? a.u[tb * nu + (lane - nx)] : 0.f);
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
      float nl = live && lane < nx ? a.grad_x[tb * nx + lane] + v : 0.f;
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

  // the workgroup's partial.  dW2 straight from its owners; the rest summed over the wavefronts in slot order, in LDS
  const int n1 = H1 * ns, n2 = H2 * H1, n3 = nx * H2;
  float *const p = a.part + (size_t)blockIdx.x * mlp2_grad_partial_floats(nx, nu, H1, H2);
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

}  // namespace dmpc
