// mlp_cost_kernels.hpp - a learned, stationary, non-quadratic stage cost on the device (MlpCost of the Python layer):
//
//     c(tau) = 1/2 tau' Q tau + p' tau + w2' act(W1 tau + b1),     tau = [x;u],  act = tanh | relu | silu | softplus
//
//   mlp_cost_approx_kernel            approximate_cost (mpc/approximate.py:18-54) in one launch: at every (t, b) the value, the
//                                     Hessian H = Qs + W1' diag(w2 act''(z)) W1 with Qs = (Q + Q')/2, and g0 = grad - H tau.
//                                     In g0 the quadratic part cancels (Qs tau - Qs tau), and W1 tau = z - b1, so
//                                         g0 = p + W1' (w2 * (act'(z) - act''(z) * (z - b1)))
//                                     is formed without that cancellation.  Any of the outputs may be left out.
//   mpc_forward_rec_mlp_cost_kernel   MPCstep.forward_rec (mpc/mpc_step.py:175-286) under a dense LinDx with this cost in place
//                                     of C_true, c_true: the pass, the search and the epilogue of mpc_forward_rec_mlp_kernel.
//   mlp_cost_param_grad_kernel        the gradient of a loss L(g0, costs) with respect to Q, p, W1, b1, w2 with tau, H and
//                                     H tau held constant; partial sums, added by mlp_cost_param_grad_reduce_kernel.
//
// Layout.  Runtime dimensions (nx <= 16, nu <= 8, H <= 256).  ONE wavefront per point - a (t, b) of the Taylor model and of the
// gradient, a trajectory of the search - four per workgroup.  The weights are staged into LDS once per workgroup: W1 [H][ns | 1]
// (lane l owns hidden units l, l + 64, l + 128, l + 192 and walks ITS rows: the odd stride puts the 64 rows on 64 banks), b1, w2,
// Q [ns][ns | 1], p - 34.7 KB at the limits.  Element i of tau lives in lane i; another lane's element is read from its register
// (v_readlane).  The Taylor model's workgroups walk the points with a grid stride, so the staging is paid once per workgroup, not
// once per four points.
// The Hessian - H ns^2 / 2 multiply-adds a point - is VALU over LDS: w2 act''(z) goes to the wavefront's LDS slice, lane e owns
// entries e, e + 64, ... of the UPPER TRIANGLE (at most 5 of the 300 at ns = 24), sums over the hidden units in ascending order
// from Qs_ij and stores the entry and its mirror image: H is symmetric to the bit.
//
// Bit-equal values.  Every kernel evaluates z through mlp_layer_from_lanes' order (bias first, the elements of tau ascending,
// explicit fmaf) and the activation through mlp_act: a value depends on (nx, nu, H), the activation and the data alone.  The search
// evaluates the candidate and the iterate in the same instruction sequence, so a candidate equal to the iterate has the iterate's
// pre-activations to the bit and the cost difference is exactly 0.
#pragma once
#include "mlp_dx_kernels.hpp"
#include "mlp_cost_launch.hpp"     // MlpCostModel, MlpCostApproxArgs

namespace dmpc {

constexpr int kCostMaxNs = kMlpMaxNx + kMlpMaxNu;
constexpr int kCostMaxH = mlp_max_hidden(1);
constexpr int kCostUnits = mlp_units(1);                       // hidden units per lane, at most
constexpr int kCostApproxWaveFloats = 2 * kCostMaxH;           // the Taylor model's slice: w2 act''(z) and g0's weights
constexpr int kCostGradCap = 256;                              // partials at most: 7.4 MB at the largest model

// THE byte count of a launch's dynamic LDS
constexpr size_t mlp_cost_lds_bytes(int nx, int nu, int H, int wave_floats) {
  const int ns = nx + nu;
  return (size_t)(H * (ns | 1) + 2 * H + ns * (ns | 1) + ns + kMlpWaves * wave_floats) * sizeof(float);
}
static_assert(mlp_cost_lds_bytes(16, 8, 256, kCostApproxWaveFloats) == 38336, "the Taylor model at every limit");
static_assert(mlp_cost_lds_bytes(16, 8, 256, kCostApproxWaveFloats) <= 64 * 1024, "no launch raises the dynamic LDS limit");

__host__ __device__ inline int mlp_cost_grad_partials(long long points) { return points < kCostGradCap ? (int)points : kCostGradCap; }
__host__ __device__ inline int mlp_cost_grad_partial_floats(int ns, int H) { return ns * ns + ns + H * ns + 2 * H; }

struct MlpCostLds {
  int ld, ldq;                     // row strides of W1 and Q
  float *W1, *b1, *w2, *Q, *p, *wave;
};

// every thread of the workgroup takes part, also those of wavefronts without a point; ends with the one barrier
__device__ __forceinline__ MlpCostLds mlp_cost_stage(const MlpCostModel &m, float *lds, const int wave_floats) {
  const int ns = m.nx + m.nu, H = m.H;
  MlpCostLds L;
  L.ld = ns | 1;
  L.ldq = ns | 1;
  L.W1 = lds;
  L.b1 = L.W1 + H * L.ld;
  L.w2 = L.b1 + H;
  L.Q = L.w2 + H;
  L.p = L.Q + ns * L.ldq;
  L.wave = L.p + ns + (threadIdx.x / 64) * wave_floats;
  mlp_stage_layer(L.W1, L.ld, L.b1, m.W1, m.b1, H, ns);
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int e = tid; e < H; e += nt) L.w2[e] = m.w2[e];
  if (m.Q != nullptr) mlp_stage_layer(L.Q, L.ldq, L.p, m.Q, m.p, ns, ns);
  __syncthreads();
  return L;
}

// mlp_act with the second derivative: a and d1 are mlp_act's own values
template <int ACT>
__device__ __forceinline__ void mlp_act2(const float z, float &a, float &d1, float &d2) {
  mlp_act<ACT>(z, a, d1);
  if constexpr (ACT == kMlpActTanh) {
    d2 = -2.0f * a * d1;
  } else if constexpr (ACT == kMlpActRelu) {
    d2 = 0.f;
  } else if constexpr (ACT == kMlpActSilu) {
    const float s = 1.0f / (1.0f + expf(-z));
    d2 = s * (1.0f - s) * (2.0f + z * (1.0f - 2.0f * s));
  } else {
    d2 = d1 * (1.0f - d1);
  }
}

// element `lane` of [x;u] at point pt (0 in lanes >= ns)
__device__ __forceinline__ float mlp_cost_tau(const float *x, const float *u, const size_t pt, const int lane, const int nx, const int nu) {
  return lane < nx ? x[pt * nx + lane] : (lane < nx + nu ? u[pt * nu + (lane - nx)] : 0.f);
}

// ---- the Taylor model (MlpCostApproxArgs: mlp_cost_launch.hpp)
// One point's model, by the whole wavefront: the value to costs[pt], g0 to g_out[pt], H to H_out[pt] (costs or the pair may be
// nullptr).  x, u, H_out, g_out, costs are the arrays' bases.  sw is the wavefront's slice of kCostApproxWaveFloats floats;
// the two fences order this point's stores to it behind the previous point's reads and in front of this point's.  Both
// callers - the Taylor model's kernel and the search's epilogue - get their bits from this one instruction sequence.
template <int ACT>
__device__ __forceinline__ void mlp_cost_taylor_point(const MlpCostLds &L, const MlpUnits<kCostUnits> &U, const int nx, const int nu,
                                                      const int H, const int lane, float *sw, const float *x, const float *u,
                                                      const size_t pt, float *H_out, float *g_out, float *costs) {
  const int ns = nx + nu;
  const int lt = lane < ns ? lane : 0;
  float *rw = sw + kCostMaxH;
  const float tau = mlp_cost_tau(x, u, pt, lane, nx, nu);
  float z[kCostUnits], sk[kCostUnits], rk[kCostUnits];
  mlp_layer_from_lanes(L.W1, L.ld, L.b1, U, ns, tau, z);
  float net = 0.f;
#pragma unroll
  for (int k = 0; k < kCostUnits; ++k) {
    const bool live = U.live(k);
    float ak, d1, d2;
    mlp_act2<ACT>(z[k], ak, d1, d2);
    const float w = live ? L.w2[U.row[k]] : 0.f;
    net = fmaf(w, live ? ak : 0.f, net);
    const float y = z[k] - (live ? L.b1[U.row[k]] : 0.f);      // (W1 tau) of this unit
    sk[k] = live ? w * d2 : 0.f;
    rk[k] = live ? w * fmaf(-d2, y, d1) : 0.f;
  }
  float q = 0.f;
  for (int j = 0; j < ns; ++j) q = fmaf(L.Q[lt * L.ldq + j], lane_value(tau, j), q);
  const float part = lane < ns ? cost_row(tau, q, L.p[lt]) : 0.f;
  const float cost = wave_sum64(part + net);
  if (costs != nullptr && lane == 0) costs[pt] = cost;
  if (H_out == nullptr) return;

  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the previous point's reads of the slice are done)
#pragma unroll
  for (int k = 0; k < kCostUnits; ++k) {
    if (U.live(k)) {
      sw[lane + 64 * k] = sk[k];
      rw[lane + 64 * k] = rk[k];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  float gj = L.p[lt];
#pragma unroll 4
  for (int h = 0; h < H; ++h) gj = fmaf(L.W1[h * L.ld + lt], rw[h], gj);
  if (lane < ns) g_out[pt * ns + lane] = gj;
  float *Hp = H_out + pt * ns * ns;
  const int ntri = ns * (ns + 1) / 2;
  for (int e = lane; e < ntri; e += 64) {
    int i = 0, r = e;
    while (r >= ns - i) {
      r -= ns - i;
      ++i;
    }
    const int j = i + r;
    float acc = 0.5f * (L.Q[i * L.ldq + j] + L.Q[j * L.ldq + i]);
#pragma unroll 4
    for (int h = 0; h < H; ++h) acc = fmaf(L.W1[h * L.ld + i] * sw[h], L.W1[h * L.ld + j], acc);
    Hp[i * ns + j] = acc;
    Hp[j * ns + i] = acc;
  }
}

// In a box-DDP chain: a.clear runs first - thread g of the grid zeroes word g of each range - and a set `done` flag ends the
// launch before its barrier.
template <int ACT>
__global__ __launch_bounds__(64 * kMlpWaves) void mlp_cost_approx_kernel(const MlpCostApproxArgs a) {
  extern __shared__ float lds[];
  a.clear.run(blockIdx.x * blockDim.x + threadIdx.x);
  if (a.done != nullptr && *a.done != 0) return;   // grid-uniform, before the barrier: the iLQR loop has stopped
  const MlpCostLds L = mlp_cost_stage(a.m, lds, kCostApproxWaveFloats);
  const int lane = threadIdx.x % 64;
  const int nx = a.m.nx, nu = a.m.nu, H = a.m.H;
  const MlpUnits<kCostUnits> U(lane, H);
  const long long stride = (long long)gridDim.x * kMlpWaves;
  for (long long pt = (long long)blockIdx.x * kMlpWaves + threadIdx.x / 64; pt < a.P; pt += stride)   // wave-uniform
    mlp_cost_taylor_point<ACT>(L, U, nx, nu, H, lane, L.wave, a.x, a.u, (size_t)pt, a.H_out, a.g_out, a.costs);
}

// ---- the line search.  a.C, a.c are not read; a.F [T-1,B,nx,ns] and a.f [T-1,B,nx] (or nullptr) are the dense LinDx.
// H_next [T,B,ns,ns], g_next [T,B,ns] (BoxDDP's chain; both or neither): the accepted trajectory IS the next iteration's nominal
// one, so after the search the wavefront walks its T points once more and stores their Taylor model through
// mlp_cost_taylor_point - bit for bit what mlp_cost_approx_kernel writes for a.x, a.u.  Every lane re-reads only what it stored
// itself (x element `lane`, control `lane - nx`), so program order is enough.  The launch then stages the wavefront slices
// (kCostApproxWaveFloats each); without the pair it stages none.  A set a.done ends the launch before its barrier.
template <int ACT>
__global__ __launch_bounds__(64 * kMlpWaves) void mpc_forward_rec_mlp_cost_kernel(const MpcFwdArgs a, const MlpCostModel m,
                                                                                  float *H_next, float *g_next) {
  extern __shared__ float lds[];
  if (a.done != nullptr && *a.done != 0) return;   // grid-uniform, before the barrier: the iLQR loop has stopped
  const MlpCostLds L = mlp_cost_stage(m, lds, H_next != nullptr ? kCostApproxWaveFloats : 0);
  const int lane = threadIdx.x % 64;
  const int b = blockIdx.x * kMlpWaves + threadIdx.x / 64;
  if (b >= a.B) return;      // (after the only barrier)
  const int nx = m.nx, nu = m.nu, ns = nx + nu;
  const int T = a.T;
  const size_t B = (size_t)a.B;
  const bool is_x = lane < nx, is_u = lane >= nx && lane < ns;
  const int mu = is_u ? lane - nx : 0;          // this lane's control (clamped for the others' addresses)
  const int lx = is_x ? lane : 0;
  const int lt = lane < ns ? lane : 0;
  const MlpUnits<kCostUnits> U(lane, m.H);

  float cost = 0.f, old_cost = 0.f;
  LineSearch ls;
  while (ls.searching(a.ls_cap)) {
    const float alpha = ls.alpha;
    const bool first = ls.n_pass == 0;
    float xc = is_x ? a.states[(size_t)b * nx + lane] : 0.f;                             // :198
    cost = 0.f;
    float delta = 0.f;   // current_cost - OLD_COST, per timestep and without cancellation (line_search.hpp)
    for (int t = 0; t < T; ++t) {
      const size_t tb = (size_t)t * B + b;
      const float x0 = a.states[tb * nx + lx];
      const float dx = is_x ? xc - x0 : 0.f;
      const float u0 = a.controls[tb * nu + mu];
      const float *Kr = a.Ks + (tb * nu + mu) * nx;
      float v = alpha * a.ks[tb * nu + mu];
      for (int i = 0; i < nx; ++i) v = fmaf(Kr[i], lane_value(dx, i), v);
      v += u0;                                                                           // :209-219
      v = box_clamp(v, a.lower[tb * nu + mu], a.upper[tb * nu + mu]);
      const float tau = is_x ? xc : (is_u ? v : 0.f);
      const float tau0 = is_x ? x0 : (is_u ? u0 : 0.f);
      if (is_u) {
        a.u[tb * nu + mu] = v;
        if (a.u_first != nullptr && first) a.u_first[tb * nu + mu] = v;                  // :260-263
      }
      if (is_x) a.x[tb * nx + lane] = xc;
      // the quadratic part: cost_row / cost_row_diff with the stationary Q, p
      float part = 0.f, part0 = 0.f, partd = 0.f;
      {
        const float *Qr = L.Q + lt * L.ldq;
        float qi = 0.f, q0 = 0.f, qd = 0.f;
        for (int j = 0; j < ns; ++j) {
          const float cij = Qr[j];
          const float tj = lane_value(tau, j), t0j = lane_value(tau0, j);
          qi = fmaf(cij, tj, qi);
          q0 = fmaf(cij, t0j, q0);
          qd = fmaf(cij, tj - t0j, qd);
        }
        const float ci = L.p[lt];
        if (lane < ns) {
          part = cost_row(tau, qi, ci);
          part0 = cost_row(tau0, q0, ci);
          partd = cost_row_diff(tau - tau0, qi, ci, tau0, qd);
        }
      }
      // the network part: the candidate and the iterate through ONE instruction sequence; sum_h w2_h (act(z'_h) - act(z0_h))
      {
        float z1[kCostUnits], z0[kCostUnits];
        mlp_bias(L.b1, U, z1);
        mlp_bias(L.b1, U, z0);
        for (int j = 0; j < ns; ++j) {
          const float tj = lane_value(tau, j), t0j = lane_value(tau0, j);
#pragma unroll
          for (int k = 0; k < kCostUnits; ++k) {
            if (k < U.n) {
              const float w = U.has[k] ? L.W1[U.row[k] * L.ld + j] : 0.f;
              z1[k] = fmaf(w, tj, z1[k]);
              z0[k] = fmaf(w, t0j, z0[k]);
            }
          }
        }
#pragma unroll
        for (int k = 0; k < kCostUnits; ++k) {
          const bool live = U.live(k);
          float a1, a0, unused;
          mlp_act<ACT>(z1[k], a1, unused);
          mlp_act<ACT>(z0[k], a0, unused);
          a1 = live ? a1 : 0.f;
          a0 = live ? a0 : 0.f;
          const float w = live ? L.w2[U.row[k]] : 0.f;
          part = fmaf(w, a1, part);
          part0 = fmaf(w, a0, part0);
          partd = fmaf(w, a1 - a0, partd);
        }
      }
      const float obj = wave_sum64(part);
      cost += obj;
      delta += wave_sum64(partd);
      if (first) old_cost += wave_sum64(part0);                                          // :191
      if (a.objs != nullptr && lane == 0) a.objs[tb] = obj;
      if (t < T - 1) {                                                                   // :229-236
        const float *Fr = a.F + (tb * nx + lx) * ns;
        float xn = a.f != nullptr ? a.f[tb * nx + lx] : 0.f;
        for (int j = 0; j < ns; ++j) xn = fmaf(Fr[j], lane_value(tau, j), xn);
        xc = is_x ? xn : 0.f;
      }
    }
    ls.advance(delta, a.ls_decay);
  }
  if (ls.worse) ls.alpha = cap_alpha_sequential(ls.alpha, a.ls_decay);
  if (lane == 0) search_store<false, false>(a, b, cost, old_cost, ls.alpha, ls.n_pass, search_flags(ls.worse, cost));
  if (H_next != nullptr) {
    // the last pass is the accepted one: its states and controls are in a.x, a.u
    for (int t = 0; t < T; ++t)
      mlp_cost_taylor_point<ACT>(L, U, nx, nu, m.H, lane, L.wave, a.x, a.u, (size_t)t * B + b, H_next, g_next, nullptr);
  }
}

// ---- the parameter gradient.  With v = dL/dg0, r = dL/dcosts at a point, q = W1 v, A = w2 act'(z), Bq = w2 act''(z) q:
//     dQ  += 1/2 (tau w' + w tau'),  w = v + r/2 tau        (= 1/2 (v tau' + tau v') + 1/2 r tau tau')
//     dp  += v + r tau
//     dW1 += A (v + r tau)' + Bq tau'       db1 += Bq + r A       dw2 += act'(z) q + r act(z)
// Wavefront g of G = mlp_cost_grad_partials(P) walks the points g, g + G, ... in ascending order with every sum in registers (a
// lane: its four hidden units' rows of dW1, 96 sums at ns = 24; entries lane, lane + 64, ... of dQ; element lane of dp) and
// stores ONE partial [dQ | dp | dW1 | db1 | dw2] at part + g * mlp_cost_grad_partial_floats.
struct MlpCostGradArgs {
  long long P;
  int G;
  MlpCostModel m;                  // (Q, p: nullptr - the gradient reads neither)
  const float *x, *u;              // [P,nx], [P,nu]
  const float *gg, *gc;            // dL/dg0 [P,ns] or nullptr, dL/dcosts [P] or nullptr
  float *part;                     // [G][partial floats]
};

template <int ACT>
__global__ __launch_bounds__(64 * kMlpWaves) void mlp_cost_param_grad_kernel(const MlpCostGradArgs a) {
  extern __shared__ float lds[];
  const MlpCostLds L = mlp_cost_stage(a.m, lds, 0);
  const int lane = threadIdx.x % 64;
  const int g = blockIdx.x * kMlpWaves + threadIdx.x / 64;
  if (g >= a.G) return;      // (after the only barrier)
  const int nx = a.m.nx, nu = a.m.nu, ns = nx + nu, H = a.m.H;
  const MlpUnits<kCostUnits> U(lane, H);
  constexpr int QE = (kCostMaxNs * kCostMaxNs + 63) / 64;      // entries of dQ a lane owns, at most
  int qi[QE], qj[QE];
#pragma unroll
  for (int k = 0; k < QE; ++k) {
    const int e = lane + 64 * k, ec = e < ns * ns ? e : ns * ns - 1;
    qi[k] = ec / ns;
    qj[k] = ec % ns;
  }
  float dW1[kCostUnits][kCostMaxNs], db1[kCostUnits], dw2[kCostUnits], dQ[QE], dp = 0.f;
#pragma unroll
  for (int k = 0; k < kCostUnits; ++k) {
    db1[k] = dw2[k] = 0.f;
#pragma unroll
    for (int j = 0; j < kCostMaxNs; ++j) dW1[k][j] = 0.f;
  }
#pragma unroll
  for (int k = 0; k < QE; ++k) dQ[k] = 0.f;

  for (long long pt = g; pt < a.P; pt += a.G) {                 // wave-uniform
    const float tau = mlp_cost_tau(a.x, a.u, (size_t)pt, lane, nx, nu);
    const float v = (a.gg != nullptr && lane < ns) ? a.gg[(size_t)pt * ns + lane] : 0.f;
    const float r = a.gc != nullptr ? a.gc[pt] : 0.f;
    float z[kCostUnits], q[kCostUnits], Ak[kCostUnits], Bk[kCostUnits];
    mlp_bias(L.b1, U, z);
#pragma unroll
    for (int k = 0; k < kCostUnits; ++k) q[k] = 0.f;
    for (int j = 0; j < ns; ++j) {
      const float tj = lane_value(tau, j), vj = lane_value(v, j);
#pragma unroll
      for (int k = 0; k < kCostUnits; ++k) {
        if (k < U.n) {
          const float w = U.has[k] ? L.W1[U.row[k] * L.ld + j] : 0.f;
          z[k] = fmaf(w, tj, z[k]);
          q[k] = fmaf(w, vj, q[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kCostUnits; ++k) {
      const bool live = U.live(k);
      float ak, d1, d2;
      mlp_act2<ACT>(z[k], ak, d1, d2);
      const float w = live ? L.w2[U.row[k]] : 0.f;
      Ak[k] = live ? w * d1 : 0.f;
      Bk[k] = live ? w * d2 * q[k] : 0.f;
      db1[k] += fmaf(r, Ak[k], Bk[k]);
      dw2[k] += live ? fmaf(d1, q[k], r * ak) : 0.f;
    }
    const float vr = fmaf(r, tau, v);
    dp += vr;
#pragma unroll
    for (int j = 0; j < kCostMaxNs; ++j) {
      if (j < ns) {                                             // wave-uniform
        const float vj = lane_value(vr, j), tj = lane_value(tau, j);
#pragma unroll
        for (int k = 0; k < kCostUnits; ++k) dW1[k][j] = fmaf(Ak[k], vj, fmaf(Bk[k], tj, dW1[k][j]));
      }
    }
    const float wq = fmaf(0.5f * r, tau, v);
#pragma unroll
    for (int k = 0; k < QE; ++k) {
      if (64 * k < ns * ns) {                                   // wave-uniform: every lane shuffles, on clamped indices
        const float ti = __shfl(tau, qi[k]), tj = __shfl(tau, qj[k]), wi = __shfl(wq, qi[k]), wj = __shfl(wq, qj[k]);
        const float add = 0.5f * fmaf(ti, wj, wi * tj);
        dQ[k] += lane + 64 * k < ns * ns ? add : 0.f;
      }
    }
  }

  float *part = a.part + (size_t)g * mlp_cost_grad_partial_floats(ns, H);
#pragma unroll
  for (int k = 0; k < QE; ++k)
    if (lane + 64 * k < ns * ns) part[lane + 64 * k] = dQ[k];
  if (lane < ns) part[ns * ns + lane] = dp;
  float *pW = part + ns * ns + ns, *pb = pW + H * ns, *pw = pb + H;
#pragma unroll
  for (int k = 0; k < kCostUnits; ++k) {
    const int h = lane + 64 * k;
    if (h < H) {
#pragma unroll
      for (int j = 0; j < kCostMaxNs; ++j)
        if (j < ns) pW[h * ns + j] = dW1[k][j];
      pb[h] = db1[k];
      pw[h] = dw2[k];
    }
  }
}

// The reduction: one thread per parameter element adds the G partials in ascending order.  (MlpGradReduceArgs has four outputs;
// this gradient has five.)
struct MlpCostGradReduceArgs {
  int G, nQ, np, nW, nH;           // ns^2, ns, H ns, H
  const float *part;
  float *dQ, *dp, *dW1, *db1, *dw2;
};

__global__ __launch_bounds__(256) void mlp_cost_param_grad_reduce_kernel(const MlpCostGradReduceArgs a) {
  const int P = a.nQ + a.np + a.nW + 2 * a.nH;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P) return;
  float s = 0.f;
#pragma unroll 8
  for (int g = 0; g < a.G; ++g) s += a.part[(size_t)g * P + e];
  if (e < a.nQ) a.dQ[e] = s;
  else if (e < a.nQ + a.np) a.dp[e - a.nQ] = s;
  else if (e < a.nQ + a.np + a.nW) a.dW1[e - a.nQ - a.np] = s;
  else if (e < a.nQ + a.np + a.nW + a.nH) a.db1[e - a.nQ - a.np - a.nW] = s;
  else a.dw2[e - a.nQ - a.np - a.nW - a.nH] = s;
}

}  // namespace dmpc
