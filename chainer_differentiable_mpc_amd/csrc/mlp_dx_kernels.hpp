// mlp_dx_kernels.hpp - a learned one-hidden-layer dynamics model on the device (MlpDx of the Python layer):
//
//     next(x, u) = W2 act(W1 [x;u] + b1) + b2 (+ x when residual),     act = tanh
//
//   mlp_rollout_linearize_kernel   get_traj + linearize_dynamics (util.py:239-277, mpc/approximate.py:77-119) in one
//                                  launch: x_{t+1} = next(x_t, u_t), F_t = [I|0] residual + W2 diag(1 - a^2) W1,
//                                  f_t = next - F_t [x_t;u_t].
//   mpc_forward_rec_mlp_kernel     MPCstep.forward_rec (mpc/mpc_step.py:175-286) with the network as the TRUE dynamics:
//                                  the clamped closed-loop rollout and per-trajectory line search of
//                                  mpc_generic_forward_kernel, the dynamics evaluated in place of F tau + f.
//
// Layout.  Runtime dimensions (nx <= 16, nu <= 8, 1 <= H <= 256), ONE wavefront per trajectory, four per workgroup.
// The weights are staged into LDS once per workgroup and shared by its wavefronts:
//     W1s [H][ns | 1]   lane l owns hidden units l, l + 64, ...: it walks ITS row, and the odd stride puts the 64 rows a
//                       wavefront reads at once on 64 different banks
//     W2s [nx][H | 1]   lanes read consecutive units of a row (no conflict); the odd stride separates the rows that the
//                       Jacobian's lanes read at once
//     b1s [H], b2s [nx]
// 25.6 + 16.4 + 1.1 KB at the largest size.  Behind them every wavefront has 672 floats of its own (1 - a^2 per hidden
// unit, the step's Jacobian).  Element i of tau = [x;u] lives in lane i; a value another lane needs is read from that
// lane's register (v_readlane), never through LDS, so the search needs no barrier after the staging one and its
// wavefronts leave the loop one by one.
//
// Bit-equal dynamics.  The search ends when a candidate collapses onto the nominal trajectory and its cost difference is
// exactly 0 (see PendulumModel in mpc_kernels.hpp).  Both kernels evaluate the network through mlp_next alone: explicit
// fmaf, inputs in ascending order, a lane's hidden units in ascending order, one butterfly reduction per output - an
// order that depends on (nx, nu, H) and on nothing else: not on B, the grid, or the wavefront's slot in its workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
// bound_tol, is_finite, wave_sum64 and MpcFwdArgs come from the MPC step's headers.  Those headers also define the
// non-template kernels of mpc_api.hip's translation unit; here their functions get internal linkage, so this translation
// unit neither defines those kernels a second time nor emits the ones it does not launch.
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "mpc_generic.hpp"
#pragma clang attribute pop

namespace dmpc {

constexpr int kMlpMaxNx = 16, kMlpMaxNu = 8, kMlpMaxHidden = 256;
constexpr int kMlpWaves = 4;                                 // trajectories (wavefronts) per workgroup
constexpr int kMlpUnits = kMlpMaxHidden / 64;                // hidden units per lane, at most
constexpr int kMlpWaveFloats = kMlpMaxHidden + kMlpMaxNx * (kMlpMaxNx + kMlpMaxNu) + 32;

struct MlpModel {
  int nx, nu, n_hidden, residual;
  const float *W1, *b1, *W2, *b2;   // [H,ns], [H], [nx,H], [nx]  (device pointers: an optimiser step is seen by the next launch)
};

struct MlpLds {
  int nsp, hp;                      // row strides of W1s and W2s
  float *W1s, *W2s, *b1s, *b2s, *wave;
};
__host__ __device__ inline int mlp_lds_floats(int nx, int nu, int H) {
  return H * ((nx + nu) | 1) + nx * (H | 1) + H + nx;
}
inline size_t mlp_lds_bytes(int nx, int nu, int H) {
  return (size_t)(mlp_lds_floats(nx, nu, H) + kMlpWaves * kMlpWaveFloats) * sizeof(float);
}

__device__ __forceinline__ float lane_value(float v, int l) {   // l is wave-uniform
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// THE activation (act 0 of the C ABI)
__device__ __forceinline__ float mlp_act(float z) { return tanhf(z); }

// every thread of the workgroup takes part, also those of wavefronts without a trajectory; ends with the one barrier
__device__ __forceinline__ MlpLds mlp_stage(const MlpModel &m, float *lds) {
  const int ns = m.nx + m.nu, H = m.n_hidden;
  MlpLds L;
  L.nsp = ns | 1;
  L.hp = H | 1;
  L.W1s = lds;
  L.W2s = L.W1s + H * L.nsp;
  L.b1s = L.W2s + m.nx * L.hp;
  L.b2s = L.b1s + H;
  L.wave = L.b2s + m.nx + (threadIdx.x / 64) * kMlpWaveFloats;
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int e = tid; e < H * ns; e += nt) L.W1s[(e / ns) * L.nsp + (e % ns)] = m.W1[e];
  for (int e = tid; e < m.nx * H; e += nt) L.W2s[(e / H) * L.hp + (e % H)] = m.W2[e];
  for (int e = tid; e < H; e += nt) L.b1s[e] = m.b1[e];
  for (int e = tid; e < m.nx; e += nt) L.b2s[e] = m.b2[e];
  __syncthreads();
  return L;
}

// ONE step of the model.  tau: element `lane` of [x;u] (anything in lanes >= ns: never read).  Returns element `lane` of the
// next state (0 in lanes >= nx) and leaves this lane's activations in a[] - 0 for units beyond H, which therefore add exact
// zeros to every sum and whose LDS addresses are clamped into range.
__device__ __forceinline__ float mlp_next(const MlpModel &m, const MlpLds &L, const int lane, const float tau,
                                          float (&a)[kMlpUnits]) {
  const int ns = m.nx + m.nu, H = m.n_hidden;
  const int n_units = (H + 63) / 64;
  int row[kMlpUnits];
  bool has[kMlpUnits];
  float z[kMlpUnits];
#pragma unroll
  for (int k = 0; k < kMlpUnits; ++k) {
    const int h = lane + 64 * k;
    has[k] = h < H;
    row[k] = has[k] ? h : H - 1;
    z[k] = has[k] ? L.b1s[row[k]] : 0.f;
  }
  for (int j = 0; j < ns; ++j) {
    const float tj = lane_value(tau, j);
#pragma unroll
    for (int k = 0; k < kMlpUnits; ++k) {
      if (k < n_units) {
        const float w = L.W1s[row[k] * L.nsp + j];
        z[k] = fmaf(has[k] ? w : 0.f, tj, z[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kMlpUnits; ++k) a[k] = (k < n_units && has[k]) ? mlp_act(z[k]) : 0.f;
  float next = 0.f;
  for (int i = 0; i < m.nx; ++i) {
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < kMlpUnits; ++k) {
      if (k < n_units) {
        const float w = L.W2s[i * L.hp + row[k]];
        part = fmaf(has[k] ? w : 0.f, a[k], part);
      }
    }
    float s = wave_sum64(part) + L.b2s[i];
    if (m.residual) s += lane_value(tau, i);
    next = lane == i ? s : next;
  }
  return next;
}

// F = d next / d [x;u] (nx x ns, row-major) at Fp and into the wavefront's LDS, f = next - F tau at fq (lanes < nx).
// VALU over LDS: 1 - a^2 of every hidden unit goes to the wavefront's scratch, then lane e owns entries e, e + 64, ... of F
// and sums over the hidden units in ascending order.  Within one wavefront LDS operations complete in program order; the
// fences keep the compiler from moving a read above the write it depends on.
__device__ __forceinline__ void mlp_jacobian_store(const MlpModel &m, const MlpLds &L, const int lane, const float tau,
                                                   const float next, const float (&a)[kMlpUnits], float *Fp, float *fq) {
  const int nx = m.nx, ns = m.nx + m.nu, H = m.n_hidden;
  float *g = L.wave, *Fs = L.wave + kMlpMaxHidden;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the previous step's reads of g and Fs are done)
#pragma unroll
  for (int k = 0; k < kMlpUnits; ++k) {
    const int h = lane + 64 * k;
    if (h < H) g[h] = fmaf(-a[k], a[k], 1.0f);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  for (int e = lane; e < nx * ns; e += 64) {
    const int i = e / ns, j = e % ns;
    const float *w2 = L.W2s + i * L.hp, *w1 = L.W1s + j;
    float acc = (m.residual && i == j) ? 1.f : 0.f;
#pragma unroll 4
    for (int h = 0; h < H; ++h) acc = fmaf(w2[h] * g[h], w1[h * L.nsp], acc);
    Fs[e] = acc;
    Fp[e] = acc;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const int r = lane < nx ? lane : 0;
  float f = next;
  for (int j = 0; j < ns; ++j) f = fmaf(-Fs[r * ns + j], lane_value(tau, j), f);
  if (fq != nullptr && lane < nx) fq[lane] = f;
}

struct MlpRolloutArgs {
  int T, B;
  MlpModel m;
  const float *x_init, *u;   // [B,nx], [T,B,nu]
  float *x, *F, *f;          // [T,B,nx]; [T-1,B,nx,ns] or nullptr; [T-1,B,nx] or nullptr
};

__global__ __launch_bounds__(64 * kMlpWaves) void mlp_rollout_linearize_kernel(const MlpRolloutArgs a) {
  extern __shared__ float lds[];
  const MlpLds L = mlp_stage(a.m, lds);
  const int lane = threadIdx.x % 64;
  const int b = blockIdx.x * kMlpWaves + threadIdx.x / 64;
  if (b >= a.B) return;      // (after the only barrier) a wavefront without a trajectory stores nothing
  const int nx = a.m.nx, nu = a.m.nu, ns = nx + nu;
  const int T = a.T;
  const size_t B = (size_t)a.B;
  float xc = lane < nx ? a.x_init[(size_t)b * nx + lane] : 0.f;
  for (int t = 0; t < T; ++t) {
    const size_t tb = (size_t)t * B + b;
    if (lane < nx) a.x[tb * nx + lane] = xc;
    if (t == T - 1) break;
    const float tau = lane < nx ? xc : (lane < ns ? a.u[tb * nu + (lane - nx)] : 0.f);
    float act[kMlpUnits];
    const float xn = mlp_next(a.m, L, lane, tau, act);
    if (a.F != nullptr) mlp_jacobian_store(a.m, L, lane, tau, xn, act, a.F + tb * nx * ns, a.f ? a.f + tb * nx : nullptr);
    xc = xn;
  }
}

// forward_rec: the arithmetic of a pass, its order and the search's decisions are mpc_generic_forward_kernel's (and
// through it mpc_forward_rec_kernel's): the cost difference per timestep without cancellation, bound_tol's snap, the
// pass cap.  a.F / a.f are not read.  The loop is wave-uniform by construction - a wavefront is one trajectory - so a
// trajectory that has finished runs, stores and commits nothing more.
__global__ __launch_bounds__(64 * kMlpWaves) void mpc_forward_rec_mlp_kernel(const MpcFwdArgs a, const MlpModel m) {
  extern __shared__ float lds[];
  const MlpLds L = mlp_stage(m, lds);
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

  float alpha = 1.0f, cost = 0.f, old_cost = 0.f;
  int n_pass = 0;
  bool worse = true;
  while (worse && n_pass < a.ls_cap) {                                                   // mpc_step.py:196
    float xc = is_x ? a.states[(size_t)b * nx + lane] : 0.f;                             // :198
    cost = 0.f;
    float delta = 0.f;   // current_cost - OLD_COST, per timestep and without cancellation (see mpc_forward_rec_kernel)
    for (int t = 0; t < T; ++t) {
      const size_t tb = (size_t)t * B + b;
      const float x0 = a.states[tb * nx + lx];
      const float dx = is_x ? xc - x0 : 0.f;
      const float u0 = a.controls[tb * nu + mu];
      const float *Kr = a.Ks + (tb * nu + mu) * nx;
      float v = alpha * a.ks[tb * nu + mu];
      for (int i = 0; i < nx; ++i) v = fmaf(Kr[i], lane_value(dx, i), v);
      v += u0;                                                                           // :209-219
      const float lb = a.lower[tb * nu + mu], ub = a.upper[tb * nu + mu];
      v = fminf(fmaxf(v, lb), ub);                                                       // :221
      v = (v - lb <= bound_tol(lb)) ? lb : v;
      v = (ub - v <= bound_tol(ub)) ? ub : v;
      const float tau = is_x ? xc : (is_u ? v : 0.f);
      const float tau0 = is_x ? x0 : (is_u ? u0 : 0.f);
      if (is_u) {
        a.u[tb * nu + mu] = v;
        if (a.u_first != nullptr && n_pass == 0) a.u_first[tb * nu + mu] = v;            // :260-263
      }
      if (is_x) a.x[tb * nx + lane] = xc;
      float part = 0.f, part0 = 0.f, partd = 0.f;                                        // :246-251, util.py:162-198
      {
        const float *Cr = a.C + (tb * ns + lt) * ns;
        float qi = 0.f, q0 = 0.f, qd = 0.f;
        for (int j = 0; j < ns; ++j) {
          const float cij = Cr[j];
          const float tj = lane_value(tau, j), t0j = lane_value(tau0, j);
          qi = fmaf(cij, tj, qi);
          q0 = fmaf(cij, t0j, q0);
          qd = fmaf(cij, tj - t0j, qd);
        }
        const float ci = a.c[tb * ns + lt];
        const float di = tau - tau0;
        if (lane < ns) {
          part = tau * fmaf(0.5f, qi, ci);
          part0 = tau0 * fmaf(0.5f, q0, ci);
          partd = fmaf(di, fmaf(0.5f, qi, ci), 0.5f * tau0 * qd);
        }
      }
      const float obj = wave_sum64(part);
      cost += obj;
      delta += wave_sum64(partd);
      if (n_pass == 0) old_cost += wave_sum64(part0);                                    // :191
      if (a.objs != nullptr && lane == 0) a.objs[tb] = obj;
      if (t < T - 1) {                                                                   // :237-240
        float act[kMlpUnits];
        xc = mlp_next(m, L, lane, tau, act);
      }
    }
    ++n_pass;
    worse = delta > 0.f;                 // :266  current_cost > OLD_COST
    if (worse) alpha *= a.ls_decay;      // :268
  }
  int info_bits = 0;
  if (worse) {                           // cap hit: the reference would still be looping; :274
    alpha /= a.ls_decay;
    info_bits |= 8;
  }
  if (!is_finite(cost)) info_bits |= 2;
  if (lane == 0) {
    a.costs[b] = cost;
    if (a.old_costs != nullptr) a.old_costs[b] = old_cost;
    a.alphas[b] = alpha;
    a.n_ls[b] = n_pass;
    if (a.info != nullptr && info_bits != 0) atomicOr(&a.info[b], info_bits);
  }
}

}  // namespace dmpc
