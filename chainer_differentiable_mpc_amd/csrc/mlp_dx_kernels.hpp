// mlp_dx_kernels.hpp - a learned dynamics model with one or two hidden layers on the device (MlpDx of the Python layer):
//
//     depth 1:  next(x, u) = W2 act(W1 [x;u] + b1) + b2 (+ x when residual),     act = tanh | relu | silu | softplus
//     depth 2:  next(x, u) = W3 act(W2 act(W1 [x;u] + b1) + b2) + b3 (+ x when residual)
//
// The activation is a template parameter of the three kernels that evaluate the network (mlp_act below is the only place
// where it is looked at): a = act(z) and d = act'(z) of the pre-activation z = W1 [x;u] + b1.  The depth is a second
// template parameter of the rollout and the search (MlpNet<DEPTH> below); the depth-one instances run the functions they
// ran before the second depth existed.  The two-layer network is described behind the one-layer functions ("Depth two").
//
//   mlp_rollout_linearize_kernel   get_traj + linearize_dynamics (util.py:239-277, mpc/approximate.py:77-119) in one
//                                  launch: x_{t+1} = next(x_t, u_t), F_t = [I|0] residual + W2 diag(d) W1,
//                                  f_t = next - F_t [x_t;u_t].
//   mpc_forward_rec_mlp_kernel     MPCstep.forward_rec (mpc/mpc_step.py:175-286) with the network as the TRUE dynamics:
//                                  the clamped closed-loop rollout and per-trajectory line search of
//                                  mpc_generic_forward_kernel, the dynamics evaluated in place of F tau + f.
//   mlp_param_grad_kernel,         the gradient of a loss of the rollout's f with respect to W1, b1, W2, b2: per-wavefront
//   mlp_param_grad_reduce_kernel   sums in registers, then a fixed-order reduction of the partials (at the end of this file).
//
// Layout.  Runtime dimensions (nx <= 16, nu <= 8, 1 <= H <= 256), ONE wavefront per trajectory, four per workgroup.
// The weights are staged into LDS once per workgroup and shared by its wavefronts:
//     W1s [H][ns | 1]   lane l owns hidden units l, l + 64, ...: it walks ITS row, and the odd stride puts the 64 rows a
//                       wavefront reads at once on 64 different banks
//     W2s [nx][H | 1]   lanes read consecutive units of a row (no conflict); the odd stride separates the rows that the
//                       Jacobian's lanes read at once
//     b1s [H], b2s [nx]
// 25.6 + 16.4 + 1.1 KB at the largest size.  Behind them every wavefront has 672 floats of its own (d per hidden
// unit, the step's Jacobian).  Element i of tau = [x;u] lives in lane i; a value another lane needs is read from that
// lane's register (v_readlane), never through LDS, so the search needs no barrier after the staging one and its
// wavefronts leave the loop one by one.
//
// Bit-equal dynamics.  The search ends when a candidate collapses onto the nominal trajectory and its cost difference is
// exactly 0 (see PendulumModel in mpc_kernels.hpp).  Both kernels evaluate the network through mlp_next alone: explicit
// fmaf, inputs in ascending order, a lane's hidden units in ascending order, one butterfly reduction per output - an
// order that depends on (nx, nu, H) and the activation and on nothing else: not on B, the grid, or the wavefront's slot in
// its workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
// line_search.hpp's pieces, is_finite and wave_sum64 come from the MPC step's headers.  Those headers also define the
// non-template kernels of mpc_api.hip's translation unit; here their functions get internal linkage, so this translation
// unit neither defines those kernels a second time nor emits the ones it does not launch.
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "mpc_generic.hpp"
#pragma clang attribute pop
#include "mlp_dx_launch.hpp"      // MlpModel, MlpRolloutArgs

namespace dmpc {

constexpr int kMlpMaxNx = 16, kMlpMaxNu = 8, kMlpMaxHidden = 256;
constexpr int kMlpWaves = 4;                                 // trajectories (wavefronts) per workgroup
constexpr int kMlpUnits = kMlpMaxHidden / 64;                // hidden units per lane, at most
constexpr int kMlpWaveFloats = kMlpMaxHidden + kMlpMaxNx * (kMlpMaxNx + kMlpMaxNu) + 32;

struct MlpLds {
  int nsp, hp;                      // row strides of W1s and W2s
  float *W1s, *W2s, *b1s, *b2s, *wave;
};
__host__ __device__ inline int mlp_lds_floats(int nx, int nu, int H) {
  return H * ((nx + nu) | 1) + nx * (H | 1) + H + nx;
}

// depth two: H1, H2 <= 128, so a lane owns at most two units of either layer
constexpr int kMlp2MaxHidden = 128;
constexpr int kMlp2Units = kMlp2MaxHidden / 64;
// a wavefront's own floats: d1 and d2 per hidden unit, N = W3 D2 W2 with an odd row stride, the step's Jacobian
constexpr int kMlp2WaveFloats = 2 * kMlp2MaxHidden + kMlpMaxNx * (kMlp2MaxHidden | 1) + kMlpMaxNx * (kMlpMaxNx + kMlpMaxNu);
__host__ __device__ inline int mlp2_lds_floats(int nx, int nu, int H1, int H2) {
  return H1 * ((nx + nu) | 1) + H2 * (H1 | 1) + nx * (H2 | 1) + H1 + H2 + nx;
}

// THE byte count of a launch's dynamic LDS, for the launchers and for dmpc_mlp_dx_supported.  H2 = 0: one hidden layer.
// `jacobian`: the launch forms F (depth one always has its slices: its instances are what they were).
inline size_t mlp_lds_bytes(int nx, int nu, int H1, int H2 = 0, bool jacobian = true) {
  if (H2 == 0) return (size_t)(mlp_lds_floats(nx, nu, H1) + kMlpWaves * kMlpWaveFloats) * sizeof(float);
  return (size_t)(mlp2_lds_floats(nx, nu, H1, H2) + (jacobian ? kMlpWaves * kMlp2WaveFloats : 0)) * sizeof(float);
}
constexpr size_t kMlpLdsLimit = 160 * 1024;   // a gfx950 CU's LDS: one workgroup of the largest two-layer model

__device__ __forceinline__ float lane_value(float v, int l) {   // l is wave-uniform
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// the `act` codes of the C ABI (include/dmpc.h; 1 is never assigned)
constexpr int kMlpActTanh = 0, kMlpActRelu = 2, kMlpActSilu = 3, kMlpActSoftplus = 4;

// THE activation: a = act(z) and d = act'(z), the only place a network's nonlinearity is evaluated.  expf / log1pf, not
// the fast intrinsics.  A NaN z gives a NaN a for every activation (relu included: `z <= 0` is false for a NaN), so the
// search's is_finite tests see what they see for tanh.  relu'(0) = 0, torch's convention.
template <int ACT>
__device__ __forceinline__ void mlp_act(const float z, float &a, float &d) {
  static_assert(ACT == kMlpActTanh || ACT == kMlpActRelu || ACT == kMlpActSilu || ACT == kMlpActSoftplus, "activation");
  if constexpr (ACT == kMlpActTanh) {
    a = tanhf(z);
    d = fmaf(-a, a, 1.0f);
  } else if constexpr (ACT == kMlpActRelu) {
    a = z <= 0.f ? 0.f : z;
    d = z > 0.f ? 1.f : 0.f;
  } else if constexpr (ACT == kMlpActSilu) {
    const float s = 1.0f / (1.0f + expf(-z));
    a = z * s;
    d = s * (1.0f + z * (1.0f - s));
  } else {
    a = fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
    d = 1.0f / (1.0f + expf(-z));
  }
}

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
// next state (0 in lanes >= nx) and leaves this lane's activations in a[] and their derivatives in d[] - both 0 for units
// beyond H, which therefore add exact zeros to every sum and whose LDS addresses are clamped into range.  A caller that
// does not read d[] does not pay for it: everything here is inlined.
template <int ACT>
__device__ __forceinline__ float mlp_next(const MlpModel &m, const MlpLds &L, const int lane, const float tau,
                                          float (&a)[kMlpUnits], float (&d)[kMlpUnits]) {
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
  for (int k = 0; k < kMlpUnits; ++k) {
    float ak, dk;
    mlp_act<ACT>(z[k], ak, dk);
    const bool live = k < n_units && has[k];
    a[k] = live ? ak : 0.f;
    d[k] = live ? dk : 0.f;
  }
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
// VALU over LDS: d of every hidden unit goes to the wavefront's scratch, then lane e owns entries e, e + 64, ... of F
// and sums over the hidden units in ascending order.  Within one wavefront LDS operations complete in program order; the
// fences keep the compiler from moving a read above the write it depends on.
__device__ __forceinline__ void mlp_jacobian_store(const MlpModel &m, const MlpLds &L, const int lane, const float tau,
                                                   const float next, const float (&d)[kMlpUnits], float *Fp, float *fq) {
  const int nx = m.nx, ns = m.nx + m.nu, H = m.n_hidden;
  float *g = L.wave, *Fs = L.wave + kMlpMaxHidden;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the previous step's reads of g and Fs are done)
#pragma unroll
  for (int k = 0; k < kMlpUnits; ++k) {
    const int h = lane + 64 * k;
    if (h < H) g[h] = d[k];
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

// ---------------------------------------------------------------------------------------------------- Depth two
// The same layout: one wavefront per trajectory, four per workgroup, the weights staged once and one barrier.
//     W1s [H1][ns | 1]   as above
//     W2s [H2][H1 | 1]   lane l owns units l, l + 64 of layer 2 and walks ITS row: 64 rows on 64 banks
//     W3s [nx][H2 | 1]   as W2s above
//     b1s [H1], b2s [H2], b3s [nx]
// 88.2 KB at the limits (nx 16, nu 8, H1 = H2 = 128).  A launch that forms Jacobians adds kMlp2WaveFloats (10.8 KB) per
// wavefront: 131.5 KB, one workgroup per CU.  A layer-1 activation another lane needs is read from that lane's register
// (v_readlane), so the step function touches no wavefront slice and the search without Jacobians has none.
struct Mlp2Lds {
  int nsp, hp1, hp2;                // row strides of W1s, W2s (and N) and W3s
  float *W1s, *W2s, *W3s, *b1s, *b2s, *b3s, *wave;
};

__device__ __forceinline__ Mlp2Lds mlp2_stage(const MlpModel &m, float *lds) {
  const int ns = m.nx + m.nu, H1 = m.n_hidden, H2 = m.n_hidden2;
  Mlp2Lds L;
  L.nsp = ns | 1;
  L.hp1 = H1 | 1;
  L.hp2 = H2 | 1;
  L.W1s = lds;
  L.W2s = L.W1s + H1 * L.nsp;
  L.W3s = L.W2s + H2 * L.hp1;
  L.b1s = L.W3s + m.nx * L.hp2;
  L.b2s = L.b1s + H1;
  L.b3s = L.b2s + H2;
  L.wave = L.b3s + m.nx + (threadIdx.x / 64) * kMlp2WaveFloats;   // (only a launch that forms Jacobians has it)
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int e = tid; e < H1 * ns; e += nt) L.W1s[(e / ns) * L.nsp + (e % ns)] = m.W1[e];
  for (int e = tid; e < H2 * H1; e += nt) L.W2s[(e / H1) * L.hp1 + (e % H1)] = m.W2[e];
  for (int e = tid; e < m.nx * H2; e += nt) L.W3s[(e / H2) * L.hp2 + (e % H2)] = m.W3[e];
  for (int e = tid; e < H1; e += nt) L.b1s[e] = m.b1[e];
  for (int e = tid; e < H2; e += nt) L.b2s[e] = m.b2[e];
  for (int e = tid; e < m.nx; e += nt) L.b3s[e] = m.b3[e];
  __syncthreads();
  return L;
}

// ONE step of the two-layer model, the only place it is evaluated.  As mlp_next: explicit fmaf; layer-1 inputs ascending,
// layer-2 inputs (the hidden units of layer 1) ascending, a lane's units ascending, one butterfly reduction per output;
// units beyond H1 / H2 hold exact zeros and read clamped addresses.  Leaves this lane's act' of both layers in d1[], d2[].
template <int ACT>
__device__ __forceinline__ float mlp2_next(const MlpModel &m, const Mlp2Lds &L, const int lane, const float tau,
                                           float (&d1)[kMlp2Units], float (&d2)[kMlp2Units]) {
  const int ns = m.nx + m.nu, H1 = m.n_hidden, H2 = m.n_hidden2;
  const int n1 = (H1 + 63) / 64, n2 = (H2 + 63) / 64;
  int row1[kMlp2Units], row2[kMlp2Units];
  bool has1[kMlp2Units], has2[kMlp2Units];
  float z1[kMlp2Units], z2[kMlp2Units], a1[kMlp2Units], a2[kMlp2Units];
#pragma unroll
  for (int k = 0; k < kMlp2Units; ++k) {
    const int h = lane + 64 * k;
    has1[k] = h < H1;
    row1[k] = has1[k] ? h : H1 - 1;
    z1[k] = has1[k] ? L.b1s[row1[k]] : 0.f;
    has2[k] = h < H2;
    row2[k] = has2[k] ? h : H2 - 1;
    z2[k] = has2[k] ? L.b2s[row2[k]] : 0.f;
  }
  for (int j = 0; j < ns; ++j) {
    const float tj = lane_value(tau, j);
#pragma unroll
    for (int k = 0; k < kMlp2Units; ++k) {
      if (k < n1) {
        const float w = L.W1s[row1[k] * L.nsp + j];
        z1[k] = fmaf(has1[k] ? w : 0.f, tj, z1[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kMlp2Units; ++k) {
    float ak, dk;
    mlp_act<ACT>(z1[k], ak, dk);
    const bool live = k < n1 && has1[k];
    a1[k] = live ? ak : 0.f;
    d1[k] = live ? dk : 0.f;
  }
#pragma unroll
  for (int k1 = 0; k1 < kMlp2Units; ++k1) {        // unit h = 64 k1 + l of layer 1 lives in a1[k1] of lane l
    const int left = H1 - 64 * k1, cnt = left < 64 ? left : 64;
    for (int l = 0; l < cnt; ++l) {
      const float ah = lane_value(a1[k1], l);
#pragma unroll
      for (int k = 0; k < kMlp2Units; ++k) {
        if (k < n2) {
          const float w = L.W2s[row2[k] * L.hp1 + 64 * k1 + l];
          z2[k] = fmaf(has2[k] ? w : 0.f, ah, z2[k]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kMlp2Units; ++k) {
    float ak, dk;
    mlp_act<ACT>(z2[k], ak, dk);
    const bool live = k < n2 && has2[k];
    a2[k] = live ? ak : 0.f;
    d2[k] = live ? dk : 0.f;
  }
  float next = 0.f;
  for (int i = 0; i < m.nx; ++i) {
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < kMlp2Units; ++k) {
      if (k < n2) {
        const float w = L.W3s[i * L.hp2 + row2[k]];
        part = fmaf(has2[k] ? w : 0.f, a2[k], part);
      }
    }
    float s = wave_sum64(part) + L.b3s[i];
    if (m.residual) s += lane_value(tau, i);
    next = lane == i ? s : next;
  }
  return next;
}

// F = [I|0] residual + W3 D2 W2 D1 W1 at Fp, f = next - F tau at fq (lanes < nx).  VALU over LDS, in two products through the
// wavefront's slice, every sum over hidden units ascending:
//   N = W3 D2 W2 (nx x H1): a lane owns columns lane, lane + 64 and takes the rows four at a time - per unit of layer 2 one
//       d2, the lane's two W2 entries (consecutive lanes, consecutive words) and four W3 entries (one word for the wavefront)
//       feed eight fused multiply-adds;
//   F = N D1 W1 + [I|0]: lane e owns entries e, e + 64, ... as in mlp_jacobian_store.
__device__ __forceinline__ void mlp2_jacobian_store(const MlpModel &m, const Mlp2Lds &L, const int lane, const float tau,
                                                    const float next, const float (&d1)[kMlp2Units],
                                                    const float (&d2)[kMlp2Units], float *Fp, float *fq) {
  const int nx = m.nx, ns = m.nx + m.nu, H1 = m.n_hidden, H2 = m.n_hidden2;
  const int n1 = (H1 + 63) / 64;
  float *g1 = L.wave, *g2 = g1 + kMlp2MaxHidden, *Ns = g2 + kMlp2MaxHidden, *Fs = Ns + kMlpMaxNx * (kMlp2MaxHidden | 1);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the previous step's reads of the slice are done)
  int col[kMlp2Units];
  bool has[kMlp2Units];
#pragma unroll
  for (int k = 0; k < kMlp2Units; ++k) {
    const int h = lane + 64 * k;
    has[k] = h < H1;
    col[k] = has[k] ? h : H1 - 1;
    if (h < H1) g1[h] = d1[k];
    if (h < H2) g2[h] = d2[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  for (int i0 = 0; i0 < nx; i0 += 4) {
    int r[4];
    float acc[kMlp2Units][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      r[q] = (i0 + q < nx ? i0 + q : nx - 1) * L.hp2;
#pragma unroll
      for (int k = 0; k < kMlp2Units; ++k) acc[k][q] = 0.f;
    }
    for (int h = 0; h < H2; ++h) {
      const float dd = g2[h];
      float w2[kMlp2Units];
#pragma unroll
      for (int k = 0; k < kMlp2Units; ++k) w2[k] = k < n1 ? L.W2s[h * L.hp1 + col[k]] : 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float w3d = L.W3s[r[q] + h] * dd;
#pragma unroll
        for (int k = 0; k < kMlp2Units; ++k) acc[k][q] = fmaf(w3d, w2[k], acc[k][q]);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int k = 0; k < kMlp2Units; ++k)
        if (i0 + q < nx && k < n1 && has[k]) Ns[(i0 + q) * L.hp1 + col[k]] = acc[k][q];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  for (int e = lane; e < nx * ns; e += 64) {
    const int i = e / ns, j = e % ns;
    const float *nr = Ns + i * L.hp1, *w1 = L.W1s + j;
    float acc = (m.residual && i == j) ? 1.f : 0.f;
#pragma unroll 4
    for (int h = 0; h < H1; ++h) acc = fmaf(nr[h] * g1[h], w1[h * L.nsp], acc);
    Fs[e] = acc;
    Fp[e] = acc;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const int rr = lane < nx ? lane : 0;
  float f = next;
  for (int j = 0; j < ns; ++j) f = fmaf(-Fs[rr * ns + j], lane_value(tau, j), f);
  if (fq != nullptr && lane < nx) fq[lane] = f;
}

// What the rollout and the search know of a network's depth: how its weights are staged, ONE step, that step's Jacobian.
template <int DEPTH>
struct MlpNet;
template <>
struct MlpNet<1> {
  using Lds = MlpLds;
  float a[kMlpUnits], d[kMlpUnits];
  static __device__ __forceinline__ Lds stage(const MlpModel &m, float *lds) { return mlp_stage(m, lds); }
  template <int ACT>
  __device__ __forceinline__ float next(const MlpModel &m, const Lds &L, const int lane, const float tau) {
    return mlp_next<ACT>(m, L, lane, tau, a, d);
  }
  __device__ __forceinline__ void jacobian_store(const MlpModel &m, const Lds &L, const int lane, const float tau,
                                                 const float xn, float *Fp, float *fq) const {
    mlp_jacobian_store(m, L, lane, tau, xn, d, Fp, fq);
  }
};
template <>
struct MlpNet<2> {
  using Lds = Mlp2Lds;
  float d1[kMlp2Units], d2[kMlp2Units];
  static __device__ __forceinline__ Lds stage(const MlpModel &m, float *lds) { return mlp2_stage(m, lds); }
  template <int ACT>
  __device__ __forceinline__ float next(const MlpModel &m, const Lds &L, const int lane, const float tau) {
    return mlp2_next<ACT>(m, L, lane, tau, d1, d2);
  }
  __device__ __forceinline__ void jacobian_store(const MlpModel &m, const Lds &L, const int lane, const float tau,
                                                 const float xn, float *Fp, float *fq) const {
    mlp2_jacobian_store(m, L, lane, tau, xn, d1, d2, Fp, fq);
  }
};

// (MlpRolloutArgs: mlp_dx_launch.hpp.)  In a box-DDP chain: a.clear runs first - thread g of the grid zeroes word g of each
// range, and the grid has at least max(B, 256) threads - and a set `done` flag ends the launch before its barrier.
template <int ACT, int DEPTH>
__device__ __forceinline__ void mlp_rollout_linearize_body(const MlpRolloutArgs &a, float *lds) {
  a.clear.run(blockIdx.x * blockDim.x + threadIdx.x);
  if (a.done != nullptr && *a.done != 0) return;   // grid-uniform: the iLQR loop has stopped
  const typename MlpNet<DEPTH>::Lds L = MlpNet<DEPTH>::stage(a.m, lds);
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
    MlpNet<DEPTH> net;
    const float xn = net.template next<ACT>(a.m, L, lane, tau);
    if (a.F != nullptr) net.jacobian_store(a.m, L, lane, tau, xn, a.F + tb * nx * ns, a.f ? a.f + tb * nx : nullptr);
    xc = xn;
  }
}

// The kernels.  The depth is the second template parameter; the depth-one instances keep the one-parameter names they had
// before the second depth existed (profilers' lists and the recorded search values name them), so each kernel is a pair of
// overloaded templates over one body.
template <int ACT>
__global__ __launch_bounds__(64 * kMlpWaves) void mlp_rollout_linearize_kernel(const MlpRolloutArgs a) {
  extern __shared__ float lds[];
  mlp_rollout_linearize_body<ACT, 1>(a, lds);
}
template <int ACT, int DEPTH>
__global__ __launch_bounds__(64 * kMlpWaves) void mlp_rollout_linearize_kernel(const MlpRolloutArgs a) {
  static_assert(DEPTH == 2, "the depth-one kernel is mlp_rollout_linearize_kernel<ACT>");
  extern __shared__ float lds[];
  mlp_rollout_linearize_body<ACT, DEPTH>(a, lds);
}

// forward_rec: the arithmetic of a pass, its order and the search's decisions are mpc_generic_forward_kernel's (and
// through it mpc_forward_rec_kernel's): the cost difference per timestep without cancellation, box_clamp's snap, the
// pass cap.  a.F / a.f are not read.  The loop is wave-uniform by construction - a wavefront is one trajectory - so a
// trajectory that has finished runs, stores and commits nothing more.
// a.F_next (BoxDDP's chain): the accepted trajectory IS the next iteration's nominal one, so after the search the wavefront
// walks it once more and stores its Jacobians, F_next [T-1,B,nx,ns] - through mlp_next and mlp_jacobian_store on the values
// mlp_rollout_linearize_kernel would start from, hence bit for bit what that kernel would store.  a.f_next, a.c_next: not written.
// Depth two: the wavefront slices exist only when a.F_next is given (mlp_lds_bytes).
template <int ACT, int DEPTH>
__device__ __forceinline__ void mpc_forward_rec_mlp_body(const MpcFwdArgs &a, const MlpModel &m, float *lds) {
  if (a.done != nullptr && *a.done != 0) return;   // grid-uniform, before the barrier: the iLQR loop has stopped
  const typename MlpNet<DEPTH>::Lds L = MlpNet<DEPTH>::stage(m, lds);
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

  float cost = 0.f, old_cost = 0.f;
  LineSearch ls;
  while (ls.searching(a.ls_cap)) {
    const float alpha = ls.alpha;
    const bool first = ls.n_pass == 0;
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
      v = box_clamp(v, a.lower[tb * nu + mu], a.upper[tb * nu + mu]);
      const float tau = is_x ? xc : (is_u ? v : 0.f);
      const float tau0 = is_x ? x0 : (is_u ? u0 : 0.f);
      if (is_u) {
        a.u[tb * nu + mu] = v;
        if (a.u_first != nullptr && first) a.u_first[tb * nu + mu] = v;                  // :260-263
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
          part = cost_row(tau, qi, ci);
          part0 = cost_row(tau0, q0, ci);
          partd = cost_row_diff(di, qi, ci, tau0, qd);
        }
      }
      const float obj = wave_sum64(part);
      cost += obj;
      delta += wave_sum64(partd);
      if (first) old_cost += wave_sum64(part0);                                          // :191
      if (a.objs != nullptr && lane == 0) a.objs[tb] = obj;
      if (t < T - 1) {                                                                   // :237-240
        MlpNet<DEPTH> net;
        xc = net.template next<ACT>(m, L, lane, tau);
      }
    }
    ls.advance(delta, a.ls_decay);
  }
  if (ls.worse) ls.alpha = cap_alpha_sequential(ls.alpha, a.ls_decay);
  // info_in, info_store: dmpc_mpc_forward_rec_mlp has neither (its MpcFwdArgs leaves both zero)
  if (lane == 0) search_store<false, false>(a, b, cost, old_cost, ls.alpha, ls.n_pass, search_flags(ls.worse, cost));
  if (a.F_next != nullptr) {
    // the last pass is the accepted one: its controls are in a.u, each re-read by the lane that stored it; the states are
    // re-evaluated from states[0] by the function that formed them
    float xc = is_x ? a.states[(size_t)b * nx + lane] : 0.f;
    for (int t = 0; t < T - 1; ++t) {
      const size_t tb = (size_t)t * B + b;
      const float v = a.u[tb * nu + mu];
      const float tau = is_x ? xc : (is_u ? v : 0.f);
      MlpNet<DEPTH> net;
      const float xn = net.template next<ACT>(m, L, lane, tau);
      net.jacobian_store(m, L, lane, tau, xn, a.F_next + tb * nx * ns, nullptr);
      xc = xn;
    }
  }
}

template <int ACT>
__global__ __launch_bounds__(64 * kMlpWaves) void mpc_forward_rec_mlp_kernel(const MpcFwdArgs a, const MlpModel m) {
  extern __shared__ float lds[];
  mpc_forward_rec_mlp_body<ACT, 1>(a, m, lds);
}
template <int ACT, int DEPTH>
__global__ __launch_bounds__(64 * kMlpWaves) void mpc_forward_rec_mlp_kernel(const MpcFwdArgs a, const MlpModel m) {
  static_assert(DEPTH == 2, "the depth-one kernel is mpc_forward_rec_mlp_kernel<ACT>");
  extern __shared__ float lds[];
  mpc_forward_rec_mlp_body<ACT, DEPTH>(a, m, lds);
}

// The gradient of L(f) with respect to W1, b1, W2, b2 for f_t = next(x_t, u_t) - F_t [x_t;u_t] along the rolled states,
// F_t a CONSTANT with the value of the live Jacobian (MlpDx.linearize; mpc/approximate.py:77-119).  With z_t = [x_t;u_t],
// a_t = act(W1 z_t + b1), d_t = act'(W1 z_t + b1), g_t = dL/df_t, lam_{T-1} = 0, for t = T-2 .. 0:
//     r     = g_t + lam_{t+1}
//     delta = d_t * (W2^T r)
//     dW2 += r a_t^T ;  db2 += r ;  dW1 += delta z_t^T ;  db1 += delta
//     e     = d_t * (W2^T lam_{t+1}) ;  du_t = W1[:, nx:]^T e ;  lam_t = W1[:, :nx]^T e (+ lam_{t+1} when residual)
// Every term of lam_t carries a factor lam_{t+1}, and lam_{T-1} = 0: lam_t = 0, e = 0 and du_t = 0 for every t, as exact
// zeros in any arithmetic and for every activation - next's derivative through z_t and F_t's cancel at every step,
// nothing is left to carry.
// So r = g_t, the lines of e, du and lam are not evaluated, and d_x_init, d_u are stored as the zeros they are.
//
// One wavefront per trajectory as above; wavefront w of G serves trajectories w, w + G, ... in ascending order, t
// descending, and keeps the sums for ITS hidden units (lane, lane + 64, ...) in registers - rows of dW1, columns of dW2,
// db1; lanes < nx keep db2 - every array indexed by unrolled loops with wave-uniform guards, never by a runtime value.
// It stores one partial [dW1 | db1 | dW2 | db2], laid out as the parameters are, at part + w * P.
// mlp_param_grad_reduce_kernel adds the G partials per element in ascending order: no atomics, and a result that depends
// on (T, B, nx, nu, H) and the data alone.
constexpr int kMlpGradCap = 512;                             // partials at most: 21.5 MB at the largest model
__host__ __device__ inline int mlp_grad_partials(int B) { return B < kMlpGradCap ? B : kMlpGradCap; }
__host__ __device__ inline int mlp_grad_partial_floats(int nx, int nu, int H) { return H * (nx + nu) + H + nx * H + nx; }

struct MlpGradArgs {
  int T, B, G;
  MlpModel m;
  const float *x, *u, *grad_f;   // [T,B,nx] as the rollout stored them, [T,B,nu], [T-1,B,nx]
  float *part;                   // [G][P]
  float *d_x_init, *d_u;         // [B,nx], [T,B,nu], each or nullptr
};

template <int ACT>
__global__ __launch_bounds__(64 * kMlpWaves) void mlp_param_grad_kernel(const MlpGradArgs a) {
  extern __shared__ float lds[];
  const MlpLds L = mlp_stage(a.m, lds);
  const int lane = threadIdx.x % 64;
  const int w = blockIdx.x * kMlpWaves + threadIdx.x / 64;
  if (w >= a.G) return;      // (after the only barrier)
  const int nx = a.m.nx, nu = a.m.nu, ns = nx + nu, H = a.m.n_hidden;
  const int n_units = (H + 63) / 64;
  const int T = a.T;
  const size_t B = (size_t)a.B;
  int row[kMlpUnits];
  bool has[kMlpUnits];
#pragma unroll
  for (int k = 0; k < kMlpUnits; ++k) {
    has[k] = lane + 64 * k < H;
    row[k] = has[k] ? lane + 64 * k : H - 1;
  }
  float dW1[kMlpUnits][kMlpMaxNx + kMlpMaxNu] = {}, dW2[kMlpUnits][kMlpMaxNx] = {}, db1[kMlpUnits] = {}, db2 = 0.f;

  for (size_t b = w; b < B; b += a.G) {
    if (a.d_x_init != nullptr && lane < nx) a.d_x_init[b * nx + lane] = 0.f;
    if (a.d_u != nullptr && lane < nu)
      for (int t = 0; t < T; ++t) a.d_u[((size_t)t * B + b) * nu + lane] = 0.f;
    for (int t = T - 2; t >= 0; --t) {
      const size_t tb = (size_t)t * B + b;
      const float tau = lane < nx ? a.x[tb * nx + lane] : (lane < ns ? a.u[tb * nu + (lane - nx)] : 0.f);
      const float r = lane < nx ? a.grad_f[tb * nx + lane] : 0.f;
      float act[kMlpUnits], dact[kMlpUnits];
      (void)mlp_next<ACT>(a.m, L, lane, tau, act, dact);
      db2 += r;
      float s[kMlpUnits] = {};                               // W2^T r at this lane's units
#pragma unroll
      for (int i = 0; i < kMlpMaxNx; ++i) {
        if (i < nx) {
          const float ri = lane_value(r, i);
#pragma unroll
          for (int k = 0; k < kMlpUnits; ++k) {
            if (k < n_units) {
              const float w2 = L.W2s[i * L.hp + row[k]];
              s[k] = fmaf(has[k] ? w2 : 0.f, ri, s[k]);
              dW2[k][i] = fmaf(ri, act[k], dW2[k][i]);
            }
          }
        }
      }
      float delta[kMlpUnits];
#pragma unroll
      for (int k = 0; k < kMlpUnits; ++k) {
        delta[k] = dact[k] * s[k];
        db1[k] += delta[k];
      }
#pragma unroll
      for (int j = 0; j < kMlpMaxNx + kMlpMaxNu; ++j) {
        if (j < ns) {
          const float tj = lane_value(tau, j);
#pragma unroll
          for (int k = 0; k < kMlpUnits; ++k)
            if (k < n_units) dW1[k][j] = fmaf(delta[k], tj, dW1[k][j]);
        }
      }
    }
  }

  float *p = a.part + (size_t)w * mlp_grad_partial_floats(nx, nu, H);
  float *pb1 = p + H * ns, *pW2 = pb1 + H, *pb2 = pW2 + nx * H;
#pragma unroll
  for (int k = 0; k < kMlpUnits; ++k) {
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

struct MlpGradReduceArgs {
  int G, nx, nu, n_hidden;
  const float *part;               // [G][P]
  float *dW1, *db1, *dW2, *db2;    // [H,ns], [H], [nx,H], [nx]
};

// one thread per parameter element; G = 0 stores zeros (T = 1: no dynamics step, no partials)
__global__ __launch_bounds__(256) void mlp_param_grad_reduce_kernel(const MlpGradReduceArgs a) {
  const int H = a.n_hidden, n1 = H * (a.nx + a.nu), n2 = a.nx * H;
  const int P = mlp_grad_partial_floats(a.nx, a.nu, H);
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P) return;
  float s = 0.f;
#pragma unroll 8
  for (int w = 0; w < a.G; ++w) s += a.part[(size_t)w * P + e];
  if (e < n1) a.dW1[e] = s;
  else if (e < n1 + H) a.db1[e - n1] = s;
  else if (e < n1 + H + n2) a.dW2[e - n1 - H] = s;
  else a.db2[e - n1 - H - n2] = s;
}

}  // namespace dmpc
