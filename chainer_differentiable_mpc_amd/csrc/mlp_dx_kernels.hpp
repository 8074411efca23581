// mlp_dx_kernels.hpp - a learned dynamics model with DEPTH = 1 or 2 hidden layers on the device (MlpDx of the Python layer):
//
//     a_0 = [x;u],   z_l = W_l a_{l-1} + b_l,  a_l = act(z_l)   for the hidden layers l = 1 .. DEPTH,
//     next(x, u) = W_{DEPTH+1} a_DEPTH + b_{DEPTH+1} (+ x when residual),        act = tanh | relu | silu | softplus
//
// The network is written ONCE, by layers, each piece templated on the hidden units a lane owns (UNITS: 4 at depth one, H <= 256;
// 2 at depth two, H1, H2 <= 128 - the register arrays have that size, so the two depths do not share a value of it):
//     MlpUnits                 which units of a layer this lane owns (lane, lane + 64, ...), clamped addresses, the live mask
//     mlp_layer_from_lanes     a hidden layer whose inputs sit one per lane: layer 1
//     mlp_layer_from_units     a hidden layer whose inputs are the previous layer's units in registers: layer 2 (and a third)
//     mlp_activate             mlp_act<ACT> on one of a lane's units under the live mask: a = act(z), d = act'(z), zeros beyond the width
//     mlp_output_layer         one butterfly reduction per output, bias, residual
//     mlp_fold_output          N = W3 D2 W2: the output layer folded through layer 2 (depth two's Jacobian only)
//     mlp_jacobian_tail        F = left D1 W1 + [I|0], its stores, f = next - F tau;  left = W2 at depth one, N at depth two
// MlpNet<DEPTH> composes them into `next` and `jacobian_store`; the activation and the depth are template parameters of the
// kernels, and mlp_act is the only place where the activation is looked at.
//
//   mlp_rollout_linearize_kernel   get_traj + linearize_dynamics (util.py:239-277, mpc/approximate.py:77-119) in one
//                                  launch: x_{t+1} = next(x_t, u_t), F_t = d next / d [x;u], f_t = next - F_t [x_t;u_t].
//   mpc_forward_rec_mlp_kernel     MPCstep.forward_rec (mpc/mpc_step.py:175-286) with the network as the TRUE dynamics:
//                                  the clamped closed-loop rollout and per-trajectory line search of
//                                  mpc_generic_forward_kernel, the dynamics evaluated in place of F tau + f.
//   mlp_param_grad_kernel,         the gradient of a loss of the rollout's f with respect to W1, b1, W2, b2 (depth one): per-wavefront
//   mlp_param_grad_reduce_kernel   sums in registers, then a fixed-order reduction of the partials (at the end of this file).
//                                  The same sweeps with the co-state carried, for a loss of the rolled states themselves, are
//                                  siblings in mlp_rollout_grad_kernels.hpp; they store these partials for these reductions.
//
// Layout.  Runtime dimensions (nx <= 16, nu <= 8), ONE wavefront per trajectory, four per workgroup.  The weights are
// staged into LDS once per workgroup (mlp_stage) and shared by its wavefronts - the matrices in layer order, then the biases:
//     W[l] [out_l][in_l | 1]   a hidden layer: lane l owns units l, l + 64, ...: it walks ITS row, and the odd stride puts the 64
//                              rows a wavefront reads at once on 64 different banks.  The output layer: lanes read consecutive
//                              units of a row (no conflict); the odd stride separates the rows the Jacobian's lanes read at once
//     b[l] [out_l]
// 43.1 KB at depth one's largest size, 88.2 KB at depth two's (nx 16, nu 8, H1 = H2 = 128).  Behind them every wavefront has a
// slice of its own (mlp_wave_floats: d per hidden unit, depth two's N, the step's Jacobian): 672 floats at depth one, which
// every depth-one launch carries; 2,704 at depth two, only in a launch that forms Jacobians - 131.5 KB then, one workgroup per
// CU.  Element i of tau = [x;u] lives in lane i; a value another lane needs - an element of tau, a layer-1 activation - is read
// from that lane's register (v_readlane), never through LDS, so the step function touches no slice, the search needs no
// barrier after the staging one and its wavefronts leave the loop one by one.
//
// Bit-equal dynamics.  The search ends when a candidate collapses onto the nominal trajectory and its cost difference is
// exactly 0 (see PendulumModel in mpc_kernels.hpp).  Every kernel evaluates the network through the pieces above alone:
// explicit fmaf, a layer's inputs in ascending order, a lane's units in ascending order, one butterfly reduction per output;
// units beyond a width hold exact zeros and read clamped addresses - an order that depends on (nx, nu, the widths) and the
// activation and on nothing else: not on B, the grid, or the wavefront's slot in its workgroup.
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

constexpr int kMlpMaxNx = 16, kMlpMaxNu = 8;
constexpr int kMlpWaves = 4;                                 // trajectories (wavefronts) per workgroup
constexpr int mlp_max_hidden(int depth) { return depth == 1 ? 256 : 128; }
constexpr int mlp_units(int depth) { return mlp_max_hidden(depth) / 64; }      // hidden units per lane, at most
// a wavefront's own floats: d per hidden unit and layer; depth two: N with an odd row stride (depth one: 32 floats its
// launches have always carried); the step's Jacobian
constexpr int mlp_wave_floats(int depth) {
  return depth * mlp_max_hidden(depth) + (depth == 1 ? 32 : kMlpMaxNx * (mlp_max_hidden(depth) | 1)) + kMlpMaxNx * (kMlpMaxNx + kMlpMaxNu);
}

// THE byte count of a launch's dynamic LDS, for the launchers and for dmpc_mlp_dx_supported.  H2 = 0: one hidden layer.
// `jacobian`: the launch forms F (depth one always has its slices: its instances are what they were).
constexpr size_t mlp_lds_bytes(int nx, int nu, int H1, int H2 = 0, bool jacobian = true) {
  const int depth = H2 > 0 ? 2 : 1, last = H2 > 0 ? H2 : H1;
  int floats = H1 * ((nx + nu) | 1) + H1 + nx * (last | 1) + nx;
  if (depth == 2) floats += H2 * (H1 | 1) + H2;
  if (depth == 1 || jacobian) floats += kMlpWaves * mlp_wave_floats(depth);
  return (size_t)floats * sizeof(float);
}
static_assert(mlp_lds_bytes(16, 8, 256) == 53888, "depth one at every limit");
static_assert(mlp_lds_bytes(16, 8, 128, 128, false) == 88192, "depth two at every limit, no Jacobian slices");
static_assert(mlp_lds_bytes(16, 8, 128, 128, true) == 131456, "depth two at every limit, with its Jacobian slices");
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

// layer l of a DEPTH-layer model: its inputs and outputs (l and DEPTH are compile-time constants wherever this is called)
__device__ __forceinline__ int mlp_in(const MlpModel &m, int l) { return l == 0 ? m.nx + m.nu : m.H[l - 1]; }
__device__ __forceinline__ int mlp_out(const MlpModel &m, int l, int depth) { return l < depth ? m.H[l] : m.nx; }

// The staged network: layer l's matrix with row stride ld[l] = in_l | 1 and its bias; `wave`: this wavefront's slice (only a
// launch that forms Jacobians, or a depth-one launch, has it).
template <int DEPTH>
struct MlpLds {
  int ld[DEPTH + 1];
  float *W[DEPTH + 1], *b[DEPTH + 1], *wave;
};

// one padded matrix and its bias into LDS, by every thread of the workgroup
__device__ __forceinline__ void mlp_stage_layer(float *Ws, const int ld, float *bs, const float *W, const float *b, const int rows,
                                                const int cols) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int e = tid; e < rows * cols; e += nt) Ws[(e / cols) * ld + (e % cols)] = W[e];
  for (int e = tid; e < rows; e += nt) bs[e] = b[e];
}

// every thread of the workgroup takes part, also those of wavefronts without a trajectory; ends with the one barrier
template <int DEPTH>
__device__ __forceinline__ MlpLds<DEPTH> mlp_stage(const MlpModel &m, float *lds) {
  MlpLds<DEPTH> L;
  float *p = lds;
#pragma unroll
  for (int l = 0; l <= DEPTH; ++l) {
    L.ld[l] = mlp_in(m, l) | 1;
    L.W[l] = p;
    p += mlp_out(m, l, DEPTH) * L.ld[l];
  }
#pragma unroll
  for (int l = 0; l <= DEPTH; ++l) {
    L.b[l] = p;
    p += mlp_out(m, l, DEPTH);
  }
  L.wave = p + (threadIdx.x / 64) * mlp_wave_floats(DEPTH);
#pragma unroll
  for (int l = 0; l <= DEPTH; ++l) mlp_stage_layer(L.W[l], L.ld[l], L.b[l], m.layer[l].W, m.layer[l].b, mlp_out(m, l, DEPTH), mlp_in(m, l));
  __syncthreads();
  return L;
}

// The units of a layer of width H that this lane owns: unit k is lane + 64 k.  Units beyond H hold exact zeros, add exact
// zeros to every sum, and their LDS addresses are clamped into range (row[]); `n` is wave-uniform.
template <int UNITS>
struct MlpUnits {
  int n, row[UNITS];
  bool has[UNITS];
  __device__ __forceinline__ MlpUnits(const int lane, const int H) : n((H + 63) / 64) {
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      const int h = lane + 64 * k;
      has[k] = h < H;
      row[k] = has[k] ? h : H - 1;
    }
  }
  __device__ __forceinline__ bool live(const int k) const { return k < n && has[k]; }
};

template <int UNITS>
__device__ __forceinline__ void mlp_bias(const float *bs, const MlpUnits<UNITS> &U, float (&z)[UNITS]) {
#pragma unroll
  for (int k = 0; k < UNITS; ++k) z[k] = U.has[k] ? bs[U.row[k]] : 0.f;
}

// z = W tau + b at this lane's units, element j of tau in lane j (anything in lanes >= n_in: never read); j ascending
template <int UNITS>
__device__ __forceinline__ void mlp_layer_from_lanes(const float *Ws, const int ld, const float *bs, const MlpUnits<UNITS> &U,
                                                     const int n_in, const float tau, float (&z)[UNITS]) {
  mlp_bias(bs, U, z);
  for (int j = 0; j < n_in; ++j) {
    const float tj = lane_value(tau, j);
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      if (k < U.n) {
        const float w = Ws[U.row[k] * ld + j];
        z[k] = fmaf(U.has[k] ? w : 0.f, tj, z[k]);
      }
    }
  }
}

// z = W a_in + b at this lane's units, unit h = 64 k1 + l of the n_in inputs in a_in[k1] of lane l; h ascending
template <int UNITS_IN, int UNITS_OUT>
__device__ __forceinline__ void mlp_layer_from_units(const float *Ws, const int ld, const float *bs, const MlpUnits<UNITS_OUT> &U,
                                                     const int n_in, const float (&a_in)[UNITS_IN], float (&z)[UNITS_OUT]) {
  mlp_bias(bs, U, z);
#pragma unroll
  for (int k1 = 0; k1 < UNITS_IN; ++k1) {
    const int left = n_in - 64 * k1, cnt = left < 64 ? left : 64;
    for (int l = 0; l < cnt; ++l) {
      const float ah = lane_value(a_in[k1], l);
#pragma unroll
      for (int k = 0; k < UNITS_OUT; ++k) {
        if (k < U.n) {
          const float w = Ws[U.row[k] * ld + 64 * k1 + l];
          z[k] = fmaf(U.has[k] ? w : 0.f, ah, z[k]);
        }
      }
    }
  }
}

// a = act(z), d = act'(z) of ONE of this lane's units under the live mask (U.live(k)): both 0 beyond the width.  A caller that
// does not read d does not pay for it: everything here is inlined.  The loop over a lane's units is the caller's - as a loop over
// arrays inside this function the softplus instances hold 3 to 5 more VGPRs, and the depth-two softplus search 73: 6 waves, not 7.
template <int ACT>
__device__ __forceinline__ void mlp_activate(const bool live, const float z, float &a, float &d) {
  float ak, dk;
  mlp_act<ACT>(z, ak, dk);
  a = live ? ak : 0.f;
  d = live ? dk : 0.f;
}

// element `lane` of W a + b (+ x when residual) over the last hidden layer's units (0 in lanes >= nx): one butterfly per output
template <int UNITS>
__device__ __forceinline__ float mlp_output_layer(const float *Ws, const int ld, const float *bs, const MlpUnits<UNITS> &U,
                                                  const MlpModel &m, const int lane, const float tau, const float (&a)[UNITS]) {
  float next = 0.f;
  for (int i = 0; i < m.nx; ++i) {
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      if (k < U.n) {
        const float w = Ws[i * ld + U.row[k]];
        part = fmaf(U.has[k] ? w : 0.f, a[k], part);
      }
    }
    float s = wave_sum64(part) + bs[i];
    if (m.residual) s += lane_value(tau, i);
    next = lane == i ? s : next;
  }
  return next;
}

// N = W3 D2 W2 (nx x H1, row stride ld2) into the wavefront's slice, g2 = diag(D2) read from it: a lane owns columns lane,
// lane + 64 (U: the units of layer 1) and takes the rows four at a time - per unit of layer 2 one d2, the lane's W2 entries
// (consecutive lanes, consecutive words) and four W3 entries (one word for the wavefront) feed the fused multiply-adds; the
// sum over the units of layer 2 ascending, a ragged last group of rows on clamped addresses.
template <int UNITS>
__device__ __forceinline__ void mlp_fold_output(const float *W3s, const int ld3, const float *g2, const float *W2s, const int ld2,
                                                const MlpUnits<UNITS> &U, const int nx, const int H2, float *Ns) {
  for (int i0 = 0; i0 < nx; i0 += 4) {
    int r[4];
    float acc[UNITS][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      r[q] = (i0 + q < nx ? i0 + q : nx - 1) * ld3;
#pragma unroll
      for (int k = 0; k < UNITS; ++k) acc[k][q] = 0.f;
    }
    for (int h = 0; h < H2; ++h) {
      const float dd = g2[h];
      float w2[UNITS];
#pragma unroll
      for (int k = 0; k < UNITS; ++k) w2[k] = k < U.n ? W2s[h * ld2 + U.row[k]] : 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float w3d = W3s[r[q] + h] * dd;
#pragma unroll
        for (int k = 0; k < UNITS; ++k) acc[k][q] = fmaf(w3d, w2[k], acc[k][q]);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int k = 0; k < UNITS; ++k)
        if (i0 + q < nx && k < U.n && U.has[k]) Ns[(i0 + q) * ld2 + U.row[k]] = acc[k][q];
    }
  }
}

// F = left D1 W1 + [I|0] residual (nx x ns, row-major) at Fp and at Fs in the wavefront's slice, f = next - F tau at fq (lanes
// < nx).  `left` (nx x H1, row stride ldl) is the network behind layer 1: the output layer's matrix at depth one, N at depth
// two; g1 = diag(D1) from the slice.  VALU over LDS: lane e owns entries e, e + 64, ... of F and sums over the units of
// layer 1 in ascending order.
__device__ __forceinline__ void mlp_jacobian_tail(const MlpModel &m, const float *left, const int ldl, const float *g1, const float *W1s,
                                                  const int nsp, float *Fs, const int lane, const float tau, const float next,
                                                  float *Fp, float *fq) {
  const int nx = m.nx, ns = m.nx + m.nu, H = m.H[0];
  for (int e = lane; e < nx * ns; e += 64) {
    const int i = e / ns, j = e % ns;
    const float *lr = left + i * ldl, *w1 = W1s + j;
    float acc = (m.residual && i == j) ? 1.f : 0.f;
#pragma unroll 4
    for (int h = 0; h < H; ++h) acc = fmaf(lr[h] * g1[h], w1[h * nsp], acc);
    Fs[e] = acc;
    Fp[e] = acc;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const int r = lane < nx ? lane : 0;
  float f = next;
  for (int j = 0; j < ns; ++j) f = fmaf(-Fs[r * ns + j], lane_value(tau, j), f);
  if (fq != nullptr && lane < nx) fq[lane] = f;
}

// What the rollout and the search know of a network: how its weights are staged, ONE step (the only place the network is
// evaluated), that step's Jacobian.  d[l]: this lane's act' of hidden layer l + 1, left by `next` for `jacobian_store`.
template <int DEPTH>
struct MlpNet {
  static_assert(DEPTH >= 1 && DEPTH <= kMlpMaxDepth, "depth");
  static constexpr int UNITS = mlp_units(DEPTH);
  using Lds = MlpLds<DEPTH>;
  float d[DEPTH][UNITS];
  static __device__ __forceinline__ Lds stage(const MlpModel &m, float *lds) { return mlp_stage<DEPTH>(m, lds); }

  // tau: element `lane` of [x;u].  Returns element `lane` of the next state (0 in lanes >= nx).
  template <int ACT>
  __device__ __forceinline__ float next(const MlpModel &m, const Lds &L, const int lane, const float tau) {
    static_assert(DEPTH <= 2, "a third hidden layer is one more mlp_layer_from_units");
    const MlpUnits<UNITS> U1(lane, m.H[0]), UL(lane, m.H[DEPTH - 1]);   // the units of layer 1 and of the last hidden layer
    float a1[UNITS], a[UNITS], z[UNITS];
    mlp_layer_from_lanes(L.W[0], L.ld[0], L.b[0], U1, m.nx + m.nu, tau, z);
#pragma unroll
    for (int k = 0; k < UNITS; ++k) mlp_activate<ACT>(U1.live(k), z[k], (DEPTH == 1 ? a : a1)[k], d[0][k]);
    if constexpr (DEPTH == 2) {
      mlp_layer_from_units(L.W[1], L.ld[1], L.b[1], UL, m.H[0], a1, z);
#pragma unroll
      for (int k = 0; k < UNITS; ++k) mlp_activate<ACT>(UL.live(k), z[k], a[k], d[1][k]);
    }
    return mlp_output_layer(L.W[DEPTH], L.ld[DEPTH], L.b[DEPTH], UL, m, lane, tau, a);
  }

  // F = d next / d [x;u] at Fp, f = next - F tau at fq.  The slice: d of every hidden unit, layer by layer (g), depth two's N,
  // then F.  Within one wavefront LDS operations complete in program order; the fences keep the compiler from moving a read
  // above the write it depends on.
  __device__ __forceinline__ void jacobian_store(const MlpModel &m, const Lds &L, const int lane, const float tau, const float xn,
                                                 float *Fp, float *fq) const {
    static_assert(DEPTH <= 2, "a third hidden layer folds through mlp_fold_output once more");
    constexpr int HMAX = mlp_max_hidden(DEPTH);
    float *g = L.wave, *Ns = g + DEPTH * HMAX, *Fs = DEPTH == 1 ? Ns : Ns + kMlpMaxNx * (HMAX | 1);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the previous step's reads of the slice are done)
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      const int h = lane + 64 * k;
#pragma unroll
      for (int l = 0; l < DEPTH; ++l)
        if (h < m.H[l]) g[l * HMAX + h] = d[l][k];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if constexpr (DEPTH == 1) {
      mlp_jacobian_tail(m, L.W[1], L.ld[1], g, L.W[0], L.ld[0], Fs, lane, tau, xn, Fp, fq);
    } else {
      mlp_fold_output(L.W[2], L.ld[2], g + HMAX, L.W[1], L.ld[1], MlpUnits<UNITS>(lane, m.H[0]), m.nx, m.H[1], Ns);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      mlp_jacobian_tail(m, Ns, L.ld[1], g, L.W[0], L.ld[0], Fs, lane, tau, xn, Fp, fq);
    }
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
// walks it once more and stores its Jacobians, F_next [T-1,B,nx,ns] - through MlpNet's next and jacobian_store on the values
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
      const float tau = lane < nx ? a.x[tb * nx + lane] : (lane < ns ? a.u[tb * nu + (lane - nx)] : 0.f);
      const float r = lane < nx ? a.grad_f[tb * nx + lane] : 0.f;
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

// The same gradient with TWO hidden layers (include/dmpc_mlp_grad.h).  As above the co-state is exactly zero, r = g_t, and each
// step adds, with tau = [x_t;u_t] and the forward pieces of MlpNet<2> (mlp_layer_from_lanes, mlp_layer_from_units, mlp_activate):
//     dW3 += r a2^T ;  db3 += r ;  e2 = d2 * (W3^T r) ;  dW2 += e2 a1^T ;  db2 += e2 ;  e1 = d1 * (W2^T e2) ;  dW1 += e1 tau^T ;  db1 += e1
//
// One wavefront per trajectory, four per workgroup; workgroup g of G serves the trajectory groups g, g + G, ... in ascending
// order (b = 4 group + slot), t descending.  Who keeps what:
//     a wavefront, in the registers of the lane that owns the unit (lane, lane + 64):
//         rows of dW1 and db1 (layer-1 units), columns of dW3 and db2 (layer-2 units), db3 (lanes < nx)   - 85 per lane
//     the workgroup: dW2 [H2,H1], up to 16,384 sums - wavefront w keeps rows 32 w .. 32 w + 31, a lane columns lane and
//         lane + 64 of them: 64 per lane.  Each step every wavefront publishes a1 and e2 of ITS trajectory (both complete to 128
//         entries, exact zeros beyond the widths) into a double-buffered exchange behind the staged weights, and after ONE
//         workgroup barrier every wavefront adds the four outer products into its rows: plain fmaf, slot ascending.
// The barrier is workgroup-uniform: every wavefront runs the trip counts of its workgroup.  A slot without a trajectory (b >= B)
// walks the clamped addresses of trajectory B - 1 and replaces every activation and derivative by 0, so all it adds are exact
// zeros.  Two buffers suffice: a wavefront that writes buffer n & 1 at step n + 2 has passed barrier n + 1, behind which
// nobody reads step n's.
// At the end the four wavefronts' register sums are added in slot order 0, 1, 2, 3 in LDS (over the weights, which nobody reads
// any more) and the workgroup stores ONE partial [dW1 | db1 | dW2 | dW3 | db2 | db3] - the order of the packed weights - at
// part + g * P.  mlp2_param_grad_reduce_kernel adds the G partials per element in ascending order: no atomics, a result that
// depends on (T, B, nx, nu, H1, H2) and the data alone.
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

template <int ACT>
__global__ __launch_bounds__(64 * kMlpWaves) void mlp2_param_grad_kernel(const MlpGradArgs a) {
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
  const MlpUnits<UNITS> U1(lane, H1), U2(lane, H2);
  const int row0 = ROWS * wv;
  float dW1[UNITS][kMlpMaxNx + kMlpMaxNu] = {}, db1[UNITS] = {}, dW3[UNITS][kMlpMaxNx] = {}, db2[UNITS] = {}, db3 = 0.f;
  float dW2[ROWS][UNITS] = {};
  int step = 0;

  for (int grp = blockIdx.x; grp < groups; grp += a.G) {      // workgroup-uniform
    const size_t b0 = (size_t)grp * kMlpWaves + wv;
    const bool live = b0 < B;                                  // wave-uniform
    const size_t b = live ? b0 : B - 1;
    if (live) {
      if (a.d_x_init != nullptr && lane < nx) a.d_x_init[b * nx + lane] = 0.f;
      if (a.d_u != nullptr && lane < nu)
        for (int t = 0; t < T; ++t) a.d_u[((size_t)t * B + b) * nu + lane] = 0.f;
    }
    for (int t = T - 2; t >= 0; --t, ++step) {
      const size_t tb = (size_t)t * B + b;
      const float tau = lane < nx ? a.x[tb * nx + lane] : (lane < ns ? a.u[tb * nu + (lane - nx)] : 0.f);
      const float r = live && lane < nx ? a.grad_f[tb * nx + lane] : 0.f;
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

struct Mlp2GradReduceArgs {
  int G, n1, nb1, n2, nb2;         // partials; elements of dW1, db1, [dW2 | dW3], [db2 | db3] - a partial in this order
  const float *part;               // [G][P]
  float *dW1, *db1, *dW2, *db2;    // [H1,ns], [H1], [H2*H1 | nx*H2], [H2 | nx]
};

// one thread per parameter element; G = 0 stores zeros (T = 1: no dynamics step, no partials)
__global__ __launch_bounds__(256) void mlp2_param_grad_reduce_kernel(const Mlp2GradReduceArgs a) {
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

}  // namespace dmpc
