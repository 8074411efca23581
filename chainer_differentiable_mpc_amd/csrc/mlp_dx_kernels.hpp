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
// The reverse sweeps over the rollout - the gradients with respect to the weights - are built on these pieces in
// mlp_grad_kernels.hpp.
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

}  // namespace dmpc
