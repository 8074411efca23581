// il_kernels.hpp - the three kernels of the imitation-learning update (env_dx/il_exp.py:191-316) that run around the
// box-DDP chain and the tiled-cost gradient: the batch gather with the cost map, the imitation loss with its gradient
// seed, and the chain rule from (dQ, dp) to the cost net's parameters followed by the RMSprop step.
//
// Parameter vector of a cost net (n = n_sc <= 8): [learn_q_logit (n), learn_p (n), lower_without_diag (n(n-1)/2)];
// the last group exists for the lower-triangle nets only.  kind (env_dx/pendulum_net.py):
//   0 Pendulum_Net_cost_logit                            Q = diag(q),          p = sqrt(q) * learn_p
//   1 Pendulum_Net_cost_lower_triangle                   Q = L L^T,            p = learn_p
//   2 Pendulum_Net_cost_logit_strange_obervation         Q = O^T diag(q) O,    p = (sqrt(q) * learn_p) O
//   3 Pendulum_Net_cost_lower_triangle_strange_obervation Q = O^T L L^T O,     p = learn_p O
// with q = sigmoid(learn_q_logit), L lower triangular with q on its diagonal and lower_without_diag below it in
// np.tril_indices(n, -1) order (row-major), O = OBSERVATION_MATRIX (n = 4 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dmpc {

constexpr int kIlMaxSc = 8;
constexpr int kIlLossThreads = 1024;

__device__ __constant__ float kIlObservation[4][4] = {
    {0.f, 4.f, 1.f, 0.f}, {1.f, 0.f, 4.f, 0.f}, {0.f, 4.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 1.f}};

__host__ __device__ inline int il_n_params(int kind, int n) {
  return (kind == 1 || kind == 3) ? 2 * n + n * (n - 1) / 2 : 2 * n;
}

__device__ inline float il_sigmoid(float a) { return 1.0f / (1.0f + expf(-a)); }

// Products and sums of the cost map are rounded one by one (contraction to fma is off: HIP's __fadd_rn / __fmul_rn are
// plain operators), in the order pendulum_net.py's torch restatement sums them, so that both routes of IL_Exp hand the
// solver the same (Q, p) bit for bit.
__device__ inline float il_mad(float s, float a, float b) {
#pragma clang fp contract(off)
  return s + a * b;
}

// L [n][n] of a lower-triangle net: q on the diagonal, lower_without_diag below it
__device__ inline void il_lower(int n, const float *prm, float L[kIlMaxSc][kIlMaxSc]) {
  const float *l = prm + 2 * n;
  int k = 0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) L[i][j] = 0.f;
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < i; ++j) L[i][j] = l[k++];
    L[i][i] = il_sigmoid(prm[i]);
  }
}

// (Q [n][n], p [n]) of the net `kind` at the parameters prm - one lane, n <= 8
__device__ inline void il_cost_map(int kind, int n, const float *prm, float Q[kIlMaxSc][kIlMaxSc], float p[kIlMaxSc]) {
  float M[kIlMaxSc][kIlMaxSc];
  float pt[kIlMaxSc];
  if (kind == 0 || kind == 2) {
    for (int i = 0; i < n; ++i) {
      const float q = il_sigmoid(prm[i]);
      for (int j = 0; j < n; ++j) M[i][j] = 0.f;
      M[i][i] = q;
      pt[i] = __fmul_rn(sqrtf(q), prm[n + i]);
    }
  } else {
    float L[kIlMaxSc][kIlMaxSc];
    il_lower(n, prm, L);
    for (int i = 0; i < n; ++i) {
      for (int j = 0; j < n; ++j) {
        float s = 0.f;
        for (int k = 0; k < n; ++k) s = il_mad(s, L[i][k], L[j][k]);
        M[i][j] = s;
      }
      pt[i] = prm[n + i];
    }
  }
  if (kind == 2 || kind == 3) {       // Q = O^T M O, p = pt O
    float MO[kIlMaxSc][kIlMaxSc];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        float s = 0.f;
        for (int k = 0; k < 4; ++k) s = il_mad(s, M[i][k], kIlObservation[k][j]);
        MO[i][j] = s;
      }
    for (int i = 0; i < 4; ++i) {
      for (int j = 0; j < 4; ++j) {
        float s = 0.f;
        for (int k = 0; k < 4; ++k) s = il_mad(s, kIlObservation[k][i], MO[k][j]);
        Q[i][j] = s;
      }
      float s = 0.f;
      for (int k = 0; k < 4; ++k) s = il_mad(s, pt[k], kIlObservation[k][i]);
      p[i] = s;
    }
  } else {
    for (int i = 0; i < n; ++i) {
      for (int j = 0; j < n; ++j) Q[i][j] = M[i][j];
      p[i] = pt[i];
    }
  }
}

// Gathers the batch idx[0..B) of one split (tau [N,T,ns], warm [N,T,nu]) into the solver's time-major inputs and tiles the
// cost map over time and batch.  Every workgroup forms (Q, p) in LDS from the parameter vector (a few hundred flops), then
// the grid strides over the outputs; workgroup 0 also writes Q and p.  u_init: the warm start, or zeros when warm is NULL.
__global__ __launch_bounds__(256) void il_batch_begin_kernel(int kind, int N, int T, int B, int nx, int nu, const float *__restrict__ tau,
                                                             const float *__restrict__ warm, const int32_t *__restrict__ idx,
                                                             const float *__restrict__ prm, float *__restrict__ x_init,
                                                             float *__restrict__ us, float *__restrict__ u_init,
                                                             float *__restrict__ Q_out, float *__restrict__ p_out,
                                                             float *__restrict__ C, float *__restrict__ c) {
  const int ns = nx + nu;
  __shared__ float sQ[kIlMaxSc * kIlMaxSc];
  __shared__ float sp[kIlMaxSc];
  if (threadIdx.x == 0) {
    float Q[kIlMaxSc][kIlMaxSc], p[kIlMaxSc];
    il_cost_map(kind, ns, prm, Q, p);
    for (int i = 0; i < ns; ++i) {
      for (int j = 0; j < ns; ++j) sQ[i * ns + j] = Q[i][j];
      sp[i] = p[i];
    }
  }
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0) {
    for (int e = threadIdx.x; e < ns * ns; e += blockDim.x) Q_out[e] = sQ[e];
    for (int e = threadIdx.x; e < ns; e += blockDim.x) p_out[e] = sp[e];
  }
  const size_t TB = (size_t)T * B;
  const size_t nC = TB * ns * ns;
  for (size_t e = tid; e < nC; e += stride) C[e] = sQ[e % (ns * ns)];
  for (size_t e = tid; e < TB * ns; e += stride) c[e] = sp[e % ns];
  for (size_t e = tid; e < (size_t)B * nx; e += stride) {
    const size_t b = e / nx, i = e % nx;
    const int r = idx[b];
    x_init[e] = (r >= 0 && r < N) ? tau[(size_t)r * T * ns + i] : 0.f;
  }
  for (size_t e = tid; e < TB * nu; e += stride) {     // e = (t * B + b) * nu + j
    const size_t j = e % nu, tb = e / nu, b = tb % B, t = tb / B;
    const int r = idx[b];
    const bool in = r >= 0 && r < N;        // (an index outside the split reads and writes nothing)
    const size_t row = (size_t)(in ? r : 0) * T + t;
    us[e] = in ? tau[row * ns + nx + j] : 0.f;
    if (u_init != nullptr) u_init[e] = (warm != nullptr && in) ? warm[row * nu + j] : 0.f;
  }
}

// One workgroup: loss = mean((u - us)^2) over T*B*nu into *loss (a fixed summation order: deterministic), the gradient seed
// grad_u = 2 (u - us) / (T*B*nu) (if grad_u), and u scattered into the split's warm-start buffer warm[idx[b], t, :] (if warm).
__global__ __launch_bounds__(kIlLossThreads) void il_loss_kernel(int N, int T, int B, int nu, const float *__restrict__ u,
                                                                 const float *__restrict__ us, const int32_t *__restrict__ idx,
                                                                 float *__restrict__ loss, float *__restrict__ grad_u,
                                                                 float *__restrict__ warm) {
  __shared__ float part[kIlLossThreads];
  const size_t n = (size_t)T * B * nu;
  const float scale = 2.0f / (float)n;
  float s = 0.f;
  for (size_t e = threadIdx.x; e < n; e += blockDim.x) {
    const float d = u[e] - us[e];
    s += d * d;
    if (grad_u != nullptr) grad_u[e] = scale * d;
    if (warm != nullptr) {
      const size_t j = e % nu, tb = e / nu, b = tb % B, t = tb / B;
      const int r = idx[b];
      if (r >= 0 && r < N) warm[((size_t)r * T + t) * nu + j] = u[e];
    }
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = blockDim.x / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = part[0] / (float)n;
}

// One lane: gradient of the parameters from (dQ [n,n], dp [n]) through the cost map, then RMSprop on the groups whose bit is
// set in enable_mask (1 learn_q_logit, 2 learn_p, 4 lower_without_diag):
//   ms = alpha ms + (1 - alpha) g^2;  theta -= lr g / (sqrt(ms) + eps)
// A disabled group keeps its parameters and its ms bit for bit; grad receives every group's gradient.
__global__ __launch_bounds__(64) void il_param_step_kernel(int kind, int n, const float *__restrict__ dQ,
                                                           const float *__restrict__ dp, float *__restrict__ prm,
                                                           float *__restrict__ ms, float *__restrict__ grad, int enable_mask,
                                                           float lr, float alpha, float eps) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  float dM[kIlMaxSc][kIlMaxSc], dpt[kIlMaxSc];
  if (kind == 2 || kind == 3) {       // dM = O dQ O^T, dpt = O dp
    float dQOt[4][4];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        float s = 0.f;
        for (int k = 0; k < 4; ++k) s += dQ[i * 4 + k] * kIlObservation[j][k];
        dQOt[i][j] = s;
      }
    for (int i = 0; i < 4; ++i) {
      for (int j = 0; j < 4; ++j) {
        float s = 0.f;
        for (int k = 0; k < 4; ++k) s += kIlObservation[i][k] * dQOt[k][j];
        dM[i][j] = s;
      }
      float s = 0.f;
      for (int k = 0; k < 4; ++k) s += kIlObservation[i][k] * dp[k];
      dpt[i] = s;
    }
  } else {
    for (int i = 0; i < n; ++i) {
      for (int j = 0; j < n; ++j) dM[i][j] = dQ[i * n + j];
      dpt[i] = dp[i];
    }
  }
  float g[2 * kIlMaxSc + kIlMaxSc * (kIlMaxSc - 1) / 2];
  if (kind == 0 || kind == 2) {
    for (int i = 0; i < n; ++i) {
      const float q = il_sigmoid(prm[i]);
      const float sq = sqrtf(q);
      // torch's backward formulas: sqrt' = g / (2 sqrt(q)), sigmoid' = g (1 - y) y
      const float dq = __fadd_rn(dM[i][i], __fdiv_rn(__fmul_rn(dpt[i], prm[n + i]), __fmul_rn(2.f, sq)));
      g[i] = __fmul_rn(__fmul_rn(dq, __fsub_rn(1.f, q)), q);
      g[n + i] = __fmul_rn(dpt[i], sq);
    }
  } else {                            // M = L L^T: dL = (dM + dM^T) L
    float L[kIlMaxSc][kIlMaxSc];
    il_lower(n, prm, L);
    float dL[kIlMaxSc][kIlMaxSc];
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        float s = 0.f;
        for (int k = 0; k < n; ++k) s += (dM[i][k] + dM[k][i]) * L[k][j];
        dL[i][j] = s;
      }
    int k = 2 * n;
    for (int i = 0; i < n; ++i) {
      for (int j = 0; j < i; ++j) g[k++] = dL[i][j];
      const float q = L[i][i];
      g[i] = __fmul_rn(__fmul_rn(dL[i][i], __fsub_rn(1.f, q)), q);
      g[n + i] = dpt[i];
    }
  }
  const int np = il_n_params(kind, n);
  for (int e = 0; e < np; ++e) {
    grad[e] = g[e];
    const int bit = e < n ? 1 : (e < 2 * n ? 2 : 4);
    if (!(enable_mask & bit)) continue;
    const float m = alpha * ms[e] + (1.f - alpha) * (g[e] * g[e]);
    ms[e] = m;
    prm[e] = prm[e] - lr * (g[e] / (sqrtf(m) + eps));
  }
}

}  // namespace dmpc
