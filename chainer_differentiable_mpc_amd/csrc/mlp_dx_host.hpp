// mlp_dx_host.hpp - the host side that the two MlpDx translation units share (mlp_dx_api.hip, mlp_rollout_grad_api.hip): the size
// check, the activation dispatch, the launch with dynamic LDS, and THE entry point of the gradient sweeps
// (mlp_grad_kernels.hpp) - checks, T = 1, launch, reduce.  Everything is static or a template: each translation unit
// instantiates the kernels of its own entry points and no others.  `n_hidden` is the code H1 | (H2 << 16) of DMPC_MLP_HIDDEN2.
#pragma once
#include <type_traits>

#include "../../include/dmpc.h"
#include "api_util.hpp"
#include "mlp_grad_kernels.hpp"

namespace dmpc {

// 0: launch; DMPC_E_BADARG / DMPC_E_UNSUPPORTED otherwise
static int mlp_check(int nx, int nu, int n_hidden, int act) {
  if (nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (act != kMlpActTanh && act != kMlpActRelu && act != kMlpActSilu && act != kMlpActSoftplus) return DMPC_E_UNSUPPORTED;
  if (nx > kMlpMaxNx || nu > kMlpMaxNu || n_hidden < 1) return DMPC_E_UNSUPPORTED;
  const int H1 = mlp_hidden1(n_hidden), H2 = mlp_hidden2(n_hidden);
  if (H2 == 0 ? H1 > mlp_max_hidden(1) : (H1 < 1 || H1 > mlp_max_hidden(2) || H2 > mlp_max_hidden(2))) return DMPC_E_UNSUPPORTED;
  if (mlp_lds_bytes(nx, nu, H1, H2) > kMlpLdsLimit) return DMPC_E_UNSUPPORTED;
  return 0;
}

// fn(std::integral_constant<int, ACT>) for an `act` that mlp_check has passed
template <typename Fn>
static void mlp_with_act(int act, Fn &&fn) {
  switch (act) {
    case kMlpActRelu: fn(std::integral_constant<int, kMlpActRelu>{}); break;
    case kMlpActSilu: fn(std::integral_constant<int, kMlpActSilu>{}); break;
    case kMlpActSoftplus: fn(std::integral_constant<int, kMlpActSoftplus>{}); break;
    default: fn(std::integral_constant<int, kMlpActTanh>{}); break;
  }
}

// launch `kernel` with `bytes` of dynamic LDS, one wavefront for each of B; beyond the 64 KB a kernel has by default the limit is raised first
template <typename K, typename... Args>
static void mlp_launch(K kernel, int B, size_t bytes, hipStream_t stream, const Args &...args) {
  if (bytes > 64 * 1024) set_max_lds(reinterpret_cast<const void *>(kernel), (int)bytes);
  DMPC_LAUNCH_GGL(kernel, dim3((B + kMlpWaves - 1) / kMlpWaves), dim3(64 * kMlpWaves), bytes, stream, args...);
}

// ---- the gradient sweeps.  The partials of a sweep over B trajectories and the floats of one, for sizes mlp_check has passed
static int mlp_grad_partials_of(int B, int n_hidden) { return mlp_hidden2(n_hidden) == 0 ? mlp_grad_partials(B) : mlp2_grad_partials(B); }
static size_t mlp_grad_workspace(int B, int nx, int nu, int n_hidden) {
  const int H1 = mlp_hidden1(n_hidden), H2 = mlp_hidden2(n_hidden);
  const int P = H2 == 0 ? mlp_grad_partial_floats(nx, nu, H1) : mlp2_grad_partial_floats(nx, nu, H1, H2);
  return (size_t)mlp_grad_partials_of(B, n_hidden) * P * sizeof(float);
}

// dmpc_mlp_param_grad (only_depth 1), dmpc_mlp2_param_grad (2): CARRY = false, g = dL/df [T-1,B,nx], needed when T > 1;
// dmpc_mlp_rollout_grad (only_depth 0: either): CARRY = true, g = dL/dx [T,B,nx].  Every check comes before the first HIP call.
template <bool CARRY>
static int mlp_grad_entry(int only_depth, int T, int B, int nx, int nu, int n_hidden, int act, int residual, const float *W1,
                          const float *b1, const float *W2, const float *b2, const float *x, const float *u, const float *g,
                          float *dW1, float *db1, float *dW2, float *db2, float *d_x_init, float *d_u, void *ws, size_t ws_bytes,
                          hipStream_t stream) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!W1 || !b1 || !W2 || !b2 || !x || !u || !dW1 || !db1 || !dW2 || !db2) return DMPC_E_BADARG;
  if ((CARRY || T > 1) && !g) return DMPC_E_BADARG;
  const int rc = mlp_check(nx, nu, n_hidden, act);
  if (rc != 0) return rc;
  const int H1 = mlp_hidden1(n_hidden), H2 = mlp_hidden2(n_hidden), depth = H2 == 0 ? 1 : 2;
  if (only_depth != 0 && depth != only_depth) return DMPC_E_UNSUPPORTED;   // the other depth has an entry point of its own
  if ((size_t)T * B * nx * (nx + nu) >= ((size_t)1 << 31)) return DMPC_E_UNSUPPORTED;   // (the rollout's own limit)
  if (T > 1 && (ws == nullptr || ws_bytes < mlp_grad_workspace(B, nx, nu, n_hidden))) return DMPC_E_WORKSPACE;
  const int G = T > 1 ? mlp_grad_partials_of(B, n_hidden) : 0;
  if (T == 1) {            // no dynamics step: the state IS x_init, nothing reaches u or a weight
    hipError_t e = hipSuccess;
    if (d_x_init != nullptr)
      e = CARRY ? hipMemcpyAsync(d_x_init, g, (size_t)B * nx * sizeof(float), hipMemcpyDeviceToDevice, stream)
                : hipMemsetAsync(d_x_init, 0, (size_t)B * nx * sizeof(float), stream);
    if (e == hipSuccess && d_u != nullptr) e = hipMemsetAsync(d_u, 0, (size_t)B * nu * sizeof(float), stream);
    if (e != hipSuccess) return (int)e;
  } else {
    // (the rollout kernels take a derived, empty struct only so that each kernel keeps the full name a profiler lists)
    using Args = std::conditional_t<CARRY, MlpRolloutGradArgs, MlpGradArgs>;
    const MlpGradArgs base{T, B, G, mlp_model(nx, nu, n_hidden, residual, W1, b1, W2, b2), x, u, g, static_cast<float *>(ws), d_x_init, d_u};
    const Args ga{base};
    mlp_with_act(act, [&](auto A) {
      constexpr int ACT = decltype(A)::value;
      void (*one)(const Args), (*two)(const Args);
      if constexpr (CARRY) one = &mlp_rollout_grad_kernel<ACT>, two = &mlp2_rollout_grad_kernel<ACT>;
      else one = &mlp_param_grad_kernel<ACT>, two = &mlp2_param_grad_kernel<ACT>;
      if (depth == 1) mlp_launch(one, G, mlp_lds_bytes(nx, nu, H1), stream, ga);                        // G wavefronts
      else mlp_launch(two, G * kMlpWaves, mlp2_grad_lds_bytes(nx, nu, H1, H2), stream, ga);             // G workgroups
    });
  }
  const MlpGradReduceArgs rd{G, H1 * (nx + nu), H1, depth == 1 ? nx * H1 : H2 * H1 + nx * H2, depth == 1 ? nx : H2 + nx,
                             static_cast<const float *>(ws), dW1, db1, dW2, db2};
  const dim3 grid((rd.n1 + rd.nb1 + rd.n2 + rd.nb2 + 255) / 256);
  if (depth == 1) DMPC_LAUNCH_GGL(mlp_param_grad_reduce_kernel, grid, dim3(256), 0, stream, rd);
  else DMPC_LAUNCH_GGL(mlp2_param_grad_reduce_kernel, grid, dim3(256), 0, stream, Mlp2GradReduceArgs{rd});
  return (int)hipGetLastError();
}

}  // namespace dmpc
