// mlp_rollout_grad_api.hip - C-ABI entry points of include/dmpc_mlp_rollout_grad.h: the vector-Jacobian product of the MlpDx
// rollout, one reverse-sweep kernel that carries the co-state (mlp_rollout_grad_kernels.hpp) and the fixed-order reduction of
// the weight gradient's entry points (mlp_dx_kernels.hpp), whose partial layouts and caps the sweep keeps.  Every argument and
// size check comes before the first HIP call.  No environment variable is read here.
#include <hip/hip_runtime.h>

#include "../../include/dmpc.h"
#include "../../include/dmpc_mlp_rollout_grad.h"
#include "api_util.hpp"
// the kernel headers with internal linkage: this translation unit's instances of the templates are its own, and it neither
// defines mlp_dx_api.hip's non-template kernels a second time nor emits the ones it does not launch
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "mlp_rollout_grad_kernels.hpp"
#pragma clang attribute pop

namespace dmpc {

template <int ACT>
static void launch_rollout_grad_as(const MlpRolloutGradArgs &a, hipStream_t stream) {
  const MlpModel &m = a.m;
  if (m.depth == 2) {       // a grid of G workgroups
    void (*kernel)(const MlpRolloutGradArgs) = &mlp2_rollout_grad_kernel<ACT>;
    const size_t bytes = mlp2_grad_lds_bytes(m.nx, m.nu, m.H[0], m.H[1]);
    if (bytes > 64 * 1024) set_max_lds(reinterpret_cast<const void *>(kernel), (int)bytes);
    DMPC_LAUNCH_GGL(kernel, dim3(a.G), dim3(64 * kMlpWaves), bytes, stream, a);
  } else {                  // G wavefronts, four per workgroup
    void (*kernel)(const MlpRolloutGradArgs) = &mlp_rollout_grad_kernel<ACT>;
    DMPC_LAUNCH_GGL(kernel, dim3((a.G + kMlpWaves - 1) / kMlpWaves), dim3(64 * kMlpWaves), mlp_lds_bytes(m.nx, m.nu, m.H[0]), stream, a);
  }
}

// an `act` that dmpc_mlp_dx_supported has passed
static void launch_rollout_grad(const MlpRolloutGradArgs &a, int act, hipStream_t stream) {
  switch (act) {
    case kMlpActRelu: launch_rollout_grad_as<kMlpActRelu>(a, stream); break;
    case kMlpActSilu: launch_rollout_grad_as<kMlpActSilu>(a, stream); break;
    case kMlpActSoftplus: launch_rollout_grad_as<kMlpActSoftplus>(a, stream); break;
    default: launch_rollout_grad_as<kMlpActTanh>(a, stream); break;
  }
}

static size_t rollout_grad_partial_floats(int nx, int nu, int n_hidden) {
  const int H1 = mlp_hidden1(n_hidden), H2 = mlp_hidden2(n_hidden);
  return H2 == 0 ? mlp_grad_partial_floats(nx, nu, H1) : mlp2_grad_partial_floats(nx, nu, H1, H2);
}

}  // namespace dmpc

using namespace dmpc;

extern "C" {

int dmpc_mlp_rollout_grad_partials(int B, int n_hidden) {
  if (B <= 0 || n_hidden < 1) return 0;
  return mlp_hidden2(n_hidden) == 0 ? mlp_grad_partials(B) : mlp2_grad_partials(B);
}

size_t dmpc_mlp_rollout_grad_workspace_bytes(int B, int nx, int nu, int n_hidden) {
  if (B <= 0 || nx <= 0 || nu <= 0 || !dmpc_mlp_dx_supported(nx, nu, n_hidden, kMlpActTanh)) return 0;
  return (size_t)dmpc_mlp_rollout_grad_partials(B, n_hidden) * rollout_grad_partial_floats(nx, nu, n_hidden) * sizeof(float);
}

int dmpc_mlp_rollout_grad(int T, int B, int nx, int nu, int n_hidden, int act, int residual, const float *W1,
                          const float *b1, const float *W2, const float *b2, const float *x, const float *u,
                          const float *grad_x, float *dW1, float *db1, float *dW2, float *db2, float *d_x_init, float *d_u,
                          void *ws, size_t ws_bytes, dmpc_stream_t stream_) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!W1 || !b1 || !W2 || !b2 || !x || !u || !grad_x || !dW1 || !db1 || !dW2 || !db2) return DMPC_E_BADARG;
  if (!dmpc_mlp_dx_supported(nx, nu, n_hidden, act)) return DMPC_E_UNSUPPORTED;
  if ((size_t)T * B * nx * (nx + nu) >= ((size_t)1 << 31)) return DMPC_E_UNSUPPORTED;   // (the rollout's own limit)
  if (T > 1 && (ws == nullptr || ws_bytes < dmpc_mlp_rollout_grad_workspace_bytes(B, nx, nu, n_hidden))) return DMPC_E_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int H1 = mlp_hidden1(n_hidden), H2 = mlp_hidden2(n_hidden);
  const int G = T > 1 ? dmpc_mlp_rollout_grad_partials(B, n_hidden) : 0;
  if (T == 1) {            // no dynamics step: the state IS x_init, nothing reaches u or a weight
    hipError_t e = hipSuccess;
    if (d_x_init != nullptr) e = hipMemcpyAsync(d_x_init, grad_x, (size_t)B * nx * sizeof(float), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess && d_u != nullptr) e = hipMemsetAsync(d_u, 0, (size_t)B * nu * sizeof(float), stream);
    if (e != hipSuccess) return (int)e;
  } else {
    MlpRolloutGradArgs ga{T, B, G, mlp_model(nx, nu, n_hidden, residual, W1, b1, W2, b2), x, u, grad_x, static_cast<float *>(ws), d_x_init, d_u};
    launch_rollout_grad(ga, act, stream);
  }
  const int P = (int)rollout_grad_partial_floats(nx, nu, n_hidden);
  if (H2 == 0) {
    MlpGradReduceArgs rd{G, nx, nu, n_hidden, static_cast<const float *>(ws), dW1, db1, dW2, db2};
    DMPC_LAUNCH_GGL(mlp_param_grad_reduce_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, rd);
  } else {
    Mlp2GradReduceArgs rd{G, H1 * (nx + nu), H1, H2 * H1 + nx * H2, H2 + nx, static_cast<const float *>(ws), dW1, db1, dW2, db2};
    DMPC_LAUNCH_GGL(mlp2_param_grad_reduce_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, rd);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
