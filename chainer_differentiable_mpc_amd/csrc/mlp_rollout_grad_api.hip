// mlp_rollout_grad_api.hip - C-ABI entry points of include/dmpc_mlp_rollout_grad.h: the vector-Jacobian product of the MlpDx
// rollout, the reverse sweep that carries the co-state (mlp_grad_kernels.hpp) and the fixed-order reduction of its partials, over
// the entry point the weight gradients share (mlp_grad_entry, mlp_dx_host.hpp).  Every argument and size check comes before the
// first HIP call.  No environment variable is read here.
#include <hip/hip_runtime.h>

#include "../../include/dmpc.h"
#include "../../include/dmpc_mlp_rollout_grad.h"
#include "api_util.hpp"
// the kernel headers with internal linkage: this translation unit's instances of the templates are its own, and it neither
// defines mlp_dx_api.hip's non-template kernels a second time nor emits the ones it does not launch
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "mlp_dx_host.hpp"
#pragma clang attribute pop

using namespace dmpc;

extern "C" {

int dmpc_mlp_rollout_grad_partials(int B, int n_hidden) {
  if (B <= 0 || n_hidden < 1) return 0;
  return mlp_grad_partials_of(B, n_hidden);
}

size_t dmpc_mlp_rollout_grad_workspace_bytes(int B, int nx, int nu, int n_hidden) {
  if (B <= 0 || mlp_check(nx, nu, n_hidden, kMlpActTanh) != 0) return 0;
  return mlp_grad_workspace(B, nx, nu, n_hidden);
}

int dmpc_mlp_rollout_grad(int T, int B, int nx, int nu, int n_hidden, int act, int residual, const float *W1,
                          const float *b1, const float *W2, const float *b2, const float *x, const float *u,
                          const float *grad_x, float *dW1, float *db1, float *dW2, float *db2, float *d_x_init, float *d_u,
                          void *ws, size_t ws_bytes, dmpc_stream_t stream_) {
  return mlp_grad_entry<true>(/*only_depth=*/0, T, B, nx, nu, n_hidden, act, residual, W1, b1, W2, b2, x, u, grad_x, dW1, db1, dW2,
                              db2, d_x_init, d_u, ws, ws_bytes, static_cast<hipStream_t>(stream_));
}

}  // extern "C"
