// il_api.hip - the imitation-learning update around the box-DDP chain (include/dmpc.h): batch gather + cost map,
// imitation loss + gradient seed + warm-start scatter, and the parameter step (chain rule + RMSprop).  il_exp.py drives them.
#include <hip/hip_runtime.h>

#include "../../include/dmpc.h"
#include "api_util.hpp"
#include "il_kernels.hpp"

using namespace dmpc;

namespace {

bool il_kind_ok(int kind, int n_sc) {
  if (kind < 0 || kind > 3 || n_sc < 1 || n_sc > kIlMaxSc) return false;
  return kind < 2 || n_sc == 4;        // OBSERVATION_MATRIX is 4 x 4
}

}  // namespace

extern "C" {

int dmpc_il_n_params(int kind, int n_sc) {
  if (!il_kind_ok(kind, n_sc)) return DMPC_E_UNSUPPORTED;
  return il_n_params(kind, n_sc);
}

int dmpc_il_batch_begin(int kind, int N, int T, int B, int nx, int nu, const float *tau, const float *warm,
                        const int32_t *idx, const float *params, float *x_init, float *us, float *u_init, float *Q,
                        float *p, float *C, float *c, dmpc_stream_t stream_) {
  if (N <= 0 || T <= 0 || B <= 0 || nx <= 0 || nu <= 0 || !tau || !idx || !params || !x_init || !us || !Q || !p || !C ||
      !c)
    return DMPC_E_BADARG;
  if (!il_kind_ok(kind, nx + nu)) return DMPC_E_UNSUPPORTED;
  if ((size_t)T * B * (nx + nu) * (nx + nu) >= (size_t(1) << 31)) return DMPC_E_UNSUPPORTED;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const size_t work = (size_t)T * B * (nx + nu) * (nx + nu);
  const int grid = (int)((work + 255) / 256 < 1024 ? (work + 255) / 256 : 1024);
  DMPC_LAUNCH_GGL(il_batch_begin_kernel, dim3(grid), dim3(256), 0, stream, kind, N, T, B, nx, nu, tau, warm, idx, params,
                  x_init, us, u_init, Q, p, C, c);
  return (int)hipGetLastError();
}

int dmpc_il_loss(int N, int T, int B, int nu, const float *u, const float *us, const int32_t *idx, float *loss,
                 float *grad_u, float *warm, dmpc_stream_t stream_) {
  if (N <= 0 || T <= 0 || B <= 0 || nu <= 0 || !u || !us || !loss || (warm && !idx)) return DMPC_E_BADARG;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DMPC_LAUNCH_GGL(il_loss_kernel, dim3(1), dim3(kIlLossThreads), 0, stream, N, T, B, nu, u, us, idx, loss, grad_u, warm);
  return (int)hipGetLastError();
}

int dmpc_il_param_step(int kind, int n_sc, const float *dQ, const float *dp, float *params, float *ms, float *grad,
                       int enable_mask, float lr, float alpha, float eps, dmpc_stream_t stream_) {
  if (!dQ || !dp || !params || !ms || !grad) return DMPC_E_BADARG;
  if (!il_kind_ok(kind, n_sc)) return DMPC_E_UNSUPPORTED;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DMPC_LAUNCH_GGL(il_param_step_kernel, dim3(1), dim3(64), 0, stream, kind, n_sc, dQ, dp, params, ms, grad, enable_mask, lr,
                  alpha, eps);
  return (int)hipGetLastError();
}

}  // extern "C"
