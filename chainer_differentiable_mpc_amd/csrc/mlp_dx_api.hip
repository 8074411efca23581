// mlp_dx_api.hip - C-ABI entry points of the learned dynamics model with one or two hidden layers (include/dmpc.h section E,
// "MlpDx"): the nominal rollout with its analytic linearisation, MPCstep.forward_rec with the network as the true
// dynamics, and the gradient of the linearisation's f with respect to the weights (one hidden layer: include/dmpc.h; two:
// include/dmpc_mlp_grad.h).  Every argument and size check comes before the first HIP call.  The activation and the depth are template parameters of the kernels; mlp_with_act and
// the launchers pick the instance.  `n_hidden` is the code H1 | (H2 << 16) of DMPC_MLP_HIDDEN2 throughout.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/dmpc.h"
#include "../../include/dmpc_mlp_grad.h"
#include "api_util.hpp"
#include "mlp_dx_kernels.hpp"

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

// launch `kernel` with `bytes` of dynamic LDS; beyond the 64 KB a kernel has by default the limit is raised first
template <typename K, typename... Args>
static void mlp_launch(K kernel, int B, size_t bytes, hipStream_t stream, const Args &...args) {
  if (bytes > 64 * 1024) set_max_lds(reinterpret_cast<const void *>(kernel), (int)bytes);
  DMPC_LAUNCH_GGL(kernel, dim3((B + kMlpWaves - 1) / kMlpWaves), dim3(64 * kMlpWaves), bytes, stream, args...);
}

// the two launchers of mlp_dx_launch.hpp: the entry points below and dmpc_box_ddp's chain (mpc_api.hip) go through them
void launch_mlp_rollout(const MlpRolloutArgs &a, int act, hipStream_t stream) {
  const size_t bytes = mlp_lds_bytes(a.m.nx, a.m.nu, a.m.H[0], a.m.H[1], a.F != nullptr);
  mlp_with_act(act, [&](auto A) {
    constexpr int ACT = decltype(A)::value;
    void (*kernel)(const MlpRolloutArgs) =
        a.m.depth == 2 ? &mlp_rollout_linearize_kernel<ACT, 2> : &mlp_rollout_linearize_kernel<ACT>;
    mlp_launch(kernel, a.B, bytes, stream, a);
  });
}

void launch_mlp_search(const MpcFwdArgs &a, const MlpModel &m, int act, hipStream_t stream) {
  const size_t bytes = mlp_lds_bytes(m.nx, m.nu, m.H[0], m.H[1], a.F_next != nullptr);
  mlp_with_act(act, [&](auto A) {
    constexpr int ACT = decltype(A)::value;
    void (*kernel)(const MpcFwdArgs, const MlpModel) =
        m.depth == 2 ? &mpc_forward_rec_mlp_kernel<ACT, 2> : &mpc_forward_rec_mlp_kernel<ACT>;
    mlp_launch(kernel, a.B, bytes, stream, a, m);
  });
}

}  // namespace dmpc

using namespace dmpc;

extern "C" {

int dmpc_mlp_dx_supported(int nx, int nu, int n_hidden, int act) { return mlp_check(nx, nu, n_hidden, act) == 0 ? 1 : 0; }

int dmpc_mlp_rollout_linearize(int T, int B, int nx, int nu, int n_hidden, int act, int residual, const float *W1,
                               const float *b1, const float *W2, const float *b2, const float *x_init, const float *u,
                               float *x_out, float *F_out, float *f_out, dmpc_stream_t stream_) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!W1 || !b1 || !W2 || !b2 || !x_init || !u || !x_out) return DMPC_E_BADARG;
  if (f_out != nullptr && F_out == nullptr) return DMPC_E_BADARG;
  const int rc = mlp_check(nx, nu, n_hidden, act);
  if (rc != 0) return rc;
  if ((size_t)T * B * nx * (nx + nu) >= ((size_t)1 << 31)) return DMPC_E_UNSUPPORTED;
  MlpRolloutArgs ra{T, B, mlp_model(nx, nu, n_hidden, residual, W1, b1, W2, b2), x_init, u, x_out, F_out, f_out};
  launch_mlp_rollout(ra, act, static_cast<hipStream_t>(stream_));   // (no `done` flag, nothing to clear)
  return (int)hipGetLastError();
}

int dmpc_mpc_forward_rec_mlp(int T, int B, int nx, int nu, int n_hidden, int act, int residual, const float *W1,
                             const float *b1, const float *W2, const float *b2, const float *Ks, const float *ks,
                             const float *controls, const float *states, const float *u_lower, const float *u_upper,
                             const float *C_true, const float *c_true, float ls_decay, int max_ls_iter, float *x_out,
                             float *u_out, float *costs, float *old_costs, float *alphas, float *objs, float *u_first,
                             int32_t *n_ls_iter, int32_t *info, dmpc_stream_t stream_) {
  if (T <= 1 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!W1 || !b1 || !W2 || !b2 || !Ks || !ks || !controls || !states || !u_lower || !u_upper || !C_true || !c_true ||
      !x_out || !u_out || !costs || !alphas || !n_ls_iter)
    return DMPC_E_BADARG;
  const int rc = mlp_check(nx, nu, n_hidden, act);
  if (rc != 0) return rc;
  if ((size_t)T * B * (nx + nu) * (nx + nu) >= ((size_t)1 << 31)) return DMPC_E_UNSUPPORTED;
  MpcFwdArgs fa{T, B, Ks, ks, controls, states, u_lower, u_upper, C_true, c_true, nullptr, nullptr, ls_decay,
                max_ls_iter, /*ls_cap=*/64, x_out, u_out, u_first, costs, old_costs, alphas, objs, n_ls_iter, info};
  const MlpModel m = mlp_model(nx, nu, n_hidden, residual, W1, b1, W2, b2);
  launch_mlp_search(fa, m, act, static_cast<hipStream_t>(stream_));  // (fa.done, fa.F_next: nullptr)
  return (int)hipGetLastError();
}

int dmpc_mlp_param_grad_partials(int B) { return B > 0 ? mlp_grad_partials(B) : 0; }

size_t dmpc_mlp_param_grad_workspace_bytes(int B, int nx, int nu, int n_hidden) {
  if (B <= 0 || mlp_check(nx, nu, n_hidden, 0) != 0 || mlp_hidden2(n_hidden) != 0) return 0;   // (one hidden layer only)
  return (size_t)mlp_grad_partials(B) * mlp_grad_partial_floats(nx, nu, n_hidden) * sizeof(float);
}

int dmpc_mlp_param_grad(int T, int B, int nx, int nu, int n_hidden, int act, int residual, const float *W1,
                        const float *b1, const float *W2, const float *b2, const float *x, const float *u,
                        const float *grad_f, float *dW1, float *db1, float *dW2, float *db2, float *d_x_init, float *d_u,
                        void *ws, size_t ws_bytes, dmpc_stream_t stream_) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!W1 || !b1 || !W2 || !b2 || !x || !u || !dW1 || !db1 || !dW2 || !db2) return DMPC_E_BADARG;
  if (T > 1 && !grad_f) return DMPC_E_BADARG;
  const int rc = mlp_check(nx, nu, n_hidden, act);
  if (rc != 0) return rc;
  if (mlp_hidden2(n_hidden) != 0) return DMPC_E_UNSUPPORTED;   // two hidden layers: the weight gradient is the live route's
  if ((size_t)T * B * nx * (nx + nu) >= ((size_t)1 << 31)) return DMPC_E_UNSUPPORTED;   // (the rollout's own limit)
  if (T > 1 && (ws == nullptr || ws_bytes < dmpc_mlp_param_grad_workspace_bytes(B, nx, nu, n_hidden))) return DMPC_E_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int G = T > 1 ? mlp_grad_partials(B) : 0;
  if (T == 1) {            // no dynamics step: every gradient is zero
    hipError_t e = hipSuccess;
    if (d_x_init != nullptr) e = hipMemsetAsync(d_x_init, 0, (size_t)B * nx * sizeof(float), stream);
    if (e == hipSuccess && d_u != nullptr) e = hipMemsetAsync(d_u, 0, (size_t)B * nu * sizeof(float), stream);
    if (e != hipSuccess) return (int)e;
  } else {
    MlpGradArgs ga{T, B, G, mlp_model(nx, nu, n_hidden, residual, W1, b1, W2, b2), x, u, grad_f, static_cast<float *>(ws), d_x_init, d_u};
    mlp_with_act(act, [&](auto A) {
      DMPC_LAUNCH_GGL(mlp_param_grad_kernel<decltype(A)::value>, dim3((G + kMlpWaves - 1) / kMlpWaves),
                      dim3(64 * kMlpWaves), mlp_lds_bytes(nx, nu, n_hidden), stream, ga);
    });
  }
  MlpGradReduceArgs rd{G, nx, nu, n_hidden, static_cast<const float *>(ws), dW1, db1, dW2, db2};
  DMPC_LAUNCH_GGL(mlp_param_grad_reduce_kernel, dim3((mlp_grad_partial_floats(nx, nu, n_hidden) + 255) / 256), dim3(256), 0,
                  stream, rd);
  return (int)hipGetLastError();
}

// ---- two hidden layers (include/dmpc_mlp_grad.h) ----
int dmpc_mlp2_param_grad_partials(int B) { return B > 0 ? mlp2_grad_partials(B) : 0; }

size_t dmpc_mlp2_param_grad_workspace_bytes(int B, int nx, int nu, int n_hidden) {
  if (B <= 0 || mlp_check(nx, nu, n_hidden, 0) != 0 || mlp_hidden2(n_hidden) == 0) return 0;   // (two hidden layers only)
  return (size_t)mlp2_grad_partials(B) * mlp2_grad_partial_floats(nx, nu, mlp_hidden1(n_hidden), mlp_hidden2(n_hidden)) * sizeof(float);
}

int dmpc_mlp2_param_grad(int T, int B, int nx, int nu, int n_hidden, int act, int residual, const float *W1,
                         const float *b1, const float *W2, const float *b2, const float *x, const float *u,
                         const float *grad_f, float *dW1, float *db1, float *dW2, float *db2, float *d_x_init, float *d_u,
                         void *ws, size_t ws_bytes, dmpc_stream_t stream_) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!W1 || !b1 || !W2 || !b2 || !x || !u || !dW1 || !db1 || !dW2 || !db2) return DMPC_E_BADARG;
  if (T > 1 && !grad_f) return DMPC_E_BADARG;
  const int rc = mlp_check(nx, nu, n_hidden, act);
  if (rc != 0) return rc;
  const int H1 = mlp_hidden1(n_hidden), H2 = mlp_hidden2(n_hidden);
  if (H2 == 0) return DMPC_E_UNSUPPORTED;   // one hidden layer: dmpc_mlp_param_grad
  if ((size_t)T * B * nx * (nx + nu) >= ((size_t)1 << 31)) return DMPC_E_UNSUPPORTED;   // (the rollout's own limit)
  if (T > 1 && (ws == nullptr || ws_bytes < dmpc_mlp2_param_grad_workspace_bytes(B, nx, nu, n_hidden))) return DMPC_E_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int G = T > 1 ? mlp2_grad_partials(B) : 0;
  if (T == 1) {            // no dynamics step: every gradient is zero
    hipError_t e = hipSuccess;
    if (d_x_init != nullptr) e = hipMemsetAsync(d_x_init, 0, (size_t)B * nx * sizeof(float), stream);
    if (e == hipSuccess && d_u != nullptr) e = hipMemsetAsync(d_u, 0, (size_t)B * nu * sizeof(float), stream);
    if (e != hipSuccess) return (int)e;
  } else {
    MlpGradArgs ga{T, B, G, mlp_model(nx, nu, n_hidden, residual, W1, b1, W2, b2), x, u, grad_f, static_cast<float *>(ws), d_x_init, d_u};
    mlp_with_act(act, [&](auto A) {      // a grid of G workgroups: mlp_launch counts four trajectories to one
      mlp_launch(&mlp2_param_grad_kernel<decltype(A)::value>, G * kMlpWaves, mlp2_grad_lds_bytes(nx, nu, H1, H2), stream, ga);
    });
  }
  Mlp2GradReduceArgs rd{G, H1 * (nx + nu), H1, H2 * H1 + nx * H2, H2 + nx, static_cast<const float *>(ws), dW1, db1, dW2, db2};
  DMPC_LAUNCH_GGL(mlp2_param_grad_reduce_kernel, dim3((mlp2_grad_partial_floats(nx, nu, H1, H2) + 255) / 256), dim3(256), 0,
                  stream, rd);
  return (int)hipGetLastError();
}

}  // extern "C"
