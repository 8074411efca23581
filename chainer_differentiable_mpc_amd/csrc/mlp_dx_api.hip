// mlp_dx_api.hip - C-ABI entry points of the learned dynamics model with one or two hidden layers (include/dmpc.h section E,
// "MlpDx"): the nominal rollout with its analytic linearisation, MPCstep.forward_rec with the network as the true
// dynamics, and the gradient of the linearisation's f with respect to the weights (one hidden layer: include/dmpc.h; two:
// include/dmpc_mlp_grad.h; both over mlp_grad_entry of mlp_dx_host.hpp).  Every argument and size check comes before the first
// HIP call.  The activation and the depth are template parameters of the kernels; mlp_with_act and the launchers pick the instance.  `n_hidden` is the code H1 | (H2 << 16) of DMPC_MLP_HIDDEN2 throughout.
#include <hip/hip_runtime.h>

#include "../../include/dmpc.h"
#include "../../include/dmpc_mlp_grad.h"
#include "mlp_dx_host.hpp"

namespace dmpc {

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
  return mlp_grad_workspace(B, nx, nu, n_hidden);
}

int dmpc_mlp_param_grad(int T, int B, int nx, int nu, int n_hidden, int act, int residual, const float *W1,
                        const float *b1, const float *W2, const float *b2, const float *x, const float *u,
                        const float *grad_f, float *dW1, float *db1, float *dW2, float *db2, float *d_x_init, float *d_u,
                        void *ws, size_t ws_bytes, dmpc_stream_t stream_) {
  return mlp_grad_entry<false>(/*only_depth=*/1, T, B, nx, nu, n_hidden, act, residual, W1, b1, W2, b2, x, u, grad_f, dW1, db1, dW2,
                               db2, d_x_init, d_u, ws, ws_bytes, static_cast<hipStream_t>(stream_));
}

// ---- two hidden layers (include/dmpc_mlp_grad.h) ----
int dmpc_mlp2_param_grad_partials(int B) { return B > 0 ? mlp2_grad_partials(B) : 0; }

size_t dmpc_mlp2_param_grad_workspace_bytes(int B, int nx, int nu, int n_hidden) {
  if (B <= 0 || mlp_check(nx, nu, n_hidden, 0) != 0 || mlp_hidden2(n_hidden) == 0) return 0;   // (two hidden layers only)
  return mlp_grad_workspace(B, nx, nu, n_hidden);
}

int dmpc_mlp2_param_grad(int T, int B, int nx, int nu, int n_hidden, int act, int residual, const float *W1,
                         const float *b1, const float *W2, const float *b2, const float *x, const float *u,
                         const float *grad_f, float *dW1, float *db1, float *dW2, float *db2, float *d_x_init, float *d_u,
                         void *ws, size_t ws_bytes, dmpc_stream_t stream_) {
  return mlp_grad_entry<false>(/*only_depth=*/2, T, B, nx, nu, n_hidden, act, residual, W1, b1, W2, b2, x, u, grad_f, dW1, db1, dW2,
                               db2, d_x_init, d_u, ws, ws_bytes, static_cast<hipStream_t>(stream_));
}

}  // extern "C"
