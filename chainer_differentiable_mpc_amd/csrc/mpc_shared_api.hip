// mpc_shared_api.hip - MPCstep.backward (mpc/mpc_step.py:330-460) for dynamics that are ONE [A|B] tiled over the batch (and
// over time): the parameter-shaped gradients of mpc/mpc_net.py's learnable models (include/dmpc.h,
// dmpc_mpc_step_backward_shared).  The chain of dmpc_mpc_step_backward with the co-state kernel writing its
// rows lambda_t, d_lambda_t instead of dense dC / dF, then the fixed-order reduction of the shared LQR (lqr_shared.hpp 3b,
// 3c) with the MPC step's output sign: no [T,B,ns,ns] or [T-1,B,nx,ns] gradient exists, no atomics, no host decision.
#include <hip/hip_runtime.h>

#include "../../include/dmpc.h"
#include "api_util.hpp"
#include "costate_args.hpp"

using namespace dmpc;

namespace {

constexpr uint32_t kTimeBits = DMPC_SHARED_C_TIME | DMPC_SHARED_F_TIME | DMPC_SHARED_CVEC_TIME | DMPC_SHARED_FVEC_TIME;

// -[grad_x; grad_u] | x_init = 0 | d_tau' = (dx, du) | active set | lambda, d_lambda | partials | the LQR solve's workspace
struct SharedMpcWs {
  size_t neg, x0, dx, du, mask, lam, dlam, part, lqr, total;
};
SharedMpcWs ws_layout(int T, int B, int nx, int nu) {
  SharedMpcWs w{};
  const size_t tb = (size_t)T * B;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += round_up(bytes, 256);
    return o;
  };
  w.neg = take(tb * (nx + nu) * sizeof(float));
  w.x0 = take((size_t)B * nx * sizeof(float));
  w.dx = take(tb * nx * sizeof(float));
  w.du = take(tb * nu * sizeof(float));
  w.mask = take(tb * nu);
  w.lam = take(tb * nx * sizeof(float));
  w.dlam = take(tb * nx * sizeof(float));
  w.part = take(shared_reduce_part_bytes(T, B, nx, nu));
  w.lqr = off;
  off += round_up(dmpc_lqr_workspace_bytes(T, B, nx, nu), 256);
  w.total = off;
  return w;
}

}  // namespace

extern "C" {

size_t dmpc_mpc_step_shared_grad_workspace_bytes(int T, int B, int nx, int nu) {
  if (T <= 1 || B <= 0 || nx <= 0 || nu <= 0 || !shared_reduce_supported(T, nx, nu)) return 0;
  return ws_layout(T, B, nx, nu).total;
}

int dmpc_mpc_step_backward_shared(int T, int B, int nx, int nu, uint32_t layout, const float *C_hat, const float *c_hat,
                                  const float *F_hat, const float *x, const float *u, const float *u_lower,
                                  const float *u_upper, const float *grad_x, const float *grad_u, float *d_x_init, float *dC,
                                  float *dc, float *dF, float *df, const float *detach_norm, const int32_t *detach_flag,
                                  float detach_eps, void *ws, size_t ws_bytes, int32_t *info, dmpc_stream_t stream_) {
  if (T <= 1 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (layout & ~kTimeBits) return DMPC_E_BADARG;      // (the *_BATCH bits: a gradient per trajectory is dmpc_mpc_step_backward's)
  if (!C_hat || !c_hat || !F_hat || !x || !u || !u_lower || !u_upper || !d_x_init || !ws) return DMPC_E_BADARG;
  if (!aligned16(C_hat) || !aligned16(c_hat) || !aligned16(F_hat) || !aligned16(ws)) return DMPC_E_BADARG;
  if (!shared_reduce_supported(T, nx, nu)) return DMPC_E_UNSUPPORTED;      // (nothing launched)
  const SharedMpcWs w = ws_layout(T, B, nx, nu);
  if (ws_bytes < w.total) return DMPC_E_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char *base = static_cast<char *>(ws);
  auto fp = [&](size_t o) { return reinterpret_cast<float *>(base + o); };
  float *neg = fp(w.neg), *x0 = fp(w.x0), *dx = fp(w.dx), *du = fp(w.du), *lam = fp(w.lam), *dlam = fp(w.dlam);
  uint8_t *mask = reinterpret_cast<uint8_t *>(base + w.mask);
  launch_active_mask(T, B, nx, nu, u, u_lower, u_upper, grad_x, grad_u, mask, neg, x0, nullptr, nullptr, detach_norm,
                     detach_flag, detach_eps, stream);
  // LQR_active(0, C, -d_tau, F, None, u_zero_Index=active)                               mpc_step.py:374-376
  int rc = dmpc_lqr_solve(T, B, nx, nu, C_hat, neg, F_hat, nullptr, x0, mask, nullptr, nullptr, dx, du, base + w.lqr,
                          w.total - w.lqr, info, stream_);
  if (rc != 0) return rc;
  // the co-state sweeps with their rows as the only per-trajectory output (and d_x_init = -d_lambda_0)    :383-446
  CostateArgs a{T, B, C_hat, c_hat, F_hat, x, u, dx, du, neg, 1.0f, -1.0f, /*dC_mode=*/1, /*df_shift=*/1,
                d_x_init, nullptr, nullptr, nullptr, nullptr};
  a.lam_out = lam;
  a.dlam_out = dlam;
  rc = launch_costate(nx, nu, a, stream);
  if (rc != 0) return rc;
  // dC = -1/2 (dtau (x) tau + tau (x) dtau), dc = -dtau, dF_t = -(dlam_{t+1} (x) tau_t + lam_{t+1} (x) dtau_t), df_t = -dlam_{t+1}:
  // minus the reduction's strict_math forms, summed over the batch (and over time where the layout has no time axis)
  return shared_grad_reduce(T, B, nx, nu, layout, 1, -1.0f, x, u, dx, du, nx, nu, lam, dlam, fp(w.part), dC, dc, dF, df, stream);
}

}  // extern "C"
