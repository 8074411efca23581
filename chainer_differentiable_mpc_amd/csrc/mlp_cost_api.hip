// mlp_cost_api.hip - C-ABI entry points of include/dmpc_mlp_cost.h: the learned stage cost of mlp_cost_kernels.hpp - its Taylor
// model, MPCstep.forward_rec with it as the true cost under a dense LinDx, and its parameter gradient with the fixed-order
// reduction.  Every argument and size check comes before the first HIP call.  No allocation, no host synchronisation.  No
// environment variable is read here.
#include <hip/hip_runtime.h>

#include "../../include/dmpc.h"
#include "../../include/dmpc_mlp_cost.h"
#include "api_util.hpp"
// the kernel headers with internal linkage: this translation unit's instances of the templates are its own, and it neither
// defines another translation unit's non-template kernels a second time nor emits the ones it does not launch
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "mlp_dx_host.hpp"
#pragma clang attribute pop
// (outside the attribute: the two launchers declared here are what mpc_api.hip's chain calls)
#include "mlp_cost_launch.hpp"
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "mlp_cost_kernels.hpp"
#pragma clang attribute pop

namespace dmpc {

constexpr int kCostApproxGroups = 2048;      // workgroups of the Taylor model at most: eight per CU, each walks its points

// the two launchers of mlp_cost_launch.hpp: the entry points below and dmpc_box_ddp_mlp_cost's chain (mpc_api.hip) go through them
void launch_mlp_cost_approx(const MlpCostApproxArgs &a, int act, hipStream_t stream) {
  const long long groups = (a.P + kMlpWaves - 1) / kMlpWaves;
  const dim3 grid((unsigned)(groups < kCostApproxGroups ? groups : kCostApproxGroups));
  const size_t bytes = mlp_cost_lds_bytes(a.m.nx, a.m.nu, a.m.H, kCostApproxWaveFloats);
  mlp_with_act(act, [&](auto A) {
    DMPC_LAUNCH_GGL(mlp_cost_approx_kernel<decltype(A)::value>, grid, dim3(64 * kMlpWaves), bytes, stream, a);
  });
}

void launch_mlp_cost_search(const MpcFwdArgs &a, const MlpCostModel &m, int act, float *H_next, float *g_next, hipStream_t stream) {
  const size_t bytes = mlp_cost_lds_bytes(m.nx, m.nu, m.H, H_next != nullptr ? kCostApproxWaveFloats : 0);
  mlp_with_act(act, [&](auto A) {
    DMPC_LAUNCH_GGL(mpc_forward_rec_mlp_cost_kernel<decltype(A)::value>, dim3((a.B + kMlpWaves - 1) / kMlpWaves), dim3(64 * kMlpWaves),
                    bytes, stream, a, m, H_next, g_next);
  });
}

}  // namespace dmpc

using namespace dmpc;

namespace {

// 0: launch; DMPC_E_BADARG / DMPC_E_UNSUPPORTED otherwise
int cost_check(int nx, int nu, int H, int act) {
  if (nx <= 0 || nu <= 0 || H <= 0) return DMPC_E_BADARG;
  if (act != kMlpActTanh && act != kMlpActRelu && act != kMlpActSilu && act != kMlpActSoftplus) return DMPC_E_UNSUPPORTED;
  if (nx > kMlpMaxNx || nu > kMlpMaxNu || H > kCostMaxH) return DMPC_E_UNSUPPORTED;
  return 0;
}

}  // namespace

extern "C" {

int dmpc_mlp_cost_supported(int nx, int nu, int n_hidden, int act) { return cost_check(nx, nu, n_hidden, act) == 0 ? 1 : 0; }

int dmpc_mlp_cost_approx(int T, int B, int nx, int nu, int n_hidden, int act, const float *Q, const float *p, const float *W1,
                         const float *b1, const float *w2, const float *x, const float *u, float *H_out, float *g_out,
                         float *costs_out, dmpc_stream_t stream_) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0 || n_hidden <= 0) return DMPC_E_BADARG;
  if (!Q || !p || !W1 || !b1 || !w2 || !x || !u) return DMPC_E_BADARG;
  if ((H_out == nullptr) != (g_out == nullptr) || (H_out == nullptr && costs_out == nullptr)) return DMPC_E_BADARG;
  const int rc = cost_check(nx, nu, n_hidden, act);
  if (rc != 0) return rc;
  const long long P = (long long)T * B;
  if ((size_t)P * (nx + nu) * (nx + nu) >= ((size_t)1 << 31)) return DMPC_E_UNSUPPORTED;
  const MlpCostApproxArgs aa{P, MlpCostModel{nx, nu, n_hidden, Q, p, W1, b1, w2}, x, u, H_out, g_out, costs_out};
  launch_mlp_cost_approx(aa, act, static_cast<hipStream_t>(stream_));   // (no `done` flag, nothing to clear)
  return (int)hipGetLastError();
}

int dmpc_mpc_forward_rec_mlp_cost(int T, int B, int nx, int nu, int n_hidden, int act, const float *Q, const float *p,
                                  const float *W1, const float *b1, const float *w2, const float *Ks, const float *ks,
                                  const float *controls, const float *states, const float *u_lower, const float *u_upper,
                                  const float *F_true, const float *f_true, float ls_decay, int max_ls_iter, float *x_out,
                                  float *u_out, float *costs, float *old_costs, float *alphas, float *objs, float *u_first,
                                  int32_t *n_ls_iter, int32_t *info, dmpc_stream_t stream_) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0 || n_hidden <= 0) return DMPC_E_BADARG;
  if (!Q || !p || !W1 || !b1 || !w2 || !Ks || !ks || !controls || !states || !u_lower || !u_upper || !x_out || !u_out || !costs ||
      !alphas || !n_ls_iter)
    return DMPC_E_BADARG;
  if (T > 1 && !F_true) return DMPC_E_BADARG;      // (T = 1: no dynamics step, F_true and f_true are not read)
  const int rc = cost_check(nx, nu, n_hidden, act);
  if (rc != 0) return rc;
  if ((size_t)T * B * nx * (nx + nu) >= ((size_t)1 << 31)) return DMPC_E_UNSUPPORTED;
  const MpcFwdArgs fa{T, B, Ks, ks, controls, states, u_lower, u_upper, nullptr, nullptr, F_true, f_true, ls_decay,
                      max_ls_iter, /*ls_cap=*/64, x_out, u_out, u_first, costs, old_costs, alphas, objs, n_ls_iter, info};
  const MlpCostModel m{nx, nu, n_hidden, Q, p, W1, b1, w2};
  launch_mlp_cost_search(fa, m, act, nullptr, nullptr, static_cast<hipStream_t>(stream_));   // (fa.done: nullptr; no epilogue)
  return (int)hipGetLastError();
}

size_t dmpc_mlp_cost_param_grad_workspace_bytes(int T, int B, int nx, int nu, int n_hidden) {
  if (T <= 0 || B <= 0 || cost_check(nx, nu, n_hidden, kMlpActTanh) != 0) return 0;
  return (size_t)mlp_cost_grad_partials((long long)T * B) * mlp_cost_grad_partial_floats(nx + nu, n_hidden) * sizeof(float);
}

int dmpc_mlp_cost_param_grad(int T, int B, int nx, int nu, int n_hidden, int act, const float *W1, const float *b1,
                             const float *w2, const float *x, const float *u, const float *grad_g, const float *grad_costs,
                             float *dQ, float *dp, float *dW1, float *db1, float *dw2, void *ws, size_t ws_bytes,
                             dmpc_stream_t stream_) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0 || n_hidden <= 0) return DMPC_E_BADARG;
  if (!W1 || !b1 || !w2 || !x || !u || !dQ || !dp || !dW1 || !db1 || !dw2) return DMPC_E_BADARG;
  if (!grad_g && !grad_costs) return DMPC_E_BADARG;
  const int rc = cost_check(nx, nu, n_hidden, act);
  if (rc != 0) return rc;
  const long long P = (long long)T * B;
  if ((size_t)P * (nx + nu) * (nx + nu) >= ((size_t)1 << 31)) return DMPC_E_UNSUPPORTED;
  if (ws == nullptr || ws_bytes < dmpc_mlp_cost_param_grad_workspace_bytes(T, B, nx, nu, n_hidden)) return DMPC_E_WORKSPACE;
  const int ns = nx + nu, G = mlp_cost_grad_partials(P);
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const MlpCostGradArgs ga{P, G, MlpCostModel{nx, nu, n_hidden, nullptr, nullptr, W1, b1, w2}, x, u, grad_g, grad_costs,
                           static_cast<float *>(ws)};
  const size_t bytes = mlp_cost_lds_bytes(nx, nu, n_hidden, 0);
  mlp_with_act(act, [&](auto A) {
    DMPC_LAUNCH_GGL(mlp_cost_param_grad_kernel<decltype(A)::value>, dim3((G + kMlpWaves - 1) / kMlpWaves), dim3(64 * kMlpWaves), bytes,
                    stream, ga);
  });
  const MlpCostGradReduceArgs rd{G, ns * ns, ns, n_hidden * ns, n_hidden, static_cast<const float *>(ws), dQ, dp, dW1, db1, dw2};
  DMPC_LAUNCH_GGL(mlp_cost_param_grad_reduce_kernel, dim3((rd.nQ + rd.np + rd.nW + 2 * rd.nH + 255) / 256), dim3(256), 0, stream, rd);
  return (int)hipGetLastError();
}

}  // extern "C"
