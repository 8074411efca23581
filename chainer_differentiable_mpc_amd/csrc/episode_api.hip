// episode_api.hip - C-ABI entry points of include/dmpc_episode.h: a closed-loop MPC episode as one chain of launches.  Per
// step dmpc_box_ddp (mpc_api.hip, called as it is) and ONE launch of episode_advance_kernel (episode_kernels.hpp): plant step,
// logs, stage cost, the shifted warm start.  Every argument and size check comes before the first HIP call - this file's own
// first, then dmpc_box_ddp's at step 0, which launches nothing when it refuses.  No environment variable is read here.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/dmpc.h"
#include "../../include/dmpc_episode.h"
#include "api_util.hpp"
#include "episode_kernels.hpp"

namespace dmpc {

// the caller's workspace: dmpc_box_ddp's, the hand-over buffers, the solve's outputs
struct EpisodeWs {
  size_t ddp, ddp_bytes, x_cur, u_warm, x_best, u_best, costs, norm_best, norm_last, state, info, total;
};
static EpisodeWs episode_layout(int T, int B, int nx, int nu) {
  const size_t TB = (size_t)T * B, fl = sizeof(float);
  EpisodeWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += round_up(bytes, 256);
    return o;
  };
  w.ddp_bytes = dmpc_box_ddp_workspace_bytes(T, B, nx, nu);
  w.ddp = take(w.ddp_bytes);
  w.x_cur = take((size_t)B * nx * fl);
  w.u_warm = take(TB * nu * fl);
  w.x_best = take(TB * nx * fl);
  w.u_best = take(TB * nu * fl);
  w.costs = take((size_t)B * fl);
  w.norm_best = take((size_t)B * fl);
  w.norm_last = take((size_t)B * fl);
  w.state = take(8 * sizeof(int32_t));
  w.info = take((size_t)B * sizeof(int32_t));
  w.total = off;
  return w;
}

// a code of plant_params: a non-negative integral float -> int (large values saturate: no size or activation the kernels serve)
static bool plant_code(float v, int cap, int &out) {
  if (!(v >= 0.f) || v != floorf(v)) return false;   // (a NaN fails `>=`)
  out = v >= (float)cap ? cap : (int)v;
  return true;
}

template <int PLANT, int ACT, int DEPTH>
static void launch_advance_as(const EpisodeAdvanceArgs &a, size_t lds_bytes, hipStream_t stream) {
  void (*kernel)(const EpisodeAdvanceArgs) = &episode_advance_kernel<PLANT, ACT, DEPTH>;
  if (lds_bytes > 64 * 1024) set_max_lds(reinterpret_cast<const void *>(kernel), (int)lds_bytes);
  DMPC_LAUNCH_GGL(kernel, dim3((a.B + kMlpWaves - 1) / kMlpWaves), dim3(64 * kMlpWaves), lds_bytes, stream, a);
}

template <int DEPTH>
static void launch_advance_mlp(const EpisodeAdvanceArgs &a, int act, size_t lds_bytes, hipStream_t stream) {
  switch (act) {
    case kMlpActRelu: launch_advance_as<2, kMlpActRelu, DEPTH>(a, lds_bytes, stream); break;
    case kMlpActSilu: launch_advance_as<2, kMlpActSilu, DEPTH>(a, lds_bytes, stream); break;
    case kMlpActSoftplus: launch_advance_as<2, kMlpActSoftplus, DEPTH>(a, lds_bytes, stream); break;
    default: launch_advance_as<2, kMlpActTanh, DEPTH>(a, lds_bytes, stream); break;
  }
}

// plant_kind and, for a network, an `act` that dmpc_mlp_dx_supported has passed
static void launch_advance(const EpisodeAdvanceArgs &a, int plant_kind, int act, hipStream_t stream) {
  if (plant_kind == 0) return launch_advance_as<0, kMlpActTanh, 1>(a, 0, stream);
  if (plant_kind == 1) return launch_advance_as<1, kMlpActTanh, 1>(a, 0, stream);
  const size_t bytes = mlp_lds_bytes(a.m.nx, a.m.nu, a.m.H[0], a.m.H[1], false);   // the step forms no Jacobian
  if (a.m.depth == 2) launch_advance_mlp<2>(a, act, bytes, stream);
  else launch_advance_mlp<1>(a, act, bytes, stream);
}

}  // namespace dmpc

using namespace dmpc;

extern "C" {

size_t dmpc_mpc_episode_workspace_bytes(int T, int B, int nx, int nu) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return 0;
  return episode_layout(T, B, nx, nu).total;
}

int dmpc_mpc_episode(int n_steps, int T, int B, int nx, int nu, const float *x_init, const float *C, const float *c,
                     const float *F, const float *f, int dyn_kind, const float *dyn_params, const float *plant_F,
                     const float *plant_f, int plant_kind, const float *plant_params, const float *u_init,
                     const float *u_lower, const float *u_upper, float eps, int not_improved_lim, float ls_decay,
                     int max_ls_iter, float best_cost_eps, int max_iter, int n_qp_iter_max, int scrambled_norm,
                     float *x_log, float *u_log, float *stage_cost, float *x_plan, float *u_plan, int32_t *state_log,
                     void *ws, size_t ws_bytes, int32_t *info, dmpc_stream_t stream_) {
  if (n_steps < 1 || T < 2 || B <= 0 || nx <= 0 || nu <= 0 || max_iter <= 0 || n_qp_iter_max <= 0) return DMPC_E_BADARG;
  if (!x_init || !C || !c || !u_init || !u_lower || !u_upper || !x_log || !u_log || !stage_cost || !state_log || !ws)
    return DMPC_E_BADARG;
  if (plant_kind < 0 || plant_kind > 2) return DMPC_E_UNSUPPORTED;
  if (plant_kind != 1 && !plant_F) return DMPC_E_BADARG;
  if (plant_kind != 0 && !plant_params) return DMPC_E_BADARG;
  if (plant_kind == 1 && (nx != 3 || nu != 1)) return DMPC_E_UNSUPPORTED;
  int p_hidden = 0, p_act = 0, p_residual = 0;
  if (plant_kind == 2) {
    if (plant_f != nullptr) return DMPC_E_BADARG;
    if (!plant_code(plant_params[0], 1 << 24, p_hidden) || !plant_code(plant_params[1], 1000000, p_act)) return DMPC_E_BADARG;
    if (plant_params[2] != 0.f && plant_params[2] != 1.f) return DMPC_E_BADARG;
    p_residual = plant_params[2] != 0.f;
    if (p_hidden >= (1 << 24)) p_hidden = 0;   // (0: no size the kernels serve)
    if (!dmpc_mlp_dx_supported(nx, nu, p_hidden, p_act)) return DMPC_E_UNSUPPORTED;
  }
  if (nx + nu > kEpisodeMaxNs) return DMPC_E_UNSUPPORTED;
  if (!aligned16(ws)) return DMPC_E_BADARG;
  const EpisodeWs w = episode_layout(T, B, nx, nu);
  if (ws_bytes < w.total) return DMPC_E_WORKSPACE;

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char *base = static_cast<char *>(ws);
  auto fp = [&](size_t off) { return reinterpret_cast<float *>(base + off); };
  auto ip = [&](size_t off) { return reinterpret_cast<int32_t *>(base + off); };
  float *x_cur = fp(w.x_cur), *u_warm = fp(w.u_warm), *x_best = fp(w.x_best), *u_best = fp(w.u_best);
  int32_t *state = ip(w.state), *info_step = ip(w.info);
  const size_t n_x = (size_t)B * nx, n_u = (size_t)B * nu;

  EpisodeAdvanceArgs a{};
  a.T = T; a.B = B; a.nx = nx; a.nu = nu;
  a.u_best = u_best; a.C = C; a.c = c; a.state = state; a.info_step = info_step;
  a.plant_F = plant_kind == 0 ? plant_F : nullptr;
  a.plant_f = plant_kind == 0 ? plant_f : nullptr;
  if (plant_kind == 1) {
    a.pend_g = plant_params[0]; a.pend_m = plant_params[1]; a.pend_l = plant_params[2];
    a.pend_dt = plant_params[3]; a.pend_max_torque = plant_params[4];
  }
  if (plant_kind == 2) a.m = mlp_model_packed(nx, nu, p_hidden, p_residual, plant_F);
  a.info = info; a.x_cur = x_cur; a.u_warm = u_warm; a.x_best = x_best;

  for (int k = 0; k < n_steps; ++k) {
    // the solve: from the caller's state and controls at step 0, then from what the previous advance left.  Its own checks
    // (the model, the routes) come before its first launch, so a refusal at step 0 has launched nothing.
    const int rc = dmpc_box_ddp(T, B, nx, nu, k == 0 ? x_init : x_cur, C, c, F, f, dyn_kind, dyn_params, k == 0 ? u_init : u_warm,
                                u_lower, u_upper, eps, not_improved_lim, ls_decay, max_ls_iter, best_cost_eps, max_iter,
                                n_qp_iter_max, scrambled_norm, /*batch_coupled=*/0, x_best, u_best, fp(w.costs), fp(w.norm_best),
                                fp(w.norm_last), state, base + w.ddp, w.ddp_bytes, info_step, stream_);
    if (rc != 0) return rc;
    a.first = k == 0;
    a.x_k = k == 0 ? x_init : x_log + (size_t)k * n_x;
    a.x_first = k == 0 ? x_log : nullptr;
    a.x_next = x_log + (size_t)(k + 1) * n_x;
    a.u_now = u_log + (size_t)k * n_u;
    a.stage_cost = stage_cost + (size_t)k * B;
    a.state_now = state_log + (size_t)k * 8;
    a.x_plan = k == n_steps - 1 ? x_plan : nullptr;
    a.u_plan = k == n_steps - 1 ? u_plan : nullptr;
    launch_advance(a, plant_kind, p_act, stream);
    const int le = (int)hipGetLastError();
    if (le != 0) return le;
  }
  return 0;
}

}  // extern "C"
