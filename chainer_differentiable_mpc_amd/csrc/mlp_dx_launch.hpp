// mlp_dx_launch.hpp - what mpc_api.hip's box-DDP chain needs of the MlpDx kernels: the model, the rollout's arguments and
// the two launchers.  The kernels themselves live in mlp_dx_api.hip's translation unit (mlp_dx_kernels.hpp), which includes
// the MPC headers with internal linkage - so include this file AFTER mpc_kernels.hpp (ChainClear, MpcFwdArgs), as both
// translation units do; the include below is then a no-op.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpc_kernels.hpp"

namespace dmpc {

struct MlpModel {
  int nx, nu, n_hidden, residual;
  const float *W1, *b1, *W2, *b2;   // [H,ns], [H], [nx,H], [nx]  (device pointers: an optimiser step is seen by the next launch)
};

// the weights as ONE array [W1 | b1 | W2 | b2] (dmpc_box_ddp, dyn_kind 2)
inline MlpModel mlp_model_packed(int nx, int nu, int n_hidden, int residual, const float *packed) {
  const float *b1 = packed + (size_t)n_hidden * (nx + nu), *W2 = b1 + n_hidden, *b2 = W2 + (size_t)nx * n_hidden;
  return MlpModel{nx, nu, n_hidden, residual != 0 ? 1 : 0, packed, b1, W2, b2};
}

struct MlpRolloutArgs {
  int T, B;
  MlpModel m;
  const float *x_init, *u;   // [B,nx], [T,B,nu]
  float *x, *F, *f;          // [T,B,nx]; [T-1,B,nx,ns] or nullptr; [T-1,B,nx] or nullptr
  const int32_t *done = nullptr;   // device flag of the BoxDDP loop: non-zero -> no-op
  ChainClear clear;                // first launch of a box-DDP chain: words to zero (loop state, meeting words, flags)
};

// mlp_rollout_linearize_kernel<act> / mpc_forward_rec_mlp_kernel<act> on `stream`, for sizes and an `act` that
// dmpc_mlp_dx_supported has passed.  The search writes the accepted trajectory's Jacobians when a.F_next is given.
void launch_mlp_rollout(const MlpRolloutArgs &a, int act, hipStream_t stream);
void launch_mlp_search(const MpcFwdArgs &a, const MlpModel &m, int act, hipStream_t stream);

}  // namespace dmpc
