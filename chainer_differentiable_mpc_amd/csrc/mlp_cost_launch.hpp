// mlp_cost_launch.hpp - what mpc_api.hip's box-DDP chain needs of the MlpCost kernels: the model, the Taylor model's arguments
// and the two launchers.  The kernels themselves live in mlp_cost_api.hip's translation unit (mlp_cost_kernels.hpp), which
// includes the MPC headers with internal linkage - so include this file AFTER mpc_kernels.hpp (ChainClear, MpcFwdArgs), as both
// translation units do; the include below is then a no-op.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpc_kernels.hpp"

namespace dmpc {

//     c(tau) = 1/2 tau' Q tau + p' tau + w2' act(W1 tau + b1),     tau = [x;u], ns = nx + nu
struct MlpCostModel {
  int nx, nu, H;
  const float *Q, *p, *W1, *b1, *w2;   // device pointers ([ns,ns], [ns], [H,ns], [H], [H]); Q, p: nullptr where a kernel reads neither
};

// the weights as ONE array (dmpc_box_ddp_mlp_cost): [Q (ns*ns) | p (ns) | W1 (H*ns) | b1 (H) | w2 (H)]
inline MlpCostModel mlp_cost_model_packed(int nx, int nu, int H, const float *packed) {
  const size_t ns = (size_t)nx + nu;
  const float *p = packed + ns * ns, *W1 = p + ns, *b1 = W1 + (size_t)H * ns, *w2 = b1 + H;
  return MlpCostModel{nx, nu, H, packed, p, W1, b1, w2};
}

// ---- the Taylor model
struct MlpCostApproxArgs {
  long long P;                     // T * B points
  MlpCostModel m;
  const float *x, *u;              // [P,nx], [P,nu]
  float *H_out, *g_out, *costs;    // [P,ns,ns], [P,ns] (both or neither), [P]; any nullptr
  const int32_t *done = nullptr;   // device flag of the BoxDDP loop: non-zero -> no-op
  ChainClear clear;                // first launch of a box-DDP chain: words to zero (loop state, meeting words, flags)
};

// mlp_cost_approx_kernel<act> / mpc_forward_rec_mlp_cost_kernel<act> on `stream`, for sizes and an `act` that
// dmpc_mlp_cost_supported has passed.  The search stores the accepted trajectory's Taylor model when the pair H_next
// [T,B,ns,ns], g_next [T,B,ns] is given (both or neither).
void launch_mlp_cost_approx(const MlpCostApproxArgs &a, int act, hipStream_t stream);
void launch_mlp_cost_search(const MpcFwdArgs &a, const MlpCostModel &m, int act, float *H_next, float *g_next, hipStream_t stream);

}  // namespace dmpc
