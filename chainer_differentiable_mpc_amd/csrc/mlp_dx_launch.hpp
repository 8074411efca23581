// mlp_dx_launch.hpp - what mpc_api.hip's box-DDP chain needs of the MlpDx kernels: the model, the rollout's arguments and
// the two launchers.  The kernels themselves live in mlp_dx_api.hip's translation unit (mlp_dx_kernels.hpp), which includes
// the MPC headers with internal linkage - so include this file AFTER mpc_kernels.hpp (ChainClear, MpcFwdArgs), as both
// translation units do; the include below is then a no-op.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "mpc_kernels.hpp"

namespace dmpc {

// DEPTH hidden layers (1 or 2) of widths H[0], H[1] and the output layer behind them: layer[l] has W [out_l, in_l] and b,
//     in_0 = nx + nu, in_l = H[l-1];   out_l = H[l] for l < depth, nx for the output layer l = depth
//     next = W[depth] act(... act(W[0] [x;u] + b[0]) ...) + b[depth] (+ x when residual)
constexpr int kMlpMaxDepth = 2;
struct MlpModel {
  int nx, nu, H[kMlpMaxDepth], residual, depth;
  struct Layer {
    const float *W, *b;   // device pointers: an optimiser step is seen by the next launch
  } layer[kMlpMaxDepth + 1];
};

// The `n_hidden` argument of the C ABI is H1 | (H2 << 16) (DMPC_MLP_HIDDEN2 of include/dmpc.h); H2 = 0: one hidden layer.
inline int mlp_hidden1(int code) { return code & 0xffff; }
inline int mlp_hidden2(int code) { return code >> 16; }

// the model as the C ABI passes it: for two layers W2 points to [W2 (H2*H1) | W3 (nx*H2)] and b2 to [b2 (H2) | b3 (nx)]
inline MlpModel mlp_model(int nx, int nu, int code, int residual, const float *W1, const float *b1, const float *W2,
                          const float *b2) {
  const int H1 = mlp_hidden1(code), H2 = mlp_hidden2(code);
  if (H2 == 0) return MlpModel{nx, nu, {H1, 0}, residual != 0 ? 1 : 0, 1, {{W1, b1}, {W2, b2}, {nullptr, nullptr}}};
  return MlpModel{nx, nu, {H1, H2}, residual != 0 ? 1 : 0, 2, {{W1, b1}, {W2, b2}, {W2 + (size_t)H2 * H1, b2 + H2}}};
}

// the weights as ONE array (dmpc_box_ddp, dyn_kind 2): [W1 | b1 | W2 | b2], or [W1 | b1 | W2 | W3 | b2 | b3] - the tails
// behind b1 are then what mlp_model takes as W2 and b2
inline MlpModel mlp_model_packed(int nx, int nu, int code, int residual, const float *packed) {
  const int H1 = mlp_hidden1(code), H2 = mlp_hidden2(code);
  const float *b1 = packed + (size_t)H1 * (nx + nu), *W2 = b1 + H1;
  const float *b2 = W2 + (H2 > 0 ? (size_t)H2 * H1 + (size_t)nx * H2 : (size_t)nx * H1);
  return mlp_model(nx, nu, code, residual, packed, b1, W2, b2);
}

struct MlpRolloutArgs {
  int T, B;
  MlpModel m;
  const float *x_init, *u;   // [B,nx], [T,B,nu]
  float *x, *F, *f;          // [T,B,nx]; [T-1,B,nx,ns] or nullptr; [T-1,B,nx] or nullptr
  const int32_t *done = nullptr;   // device flag of the BoxDDP loop: non-zero -> no-op
  ChainClear clear;                // first launch of a box-DDP chain: words to zero (loop state, meeting words, flags)
};

// mlp_rollout_linearize_kernel<act, depth> / mpc_forward_rec_mlp_kernel<act, depth> on `stream`, for sizes and an `act` that
// dmpc_mlp_dx_supported has passed; the depth is the model's.  The search writes the accepted trajectory's Jacobians when a.F_next is given.
void launch_mlp_rollout(const MlpRolloutArgs &a, int act, hipStream_t stream);
void launch_mlp_search(const MpcFwdArgs &a, const MlpModel &m, int act, hipStream_t stream);

}  // namespace dmpc
