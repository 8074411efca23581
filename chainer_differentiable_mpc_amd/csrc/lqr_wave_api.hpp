// lqr_wave_api.hpp - launchers of the matrix-core backward sweep for the large shapes (lqr_wave_mfma.hpp), kept in their
// own translation unit (lqr_wave_api.hip) so that the kernel can be rebuilt without the generated streams of lqr_api.hip,
// and the few launch helpers the two translation units share.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "api_util.hpp"
#include "lqr_kernels.hpp"

namespace dmpc {

// One launcher per kernel template: what the route of lqr_api.hip returns (a.nx_log, a.nu_log: the problem's own dimensions).
using LqrLauncher = int (*)(const LqrArgs &a, hipStream_t stream);

// Runtime bools as template arguments: with_bools(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...)
template <class F>
int with_bools(F f) { return f(); }
template <class F, class... Bools>
int with_bools(F f, bool b, Bools... rest) {
  return b ? with_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
           : with_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// four trajectories per wavefront, four wavefronts per workgroup
inline dim3 four_traj_per_wave_grid(int B) { const int waves = (B + 3) / 4; return dim3((waves + 3) / 4); }

template <class Kernel, class... Args>
int launch_kernel(Kernel kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args &...args) {
  DMPC_LAUNCH_GGL(kernel, grid, block, lds, stream, args...);
  return (int)hipGetLastError();
}
// ... of a kernel whose dynamic LDS may pass the 64 KB a kernel gets without asking
template <class Kernel, class... Args>
int launch_kernel_big_lds(Kernel kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args &...args) {
  if (lds > 64 * 1024) set_max_lds(reinterpret_cast<const void *>(kernel), (int)lds);
  return launch_kernel(kernel, grid, block, lds, stream, args...);
}

// The sweep of a shape that IS one of the wavefront-per-trajectory instances (Ks / ks of `a`, else its workspace, receive the
// gains; with `rollout` the same launch goes on with the forward sweep): the 16x16x4 tile kernel where it serves the call, else
// the 4x4x1 kernel; nullptr for other shapes and with DMPC_NO_WAVE_MFMA=1.
LqrLauncher lqr_wave_exact_launcher(int nx, int nu, bool masked, bool rollout);
// ... of a smaller problem padded inside the smallest instance that holds it (up to 32 states, 8 controls)
LqrLauncher lqr_wave_padded_sweep_launcher(int nx, int nu, bool masked);
// the rollout of a padded problem with its inputs staged through LDS; nullptr where it does not apply
LqrLauncher lqr_staged_forward_launcher(int T, int nx, int nu, bool masked);

// MPCstep.backward_rec with the box QP inside the sweep (a.mpc_* set); (16,8) and (32,8); DMPC_E_UNSUPPORTED otherwise
int launch_mpc_wave_backward(int nx, int nu, const LqrArgs &a, hipStream_t stream);
// ... of a smaller problem (a.nx_log, a.nu_log) padded inside the (cnx, cnu) instance
int launch_mpc_wave_container_backward(int cnx, int cnu, const LqrArgs &a, hipStream_t stream);

}  // namespace dmpc
