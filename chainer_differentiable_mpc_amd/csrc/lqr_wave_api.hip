// lqr_wave_api.hip - instances and launchers of lqr_wave_mfma_backward (LqrRecursion.backward, lqr/lqr_recursion.py:69-158,
// and LQR_active's sweep, mpc/active_constrained_lqr.py:67-151, at the large shapes).
#include <hip/hip_runtime.h>

#include "../../include/dmpc.h"
#include "api_util.hpp"
#include "knobs.hpp"
#include "lqr_wave_api.hpp"
#include "lqr_staged_forward.hpp"
#include "lqr_wave_mfma.hpp"
#include "lqr_tile16.hpp"

namespace dmpc {

// a trajectory per wavefront, four wavefronts per workgroup (one per SIMD)
static dim3 traj_per_wave_grid(int B) { return dim3((B + 3) / 4); }

// the plain (unclamped) sweep on 16x16x4 tiles (lqr_tile16.hpp)
template <int NX, int NU, bool ROLLOUT>
static int launch_tile16(const LqrArgs &a, hipStream_t stream) {
  constexpr size_t lds = Tile16Layout<NX, NU>::lds_bytes();
  static_assert(DMPC_T16_OCC * lds <= 160 * 1024, "DMPC_T16_OCC workgroups per CU");
  return launch_kernel_big_lds(lqr_tile16_kernel<NX, NU, ROLLOUT>, traj_per_wave_grid(a.B), dim3(256), lds, stream, a);
}
// the sweep on 4x4x1 outer products (lqr_wave_mfma.hpp), plain or LQR_active; PAD: of a smaller problem inside the instance
template <int NX, int NU, bool MASKED, bool ROLLOUT, bool PAD>
static int launch_wave_mfma(const LqrArgs &a, hipStream_t stream) {
  return launch_kernel(lqr_wave_mfma_backward<NX, NU, MASKED, ROLLOUT, PAD>, traj_per_wave_grid(a.B), dim3(256), 0, stream, a);
}
template <int NX, int NU, bool PAD>
static int launch_mpc_wave(const LqrArgs &a, hipStream_t stream) {
  return launch_kernel(lqr_wave_mfma_backward<NX, NU, false, false, PAD, true>, traj_per_wave_grid(a.B), dim3(256), 0, stream, a);
}
// (the rows through an LDS ring: lqr_staged_forward.hpp; gains from a.Ks / a.ks, else the workspace)
static int launch_staged_forward(const LqrArgs &a, hipStream_t stream) {
  return launch_kernel_big_lds(lqr_staged_forward_kernel, dim3(a.B), dim3(64), lqr_staged_fwd_lds_bytes(a.nx_log, a.nu_log), stream,
                               a, a.nx_log, a.nu_log);
}

LqrLauncher lqr_wave_exact_launcher(int nx, int nu, bool masked, bool rollout) {
  if (knob_on<Knob::DMPC_NO_WAVE_MFMA>()) return nullptr;
  // DMPC_NO_TILE16=1: the plain sweep on the 4x4x1 outer-product kernel too (A/B timing)
  const bool tiles = !masked && !knob_on<Knob::DMPC_NO_TILE16>();
#define X(NX_, NU_) \
  if (tiles && nx == NX_ && nu == NU_) return rollout ? launch_tile16<NX_, NU_, true> : launch_tile16<NX_, NU_, false>;
  // ((16,8) stays on the 4x4x1 kernel: 388 against 384 us at B = 4096, T = 50 - profiles/r05/tile16_shapes.txt)
  X(32, 8) X(24, 8) X(32, 4) X(24, 4)
#undef X
#define X(NX_, NU_)                                                                                                      \
  if (nx == NX_ && nu == NU_)                                                                                            \
    return masked ? (rollout ? launch_wave_mfma<NX_, NU_, true, true, false> : launch_wave_mfma<NX_, NU_, true, false, false>) \
                  : (rollout ? launch_wave_mfma<NX_, NU_, false, true, false> : launch_wave_mfma<NX_, NU_, false, false, false>);
  // (32,8) is config 5's shape; the others are the sizes of the padded instances themselves, which then run the exact kernel
  // (compile-time strides, 16-byte LDS-DMA, the rollout in the same launch) instead of their own container: (24,8) at
  // B = 4096, T = 50 1.01 -> ~0.6 ms
  X(32, 8) X(24, 8) X(24, 4) X(32, 4) X(16, 8)
#undef X
  return nullptr;
}

// MPCstep.backward_rec at the wavefront-per-trajectory shapes: the sweep with the box QP inside (a.mpc_* set)
int launch_mpc_wave_backward(int nx, int nu, const LqrArgs &a, hipStream_t stream) {
#define X(NX_, NU_) \
  if (nx == NX_ && nu == NU_) return launch_mpc_wave<NX_, NU_, false>(a, stream);
  X(16, 8) X(32, 8)
#undef X
  return DMPC_E_UNSUPPORTED;
}
int launch_mpc_wave_container_backward(int cnx, int cnu, const LqrArgs &a, hipStream_t stream) {
#define X(NX_, NU_) \
  if (cnx == NX_ && cnu == NU_) return launch_mpc_wave<NX_, NU_, true>(a, stream);
  X(16, 8) X(32, 8)
#undef X
  return DMPC_E_UNSUPPORTED;
}

// The sweep runs in the smallest instance that holds the problem (fewest columns first), whichever container the caller's
// forward-only kernel is: the gains travel at the problem's own strides.  Measured and dropped (round 4, B = 4096, T = 50):
// a test of rows and tiles at run time instead (uniform branches around the matrix-core blocks of one (32,8) instance:
// (31,8) 1.43 -> 1.62 ms), and a rollout in the same launch with one 4-byte load per row element at the problem's
// strides ((20,6) 0.96 -> 1.18 ms; the forward-only container kernel of lqr_kernels.hpp stays a launch of its own).
LqrLauncher lqr_wave_padded_sweep_launcher(int nx, int nu, bool masked) {
#define X(NX_, NU_) \
  if (nx <= NX_ && nu <= NU_) return masked ? launch_wave_mfma<NX_, NU_, true, false, true> : launch_wave_mfma<NX_, NU_, false, false, true>;
  X(16, 8) X(24, 4) X(24, 8) X(32, 4) X(32, 8)
#undef X
  return nullptr;
}

// not for the clamped rollout, T == 1 or DMPC_NO_STAGED_FWD=1
LqrLauncher lqr_staged_forward_launcher(int T, int nx, int nu, bool masked) {
  const bool takes = !knob_on<Knob::DMPC_NO_STAGED_FWD>() && !masked && T >= 2 && nx + nu <= 63 &&
                     lqr_staged_fwd_lds_bytes(nx, nu) <= 150 * 1024;
  return takes ? launch_staged_forward : nullptr;
}

}  // namespace dmpc
