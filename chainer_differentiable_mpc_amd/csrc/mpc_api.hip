// mpc_api.hip - C-ABI entry points of the projected-Newton QP and of the MPC step
// (include/dmpc.h sections C and E).  Replaces PNQP (mpc/pnqp.py:37-201), MPCstep.forward /
// backward_rec / forward_rec / backward (mpc/mpc_step.py:70-460) of the reference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/dmpc.h"
#include "../../include/dmpc_mlp_cost.h"
#include "api_util.hpp"
#include "knobs.hpp"
#include "costate_args.hpp"
#include "box_ddp_kernels.hpp"
#include "mpc_asm_kernel.hpp"
#include "mpc_dma_kernels.hpp"
#include "mpc_fwd_asm_kernel.hpp"
#include "mpc_step_fused_kernel.hpp"
#include "lqr_wide_kernel.hpp"
#include "mpc_wide_forward_kernel.hpp"
#include "lqr_wave_api.hpp"
#include "mpc_generic.hpp"
#include "mpc_tiled.hpp"
#include "mpc_coupled.hpp"
#include "mpc_kernels.hpp"
#include "mlp_dx_launch.hpp"
#include "mlp_cost_launch.hpp"

namespace dmpc {

// Standalone PNQP: one lane per QP, everything in registers.
struct PnqpArgs {
  int B;
  const float *H, *q, *lower, *upper, *x_init;
  int n_iter;
  float *x_out, *fac;
  int32_t *piv;
  float *index_f;
  int32_t *n_iter_out, *info;
  unsigned *sync;   // batch-coupled termination (pnqp_device.hpp): pnqp_sync_slots(n_iter) zeroed slots, or nullptr
};

template <int N>
__global__ __launch_bounds__(256) void pnqp_kernel(const PnqpArgs a) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = b < a.B;
  if (!live) {
    if (a.sync == nullptr) return;
    b = a.B - 1;   // coupled: padding lanes repeat the last row (neutral in the any-reductions) and take every barrier
  }
  float Hm[N][N], qv[N], lo[N], hi[N], x[N];
#pragma unroll
  for (int r = 0; r < N; ++r) {
#pragma unroll
    for (int c = 0; c < N; ++c) Hm[r][c] = a.H[((size_t)b * N + r) * N + c];
    qv[r] = a.q[(size_t)b * N + r];
    lo[r] = a.lower[(size_t)b * N + r];
    hi[r] = a.upper[(size_t)b * N + r];
    x[r] = a.x_init != nullptr ? a.x_init[(size_t)b * N + r] : 0.f;
  }
  PnqpResult<N> res;
  QpTermination term;
  term.slots = a.sync;
  term.n_blocks = gridDim.x;
  pnqp_solve<N>(Hm, qv, lo, hi, x, a.x_init != nullptr, a.n_iter, res, term);
  if (!live) return;
#pragma unroll
  for (int r = 0; r < N; ++r) {
    a.x_out[(size_t)b * N + r] = x[r];
    a.index_f[(size_t)b * N + r] = res.free_[r] ? 1.0f : 0.0f;
    if (a.piv != nullptr) a.piv[(size_t)b * N + r] = res.piv[r];
#pragma unroll
    for (int c = 0; c < N; ++c) a.fac[((size_t)b * N + r) * N + c] = res.fac[r][c];
  }
  a.n_iter_out[b] = res.it;
  if (a.info != nullptr && !res.converged) atomicOr(&a.info[b], DMPC_INFO_QP_ITERCAP);
}

// A kernel whose workgroups meet at grid barriers needs all of them resident: cooperative launch (the runtime refuses a grid
// that does not fit instead of letting it deadlock).  The runtime's own limit - hipOccupancyMaxActiveBlocksPerMultiprocessor x
// CUs - is not safe on gfx950: mpc_coupled.hpp's kernel (7 workgroups per CU by that count) was ACCEPTED at 1,792 workgroups
// and deadlocked at its first barrier, and ran at 1,024 (round 5, scripts/coupled_grid_probe.py).  So the grids here stay at
// HALF the workgroups per CU the runtime counts (at least one).
static long long resident_workgroups(const void *kernel, int threads, size_t lds) {
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds) != hipSuccess || cus <= 0 || per_cu <= 0) {
    (void)hipGetLastError();
    return 0;
  }
  return (long long)cus * std::max(1, per_cu / 2);
}

static int launch_cooperative(const void *kernel, dim3 grid, dim3 block, void **args, size_t lds, hipStream_t stream) {
  if ((long long)grid.x > resident_workgroups(kernel, (int)block.x, lds)) return DMPC_E_UNSUPPORTED;   // -> mpc_coupled.hpp's fixed grid
  note_kernel(kernel);
  const hipError_t e = hipLaunchCooperativeKernel(kernel, grid, block, args, (unsigned)lds, stream);
  if (e == hipErrorCooperativeLaunchTooLarge) {
    (void)hipGetLastError();
    return DMPC_E_UNSUPPORTED;
  }
  return (int)e;
}

// mpc_coupled.hpp's kernels: a grid that is resident whatever the batch - resident_workgroups() of this kernel, at most one per
// row; halved if the runtime still refuses
static int launch_fixed_grid(const void *kernel, int rows, void **args, hipStream_t stream) {
  long long cap = resident_workgroups(kernel, kTiledThreads, 0);
  if (cap <= 0) return DMPC_E_UNSUPPORTED;
  if (const long long v = knob_int<Knob::DMPC_FIXED_GRID_MAX>(); v >= 1) cap = v;   // (experiments)
  note_kernel(kernel);
  for (long long g = std::min<long long>(cap, rows); g >= 1; g /= 2) {
    const hipError_t e = hipLaunchCooperativeKernel(kernel, dim3((unsigned)g), dim3(kTiledThreads), args, 0, stream);
    if (e != hipErrorCooperativeLaunchTooLarge) return (int)e;
    (void)hipGetLastError();
  }
  return DMPC_E_UNSUPPORTED;
}

// A batch-coupled problem on a register kernel: cooperative, the whole batch resident; where that does not fit - and with
// DMPC_NO_COOP_REGISTER=1, read at every call - what `fixed_grid` launches instead (mpc_coupled.hpp)
template <class FixedGrid>
static int launch_coupled(const void *kernel, dim3 grid, dim3 block, void **args, size_t lds, hipStream_t stream, FixedGrid fixed_grid) {
  const int rc = knob_on_now<Knob::DMPC_NO_COOP_REGISTER>() ? DMPC_E_UNSUPPORTED
                                                            : launch_cooperative(kernel, grid, block, args, lds, stream);
  return rc == DMPC_E_UNSUPPORTED ? fixed_grid() : rc;
}

static size_t coupled_bytes(int T, int n_qp_iter) { return round_up((size_t)T * pnqp_sync_slots(n_qp_iter) * 2 * sizeof(unsigned), 256); }
// the fixed-grid form's rows, behind the decision slots
static size_t coupled_traj_bytes(int B, int nx, int nu) { return round_up((size_t)B * mpc_coupled_traj_floats(nx, nu) * sizeof(float), 256); }
static size_t pnqp_coupled_row_bytes(int B, int n) { return round_up((size_t)B * pnqp_coupled_row_floats(n) * sizeof(float), 256); }

// MPCstep.backward_rec, batch-coupled, any size and any batch (mpc_coupled.hpp); a.sync zeroed, a.tiled_scratch =
// [B][mpc_coupled_traj_floats]
static int launch_mpc_back_fixed_grid(int nx, int nu, const MpcBackArgs &a, hipStream_t stream) {
  if (a.sync == nullptr) return DMPC_E_BADARG;
  if (a.tiled_scratch == nullptr) return DMPC_E_WORKSPACE;
  MpcBackArgs aa = a;
  float *scratch = a.tiled_scratch;
  void *args[] = {&aa, &nx, &nu, &scratch};
  return launch_fixed_grid(reinterpret_cast<const void *>(&mpc_coupled_backward_kernel), a.B, args, stream);
}

// ---- The instance lists, in the order they are tried.
#ifdef DMPC_EXPERIMENT_ONLY_8_2
#define DMPC_MPC_SHAPES(X) X(8, 2, 16)
#else
#define DMPC_MPC_SHAPES(X) \
  X(1, 1, 16) X(2, 1, 16) X(3, 1, 16) X(2, 2, 16) X(3, 2, 16) X(4, 2, 16) X(6, 2, 16) X(8, 2, 16) \
  X(4, 4, 16) X(8, 4, 16) X(12, 3, 16)
#endif
// The generated streams (mpc_asm_kernel.hpp, mpc_fwd_asm_kernel.hpp, mpc_step_fused_kernel.hpp); (6,2) has a search alone
#define DMPC_MPC_STREAM_SHAPES(A, SEARCH_ONLY) A(8, 2) A(3, 1) A(4, 2) SEARCH_ONLY(6, 2) A(2, 2) A(1, 1) A(2, 1) A(3, 2)
#define DMPC_NO_SHAPE(NX_, NU_)
// Containers (mpc_backward_rec_kernel / mpc_forward_rec_kernel <..., PAD>): any smaller problem runs padded inside them
// instead of on the runtime-dimension kernels of mpc_generic.hpp; tried in this order (same list as lqr_api.hip)
#ifdef DMPC_EXPERIMENT_ONLY_8_2
#define DMPC_MPC_CONTAINERS(X)
#else
#define DMPC_MPC_CONTAINERS(X) X(3, 1) X(4, 4) X(8, 2) X(8, 4) X(14, 1) X(13, 2) X(12, 3) X(11, 4)
#endif
// The wide row kernels' instances (lqr_wide_kernel<..., MPC>, mpc_wide_forward_kernel), fewest columns first
#define DMPC_MPC_WIDE_SHAPES(X) X(12, 4) X(16, 4) X(12, 8) X(16, 8)
// pnqp_kernel<N> and mpc_generic_backward_kernel<NU>: up to eight unknowns / controls (kMpcGenericMaxNu)
#define DMPC_ONE_TO_EIGHT(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

// The LDS-DMA rings of the 16-lane kernels' inputs (mpc_dma_kernels.hpp): the sweep's depth by the DMA instructions a step takes
template <int NX, int NU>
struct SweepRing {
  static constexpr int kDma = MpcBackDmaLayout<NX, NU, 2>::kDma, kDepth = kDma == 1 ? 8 : kDma <= 4 ? 4 : 2;
  static constexpr size_t kLds = MpcBackDmaLayout<NX, NU, kDepth>::lds_bytes();
  static constexpr bool kFits = kLds <= 65536;
};
template <int NX, int NU>
constexpr bool search_ring_fits() { return MpcFwdDmaLayout<NX, NU>::lds_bytes() <= 96 * 1024; }

// ---- The order of the code object.  The compiler emits the kernels in the order the translation unit first names them
// (DESIGN.md 3.4); the launchers below would name them in another.  This function names every kernel template instance of the
// family in the order the code object has had; nothing calls it.
template <class... K>
static void name_kernels(K...) {}
[[maybe_unused]] static void kernel_order() {
#define A(NX_, NU_)                                                                                                       \
  name_kernels(mpc_backward_asm_select_kernel<NX_, NU_, false, true>, mpc_backward_asm_kernel<NX_, NU_, false, true>,     \
               mpc_backward_asm_select_kernel<NX_, NU_, true, false>, mpc_backward_asm_kernel<NX_, NU_, true, false>,     \
               mpc_backward_asm_select_kernel<NX_, NU_, false, false>, mpc_backward_asm_kernel<NX_, NU_, false, false>);
  DMPC_MPC_STREAM_SHAPES(A, DMPC_NO_SHAPE)
#undef A
#define X(NX_, NU_, L_)                                                                                                   \
  if constexpr (L_ == 16 && SweepRing<NX_, NU_>::kFits)                                                                   \
    name_kernels(mpc_backward_rec_dma_select_kernel<NX_, NU_, SweepRing<NX_, NU_>::kDepth>,                               \
                 mpc_backward_rec_dma_kernel<NX_, NU_, SweepRing<NX_, NU_>::kDepth>);                                     \
  name_kernels(mpc_backward_rec_kernel<NX_, NU_, L_, false>);
  DMPC_MPC_SHAPES(X)
#undef X
#define X(NX_, NU_) name_kernels(lqr_wide_kernel<NX_, NU_, 2, 2, false, false, true>);
  DMPC_MPC_WIDE_SHAPES(X)
#undef X
#define X(NX_, NU_) name_kernels(lqr_wide_kernel<NX_, NU_, 2, 2, true, false, true>);
  DMPC_MPC_WIDE_SHAPES(X)
#undef X
#define X(NX_, NU_) name_kernels(mpc_backward_rec_kernel<NX_, NU_, 16, true>);
  DMPC_MPC_CONTAINERS(X)
#undef X
#define X(NU_) name_kernels(mpc_generic_backward_kernel<NU_>);
  DMPC_ONE_TO_EIGHT(X)
#undef X
  name_kernels(mpc_forward_rec_pendulum_spec_kernel<true>, mpc_forward_rec_pendulum_spec_kernel<false>);
#define A(NX_, NU_) name_kernels(mpc_forward_asm_kernel<NX_, NU_>);
  DMPC_MPC_STREAM_SHAPES(A, A)
#undef A
#define X(NX_, NU_, L_)                                                                                                   \
  if constexpr (L_ == 16 && search_ring_fits<NX_, NU_>()) name_kernels(mpc_forward_rec_kernel<NX_, NU_, L_, true, false>); \
  name_kernels(mpc_forward_rec_kernel<NX_, NU_, L_, false, false>);
  DMPC_MPC_SHAPES(X)
#undef X
#define X(NX_, NU_) name_kernels(mpc_wide_forward_kernel<NX_, NU_, 2, false>);
  DMPC_MPC_WIDE_SHAPES(X)
#undef X
#define X(NX_, NU_) name_kernels(mpc_wide_forward_kernel<NX_, NU_, 2, true>);
  DMPC_MPC_WIDE_SHAPES(X)
#undef X
#define X(NX_, NU_) name_kernels(mpc_forward_rec_kernel<NX_, NU_, 16, false, true>);
  DMPC_MPC_CONTAINERS(X)
#undef X
#define A(NX_, NU_)                                                                                                       \
  name_kernels(mpc_step_fused_asm_kernel<NX_, NU_, false, true>, mpc_step_fused_asm_kernel<NX_, NU_, true, false>,        \
               mpc_step_fused_asm_kernel<NX_, NU_, false, false>);
  DMPC_MPC_STREAM_SHAPES(A, DMPC_NO_SHAPE)
#undef A
#define X(N_) name_kernels(pnqp_kernel<N_>);
  DMPC_ONE_TO_EIGHT(X)
#undef X
}

// Which shapes run padded inside the wide row kernels' instances (sweep and line search alike): those without a 16-lane MPC
// container (16 and more elements of tau, or more than four controls) and, of those with one, three and four controls from
// 12 elements on - MPCstep.forward at B = 4096, T = 50: (9,4) 707 -> 605 us, (11,4) 769 -> 645, (10,3) 629 -> 578; with one
// or two controls the container's short QP wins ((13,2) 568 against 695 us, (14,1) 460 against 562).
static bool mpc_wide_padded(int nx, int nu) { return nx + nu >= 16 || nu > 4 || (nu >= 3 && nx + nu >= 12); }

template <class... P>
static bool aligned16(const P *...p) {   // nullptr counts as aligned
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 15u) == 0;
}

// workgroups that share the bookkeeping of one box-DDP iteration inside the fused sweep launch: 256 rows each
static int select_parts(int B) { const int n = (B + 255) / 256; return n < 1 ? 1 : (n > 8 ? 8 : n); }

// ---- The launchers: one per kernel template.  A job is the entry point's arguments and the problem's own dimensions; the
// launcher of a container tells its kernel the dimensions on a copy, so the caller's arguments stay as they are.
struct MpcSweepJob {
  const MpcBackArgs &a;
  int nx, nu;
  // BoxDDP's fused chain: further workgroups of the (3,1) stream and ring kernels run box_ddp_select_body(*sel), the
  // bookkeeping of the iteration before; nullptr otherwise
  const DdpSelectArgs *sel;
  unsigned *sel_sync;
};
struct MpcSearchJob {
  const MpcFwdArgs &a;
  int nx, nu;
};
using MpcSweepLauncher = int (*)(const MpcSweepJob &j, hipStream_t stream);
using MpcSearchLauncher = int (*)(const MpcSearchJob &j, hipStream_t stream);
using MpcStepLauncher = int (*)(const MpcBackArgs &ba, const MpcFwdArgs &fa, hipStream_t stream);
// a copy of the arguments that tells a padded kernel the problem's dimensions (`pad` false: the copy alone)
template <class Args>
static Args told_dims(Args a, bool pad, int nx, int nu) {
  a.nx_log = pad ? nx : a.nx_log;
  a.nu_log = pad ? nu : a.nu_log;
  return a;
}

// the three forms of the generated sweep: c as given / with f_hat / c re-centred around `states` inside the sweep
template <class F>
static int with_sweep_form(const MpcBackArgs &a, F f) {
  return with_bools([&](auto has_f, auto recentre) -> int {
    if constexpr (decltype(has_f)::value && decltype(recentre)::value) return DMPC_E_UNSUPPORTED;   // (no such stream, no such call)
    else return f(has_f, recentre);
  }, a.states == nullptr && a.f != nullptr, a.states != nullptr);
}

// The sweep as one generated instruction stream with the box QP inside (mpc_asm_kernel.hpp)
template <int NX, int NU>
static int launch_sweep_stream(const MpcSweepJob &j, hipStream_t stream) {
  const int n_sel = j.sel != nullptr ? select_parts(j.a.B) : 0;
  const dim3 grid((j.a.B + 15) / 16 + n_sel), block(256);
  constexpr size_t lds = mpc_asm_lds_bytes<NX, NU>();
  return with_sweep_form(j.a, [&](auto has_f, auto recentre) {
    constexpr bool F = decltype(has_f)::value, R = decltype(recentre)::value;
    return with_bools([&](auto select) {
      if constexpr (decltype(select)::value)
        return launch_kernel(mpc_backward_asm_select_kernel<NX, NU, F, R>, grid, block, lds, stream, j.a, *j.sel, n_sel, j.sel_sync);
      else
        return launch_kernel(mpc_backward_asm_kernel<NX, NU, F, R>, grid, block, lds, stream, j.a);
    }, j.sel != nullptr);
  });
}

// Inputs through the LDS-DMA ring of mpc_dma_kernels.hpp
template <int NX, int NU>
static int launch_sweep_ring(const MpcSweepJob &j, hipStream_t stream) {
  using Ring = SweepRing<NX, NU>;
  const int n_sel = j.sel != nullptr ? select_parts(j.a.B) : 0;
  const dim3 grid((j.a.B + 15) / 16 + n_sel), block(256);
  return with_bools([&](auto select) {
    if constexpr (decltype(select)::value)
      return launch_kernel(mpc_backward_rec_dma_select_kernel<NX, NU, Ring::kDepth>, grid, block, Ring::kLds, stream, j.a, *j.sel,
                           n_sel, j.sel_sync);
    else
      return launch_kernel(mpc_backward_rec_dma_kernel<NX, NU, Ring::kDepth>, grid, block, Ring::kLds, stream, j.a);
  }, j.sel != nullptr);
}

static int launch_sweep_fixed_grid(const MpcSweepJob &j, hipStream_t stream) { return launch_mpc_back_fixed_grid(j.nx, j.nu, j.a, stream); }
// (batch-coupled: `a` is the launcher's copy that `args` point to)
static int launch_sweep_coupled(const void *kernel, dim3 grid, dim3 block, void **args, size_t lds, const MpcSweepJob &j,
                                hipStream_t stream) {
  return launch_coupled(kernel, grid, block, args, lds, stream, [&] { return launch_sweep_fixed_grid(j, stream); });
}

// mpc_backward_rec_kernel: a lane group per trajectory, inputs through register banks.  PAD: a container
template <int NX, int NU, int L, bool PAD>
static int launch_sweep_rows(const MpcSweepJob &j, hipStream_t stream) {
  constexpr int GPB = 256 / L;
  MpcBackArgs a = told_dims(j.a, PAD, j.nx, j.nu);
  const dim3 grid((a.B + GPB - 1) / GPB), block(256);
  if (a.sync == nullptr) return launch_kernel(mpc_backward_rec_kernel<NX, NU, L, PAD>, grid, block, 0, stream, a);
  void *args[] = {&a};
  return launch_sweep_coupled(reinterpret_cast<const void *>(&mpc_backward_rec_kernel<NX, NU, L, PAD>), grid, block, args, 0, j, stream);
}

// the sweeps of lqr_wide_kernel.hpp and lqr_wave_api.hip take the box QP's arguments inside an LqrArgs
static LqrArgs as_lqr_args(const MpcBackArgs &a) {
  LqrArgs s{a.T, a.B, a.C, a.c, a.F, a.f, nullptr, nullptr, a.Ks, a.ks, nullptr, nullptr, nullptr, nullptr, a.info};
  s.mpc_controls = a.controls;
  s.mpc_lower = a.lower;
  s.mpc_upper = a.upper;
  s.mpc_states = a.states;
  s.mpc_n_qp_iter = a.n_qp_iter;
  s.mpc_n_qp_total = a.n_qp_total;
  s.mpc_done = a.done;
  s.info_store = a.info_store != 0;
  return s;
}

// (12,4), (16,4), (12,8), (16,8): the sweep on the wide row kernel with the box QP inside (lqr_wide_kernel<..., MPC>: four
// trajectories per wavefront, matrix-core products; before, the runtime-dimension kernel - 2.0 ms at (12,4), B = 4096, T = 50 -
// and, at (16,8), a wavefront per trajectory) - and, padded inside the smallest of those instances, every other shape of
// mpc_wide_padded ((5,5): 2.0 -> 1.3 ms per MPCstep.forward)
template <int NX, int NU>
static int launch_sweep_wide(const MpcSweepJob &j, hipStream_t stream) {
  const bool pad = j.nx != NX || j.nu != NU;
  const LqrArgs s = told_dims(as_lqr_args(j.a), pad, j.nx, j.nu);
  return with_bools([&](auto PAD) {
    return launch_kernel_big_lds(lqr_wide_kernel<NX, NU, 2, 2, decltype(PAD)::value, false, true>, dim3((s.B + 15) / 16), dim3(256),
                                 LqrWideLayout<NX, NU, 2, 2>::lds_bytes(), stream, s);
  }, pad);
}

// (16,8), (32,8): the matrix-core sweep with the box QP inside (lqr_wave_mfma_backward<..., MPC>) ...
static int launch_sweep_wave(const MpcSweepJob &j, hipStream_t stream) {
  return launch_mpc_wave_backward(j.nx, j.nu, as_lqr_args(j.a), stream);
}
// ... and a problem wider than the 16-lane containers padded inside one of those instances
template <int NX, int NU>
static int launch_sweep_wave_container(const MpcSweepJob &j, hipStream_t stream) {
  return launch_mpc_wave_container_backward(NX, NU, told_dims(as_lqr_args(j.a), true, j.nx, j.nu), stream);
}

// the runtime-dimension kernel (mpc_generic.hpp)
template <int NU>
static int launch_sweep_generic(const MpcSweepJob &j, hipStream_t stream) {
  const size_t lds = mpc_generic_back_lds_bytes<NU>(j.nx);
  const dim3 grid(j.a.B), block(64);
  if (j.a.sync == nullptr) return launch_kernel(mpc_generic_backward_kernel<NU>, grid, block, lds, stream, j.a, j.nx);
  MpcBackArgs a = j.a;
  int nx = j.nx;
  void *args[] = {&a, &nx};
  return launch_sweep_coupled(reinterpret_cast<const void *>(&mpc_generic_backward_kernel<NU>), grid, block, args, lds, j, stream);
}

// a workgroup per trajectory, matrices in the caller's workspace (mpc_tiled.hpp)
static size_t sweep_tiled_lds_bytes(int nx, int nu) { return (pnqp_tiled_lds_floats(nu) + (size_t)(nx + nu)) * sizeof(float); }
static int launch_sweep_tiled(const MpcSweepJob &j, hipStream_t stream) {
  return launch_kernel(mpc_tiled_backward_kernel, dim3(j.a.B), dim3(kTiledThreads), sweep_tiled_lds_bytes(j.nx, j.nu), stream, j.a,
                       j.nx, j.nu, j.a.tiled_scratch);
}

// Both generated streams in one launch (mpc_step_fused_kernel.hpp)
template <int NX, int NU>
static int launch_step_fused(const MpcBackArgs &ba, const MpcFwdArgs &fa, hipStream_t stream) {
  return with_sweep_form(ba, [&](auto has_f, auto recentre) {
    return launch_kernel(mpc_step_fused_asm_kernel<NX, NU, decltype(has_f)::value, decltype(recentre)::value>, dim3((ba.B + 15) / 16),
                         dim3(256), mpc_step_fused_lds_bytes<NX, NU>(), stream, ba, fa);
  });
}

// rollout + linearisation of the built-in pendulum: four lanes per trajectory when the 16-byte row accesses are aligned
static void launch_pendulum_rollout(const PendulumArgs &pa, hipStream_t stream) {
  if (aligned16(pa.F, pa.C) && !knob_on<Knob::DMPC_NO_SPEC4>())
    DMPC_LAUNCH_GGL(pendulum_rollout_linearize4_kernel, dim3((4 * pa.B + 255) / 256), dim3(256), 0, stream, pa);
  else
    DMPC_LAUNCH_GGL(pendulum_rollout_linearize_kernel, dim3((pa.B + 63) / 64), dim3(64), 0, stream, pa);
}

// The pendulum's line search usually walks ten or more step sizes.  A wavefront per trajectory, all inputs and candidates in LDS ...
static int launch_search_spec4(const MpcSearchJob &j, hipStream_t stream) {
  return launch_kernel(mpc_forward_rec_pendulum_spec4_kernel, dim3((j.a.B + 3) / 4), dim3(256), Spec4Layout::lds_bytes(j.a.T), stream, j.a);
}
// ... or 16 candidates per trajectory at once; every candidate keeps its trajectory in LDS (T * 4 KB per workgroup) when that fits
template <bool DMA>
static int launch_search_spec(const MpcSearchJob &j, hipStream_t stream) {
  MpcFwdArgs a = j.a;
  const size_t lds = (size_t)a.T * 4 * 256 * sizeof(float);
  a.traj_in_lds = lds <= 96 * 1024 ? 1 : 0;
  return launch_kernel(mpc_forward_rec_pendulum_spec_kernel<DMA>, dim3((a.B + 15) / 16), dim3(256),
                       (a.traj_in_lds ? lds : 0) + (DMA ? SpecDmaLayout::lds_bytes() : 0), stream, a);
}

// the line search as one generated instruction stream (mpc_fwd_asm_kernel.hpp)
template <int NX, int NU>
static int launch_search_stream(const MpcSearchJob &j, hipStream_t stream) {
  return launch_kernel(mpc_forward_asm_kernel<NX, NU>, dim3((j.a.B + 15) / 16), dim3(256), mpc_fwd_asm_lds_bytes<NX, NU>(), stream, j.a);
}

// mpc_forward_rec_kernel: a lane group per trajectory.  DMA: inputs through the LDS-DMA ring; PAD: a container
template <int NX, int NU, int L, bool DMA, bool PAD>
static int launch_search_rows(const MpcSearchJob &j, hipStream_t stream) {
  constexpr int GPB = 256 / L;
  size_t lds = 0;
  if constexpr (DMA) lds = MpcFwdDmaLayout<NX, NU>::lds_bytes();
  const MpcFwdArgs a = told_dims(j.a, PAD, j.nx, j.nu);
  return launch_kernel(mpc_forward_rec_kernel<NX, NU, L, DMA, PAD>, dim3((a.B + GPB - 1) / GPB), dim3(256), lds, stream, a);
}

// 17 to 31 elements of tau, at most 16 states: the line search of the wide row layout (mpc_wide_forward_kernel.hpp: four
// trajectories per wavefront; before, the runtime-dimension kernel - 0.68 ms at (12,4)), padded shapes as the sweep's
template <int NX, int NU>
static int launch_search_wide(const MpcSearchJob &j, hipStream_t stream) {
  using Lay = MpcWideFwdLayout<NX, NU, 2>;
  static_assert(Lay::lds_bytes() <= 160 * 1024, "ring beyond a CU's LDS");
  const bool pad = j.nx != NX || j.nu != NU;
  const MpcFwdArgs a = told_dims(j.a, pad, j.nx, j.nu);
  return with_bools([&](auto PAD) {
    return launch_kernel_big_lds(mpc_wide_forward_kernel<NX, NU, 2, decltype(PAD)::value>, dim3((a.B + 15) / 16), dim3(256),
                                 Lay::lds_bytes(), stream, a);
  }, pad);
}

// the runtime-dimension kernels (mpc_generic.hpp): the inputs of a step through an LDS ring, or fetched row by row
static int launch_search_staged(const MpcSearchJob &j, hipStream_t stream) {
  return launch_kernel_big_lds(mpc_staged_forward_kernel, dim3(j.a.B), dim3(64), mpc_staged_fwd_lds_bytes(j.nx, j.nu), stream, j.a, j.nx, j.nu);
}
static int launch_search_generic(const MpcSearchJob &j, hipStream_t stream) {
  return launch_kernel(mpc_generic_forward_kernel, dim3(j.a.B), dim3(64), mpc_generic_fwd_lds_bytes(j.nx, j.nu), stream, j.a, j.nx, j.nu);
}
static size_t search_tiled_lds_bytes(int nx, int nu) { return (size_t)(2 * nx + 2 * (nx + nu) + 4) * sizeof(float); }
static int launch_search_tiled(const MpcSearchJob &j, hipStream_t stream) {
  return launch_kernel(mpc_tiled_forward_kernel, dim3(j.a.B), dim3(kTiledThreads), search_tiled_lds_bytes(j.nx, j.nu), stream, j.a, j.nx, j.nu);
}

// ---- The routes: which kernel takes the sweep (MPCstep.backward_rec) and which the line search (forward_rec) of a call.
// They take values only, launch nothing and dereference nothing, and every entry point asks them for all it will launch
// before its first launch: a refused call has launched nothing.  (The form of a sweep - with f_hat, re-centring - picks no
// kernel family: every stream has all three, so its launcher reads it from the arguments.)
struct MpcSweepCall {
  int T, B, nx, nu;
  bool coupled;        // batch-coupled termination of the box QPs (a.sync)
  bool in_ddp_loop;    // a step of the device-driven BoxDDP loop: a `done` flag, or flags stored instead of or-ed
  bool select;         // ... with the bookkeeping of the iteration before riding along (MpcSweepJob::sel)
  bool ring_aligned;   // what the LDS-DMA ring fetches is 16-byte aligned: C, c, F, f, controls, lower, upper, states
  bool wide_aligned;   // what the wide row kernel fetches by 16 bytes is: C, c, F, f
  bool scratch;        // the caller has a tiled scratch to give
};
struct MpcSearchCall {
  int T, B, nx, nu;
  int dyn_kind;        // 0: LinDx (F, f); 1: the built-in pendulum
  bool ls_cap;         // a cap on the step sizes tried (the streams and the wide kernel need one)
  bool info_in;        // the sweep's flags arrive through a staging word (BoxDDP's fused chain)
  bool ring_aligned;   // C, c, F, f, Ks, ks, controls, lower, upper, states (the pendulum has no F, f: absent counts as aligned)
};
enum class MpcKernel { kOther, kStream, kRing, kSpec4 };
struct MpcSweepRoute {
  int code;                            // 0, or the DMPC_E_* of a refusal
  MpcSweepLauncher launch = nullptr;
  MpcKernel kind = MpcKernel::kOther;
  bool needs_scratch = false;          // a.tiled_scratch is read: the tiled kernel, and every batch-coupled call (the fixed grid)
  MpcStepLauncher fused = nullptr;     // kStream: the launch that also holds the search's stream
};
struct MpcSearchRoute {
  int code;
  MpcSearchLauncher launch = nullptr;
  MpcKernel kind = MpcKernel::kOther;
};

// four trajectories per wavefront: at least one whole wavefront and a horizon with an F ...
static bool fills_a_wave(int T, int B) { return B >= 4 && T >= 2; }
// ... and, for what goes through an LDS-DMA ring or runs padded, no ragged last wavefront
static bool whole_waves(int B) { return B >= 4 && B % 4 == 0; }
// the wide row kernels index a time step by 32 bits
static bool wide_strides_fit(int B, int nx, int nu) { return (size_t)B * (nx + nu) * (nx + nu) * 4 < ((size_t)1 << 31); }
// the runtime-dimension kernels: a wavefront's lanes hold the columns, the QP up to eight controls; beyond: mpc_tiled.hpp
static bool runtime_dims_fit(int nx, int nu) { return nx + nu + 1 <= 64 && nu <= kMpcGenericMaxNu; }

// the wide instance (index into DMPC_MPC_WIDE_SHAPES) that takes the shape - its own, or the smallest that holds a shape of
// mpc_wide_padded, whole wavefronts only - or -1
static int wide_instance(int B, int nx, int nu) {
  constexpr int dims[][2] = {
#define X(NX_, NU_) {NX_, NU_},
      DMPC_MPC_WIDE_SHAPES(X)
#undef X
  };
  for (int i = 0; i < 4; ++i)
    if (nx == dims[i][0] && nu == dims[i][1]) return i;
  if (!(nx >= 1 && nu >= 1 && mpc_wide_padded(nx, nu) && B % 4 == 0 && !knob_on<Knob::DMPC_NO_CONTAINER>())) return -1;
  for (int i = 0; i < 4; ++i)
    if (nx <= dims[i][0] && nu <= dims[i][1]) return i;
  return -1;
}
#define X(NX_, NU_) launch_sweep_wide<NX_, NU_>,
static constexpr MpcSweepLauncher kSweepWide[] = {DMPC_MPC_WIDE_SHAPES(X)};
#undef X
#define X(NX_, NU_) launch_search_wide<NX_, NU_>,
static constexpr MpcSearchLauncher kSearchWide[] = {DMPC_MPC_WIDE_SHAPES(X)};
#undef X

// a shape with a 16-lane specialisation of its own: through the ring, else (and batch-coupled) on the register banks
template <int NX, int NU, int L>
static MpcSweepRoute sweep_route_exact(const MpcSweepCall &q, bool ring) {
  if constexpr (L == 16 && SweepRing<NX, NU>::kFits) {
    if (ring) return {0, launch_sweep_ring<NX, NU>, MpcKernel::kRing};
  }
  if (q.select) return {DMPC_E_BADARG};
  return {0, launch_sweep_rows<NX, NU, L, false>, MpcKernel::kOther, q.coupled};
}

static MpcSweepRoute mpc_sweep_route(const MpcSweepCall &q) {
  const int nx = q.nx, nu = q.nu;
  // per-trajectory termination, whole wavefronts of four trajectories, 16-byte aligned runs: inputs through the LDS-DMA
  // ring of mpc_dma_kernels.hpp (DMPC_NO_MPC_DMA=1: the register-bank kernel, for A/B timing)
  const bool ring = !q.coupled && whole_waves(q.B) && !knob_on<Knob::DMPC_NO_MPC_DMA>() && q.ring_aligned;
  if (q.select && !ring) return {DMPC_E_BADARG};   // (BoxDDP asks with `select` only after a route that took the ring)
  // The sweep as one generated instruction stream: shapes the generator covers.  DMPC_NO_MPC_ASM=1: the HIP kernels (A/B timing).
  if (ring && q.T >= 2 && !knob_on<Knob::DMPC_NO_MPC_ASM>()) {
#define A(NX_, NU_) \
  if (nx == NX_ && nu == NU_) return {0, launch_sweep_stream<NX_, NU_>, MpcKernel::kStream, false, launch_step_fused<NX_, NU_>};
    DMPC_MPC_STREAM_SHAPES(A, DMPC_NO_SHAPE)
#undef A
  }
#define X(NX_, NU_, L_) \
  if (nx == NX_ && nu == NU_) return sweep_route_exact<NX_, NU_, L_>(q, ring);
  DMPC_MPC_SHAPES(X)
#undef X
  if (q.select) return {DMPC_E_BADARG};   // (bookkeeping rides in the stream and ring kernels alone)
  // DMPC_NO_WIDE=1: the kernels below
  if (!knob_on<Knob::DMPC_NO_WIDE>() && !q.coupled && fills_a_wave(q.T, q.B) && q.wide_aligned && wide_strides_fit(q.B, nx, nu)) {
    if (const int i = wide_instance(q.B, nx, nu); i >= 0) return {0, kSweepWide[i]};
  }
  // the matrix-core sweep: per-trajectory termination, not inside the device-driven BoxDDP loop (no `done` flag there)
  const bool wave = !q.coupled && !q.in_ddp_loop && !knob_on<Knob::DMPC_NO_MPC_WAVE>();
  if (wave && ((nx == 16 && nu == 8) || (nx == 32 && nu == 8)) && q.T >= 1) return {0, launch_sweep_wave};
  if (!knob_on<Knob::DMPC_NO_CONTAINER>()) {   // a smaller problem inside the first container that holds it
#define X(NX_, NU_) \
  if (nx <= NX_ && nu <= NU_) return {0, launch_sweep_rows<NX_, NU_, 16, true>, MpcKernel::kOther, q.coupled};
    DMPC_MPC_CONTAINERS(X)
#undef X
    // A padded wave instance costs what ITS shape costs (and fetches element by element, one wavefront per SIMD): measured at
    // B = 4096, T = 50 it beats the runtime-dimension kernel where the latter's QP in lane 0 is widest - (24,8) 9.2 against
    // 12.5 ms - and lost below - (20,6) 7.8 against 5.4 ms, (10,5) 5.4 against 2.9 ms.
    // (Round 4, the padded instance fetching through its LDS-DMA slot: (20,6) 3.4 against 3.8 ms - six controls and more.)
    // (Round 5, from 21 states on with three to five controls, from 24 with one or two: the runtime-dimension kernel's cost grows with nx^2 in one lane group -
    // (32,4) 7.7 ms, (32,2) 6.4, (23,4) 4.2, (24,4) 3.9 - where the padded (32,8) instance stays at ~3 ms: (32,4) 3.1, (32,2) 2.8, (24,4) 3.0.)
    const bool small = nu <= 4 && nx + nu <= 15;     // (the 16-lane containers above take these)
    if (wave && !small && nx <= 32 && nu <= 8) {
      if (nu >= 6 && nx <= 16) return {0, launch_sweep_wave_container<16, 8>};
      if (nu >= 6 || nx >= (nu >= 3 ? 21 : 24)) return {0, launch_sweep_wave_container<32, 8>};
    }
  }
  if (runtime_dims_fit(nx, nu)) {
#define X(NU_) \
  if (nu == NU_) return {0, launch_sweep_generic<NU_>, MpcKernel::kOther, q.coupled};
    DMPC_ONE_TO_EIGHT(X)
#undef X
  }
  // any other size (more than 8 controls, more than 64 columns): a workgroup per trajectory, matrices in the caller's
  // workspace (mpc_tiled.hpp; batch-coupled: mpc_coupled.hpp)
  if (!q.scratch) return {DMPC_E_WORKSPACE, nullptr, MpcKernel::kOther, true};
  if (q.coupled) return {0, launch_sweep_fixed_grid, MpcKernel::kOther, true};
  if (sweep_tiled_lds_bytes(nx, nu) > 60 * 1024) return {DMPC_E_UNSUPPORTED, nullptr, MpcKernel::kOther, true};
  return {0, launch_sweep_tiled, MpcKernel::kOther, true};
}

template <int NX, int NU, int L>
static MpcSearchRoute search_route_exact(bool ring) {
  if constexpr (L == 16 && search_ring_fits<NX, NU>()) {
    if (ring) return {0, launch_search_rows<NX, NU, L, true, false>, MpcKernel::kRing};
  }
  return {0, launch_search_rows<NX, NU, L, false, false>};
}

static MpcSearchRoute mpc_search_route(const MpcSearchCall &q) {
  const int nx = q.nx, nu = q.nu;
  const bool lin = q.dyn_kind == 0;
  // whole wavefronts of four trajectories, 16-byte aligned runs: inputs through an LDS-DMA ring
  const bool ring = whole_waves(q.B) && !knob_on<Knob::DMPC_NO_MPC_DMA>() && q.ring_aligned;
  if (q.dyn_kind == 1 && nx == 3 && nu == 1 && !knob_on<Knob::DMPC_NO_SPEC_LS>()) {
    if (q.T <= kSpec4MaxT && !knob_on<Knob::DMPC_NO_SPEC4>()) return {0, launch_search_spec4, MpcKernel::kSpec4};
    return {0, ring ? launch_search_spec<true> : launch_search_spec<false>};
  }
  // DMPC_NO_MPC_ASM=1: the HIP kernels
  if (lin && ring && q.ls_cap && !knob_on<Knob::DMPC_NO_MPC_ASM>()) {
#define A(NX_, NU_) \
  if (nx == NX_ && nu == NU_) return {0, launch_search_stream<NX_, NU_>, MpcKernel::kStream};
    DMPC_MPC_STREAM_SHAPES(A, A)
#undef A
  }
#define X(NX_, NU_, L_) \
  if (nx == NX_ && nu == NU_) return search_route_exact<NX_, NU_, L_>(lin && ring);
  DMPC_MPC_SHAPES(X)
#undef X
  if (!lin) return {DMPC_E_UNSUPPORTED};   // (a built-in dynamics has the kernels of its own shape alone)
  // DMPC_NO_WIDE=1: the kernels below
  if (!knob_on<Knob::DMPC_NO_WIDE>() && q.ls_cap && fills_a_wave(q.T, q.B) && !q.info_in && q.ring_aligned &&
      wide_strides_fit(q.B, nx, nu)) {
    if (const int i = wide_instance(q.B, nx, nu); i >= 0) return {0, kSearchWide[i]};
  }
  if (!knob_on<Knob::DMPC_NO_CONTAINER>()) {
#define X(NX_, NU_) \
  if (nx <= NX_ && nu <= NU_) return {0, launch_search_rows<NX_, NU_, 16, false, true>};
    DMPC_MPC_CONTAINERS(X)
#undef X
  }
  if (runtime_dims_fit(nx, nu)) {
    // the inputs of a step through an LDS ring (mpc_staged_forward_kernel); DMPC_NO_MPC_STAGED_FWD=1: fetched row by row
    if (!knob_on<Knob::DMPC_NO_MPC_STAGED_FWD>() && mpc_staged_fwd_lds_bytes(nx, nu) <= 150 * 1024) return {0, launch_search_staged};
    return {0, launch_search_generic};
  }
  if (search_tiled_lds_bytes(nx, nu) > 60 * 1024) return {DMPC_E_UNSUPPORTED};   // any other size: mpc_tiled.hpp
  return {0, launch_search_tiled};
}

// the values of a call, read off its arguments once
static MpcSweepCall sweep_call(int nx, int nu, const MpcBackArgs &a, bool select, bool scratch) {
  return {a.T, a.B, nx, nu, a.sync != nullptr, a.done != nullptr || a.info_store != 0, select,
          aligned16(a.C, a.c, a.F, a.f, a.controls, a.lower, a.upper, a.states), aligned16(a.C, a.c, a.F, a.f), scratch};
}
static MpcSearchCall search_call(int nx, int nu, const MpcFwdArgs &a) {
  return {a.T, a.B, nx, nu, a.dyn_kind, a.ls_cap > 0, a.info_in != nullptr,
          aligned16(a.C, a.c, a.F, a.f, a.Ks, a.ks, a.controls, a.lower, a.upper, a.states)};
}
// does a sweep of this size read a tiled scratch?  (No switch and no alignment moves a shape on or off the tiled kernel.)
static bool sweep_needs_scratch(int T, int B, int nx, int nu) {
  return mpc_sweep_route({T, B, nx, nu, false, false, false, false, false, true}).needs_scratch;
}
// Both generated streams in one launch when each route answered with its stream.  DMPC_NO_MPC_FUSED=1: two launches (A/B).
static MpcStepLauncher fused_step(const MpcSweepRoute &sweep, const MpcSearchRoute &search) {
  return search.kind == MpcKernel::kStream && !knob_on<Knob::DMPC_NO_MPC_FUSED>() ? sweep.fused : nullptr;
}

static int run_sweep(const MpcSweepRoute &r, int nx, int nu, const MpcBackArgs &a, hipStream_t stream, const DdpSelectArgs *sel = nullptr,
                     unsigned *sel_sync = nullptr) {
  if (a.sync != nullptr) {   // fresh decision slots for this launch
    const hipError_t e = hipMemsetAsync(a.sync, 0, coupled_bytes(a.T, a.n_qp_iter), stream);
    if (e != hipSuccess) return (int)e;
  }
  return r.launch({a, nx, nu, sel, sel_sync}, stream);
}

struct MpcWs {
  size_t c_back, neg, x0, dx, du, mask, sync, tiled, lqr, total;
};
constexpr int kSyncQpIterMax = 64;   // the workspace queries do not know n_qp_iter_max: sized for up to this many

static MpcWs mpc_layout(int T, int B, int nx, int nu) {
  const size_t ns = nx + nu;
  MpcWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += round_up(bytes, 256);
    return o;
  };
  w.c_back = take((size_t)T * B * ns * sizeof(float));  // forward: re-centred c ; backward: unused
  w.neg = take((size_t)T * B * ns * sizeof(float));     // backward: -[dl_dx;dl_du]
  w.x0 = take((size_t)B * nx * sizeof(float));
  w.dx = take((size_t)T * B * nx * sizeof(float));
  w.du = take((size_t)T * B * nu * sizeof(float));
  w.mask = take((size_t)T * B * nu);
  w.sync = take(coupled_bytes(T, kSyncQpIterMax));
  w.tiled = take(coupled_traj_bytes(B, nx, nu));     // the tiled sweep's matrices (+ the QP's vectors of its batch-coupled form)
  w.lqr = off;
  off += round_up(dmpc_lqr_workspace_bytes(T, B, nx, nu), 256);
  w.total = off;
  return w;
}

// workspace of the device-driven box-DDP loop (dmpc_box_ddp)
struct DdpWs {
  size_t xs, F, f, c_back, Ks, ks, x_new, u_a, u_b, u_c, u1, u1_b, costs, costs_b, old, alphas, nqp, nls, keep, info_back, stage_a,
      stage_b, sel_sync, sync, tiled, total;
};
static DdpWs ddp_layout(int T, int B, int nx, int nu) {
  const size_t ns = nx + nu, TB = (size_t)T * B, fl = sizeof(float);
  DdpWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += round_up(bytes, 256);
    return o;
  };
  w.xs = take(TB * nx * fl);
  w.F = take(TB * nx * ns * fl);   // linearisation of a built-in dynamics (unused with a LinDx)
  w.f = take(TB * nx * fl);
  w.c_back = take(TB * ns * fl);
  w.Ks = take(TB * nu * nx * fl);
  w.ks = take(TB * nu * fl);
  w.x_new = take(TB * nx * fl);
  w.u_a = take(TB * nu * fl);
  w.u_b = take(TB * nu * fl);
  w.u_c = take(TB * nu * fl);     // (third control buffer, second u1 / costs, staging flags: the one-launch iterations)
  w.u1 = take(TB * nu * fl);
  w.u1_b = take(TB * nu * fl);
  w.costs = take((size_t)B * fl);
  w.costs_b = take((size_t)B * fl);
  w.old = take((size_t)B * fl);
  w.alphas = take((size_t)B * fl);
  w.nqp = take((size_t)B * sizeof(int32_t));
  w.nls = take((size_t)B * sizeof(int32_t));
  w.keep = take((size_t)B * sizeof(int32_t));
  w.info_back = take((size_t)B * sizeof(int32_t));
  w.stage_a = take((size_t)B * sizeof(int32_t));
  w.stage_b = take((size_t)B * sizeof(int32_t));
  w.sel_sync = take(4 * sizeof(unsigned));
  w.sync = take(coupled_bytes(T, kSyncQpIterMax));
  w.tiled = take(coupled_traj_bytes(B, nx, nu));
  w.total = off;
  return w;
}

// The stage cost of a box-DDP chain: a QuadCost's C [T,B,ns,ns], c [T,B,ns], or a packed MlpCost (mlp_cost_launch.hpp), whose
// Taylor model the chain forms itself - in C_hat, c_hat behind the workspace of ddp_layout.
struct DdpCost {
  const float *C = nullptr, *c = nullptr;   // QuadCost
  bool net = false;                         // MlpCost: m, act, and whether the search also stores the next Taylor model
  MlpCostModel m{};
  int act = 0;
  bool search_approximates = false;
};
struct DdpCostWs {
  size_t C_hat, c_hat, total;
};
static DdpCostWs ddp_cost_layout(int T, int B, int nx, int nu) {
  const size_t ns = nx + nu, TB = (size_t)T * B;
  DdpCostWs w;
  w.C_hat = ddp_layout(T, B, nx, nu).total;
  w.c_hat = w.C_hat + round_up(TB * ns * ns * sizeof(float), 256);
  w.total = w.c_hat + round_up(TB * ns * sizeof(float), 256);
  return w;
}

// dmpc_mpc_step_status: one workgroup reduces the step's per-trajectory words (include/dmpc.h)
__global__ __launch_bounds__(1024) void mpc_step_status_kernel(int B, const int32_t *__restrict__ info, const int32_t *__restrict__ nqp,
                                                               const float *__restrict__ alphas, int32_t *__restrict__ status) {
  __shared__ int s_or[16], s_max[16], s_bad[16];
  __shared__ double s_sum[16];
  int o = 0, m = 0, bad = 0;
  double sum = 0.0;
  for (int b = threadIdx.x; b < B; b += 1024) {
    if (info != nullptr) {
      const int v = info[b];
      o |= v;
      bad += (v & DMPC_INFO_NONFINITE) != 0 ? 1 : 0;
    }
    if (nqp != nullptr) m = max(m, nqp[b]);
    if (alphas != nullptr) sum += (double)alphas[b];
  }
  for (int d = 32; d >= 1; d >>= 1) {
    o |= __shfl_xor(o, d);
    m = max(m, __shfl_xor(m, d));
    bad += __shfl_xor(bad, d);
    sum += __shfl_xor(sum, d);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_or[w] = o; s_max[w] = m; s_bad[w] = bad; s_sum[w] = sum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 16; ++i) { o |= s_or[i]; m = max(m, s_max[i]); bad += s_bad[i]; sum += s_sum[i]; }
    const unsigned long long bits = __double_as_longlong(sum);
    status[0] = o; status[1] = m; status[2] = bad; status[3] = 0;
    status[4] = (int32_t)(bits & 0xffffffffull); status[5] = (int32_t)(bits >> 32); status[6] = 0; status[7] = 0;
  }
}

static int grid_for(size_t n) {
  const size_t blocks = (n + 255) / 256;
  return (int)(blocks > 8192 ? 8192 : (blocks == 0 ? 1 : blocks));
}

void launch_active_mask(int T, int B, int nx, int nu, const float *u, const float *u_lower, const float *u_upper,
                        const float *grad_x, const float *grad_u, uint8_t *mask, float *neg, float *x0, float *zero_a,
                        float *zero_b, const float *detach_norm, const int32_t *detach_flag, float detach_eps,
                        hipStream_t stream) {
  const size_t rows = (size_t)T * B;
  DMPC_LAUNCH_GGL(active_mask_kernel, dim3(grid_for(rows * (nx + nu))), dim3(256), 0, stream, rows, nx, nu, u, u_lower,
                  u_upper, grad_x, grad_u, mask, neg, x0, (size_t)B * nx, zero_a, zero_b, B, detach_norm, detach_flag,
                  detach_eps);
}

}  // namespace dmpc

using namespace dmpc;

extern "C" {

size_t dmpc_coupled_workspace_bytes(int T, int n_qp_iter_max) {
  if (T <= 0 || n_qp_iter_max <= 0) return 0;
  return coupled_bytes(T, n_qp_iter_max);
}

size_t dmpc_pnqp_workspace_bytes(int B, int n, int n_iter, int batch_coupled) {
  if (B <= 0 || n <= 0 || n_iter <= 0 || !batch_coupled) return 0;
  return coupled_bytes(1, n_iter) + pnqp_coupled_row_bytes(B, n);
}

int dmpc_pnqp(int B, int n, const float *H, const float *q, const float *lower, const float *upper,
              const float *x_init, int n_iter, int batch_coupled, float *x, float *fac, int32_t *piv, float *index_f,
              int32_t *n_iter_out, void *ws, size_t ws_bytes, int32_t *info, dmpc_stream_t stream_) {
  if (B <= 0 || n <= 0 || n_iter <= 0 || !H || !q || !lower || !upper || !x || !fac || !index_f || !n_iter_out)
    return DMPC_E_BADARG;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const dim3 block(256), grid((B + 255) / 256);
  unsigned *sync = nullptr;
  if (batch_coupled) {
    if (!ws || ws_bytes < coupled_bytes(1, n_iter)) return DMPC_E_WORKSPACE;
    sync = static_cast<unsigned *>(ws);
    const hipError_t e = hipMemsetAsync(sync, 0, coupled_bytes(1, n_iter), stream);
    if (e != hipSuccess) return (int)e;
  }
  PnqpArgs a{B, H, q, lower, upper, x_init, n_iter, x, fac, piv, index_f, n_iter_out, info, sync};
  void *args[] = {&a};
  // batch-coupled on a grid that always fits (mpc_coupled.hpp): any n, any B; needs dmpc_pnqp_workspace_bytes
  auto fixed_grid = [&]() -> int {
    if (ws_bytes < dmpc_pnqp_workspace_bytes(B, n, n_iter, 1)) return DMPC_E_WORKSPACE;
    PnqpTiledArgs ta{B, n, H, q, lower, upper, x_init, n_iter, x, fac, piv, index_f, n_iter_out, info};
    float *vecs = reinterpret_cast<float *>(static_cast<char *>(ws) + coupled_bytes(1, n_iter));
    void *targs[] = {&ta, &vecs, &sync};
    return launch_fixed_grid(reinterpret_cast<const void *>(&pnqp_coupled_kernel), B, targs, stream);
  };
  void (*kernel)(const PnqpArgs) = nullptr;   // up to eight unknowns: a lane per QP
#define X(N_) \
  if (n == N_) kernel = pnqp_kernel<N_>;
  DMPC_ONE_TO_EIGHT(X)
#undef X
  if (kernel != nullptr) {
    if (sync == nullptr) return launch_kernel(kernel, grid, block, 0, stream, a);
    return launch_coupled(reinterpret_cast<const void *>(kernel), grid, block, args, 0, stream, fixed_grid);
  }
  // any n: a workgroup per QP (mpc_tiled.hpp; batch-coupled: mpc_coupled.hpp)
  if (sync != nullptr) return fixed_grid();
  const size_t shmem = pnqp_tiled_lds_floats(n) * sizeof(float);
  if (shmem > 60 * 1024) return DMPC_E_UNSUPPORTED;
  PnqpTiledArgs ta{B, n, H, q, lower, upper, x_init, n_iter, x, fac, piv, index_f, n_iter_out, info};
  return launch_kernel(pnqp_tiled_kernel, dim3(B), dim3(kTiledThreads), shmem, stream, ta);
}

size_t dmpc_mpc_backward_rec_workspace_bytes(int T, int B, int nx, int nu, int n_qp_iter_max, int batch_coupled) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return 0;
  if (batch_coupled) return coupled_bytes(T, n_qp_iter_max) + coupled_traj_bytes(B, nx, nu);
  return sweep_needs_scratch(T, B, nx, nu) ? (size_t)B * mpc_tiled_scratch_floats(nx, nu) * sizeof(float) : 0;
}

int dmpc_mpc_backward_rec(int T, int B, int nx, int nu, const float *C_hat, const float *c_hat,
                          const float *F_hat, const float *f_hat, const float *controls, const float *u_lower,
                          const float *u_upper, int n_qp_iter_max, int batch_coupled, float *Ks_out, float *ks_out,
                          int32_t *n_qp_iter, void *ws, size_t ws_bytes, int32_t *info, dmpc_stream_t stream_) {
  if (T <= 1 || B <= 0 || nx <= 0 || nu <= 0 || n_qp_iter_max <= 0) return DMPC_E_BADARG;
  if (!C_hat || !c_hat || !F_hat || !controls || !u_lower || !u_upper || !Ks_out || !ks_out || !n_qp_iter)
    return DMPC_E_BADARG;
  if (!aligned16(C_hat) || !aligned16(c_hat) || !aligned16(F_hat) || !aligned16(f_hat)) return DMPC_E_BADARG;
  if (batch_coupled && (!ws || ws_bytes < dmpc_mpc_backward_rec_workspace_bytes(T, B, nx, nu, n_qp_iter_max, 1))) return DMPC_E_WORKSPACE;
  MpcBackArgs ba{T, B, C_hat, c_hat, F_hat, f_hat, controls, u_lower, u_upper, n_qp_iter_max, Ks_out, ks_out,
                 n_qp_iter, info, nullptr, batch_coupled ? static_cast<unsigned *>(ws) : nullptr, nullptr};
  const bool scratch = batch_coupled || (ws && ws_bytes >= (size_t)B * mpc_tiled_scratch_floats(nx, nu) * sizeof(float));
  const MpcSweepRoute r = mpc_sweep_route(sweep_call(nx, nu, ba, false, scratch));
  if (r.code != 0) return r.code;
  if (r.needs_scratch)   // (batch-coupled: behind the decision slots)
    ba.tiled_scratch = reinterpret_cast<float *>(static_cast<char *>(ws) + (batch_coupled ? coupled_bytes(T, n_qp_iter_max) : 0));
  return run_sweep(r, nx, nu, ba, static_cast<hipStream_t>(stream_));
}

int dmpc_mpc_forward_rec(int T, int B, int nx, int nu, const float *Ks, const float *ks, const float *controls,
                         const float *states, const float *u_lower, const float *u_upper, const float *C_true,
                         const float *c_true, const float *F_true, const float *f_true, float ls_decay,
                         int max_ls_iter, float *x_out, float *u_out, float *costs, float *old_costs,
                         float *alphas, float *objs, float *u_first, int32_t *n_ls_iter, int32_t *info,
                         dmpc_stream_t stream_) {
  if (T <= 1 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!Ks || !ks || !controls || !states || !u_lower || !u_upper || !C_true || !c_true || !F_true || !x_out ||
      !u_out || !costs || !alphas || !n_ls_iter)
    return DMPC_E_BADARG;
  if (!aligned16(C_true) || !aligned16(F_true)) return DMPC_E_BADARG;
  MpcFwdArgs fa{T, B, Ks, ks, controls, states, u_lower, u_upper, C_true, c_true, F_true, f_true, ls_decay,
                max_ls_iter, /*ls_cap=*/64, x_out, u_out, u_first, costs, old_costs, alphas, objs, n_ls_iter, info};
  const MpcSearchRoute r = mpc_search_route(search_call(nx, nu, fa));
  return r.code != 0 ? r.code : r.launch({fa, nx, nu}, static_cast<hipStream_t>(stream_));
}

int dmpc_mpc_forward_rec_pendulum(int T, int B, const float *Ks, const float *ks, const float *controls,
                                  const float *states, const float *u_lower, const float *u_upper,
                                  const float *C_true, const float *c_true, float g, float m, float l, float dt,
                                  float max_torque, float ls_decay, int max_ls_iter, float *x_out, float *u_out,
                                  float *costs, float *old_costs, float *alphas, float *objs, float *u_first,
                                  int32_t *n_ls_iter, int32_t *info, dmpc_stream_t stream_) {
  if (T <= 1 || B <= 0) return DMPC_E_BADARG;
  if (!Ks || !ks || !controls || !states || !u_lower || !u_upper || !C_true || !c_true || !x_out || !u_out || !costs ||
      !alphas || !n_ls_iter)
    return DMPC_E_BADARG;
  if (!aligned16(C_true)) return DMPC_E_BADARG;
  MpcFwdArgs fa{T, B, Ks, ks, controls, states, u_lower, u_upper, C_true, c_true, nullptr, nullptr, ls_decay,
                max_ls_iter, /*ls_cap=*/64, x_out, u_out, u_first, costs, old_costs, alphas, objs, n_ls_iter, info,
                /*dyn_kind=*/1, g, m, l, dt, max_torque};
  const MpcSearchRoute r = mpc_search_route(search_call(3, 1, fa));
  return r.code != 0 ? r.code : r.launch({fa, 3, 1}, static_cast<hipStream_t>(stream_));
}

int dmpc_pendulum_rollout_linearize(int T, int B, const float *x_init, const float *u, float g, float m, float l,
                                    float dt, float max_torque, int clamp_grad_closed, float *x_out, float *F_out,
                                    float *f_out, dmpc_stream_t stream_) {
  if (T <= 0 || B <= 0 || !x_init || !u || !x_out) return DMPC_E_BADARG;
  if (f_out != nullptr && F_out == nullptr) return DMPC_E_BADARG;
  PendulumArgs pa{T, B, x_init, u, g, m, l, dt, max_torque, clamp_grad_closed, x_out, F_out, f_out};
  launch_pendulum_rollout(pa, static_cast<hipStream_t>(stream_));
  return (int)hipGetLastError();
}

size_t dmpc_mpc_step_workspace_bytes(int T, int B, int nx, int nu) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return 0;
  return mpc_layout(T, B, nx, nu).total;
}

int dmpc_mpc_step_forward(int T, int B, int nx, int nu, const float *C_hat, const float *c_hat,
                          const float *F_hat, const float *f_hat, const float *controls, const float *states,
                          const float *u_lower, const float *u_upper, const float *C_true, const float *c_true,
                          const float *F_true, const float *f_true, int need_expand, float ls_decay,
                          int max_ls_iter, int n_qp_iter_max, int batch_coupled, float *x_out, float *u_out,
                          float *Ks_out, float *ks_out, float *costs, float *old_costs, float *alphas, float *objs,
                          float *u_first, int32_t *n_qp_iter, int32_t *n_ls_iter, void *ws, size_t ws_bytes,
                          int32_t *info, dmpc_stream_t stream_) {
  if (T <= 1 || B <= 0 || nx <= 0 || nu <= 0 || n_qp_iter_max <= 0) return DMPC_E_BADARG;
  if (batch_coupled && n_qp_iter_max > kSyncQpIterMax) return DMPC_E_UNSUPPORTED;
  if (!C_hat || !c_hat || !F_hat || !controls || !states || !u_lower || !u_upper || !C_true || !c_true || !F_true ||
      !x_out || !u_out || !Ks_out || !ks_out || !costs || !alphas || !n_qp_iter || !n_ls_iter || !ws)
    return DMPC_E_BADARG;
  if (!aligned16(C_hat) || !aligned16(c_hat) || !aligned16(F_hat) || !aligned16(f_hat) || !aligned16(C_true) ||
      !aligned16(F_true))
    return DMPC_E_BADARG;
  const MpcWs w = mpc_layout(T, B, nx, nu);
  if (ws_bytes < w.total) return DMPC_E_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char *base = static_cast<char *>(ws);
  // Taylor re-centring (c_hat <- C [x;u] + c, f_hat <- None, mpc_step.py:305-317) happens inside the backward sweep
  const float *c_use = c_hat;
  const float *f_use = need_expand ? nullptr : f_hat;
  MpcBackArgs ba{T, B, C_hat, c_use, F_hat, f_use, controls, u_lower, u_upper, n_qp_iter_max, Ks_out, ks_out,
                 n_qp_iter, info, nullptr, batch_coupled ? reinterpret_cast<unsigned *>(base + w.sync) : nullptr,
                 need_expand ? states : nullptr};
  MpcFwdArgs fa{T, B, Ks_out, ks_out, controls, states, u_lower, u_upper, C_true, c_true, F_true, f_true, ls_decay,
                max_ls_iter, /*ls_cap=*/64, x_out, u_out, u_first, costs, old_costs, alphas, objs, n_ls_iter, info};
  // both halves are asked before anything is launched (the workspace holds a tiled scratch for whoever reads one)
  const MpcSweepRoute sweep = mpc_sweep_route(sweep_call(nx, nu, ba, false, true));
  if (sweep.code != 0) return sweep.code;
  const MpcSearchRoute search = mpc_search_route(search_call(nx, nu, fa));
  if (search.code != 0) return search.code;
  if (sweep.needs_scratch) ba.tiled_scratch = reinterpret_cast<float *>(base + w.tiled);
  if (const MpcStepLauncher fused = fused_step(sweep, search)) return fused(ba, fa, stream);
  const int rc = run_sweep(sweep, nx, nu, ba, stream);
  return rc != 0 ? rc : search.launch({fa, nx, nu}, stream);
}

int dmpc_lin_rollout(int T, int B, int nx, int nu, const float *x_init, const float *u, const float *F,
                     const float *f, float *x_out, dmpc_stream_t stream_) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0 || !x_init || !u || !x_out || (T > 1 && !F)) return DMPC_E_BADARG;
  DMPC_LAUNCH_GGL(lin_rollout_kernel, dim3((B + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream_), T, B, nx,
                     nu, x_init, u, F, f, x_out, nullptr, ChainClear{});
  return (int)hipGetLastError();
}

int dmpc_mpc_step_status(int B, const int32_t *info, const int32_t *n_qp_iter, const float *alphas, int32_t *status,
                         dmpc_stream_t stream_) {
  if (B <= 0 || !status) return DMPC_E_BADARG;
  // (not noted as "the kernel this thread launched last": dmpc_last_kernel_name() keeps naming the step's own kernel)
  hipLaunchKernelGGL(mpc_step_status_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream_), B, info, n_qp_iter, alphas,
                     status);
  return (int)hipGetLastError();
}

size_t dmpc_box_ddp_workspace_bytes(int T, int B, int nx, int nu) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return 0;
  return ddp_layout(T, B, nx, nu).total;
}

}  // extern "C"

namespace dmpc {

// The chain of dmpc_box_ddp (include/dmpc.h) and dmpc_box_ddp_mlp_cost (include/dmpc_mlp_cost.h): the arguments of the former with
// the stage cost as a descriptor.  With a QuadCost the checks, routes and launches are dmpc_box_ddp's own.  With an MlpCost
// (dyn_kind 0 only; its caller has checked the model) every iteration forms the Taylor model C_hat, c_hat at the nominal trajectory
// (mlp_cost_approx_kernel behind the rollout, or the previous search's epilogue), sweeps on it and searches on the network.
static int box_ddp_chain(int T, int B, int nx, int nu, const float *x_init, const DdpCost &cost, const float *F,
                         const float *f, int dyn_kind, const float *dyn_params, const float *u_init, const float *u_lower,
                         const float *u_upper, float eps, int not_improved_lim, float ls_decay, int max_ls_iter,
                         float best_cost_eps, int max_iter, int n_qp_iter_max, int scrambled_norm, int batch_coupled,
                         float *x_best, float *u_best, float *costs_best, float *du_norm_best, float *du_norm_last,
                         int32_t *state, void *ws, size_t ws_bytes, int32_t *info, dmpc_stream_t stream_) {
  if (T <= 1 || B <= 0 || nx <= 0 || nu <= 0 || max_iter <= 0 || n_qp_iter_max <= 0) return DMPC_E_BADARG;
  if (batch_coupled && n_qp_iter_max > kSyncQpIterMax) return DMPC_E_UNSUPPORTED;
  if (!x_init || (!cost.net && (!cost.C || !cost.c)) || !u_init || !u_lower || !u_upper || !x_best || !u_best || !costs_best ||
      !du_norm_best || !du_norm_last || !state || !ws)
    return DMPC_E_BADARG;
  if (dyn_kind == 0 && !F) return DMPC_E_BADARG;
  if (dyn_kind == 1 && (!dyn_params || nx != 3 || nu != 1)) return DMPC_E_BADARG;
  if (dyn_kind < 0 || dyn_kind > 2) return DMPC_E_UNSUPPORTED;
  // MlpDx: F is the packed weights, dyn_params = {n_hidden, act, residual, search_linearizes} on the host; n_hidden is the
  // code H1 | (H2 << 16) as an integral float (exact: it stays below 2^24)
  int mlp_hidden = 0, mlp_act = 0, mlp_residual = 0, mlp_search_lin = 0;
  if (dyn_kind == 2) {
    if (!F || f != nullptr || !dyn_params) return DMPC_E_BADARG;
    const float h = dyn_params[0], ac = dyn_params[1], res = dyn_params[2], sl = dyn_params[3];
    if (!(h >= 0.f) || h != floorf(h) || !(ac >= 0.f) || ac != floorf(ac)) return DMPC_E_BADARG;   // (a NaN fails `>=`)
    if ((res != 0.f && res != 1.f) || (sl != 0.f && sl != 1.f)) return DMPC_E_BADARG;
    mlp_hidden = h >= 16777216.f ? 0 : (int)h;   // (0: no size the kernels serve)
    mlp_act = ac > 1e6f ? 1000000 : (int)ac;
    mlp_residual = res != 0.f;
    mlp_search_lin = sl != 0.f;
    if (!dmpc_mlp_dx_supported(nx, nu, mlp_hidden, mlp_act) || batch_coupled) return DMPC_E_UNSUPPORTED;
    // (the limits of dmpc_mlp_rollout_linearize and dmpc_mpc_forward_rec_mlp)
    if ((size_t)T * B * (nx + nu) * (nx + nu) >= ((size_t)1 << 31)) return DMPC_E_UNSUPPORTED;
  }
  // (round 5: shapes that run on the tiled kernels - more than 8 controls / 64 columns - too: their matrices live in w.tiled)
  if ((size_t)T * B * (nx + nu) >= ((size_t)1 << 31)) return DMPC_E_UNSUPPORTED;  // 32-bit indices in the bookkeeping
  if (!aligned16(cost.C) || !aligned16(cost.c) || !aligned16(F) || !aligned16(f) || !aligned16(ws)) return DMPC_E_BADARG;
  const DdpWs w = ddp_layout(T, B, nx, nu);
  const DdpCostWs wc = cost.net ? ddp_cost_layout(T, B, nx, nu) : DdpCostWs{0, 0, w.total};
  if (ws_bytes < wc.total) return DMPC_E_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char *base = static_cast<char *>(ws);
  // MlpCost: the Taylor model at the nominal trajectory is what the sweep reads as C, c (the search reads neither)
  float *C_hat = cost.net ? reinterpret_cast<float *>(base + wc.C_hat) : nullptr;
  float *c_hat = cost.net ? reinterpret_cast<float *>(base + wc.c_hat) : nullptr;
  const float *C = cost.net ? C_hat : cost.C, *c = cost.net ? c_hat : cost.c;
  // ... and the search can store the next one while it stores the trajectory (search_approximates): the rollout and the
  // Taylor model's launch then run for the first iteration only
  const bool cost_lin = cost.net && cost.search_approximates;
  auto fp = [&](size_t off) { return reinterpret_cast<float *>(base + off); };
  auto ip = [&](size_t off) { return reinterpret_cast<int32_t *>(base + off); };
  float *xs = fp(w.xs), *c_back = fp(w.c_back), *Ks = fp(w.Ks), *ks = fp(w.ks), *x_new = fp(w.x_new);
  float *u_buf[2] = {fp(w.u_a), fp(w.u_b)};
  float *u1 = fp(w.u1), *costs = fp(w.costs), *alphas = fp(w.alphas);
  unsigned *sel_sync = reinterpret_cast<unsigned *>(base + w.sel_sync);
  const float *F_hat = dyn_kind == 0 ? F : fp(w.F);
  const float pg = dyn_kind == 1 ? dyn_params[0] : 0.f, pm = dyn_kind == 1 ? dyn_params[1] : 0.f,
              pl = dyn_kind == 1 ? dyn_params[2] : 0.f, pdt = dyn_kind == 1 ? dyn_params[3] : 0.f,
              pmax = dyn_kind == 1 ? dyn_params[4] : 0.f;
  const int pclosed = dyn_kind == 1 ? (dyn_params[5] != 0.f) : 0;
  const size_t rows = (size_t)T * B;
  // loop state, the bookkeeping workgroups' meeting words and the flags are cleared by the chain's first launch
  ChainClear clear;
  clear.p[0] = state; clear.n[0] = 8;
  clear.p[1] = ip(w.sel_sync); clear.n[1] = 4;
  clear.p[2] = info; clear.n[2] = info != nullptr ? B : 0;
  const int32_t *done = state + kDdpDone;
  // Pendulum: the trajectory the line search accepts IS the next iteration's nominal one, and the search writes its
  // linearisation and re-centred cost while it writes the trajectory - the rollout + linearisation kernel runs for
  // the first iteration only, the nominal states ping-pong between the two state buffers.
  const bool fuse_lin = dyn_kind == 1 && !knob_on<Knob::DMPC_NO_SPEC_LS>();
  // MlpDx: the same, on request (search_linearizes) - the search's epilogue stores the accepted trajectory's Jacobians
  // through the rollout kernel's own two functions, so both settings return the same bits.  The re-centring stays the sweep's.
  const bool mlp = dyn_kind == 2, mlp_lin = mlp && mlp_search_lin != 0;
  const MlpModel mlp_model = mlp ? mlp_model_packed(nx, nu, mlp_hidden, mlp_residual, F) : MlpModel{};
  const bool ping_pong = fuse_lin || mlp_lin || cost_lin;   // the nominal states alternate between the two state buffers
  float *x_buf[2] = {xs, x_new};
  const bool copy_here = B <= kDdpCopyHereMaxB && rows * (size_t)(nx + nu) <= kDdpCopyHereMaxElems;
  // MPCstep.forward with need_expand: f_hat = None                                        mpc_step.py:305-328
  // pendulum: c_back was re-centred by the rollout kernel / the previous line search; LinDx: the backward sweep
  // re-centres c itself
  auto back_args = [&](const float *u_cur, const float *xs_it) {
    return MpcBackArgs{T, B, C, dyn_kind == 1 ? c_back : c, F_hat, nullptr, u_cur, u_lower, u_upper, n_qp_iter_max, Ks, ks,
                       ip(w.nqp), info, done, batch_coupled ? reinterpret_cast<unsigned *>(base + w.sync) : nullptr,
                       dyn_kind == 1 ? nullptr : xs_it, 0};
  };
  bool fused_select = false;   // the bookkeeping of iteration i rides in sweep i + 1's launch
  auto fwd_args = [&](const float *u_cur, float *xs_it, float *xn_it, float *u_new, float *u1_it, float *costs_it) {
    return MpcFwdArgs{T, B, Ks, ks, u_cur, xs_it, u_lower, u_upper, C, c, dyn_kind == 0 ? F : nullptr,
                      dyn_kind == 0 ? f : nullptr, ls_decay, max_ls_iter, /*ls_cap=*/64, xn_it, u_new, u1_it, costs_it,
                      /*old_costs: nobody reads them here*/ nullptr,
                      alphas, nullptr, ip(w.nls), info, dyn_kind, pg, pm, pl, pdt, pmax, pclosed, done,
                      fuse_lin || mlp_lin ? fp(w.F) : nullptr, fuse_lin ? fp(w.f) : nullptr, fuse_lin ? c_back : nullptr, 0,
                      fused_select && info != nullptr ? ip(w.info_back) : nullptr};
  };
  // Every route the chain takes, asked before its first launch: [0] the first iteration, which reads the caller's controls in
  // place, [1] the later ones, whose controls are the workspace's.  The bookkeeping rides along (fused_select) when the first
  // sweep goes through the ring - the pendulum's fused chain alone.
  MpcSweepRoute sweep[2];
  MpcSearchRoute search[2];
  sweep[0] = mpc_sweep_route(sweep_call(nx, nu, back_args(u_init, xs), false, true));
  fused_select = fuse_lin && copy_here && (sweep[0].kind == MpcKernel::kStream || sweep[0].kind == MpcKernel::kRing);
  sweep[1] = mpc_sweep_route(sweep_call(nx, nu, back_args(u_buf[1], x_new), fused_select, true));
  // (MlpDx: the network's search is no row of mpc_search_route - it is this chain's branch on dyn_kind, checked above)
  const bool net_search = mlp || cost.net;   // (MlpCost: likewise, its search is this chain's branch on the cost)
  search[0] = net_search ? MpcSearchRoute{0} : mpc_search_route(search_call(nx, nu, fwd_args(u_init, xs, x_new, u_buf[1], u1, costs)));
  search[1] = net_search ? MpcSearchRoute{0} : mpc_search_route(search_call(nx, nu, fwd_args(u_buf[1], x_new, xs, u_buf[0], u1, costs)));
  for (const int code : {sweep[0].code, search[0].code, sweep[1].code, search[1].code})
    if (code != 0) return code;
  DdpSelectArgs sa{};
  // One launch per iteration (box_ddp_pendulum_iter_kernel) when the fused chain runs on the generated sweep and the search is
  // the wavefront-per-trajectory one: the search then runs BESIDE the previous iteration's bookkeeping, so what that reads (the controls the
  // step started from, the first pass's controls, the costs) must not be what this search writes - three control buffers in
  // rotation, two of u_first / costs, and the iteration's flags through a staging word that the bookkeeping merges.
  // The first of these launches also rolls out and linearises the nominal trajectory (the chain's first launch otherwise).
  // DMPC_NO_DDP_ITER_FUSED=1 (read at every call): rollout, sweep and search as launches of their own (A/B timing; bit-identical).
  const bool iter_fused = fuse_lin && copy_here && sweep[0].kind == MpcKernel::kStream && search[0].kind == MpcKernel::kSpec4 &&
                          aligned16(fp(w.F)) && !knob_on_now<Knob::DMPC_NO_DDP_ITER_FUSED>();
  float *u_buf3[3] = {fp(w.u_a), fp(w.u_b), fp(w.u_c)};
  float *u1_2[2] = {u1, fp(w.u1_b)}, *costs_2[2] = {costs, fp(w.costs_b)};
  int32_t *stage_2[2] = {ip(w.stage_a), ip(w.stage_b)};
  for (int it = 0; it < max_iter; ++it) {
    // (iteration 0 names the same buffers in both rotations: the choice is made inside it)
    const float *u_cur = it == 0 ? u_init : (iter_fused ? u_buf3[it % 3] : u_buf[it & 1]);   // the first iteration reads the caller's controls in place
    float *u_new = iter_fused ? u_buf3[(it + 1) % 3] : u_buf[(it & 1) ^ 1];
    float *u1_it = iter_fused ? u1_2[it & 1] : u1, *costs_it = iter_fused ? costs_2[it & 1] : costs;
    float *xs_it = ping_pong ? x_buf[it & 1] : xs;
    float *xn_it = ping_pong ? x_buf[(it & 1) ^ 1] : x_new;
    const int k = it == 0 ? 0 : 1;
    // nominal trajectory and the Taylor models around it                                    box_ddp.py:123-171
    PendulumArgs pa_first{};     // one-launch iterations: the first iteration's launch rolls out and linearises itself (pa_first.T > 0)
    if (dyn_kind == 1) {
      if (it == 0 || !fuse_lin) {
        PendulumArgs pa{T, B, x_init, u_cur, pg, pm, pl, pdt, pmax, pclosed, xs_it, fp(w.F), fp(w.f), it == 0 ? nullptr : done, C, c,
                        c_back, it == 0 ? clear : ChainClear{}};
        if (iter_fused) pa_first = pa;
        else launch_pendulum_rollout(pa, stream);
      }
    } else if (mlp) {
      // f is not formed: with need_expand the step drops f_hat                               mpc_step.py:305-328
      if (it == 0 || !mlp_lin) {
        MlpRolloutArgs ra{T, B, mlp_model, x_init, u_cur, xs_it, fp(w.F), nullptr, it == 0 ? nullptr : done,
                          it == 0 ? clear : ChainClear{}};
        launch_mlp_rollout(ra, mlp_act, stream);
      }
    } else if (it == 0 || !cost_lin) {
      DMPC_LAUNCH_GGL(lin_rollout_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, T, B, nx, nu, x_init, u_cur, F,
                         f, xs_it, it == 0 ? nullptr : done, it == 0 ? clear : ChainClear{});
      if (cost.net) {   // (never the chain's first launch: nothing to clear)
        const MlpCostApproxArgs ca{(long long)rows, cost.m, xs_it, u_cur, C_hat, c_hat, nullptr, it == 0 ? nullptr : done,
                                   ChainClear{}};
        launch_mlp_cost_approx(ca, cost.act, stream);
      }
    }
    MpcBackArgs ba = back_args(u_cur, xs_it);
    if (sweep[k].needs_scratch) ba.tiled_scratch = fp(w.tiled);
    if (fused_select && info != nullptr) {   // the sweep may run ahead of `done`: its flags count only if the search follows
      ba.info = ip(w.info_back);
      ba.info_store = 1;
    }
    MpcFwdArgs fa = fwd_args(u_cur, xs_it, xn_it, u_new, u1_it, costs_it);
    int rc;
    if (iter_fused) {
      if (info != nullptr) {     // the search may run ahead of `done` too: sweep + search flags to this iteration's staging word
        fa.info = stage_2[it & 1];
        fa.info_store = 1;
      }
      if (it == 0) ba.done = fa.done = nullptr;   // (this launch clears the flag; nothing can have stopped the loop yet)
      const int n_sel = it > 0 ? select_parts(B) : 0;
      const size_t lds = std::max(mpc_asm_lds_bytes<3, 1>(), Spec4Layout::lds_bytes(T));
      DMPC_LAUNCH_GGL(box_ddp_pendulum_iter_kernel, dim3(B / 4 + n_sel), dim3(256), lds, stream, ba, fa, sa, n_sel, sel_sync,
                      pa_first);
      rc = (int)hipGetLastError();
      if (rc != 0) return rc;
    } else {
      rc = run_sweep(sweep[k], nx, nu, ba, stream, fused_select && it > 0 ? &sa : nullptr, sel_sync);
      if (rc != 0) return rc;
      if (mlp) {
        launch_mlp_search(fa, mlp_model, mlp_act, stream);
        rc = (int)hipGetLastError();
      } else if (cost.net) {
        launch_mlp_cost_search(fa, cost.m, cost.act, cost_lin ? C_hat : nullptr, cost_lin ? c_hat : nullptr, stream);
        rc = (int)hipGetLastError();
      } else {
        rc = search[k].launch({fa, nx, nu}, stream);
      }
      if (rc != 0) return rc;
    }
    // best-so-far update and stop tests of this iteration                                   box_ddp.py:200-230
    sa = DdpSelectArgs{it, T, B, nx, nu, max_iter, not_improved_lim, scrambled_norm, eps, best_cost_eps, u_cur, u1_it, costs_it,
                       costs_best, du_norm_best, du_norm_last, ip(w.keep), state, copy_here ? 1 : 0, xn_it, u_new,
                       x_best, u_best};
    if (iter_fused && info != nullptr) {
      sa.info_stage = stage_2[it & 1];
      sa.info = info;
    }
    if (fused_select) continue;   // rides in the next sweep's launch (the last one: in the summary launch)
    if (nx == 3 && nu == 1)
      DMPC_LAUNCH_GGL((box_ddp_select_kernel<3, 1>), dim3(1), dim3(kDdpSelectThreads), 0, stream, sa);
    else
      DMPC_LAUNCH_GGL((box_ddp_select_kernel<0, 0>), dim3(1), dim3(kDdpSelectThreads), 0, stream, sa);
    if (!copy_here)
      DMPC_LAUNCH_GGL(box_ddp_keep_kernel, dim3(grid_for(rows * nx)), dim3(256), 0, stream, T, B, nx, nu,
                         ip(w.keep), xn_it, u_new, x_best, u_best);
  }
  // fused chain: the last iteration's bookkeeping - with the summary when one workgroup does it, else as the fused
  // launch splits it
  const bool split_last = fused_select && select_parts(B) > 1;
  if (split_last)
    DMPC_LAUNCH_GGL((box_ddp_select_parts_kernel<3, 1>), dim3(select_parts(B)), dim3(256), 0, stream, sa, sel_sync);
  DMPC_LAUNCH_GGL(box_ddp_summary_kernel, dim3(1), dim3(1024), 0, stream, rows * nu, B, u_init, u_lower, u_upper, info,
                     (int)DMPC_INFO_NONFINITE, du_norm_best, eps, state, sa, fused_select && !split_last ? 1 : 0);
  return (int)hipGetLastError();
}

}  // namespace dmpc

extern "C" {

int dmpc_box_ddp(int T, int B, int nx, int nu, const float *x_init, const float *C, const float *c, const float *F,
                 const float *f, int dyn_kind, const float *dyn_params, const float *u_init, const float *u_lower,
                 const float *u_upper, float eps, int not_improved_lim, float ls_decay, int max_ls_iter,
                 float best_cost_eps, int max_iter, int n_qp_iter_max, int scrambled_norm, int batch_coupled,
                 float *x_best, float *u_best, float *costs_best, float *du_norm_best, float *du_norm_last,
                 int32_t *state, void *ws, size_t ws_bytes, int32_t *info, dmpc_stream_t stream) {
  DdpCost cost;
  cost.C = C;
  cost.c = c;
  return box_ddp_chain(T, B, nx, nu, x_init, cost, F, f, dyn_kind, dyn_params, u_init, u_lower, u_upper, eps, not_improved_lim,
                       ls_decay, max_ls_iter, best_cost_eps, max_iter, n_qp_iter_max, scrambled_norm, batch_coupled, x_best, u_best,
                       costs_best, du_norm_best, du_norm_last, state, ws, ws_bytes, info, stream);
}

size_t dmpc_box_ddp_mlp_cost_workspace_bytes(int T, int B, int nx, int nu) {
  if (T <= 0 || B <= 0 || nx <= 0 || nu <= 0) return 0;
  return ddp_cost_layout(T, B, nx, nu).total;
}

int dmpc_box_ddp_mlp_cost(int T, int B, int nx, int nu, const float *x_init, const float *cost_packed, int n_hidden, int act,
                          int search_approximates, const float *F, const float *f, int dyn_kind, const float *dyn_params,
                          const float *u_init, const float *u_lower, const float *u_upper, float eps, int not_improved_lim,
                          float ls_decay, int max_ls_iter, float best_cost_eps, int max_iter, int n_qp_iter_max,
                          int scrambled_norm, int batch_coupled, float *x_best, float *u_best, float *costs_best,
                          float *du_norm_best, float *du_norm_last, int32_t *state, void *ws, size_t ws_bytes, int32_t *info,
                          dmpc_stream_t stream) {
  if (T <= 1 || B <= 0 || nx <= 0 || nu <= 0 || n_hidden <= 0 || max_iter <= 0 || n_qp_iter_max <= 0) return DMPC_E_BADARG;
  if (!cost_packed || !aligned16(cost_packed) || !F) return DMPC_E_BADARG;
  if (search_approximates != 0 && search_approximates != 1) return DMPC_E_BADARG;
  // dyn_kind 1, 2 (the pendulum, an MlpDx) are reserved: their searches would have to evaluate this cost
  if (dyn_kind != 0 || batch_coupled != 0) return DMPC_E_UNSUPPORTED;
  if (!dmpc_mlp_cost_supported(nx, nu, n_hidden, act)) return DMPC_E_UNSUPPORTED;
  // (the limit of dmpc_mlp_cost_approx)
  if ((size_t)T * B * (nx + nu) * (nx + nu) >= ((size_t)1 << 31)) return DMPC_E_UNSUPPORTED;
  DdpCost cost;
  cost.net = true;
  cost.m = mlp_cost_model_packed(nx, nu, n_hidden, cost_packed);
  cost.act = act;
  cost.search_approximates = search_approximates != 0;
  return box_ddp_chain(T, B, nx, nu, x_init, cost, F, f, dyn_kind, dyn_params, u_init, u_lower, u_upper, eps, not_improved_lim,
                       ls_decay, max_ls_iter, best_cost_eps, max_iter, n_qp_iter_max, scrambled_norm, batch_coupled, x_best, u_best,
                       costs_best, du_norm_best, du_norm_last, state, ws, ws_bytes, info, stream);
}

int dmpc_mpc_step_backward(int T, int B, int nx, int nu, const float *C_hat, const float *c_hat,
                           const float *F_hat, const float *x, const float *u, const float *u_lower,
                           const float *u_upper, const float *grad_x, const float *grad_u, float *d_x_init,
                           float *dC, float *dc, float *dF, float *df, float *dC_sum, float *dc_sum,
                           const float *detach_norm, const int32_t *detach_flag, float detach_eps, void *ws,
                           size_t ws_bytes, int32_t *info, dmpc_stream_t stream_) {
  if (T <= 1 || B <= 0 || nx <= 0 || nu <= 0) return DMPC_E_BADARG;
  if (!C_hat || !c_hat || !F_hat || !x || !u || !u_lower || !u_upper || !d_x_init || !ws) return DMPC_E_BADARG;
  if ((dC_sum == nullptr) != (dc_sum == nullptr) || (dc == nullptr && dc_sum == nullptr)) return DMPC_E_BADARG;
  // the sums are formed by the LDS-DMA co-state kernel only (whole wavefronts of four trajectories, 16-lane shapes, 16-byte
  // aligned arrays - the workspace's own are aligned by construction)
  const bool al = aligned16(x) && aligned16(u) && aligned16(C_hat) && aligned16(c_hat) && aligned16(F_hat) && aligned16(dC) &&
                  aligned16(dF);
  if (dC_sum != nullptr && !costate_sums_available(T, B, nx, nu, al)) return DMPC_E_UNSUPPORTED;   // (nothing launched)
  if (!aligned16(C_hat) || !aligned16(c_hat) || !aligned16(F_hat) || !aligned16(dC) || !aligned16(dF))
    return DMPC_E_BADARG;
  const MpcWs w = mpc_layout(T, B, nx, nu);
  if (ws_bytes < w.total) return DMPC_E_WORKSPACE;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char *base = static_cast<char *>(ws);
  float *neg = reinterpret_cast<float *>(base + w.neg);
  float *x0 = reinterpret_cast<float *>(base + w.x0);
  float *dx = reinterpret_cast<float *>(base + w.dx);
  float *du = reinterpret_cast<float *>(base + w.du);
  uint8_t *mask = reinterpret_cast<uint8_t *>(base + w.mask);
  launch_active_mask(T, B, nx, nu, u, u_lower, u_upper, grad_x, grad_u, mask, neg, x0, dC_sum, dc_sum, detach_norm, detach_flag,
                     detach_eps, stream);
  // LQR_active(0, C, -d_tau, F, None, u_zero_Index=active)                               mpc_step.py:374-376
  int rc = dmpc_lqr_solve(T, B, nx, nu, C_hat, neg, F_hat, nullptr, x0, mask, nullptr, nullptr, dx, du,
                          base + w.lqr, w.total - w.lqr, info, stream_);
  if (rc != 0) return rc;
  // d_lambda_t = C_xx dx + C_xu du - d_tau[:nx] + ...  ->  r = neg, r_sign = +1; outputs negated  :383-446
  CostateArgs a{T, B, C_hat, c_hat, F_hat, x, u, dx, du, neg, 1.0f, -1.0f, /*dC_mode=*/1, /*df_shift=*/1,
                d_x_init, dC, dc, dF, df};
  a.dC_sum = dC_sum;
  a.dc_sum = dc_sum;
  return launch_costate(nx, nu, a, stream);
}

}  // extern "C"
