// libuglad_hip.so -- kernels and C ABI of the unrolled GLAD hot path for gfx950.  See include/uglad_hip.h.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>

#include "../../include/uglad_hip.h"
#include "glad_device.h"
#include "tridiag.h"
#include "eig_lean.h"
#include "tridiag_wave.h"
#include "chol.h"
#include "cell_fwd.h"

namespace uglad {

// =============================================================================================== cell backward
// Replaces autograd through glad.py:139-144, torch_sqrtm.py:32-46, glad_params.py:61-81.
// The rhoNN / threshold backward (the expensive entrywise part) works on the upper triangle dealt out evenly over the threads,
// as in the forward epilogue; the thread that differentiates the threshold at (i,j) keeps the direct term dL/dZ_ij in a
// register and adds (G_B)_ij, which comes back through LDS from the last GEMM, at the very end.  Symmetric products
// (C = U^T G U, G_B) are formed on the 10 upper tiles only; the result leaves through LDS with coalesced stores.
#define UGLAD_CELL_BWD_NAME cell_bwd_kernel
#define UGLAD_CELL_BWD_GS 0
#include "cell_bwd.h"
#undef UGLAD_CELL_BWD_NAME
#undef UGLAD_CELL_BWD_GS
#define UGLAD_CELL_BWD_NAME cell_bwd_gs_kernel
#define UGLAD_CELL_BWD_GS 1
#include "cell_bwd.h"
#undef UGLAD_CELL_BWD_NAME
#undef UGLAD_CELL_BWD_GS

}  // namespace uglad

// the many-workgroup kernels: none templated on NT
#ifndef UGLAD_TU_NT
#include "wide_bwd.h"
#include "wide_fwd.h"
#include "wide_ns.h"
#include "ldl_wide.h"
#include "chol_wide.h"
#include "cov_wide.h"
#include "assoc_wide.h"
#include "rank_wide.h"
#include "pairwise_wide.h"
#include "wcov_wide.h"
#include "after_wide.h"
#include "score_wide.h"
#include "sort_wide.h"
#include "metrics_wide.h"
#include "graph_wide.h"
#include "eigvals_wide.h"
#include "corr_wide.h"
#endif
#include "theta0.h"
#include "loss.h"
#include "reduce.h"
#include "after_path.h"

namespace uglad {

// ---- one translation unit per NT (the build of __graft_entry__.py): compiled with -DUGLAD_TU_NT=k this file emits ONLY the
// kernels templated on NT = k (explicit instantiations; the C ABI below is skipped), compiled with -DUGLAD_TU_HOST it emits
// everything else and merely declares those instantiations.  The units compile in parallel and link into one library.
// Without either macro (emulator and sanitizer builds) the file is one self-contained unit as before.
// The lists name specialisations only; decltype supplies the signature, so a kernel's parameter list is written once, at its definition.
#define UGLAD_EMIT(...) template __global__ decltype(__VA_ARGS__) __VA_ARGS__;
#define UGLAD_DECLARE(...) extern template __global__ decltype(__VA_ARGS__) __VA_ARGS__;
#define UGLAD_KERNELS_EVERY_NT(X, NT)                                                                                         \
  X(tridiag_kernel<NT, kThreads>) X(cell_bwd_kernel<NT>) X(init_inverse_kernel<NT>) X(init_bwd_kernel<NT>) X(loss_fwd_kernel<NT>) \
  X(cov_kernel<NT>) X(map_solve_kernel<NT>) X(support_metrics_kernel<NT>) X(symeig_lean_kernel<NT>) X(cell_fwd_lean_kernel<NT>)
// the dL/dS variants (uglad_glad_backward_wrt_s) in translation units of their own (-DUGLAD_TU_GS): instantiated next to the kernels above
// they changed how the compiler treated cell_bwd_kernel<3> (80 instead of 78 SGPR spills, scripts/kernel_meta.py)
#define UGLAD_KERNELS_GS(X, NT) X(cell_bwd_gs_kernel<NT>) X(init_bwd_gs_kernel<NT>)
#define UGLAD_KERNELS_NT_LE4(X, NT) X(symeig_jacobi_kernel<NT>) X(chol_init_kernel<NT>) X(chol_loss_kernel<NT>)
// D <= 96: the tridiagonalisation with 16 column groups as at D = 128 (128 NT threads) instead of 512 threads -- with 512 the chain wave gathers
// 512 / (DP / 4) partial sums per row, 64 at DP = 32, most of them zeros (profiles/r04_tridiag_small.txt)
#define UGLAD_KERNELS_NT_LE3(X, NT) X(tridiag_kernel<NT, 128 * NT>)
// D <= 32: one wave per matrix, the matrix in its registers (tridiag_wave.h)
#define UGLAD_KERNELS_NT_EQ1(X, NT) X(tridiag_wave_kernel<NT>)
#define UGLAD_KERNELS_NT_GE5(X, NT) X(tridiag_kernel<NT, 1024>) X(cell_fwd_back_kernel<NT>)
#if defined(UGLAD_TU_NT) && defined(UGLAD_TU_ONLY)
// development (scripts/spill_check.sh): -DUGLAD_TU_ONLY='cell_fwd_lean_kernel<4>' emits that kernel alone, to read its register
// allocation in seconds (UGLAD_TU_ONLY2, UGLAD_TU_ONLY3: further kernels of the same family)
UGLAD_EMIT(UGLAD_TU_ONLY)
#ifdef UGLAD_TU_ONLY2
UGLAD_EMIT(UGLAD_TU_ONLY2)
#endif
#ifdef UGLAD_TU_ONLY3
UGLAD_EMIT(UGLAD_TU_ONLY3)
#endif
#elif defined(UGLAD_TU_NT) && defined(UGLAD_TU_GS)
UGLAD_KERNELS_GS(UGLAD_EMIT, UGLAD_TU_NT)
#elif defined(UGLAD_TU_NT)
UGLAD_KERNELS_EVERY_NT(UGLAD_EMIT, UGLAD_TU_NT)
#if UGLAD_TU_NT <= 4
UGLAD_KERNELS_NT_LE4(UGLAD_EMIT, UGLAD_TU_NT)
#if UGLAD_TU_NT <= 3
UGLAD_KERNELS_NT_LE3(UGLAD_EMIT, UGLAD_TU_NT)
#endif
#if UGLAD_TU_NT == 1
UGLAD_KERNELS_NT_EQ1(UGLAD_EMIT, UGLAD_TU_NT)
#endif
#else
UGLAD_KERNELS_NT_GE5(UGLAD_EMIT, UGLAD_TU_NT)
#endif
#elif defined(UGLAD_TU_HOST)
#define UGLAD_DECLARE_NT(NT) UGLAD_KERNELS_EVERY_NT(UGLAD_DECLARE, NT) UGLAD_KERNELS_GS(UGLAD_DECLARE, NT)
UGLAD_DECLARE_NT(1) UGLAD_DECLARE_NT(2) UGLAD_DECLARE_NT(3) UGLAD_DECLARE_NT(4)
UGLAD_KERNELS_NT_LE4(UGLAD_DECLARE, 1) UGLAD_KERNELS_NT_LE4(UGLAD_DECLARE, 2) UGLAD_KERNELS_NT_LE4(UGLAD_DECLARE, 3) UGLAD_KERNELS_NT_LE4(UGLAD_DECLARE, 4)
UGLAD_KERNELS_NT_LE3(UGLAD_DECLARE, 1) UGLAD_KERNELS_NT_LE3(UGLAD_DECLARE, 2) UGLAD_KERNELS_NT_LE3(UGLAD_DECLARE, 3)
UGLAD_KERNELS_NT_EQ1(UGLAD_DECLARE, 1)
UGLAD_DECLARE_NT(5) UGLAD_DECLARE_NT(6) UGLAD_DECLARE_NT(7) UGLAD_DECLARE_NT(8)
UGLAD_KERNELS_NT_GE5(UGLAD_DECLARE, 5) UGLAD_KERNELS_NT_GE5(UGLAD_DECLARE, 6) UGLAD_KERNELS_NT_GE5(UGLAD_DECLARE, 7) UGLAD_KERNELS_NT_GE5(UGLAD_DECLARE, 8)
#endif

}  // namespace uglad

#ifndef UGLAD_TU_NT
// =============================================================================================== the host layer (no device code)
#include "host_route.h"
#include "host_launch.h"
#include "host_api.h"
#include "host_rccl.h"
#include "host_extra.h"
#include "host_wide.h"
#endif  // !UGLAD_TU_NT
