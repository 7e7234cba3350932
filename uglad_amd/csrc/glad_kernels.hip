// libuglad_hip.so -- kernels and C ABI of the unrolled GLAD hot path for gfx950.  See include/uglad_hip.h.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>

#include "../../include/uglad_hip.h"
#include "glad_device.h"
#include "eig_dc.h"
#include "eig_lean.h"
#include "tridiag_wave.h"
#include "chol.h"

namespace uglad {

#ifdef UGLAD_STAMPS
__device__ unsigned long long g_cwg[4096][3];     // diagnostic build: per workgroup of the last lean cell_fwd: start, end, hardware id
__device__ unsigned long long g_lstamps[4][96];  // diagnostic build: solver phase stamps of workgroups 0..3 of the last lean cell_fwd
__device__ unsigned long long g_kstamps[32];  // diagnostic build: phase stamps of workgroup 0 of the last cell_fwd / cell_bwd
#define KSTAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_kstamps[i] = __builtin_amdgcn_s_memtime(); } while (0)
#elif defined(UGLAD_PHASE_EXIT)
#define KSTAMP(i) do { if (g_exit_at == 100 + (i)) __builtin_amdgcn_endpgm(); } while (0)
#else
#define KSTAMP(i) do {} while (0)
#endif

// Coalesced copy of the D x D matrix in LDS (row stride LD) to global memory: 16 bytes per lane and store where the rows allow it
// (D a multiple of 4 and an aligned destination), else 4.  The tail of such a copy is bound by the number of store
// instructions, not by bytes.
__device__ __forceinline__ void copy_out_matrix(float* __restrict__ dst, const float* __restrict__ src, int D, int LD) {
  const int tid = threadIdx.x;
  if (((D & 3) == 0) && ((reinterpret_cast<size_t>(dst) & 15) == 0)) {
    // (a half wave reads one row as 32 pieces of 16 bytes: stride 4 over the odd row stride, 8 banks hit four times.  Dealt out as
    // 4 rows x 8 pieces the reads are conflict-free, but a half wave's store is then four 128-byte segments instead of 512 contiguous
    // bytes and the forward cell as a whole 1.3 % slower on a same-box A/B: profiles/r03_lean_phase_counters.txt)
    const int D4 = D >> 2;
    for (int idx = tid; idx < D * D4; idx += kThreads) {
      const int i = idx / D4, j = 4 * (idx - i * D4);
      const float* p = src + i * LD + j;
      f4 v = {p[0], p[1], p[2], p[3]};
      *reinterpret_cast<f4*>(dst + (size_t)i * D + j) = v;
    }
  } else {
    const int si = kThreads / D, sj = kThreads - si * D;
    int i = tid / D, j = tid - i * D;
    for (int idx = tid; idx < D * D; idx += kThreads) {
      dst[idx] = src[i * LD + j];
      j += sj;
      i += si;
      if (j >= D) {
        j -= D;
        ++i;
      }
    }
  }
}

// =============================================================================================== cell forward, LDS-lean
// The same cell for D <= 128 on ONE LDS-resident matrix (eig_lean.h): ~75 KB of LDS and <= 128 registers, so two workgroups
// share a CU.  Q holds the eigenvectors, then theta_half, then Z: every hand-over is separated by a barrier.
// Tws: (M, NT, 32, 32) floats of the caller's workspace for the triangular factors of the back-transformation.
// With ONE matrix per group (a direct fit: M = 1) the workgroup is its whole batch, and the step that follows the cell -- the batch mean of
// ||Z - theta_half||^2 and LambdaNN, norm_lambda_kernel -- is done by its thread 0 right behind the norm: one launch and one hand-over less per
// unroll step (round 4: config 1's step is two latency chains and this 5 us kernel).  All null: the separate launch follows as before.
struct LamStep {
  float* nf_sum;       // (G)
  float* lam_next;     // (G)
  float* lam_in_next;  // (G, 2)
  float inv_m;
};
template <int NT>
__global__ __launch_bounds__(kThreads, NT <= 4 ? 4 : 2) void cell_fwd_lean_kernel(const float* __restrict__ S, const float* __restrict__ Zin,
                                                                    const float* __restrict__ lam_ptr,
                                                                    const float* __restrict__ params, float* __restrict__ Zout,
                                                                    float* __restrict__ half_out, float* __restrict__ U_out,
                                                                    float* __restrict__ beta_out,
                                                                    float* __restrict__ normF_partial,
                                                                    float* __restrict__ cond_max,
                                                                    const float* __restrict__ tri, float* __restrict__ Tws,
                                                                    int D, int mode, int gs, int split, LamStep ls) {
  constexpr int DP = NT * 32, LD = DP + 1;
  // the one big matrix: LDS up to D = 128; beyond, the first of the matrix's two workspace slabs (L2-resident) -- the same
  // code then runs on a global pointer, one workgroup per CU
  constexpr bool kGM = DP > 128;
  __shared__ __attribute__((aligned(16))) float sQ_lds[kGM ? 4 : DP * LD];
  float* sQ = kGM ? const_cast<float*>(tri) + (size_t)gridDim.x * kWsPerMatrix<DP> + (size_t)blockIdx.x * big_floats<DP>() : sQ_lds;
  __shared__ __attribute__((aligned(16))) LeanScratch<DP> ws;
  __shared__ float s_phi[DP], s_red[8];
  const size_t base = (size_t)blockIdx.x * D * D;
  const float* Sm = S + base;
  const float* Zm = Zin + base;
  const int grp = blockIdx.x / gs;
  params += (size_t)grp * kNParam;
  const float lam = lam_ptr[grp];
  KSTAMP(16);
#ifdef UGLAD_STAMPS
  const int tid0 = threadIdx.x;
#define tid tid0
  if (tid == 0 && blockIdx.x < 4096) {
    g_cwg[blockIdx.x][0] = __builtin_amdgcn_s_memrealtime();
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    g_cwg[blockIdx.x][2] = ((unsigned long long)xcc << 32) | hw;
  }
  if (tid < 96) ws.stamp[tid] = 0;
  __syncthreads();
  UGLAD_STAMP(ws, 0);
#undef tid
#endif
  if (kGM && split == 2) {
    // few large matrices: stop before the last merge of the divide & conquer; wide_fwd.h carries it out with many workgroups per
    // matrix and cell_fwd_back_kernel picks up from there
    symeig_lean_front<NT>(sQ, D, ws, tri + (size_t)blockIdx.x * 3 * DP, Tws + (size_t)blockIdx.x * NT * 1024);
    return;
  }
  symeig_lean<NT>(sQ, D, ws, tri + (size_t)blockIdx.x * 3 * DP, Zout + base, D, Tws + (size_t)blockIdx.x * NT * 1024);
  KSTAMP(17);
  // (shadow the ones above: nothing derived from the thread index stays live across the eigensolver, whose last merge needs every register)
  const int tid = opaque_v(threadIdx.x), lane = tid & 63, w = tid >> 6;
#ifdef UGLAD_STAMPS
  if (tid < 96 && blockIdx.x < 4) g_lstamps[blockIdx.x][tid] = ws.stamp[tid];
#endif
  // spectrum -> psi(beta) = phi(beta) + alpha beta of the shifted form theta_half = -alpha b + U diag(psi) U^T (glad_device.h)
  float alpha;
  __syncthreads();  // the scratch below aliases the solver's work area (the back-transformation ends with a barrier of its own unless there
                    // are no reflectors, D <= 2)
  {
    const float be = (tid < D) ? ws.d[tid] : 0.f;
    float cond;
    const float ps = shifted_spectrum(be, D, lam, mode, reinterpret_cast<double*>(ws.ds), alpha, cond);  // (the solver's scratch is free)
    if (tid < DP) s_phi[tid] = ps;
    if (cond_max && tid == 0) cond_max[blockIdx.x] = fmaxf(cond_max[blockIdx.x], cond);  // running maximum over the steps of a pass
    if (tid < D && beta_out) beta_out[(size_t)blockIdx.x * D + tid] = be;
  }
  if (U_out) copy_out_matrix(U_out + base, sQ, D, LD);  // the eigenvectors for the backward pass
  __syncthreads();
  KSTAMP(18);
  // U diag(psi) U^T on the upper tiles, psi applied to the A operand on its way into the MFMA
  using T = Tiles<NT, true>;
  f32x16 acc[T::kPerWave];
  {
    const int li = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int nn = 0; nn < T::kPerWave; ++nn) {
      const int t = w + kWaves * nn;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[nn][e] = 0.f;
      if (t < T::kCount) {
        int I, J;
        T::ij(t, I, J);
        const float* a = sQ + (I * 32 + li) * LD + kh;
        const float* b = sQ + (J * 32 + li) * LD + kh;
        float av[8], bv[8], pv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          av[u] = a[2 * u];
          bv[u] = b[2 * u];
          pv[u] = s_phi[2 * u + kh];
        }
        for (int k0 = 0; k0 < DP; k0 += 16) {
          const int kn = (k0 + 16 < DP) ? k0 + 16 : k0;
          float an[8], bn[8], pn[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            an[u] = a[kn + 2 * u];
            bn[u] = b[kn + 2 * u];
            pn[u] = s_phi[kn + 2 * u + kh];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) acc[nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u] * pv[u], bv[u], acc[nn], 0, 0, 0);
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            av[u] = an[u];
            bv[u] = bn[u];
            pv[u] = pn[u];
          }
        }
      }
    }
  }
  KSTAMP(19);
  // theta_half = -alpha b + (the product), b = S/lam - Z entry by entry with tridiag_kernel's rounding
  if (alpha != 0.f) {
    const float inv_lam = 1.0f / lam;
#pragma unroll
    for (int nn = 0; nn < T::kPerWave; ++nn) {
      const int t = w + kWaves * nn;
      if (t < T::kCount) {
        int I, J;
        T::ij(t, I, J);
        const int j = J * 32 + (lane & 31);
        float sv[16], zv[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = I * 32 + acc_row(e, lane);
          const bool in = i <= j && j < D;
          sv[e] = in ? Sm[i * D + j] : 0.f;
          zv[e] = in ? Zm[i * D + j] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nn][e] = fmaf(-alpha, fmaf(inv_lam, sv[e], -zv[e]), acc[nn][e]);
      }
    }
  }
  __syncthreads();  // every wave is done reading the eigenvectors
#pragma unroll
  for (int nn = 0; nn < T::kPerWave; ++nn) {  // theta_half, both triangles, into the same buffer
    const int t = w + kWaves * nn;
    if (t < T::kCount) {
      int I, J;
      T::ij(t, I, J);
      const int j = J * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = I * 32 + acc_row(e, lane);
        if (i <= j) {
          sQ[i * LD + j] = acc[nn][e];
          sQ[j * LD + i] = acc[nn][e];
        }
      }
    }
  }
  __syncthreads();
  KSTAMP(21);
  if (half_out) {  // (training) theta_half for the backward pass -- before Z overwrites it
    copy_out_matrix(half_out + base, sQ, D, LD);
    __syncthreads();
  }
  // rhoNN + soft threshold on the upper triangle dealt out evenly (rows p and D-1-p together hold D+1 of them): entry e = tid + kThreads q.  An entry
  // is read (from the upper triangle) only by the thread that then overwrites it and its mirror image with Z.
  constexpr int kMaxQ = ((DP / 2) * (DP + 1) + kThreads - 1) / kThreads;
  constexpr int kQ = kMaxQ < 6 ? kMaxQ : 6;
  const int D1 = D + 1, total = ((D + 1) / 2) * D1;
  const int sp = kThreads / D1, sc = kThreads - sp * D1;
  auto entry = [&](int e, int p, int c) -> int {
    if (e >= total) return -1;
    if (c < D - p) return (p << 16) | (p + c);
    const int i = D - 1 - p;
    return (i == p) ? -1 : ((i << 16) | (i + (c - (D - p))));
  };
  float nsum = 0.f;
  {
    int p = tid / D1, c = tid - p * D1;
    for (int q0 = 0; q0 < kMaxQ; q0 += kQ) {
      int pk[kQ];
      float xv[kQ], sv[kQ], zv[kQ], zn[kQ];
#pragma unroll
      for (int u = 0; u < kQ; ++u) {
        pk[u] = (q0 + u < kMaxQ) ? entry(tid + kThreads * (q0 + u), p, c) : -1;
        c += sc;
        p += sp;
        if (c >= D1) {
          c -= D1;
          ++p;
        }
        const int i = pk[u] >> 16, j = pk[u] & 0xffff;
        const bool in = pk[u] >= 0;
        sv[u] = in ? Sm[i * D + j] : 0.f;
        zv[u] = in ? Zm[i * D + j] : 0.f;
        xv[u] = in ? sQ[i * LD + j] : 0.f;
        zn[u] = 0.f;
      }
#pragma unroll
      for (int u = 0; u + 1 < kQ; u += 2) {  // two entries per pass on the packed pipe
        RhoAct2 act;
        rho_forward2(params, (v2f){xv[u], xv[u + 1]}, (v2f){sv[u], sv[u + 1]}, (v2f){zv[u], zv[u + 1]}, act);
        zn[u] = soft_threshold(xv[u], act.rho.x);
        zn[u + 1] = soft_threshold(xv[u + 1], act.rho.y);
      }
      if (kQ & 1) {
        RhoAct act;
        rho_forward(params, xv[kQ - 1], sv[kQ - 1], zv[kQ - 1], act);
        zn[kQ - 1] = soft_threshold(xv[kQ - 1], act.rho);
      }
#pragma unroll
      for (int u = 0; u < kQ; ++u) {
        if (pk[u] >= 0) {
          const int i = pk[u] >> 16, j = pk[u] & 0xffff;
          const float d = zn[u] - xv[u];
          nsum = fmaf((i == j) ? 1.f : 2.f, d * d, nsum);
          sQ[i * LD + j] = zn[u];
          sQ[j * LD + i] = zn[u];
        }
      }
    }
  }
  KSTAMP(22);
  nsum = block_sum(nsum, s_red);  // (its barriers also publish Z)
  if (tid == 0) {
    normF_partial[blockIdx.x] = nsum;
    if (ls.lam_next) {  // (gs = 1: this matrix is its group -- exactly norm_lambda_kernel's thread 0 on a sum of one term)
      ls.nf_sum[grp] = nsum;
      const float nrm = nsum * ls.inv_m;
      ls.lam_in_next[2 * grp] = nrm;
      ls.lam_in_next[2 * grp + 1] = lam;
      ls.lam_next[grp] = lambda_forward(params, nrm, lam);
    }
  }
  copy_out_matrix(Zout + base, sQ, D, LD);
  KSTAMP(20);
#ifdef UGLAD_STAMPS
  if (tid == 0 && blockIdx.x < 4096) g_cwg[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
#endif
}

// Few large matrices, third launch of the forward cell's eigen-decomposition: back-transformation of the merged eigenvectors (second
// slab of the matrix), beta and U out for the backward pass.  What follows (theta_half, rhoNN, norm) is wide_gemm_kernel's.
template <int NT>
__global__ __launch_bounds__(kThreads, 2) void cell_fwd_back_kernel(const float* __restrict__ tri, float* __restrict__ Tws,
                                                                    const float* __restrict__ R, float* __restrict__ U_out,
                                                                    float* __restrict__ beta_out, int D, int nm) {
  // grid (workgroups per matrix, matrices): wave w of workgroup blockIdx.x owns the 16-column strip kWaves blockIdx.x + w, kept in LDS
  constexpr int DP = NT * 32, LD = DP + 1;
  __shared__ __attribute__((aligned(16))) LeanScratch<DP> ws;
  __shared__ __attribute__((aligned(16))) float s_strips[kWaves * DP * 16];
  const int m = blockIdx.y, wg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float* Q = const_cast<float*>(tri) + (size_t)nm * kWsPerMatrix<DP> + (size_t)m * big_floats<DP>() + big_floats<DP>() / 2;
  const size_t base = (size_t)m * D * D;
  const float* tri_m = tri + (size_t)m * 3 * DP;
#ifdef UGLAD_STAMPS
  if (tid < 96) ws.stamp[tid] = 0;
  __syncthreads();
#endif
  back_transform_lean<NT>(Q, D, ws, R + base, D, tri_m + 2 * DP, Tws + (size_t)m * NT * 1024 + (size_t)wg * NT * 512, s_strips, wg);
  if (wg == 0 && beta_out && tid < D) beta_out[(size_t)m * D + tid] = tri_m[tid];
  const int strip = kWaves * wg + wv, l16 = lane & 15, g = lane >> 4;
  if (16 * strip < DP) {  // the strip back to the slab (theta_half reads it there) and out for the backward pass
    const float* sq = s_strips + (size_t)wv * DP * 16;
    const int col = 16 * strip + l16;
    for (int r0 = 0; r0 < DP; r0 += 4) {
      const int row = r0 + g;
      const float v = sq[row * 16 + l16];
      Q[row * LD + col] = v;
      if (U_out && row < D && col < D) U_out[base + (size_t)row * D + col] = v;
    }
  }
}

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

#ifndef UGLAD_TU_NT
}  // namespace uglad
#include "wide_bwd.h"
#include "wide_fwd.h"
#include "wide_ns.h"
namespace uglad {
#endif

// =============================================================================================== Theta_0 and its gradient
// One Newton step on an approximate inverse: X (symmetric, in sA; whatever sits on the padding is ignored) of A = Asrc + shift I ->
// out = X + X (I - A X), computed on the upper tiles and mirrored.  sV is scratch.  Takes X from the ~1e-6 of a spectral or Cholesky
// inverse in fp32 to the ~1e-7 of the LU-based inverse the reference calls.
template <int NT>
__device__ __forceinline__ void newton_inverse_to_global(float* __restrict__ sA, float* __restrict__ sV, float* __restrict__ out, int D,
                                                         const float* __restrict__ Asrc, float shift) {
  constexpr int DP = NT * 32, LD = DP + 1;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  using T = Tiles<NT, true>;
  f32x16 acc[T::kPerWave];
  for (int idx = tid; idx < DP * DP; idx += kThreads) {
    const int i = idx / DP, k = idx - i * DP;
    sV[i * LD + k] = (i < D && k < D) ? Asrc[i * D + k] + ((i == k) ? shift : 0.f) : 0.f;
  }
  __syncthreads();
  {  // R = I - A X (all tiles) -> sV
    using TF = Tiles<NT, false>;
    f32x16 accf[TF::kPerWave];
    gemm_lds<NT, false, false, false>(sV, sA, accf);
    __syncthreads();
#pragma unroll
    for (int n = 0; n < TF::kPerWave; ++n) {
      const int t = w + kWaves * n;
      if (t < TF::kCount) {
        int I, J;
        TF::ij(t, I, J);
        const int j = J * 32 + (lane & 31);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = I * 32 + acc_row(e, lane);
          sV[i * LD + j] = ((i == j && i < D) ? 1.f : 0.f) - accf[n][e];
        }
      }
    }
  }
  __syncthreads();
  gemm_lds<NT, false, false, true>(sA, sV, acc);  // X R on the upper tiles
#pragma unroll
  for (int n = 0; n < T::kPerWave; ++n) {
    const int t = w + kWaves * n;
    if (t < T::kCount) {
      int I, J;
      T::ij(t, I, J);
      const int j = J * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = I * 32 + acc_row(e, lane);
        if (i <= j && j < D) {
          const float v = sA[i * LD + j] + acc[n][e];
          out[i * D + j] = v;
          if (i != j) out[j * D + i] = v;
        }
      }
    }
  }
}


// f(A) = V diag(f) V^T of the symmetric matrix whose eigenvectors sit in sV (stride DP+1) -> out (D x D, global), computed on
// the upper 32x32 tiles and mirrored so the result is exactly symmetric.  sA is scratch (DP x (DP+1)).
// With Asrc != nullptr, f = 1/(eigenvalue) and the result X ~ (Asrc + shift I)^-1 gets one Newton step X <- X + X (I - A X)
// before it is stored: the eigenvectors of an fp32 solver are orthogonal to ~1e-6 (LAPACK's ssyevd is no better), which is
// the accuracy of V diag(f) V^T, while the step leaves the ~1e-7 of an LU-based inverse (what the reference calls).  That
// matters for the gradients: dL/dTheta_L = -Theta^-1 + S is a small difference of two O(1) matrices near the optimum.
template <int NT>
__device__ __forceinline__ void spectral_to_global(float* __restrict__ sA, float* __restrict__ sV,
                                                   const float* __restrict__ s_f, float* __restrict__ out, int D,
                                                   const float* __restrict__ Asrc = nullptr, float shift = 0.f) {
  constexpr int DP = NT * 32, LD = DP + 1;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int idx = tid; idx < DP * DP; idx += kThreads) {
    const int i = idx / DP, k = idx - i * DP;
    sA[i * LD + k] = sV[i * LD + k] * s_f[k];
  }
  __syncthreads();
  using T = Tiles<NT, true>;
  f32x16 acc[T::kPerWave];
  gemm_lds<NT, false, true, true>(sA, sV, acc);
  if (Asrc == nullptr) {
#pragma unroll
    for (int n = 0; n < T::kPerWave; ++n) {
      const int t = w + kWaves * n;
      if (t < T::kCount) {
        int I, J;
        T::ij(t, I, J);
        const int j = J * 32 + (lane & 31);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = I * 32 + acc_row(e, lane);
          if (i <= j && j < D) {
            out[i * D + j] = acc[n][e];
            if (i != j) out[j * D + i] = acc[n][e];
          }
        }
      }
    }
    return;
  }
  __syncthreads();  // every wave is done reading sA / sV
  // X (symmetric, zero on the padding) -> sA ; A = Asrc + shift I -> sV
#pragma unroll
  for (int n = 0; n < T::kPerWave; ++n) {
    const int t = w + kWaves * n;
    if (t < T::kCount) {
      int I, J;
      T::ij(t, I, J);
      const int j = J * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = I * 32 + acc_row(e, lane);
        if (i <= j) {
          sA[i * LD + j] = acc[n][e];
          sA[j * LD + i] = acc[n][e];
        }
      }
    }
  }
  newton_inverse_to_global<NT>(sA, sV, out, D, Asrc, shift);
}

// Theta_0 = (S + t I)^-1 through the eigendecomposition of S (the same in-LDS solver as the cell): V diag(1/(s_i + t)) V^T.
template <int NT>
__global__ __launch_bounds__(kThreads) void init_inverse_kernel(const float* __restrict__ S,
                                                                const float* __restrict__ params,
                                                                float* __restrict__ theta0,
                                                                float* __restrict__ tri, int D, int gs,
                                                                const int* __restrict__ only_flagged) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sA, eig_buf0_floats<DP>(), sV, DP * LD, tri)
  __shared__ __attribute__((aligned(16))) EigScratch<DP> ws;
  __shared__ float s_f[DP];
  if (only_flagged && only_flagged[blockIdx.x] == 0) return;  // (the Cholesky kernel has done this matrix)
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const float t = params[(size_t)(blockIdx.x / gs) * kNParam + P_T];
  symeig_from_tridiagonal<NT>(sA, sV, D, ws, tri + (size_t)blockIdx.x * 3 * DP, theta0 + base, D);
  if (tid < DP) s_f[tid] = (tid < D) ? 1.0f / (ws.d[tid] + t) : 0.f;
  __syncthreads();
  spectral_to_global<NT>(sA, sV, s_f, theta0 + base, D, S + base, t);
}

constexpr float kCholNewtonRatio = 100.f;  // max / min Cholesky pivot beyond which the matrix goes to the eigen path and its Newton step
// ---- the same two results by blocked Cholesky (chol.h), D <= 128: Theta_0 = (S + t I)^-1 ...
// flags[m] = 0: done; 1: a pivot was not > 0 (S + t I is not positive definite, or holds a NaN): the eigen path recomputes this matrix.
// (lower tiles of the DP x DP matrix: element idx of the packed storage -> (i, j); 32 consecutive idx = one row of a tile)
template <int NT>
__device__ __forceinline__ void chol_packed_coords(int idx, int& i, int& j) {
  const int t = idx >> 10, r = (idx >> 5) & 31, c = idx & 31;
  int I = 0, rem = t;
  while (rem > I) {  // slot t = I (I + 1) / 2 + J
    rem -= I + 1;
    ++I;
  }
  i = 32 * I + r;
  j = 32 * rem + c;
}

template <int NT>
__global__ __launch_bounds__(kThreads, 4) void chol_init_kernel(const float* __restrict__ S, const float* __restrict__ params,
                                                             float* __restrict__ theta0, int* __restrict__ flags, int D, int gs) {
  __shared__ __attribute__((aligned(16))) float sP[chol_lower_tiles(NT) * kTF];
  __shared__ __attribute__((aligned(16))) float sQ[(NT > 1 ? chol_offdiag_tiles(NT) : 1) * kTF];
  __shared__ int s_flag;
  __shared__ float s_log[3];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const float t = params[(size_t)(blockIdx.x / gs) * kNParam + P_T];
  // the lower tiles of S + t I (identity on the padding); eight loads in flight per thread, from clamped addresses
  constexpr int kElems = chol_lower_tiles(NT) * 1024;
  for (int idx0 = 0; idx0 < kElems; idx0 += 8 * kThreads) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = idx0 + q * kThreads + tid;
      int i, k;
      chol_packed_coords<NT>(idx < kElems ? idx : 0, i, k);
      const bool in = i < D && k < D;
      const float x = S[base + (in ? i * D + k : 0)];
      v[q] = in ? x + ((i == k) ? t : 0.f) : ((i == k) ? 1.f : 0.f);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = idx0 + q * kThreads + tid;
      if (idx < kElems) sP[(idx >> 10) * kTF + ((idx >> 5) & 31) * kTS + (idx & 31)] = v[q];
    }
  }
  __syncthreads();
  float logdet, pivot_ratio;
  bool ok = chol_inverse_packed<NT>(sP, sQ, logdet, pivot_ratio, &s_flag, s_log);
  // W^T W from a Cholesky factor is at the ~2e-7 of an LU inverse while the matrix is well conditioned (uGLAD's inputs: cond 10 ... 50).
  // Its error grows with the condition number: a matrix whose pivots spread by more than kCholNewtonRatio goes to the eigen path like one
  // that is not positive definite -- that path ends with a Newton step (Theta within 1.7e-5 instead of 2.8e-5 of fp64 at cond(S + tI) 3500).
  ok = ok && !(pivot_ratio > kCholNewtonRatio);
  if (tid == 0) flags[blockIdx.x] = ok ? 0 : 1;
  if (!ok) return;
  float* __restrict__ out = theta0 + base;
  for (int idx = tid; idx < D * D; idx += kThreads) {
    const int i = idx / D, j = idx - i * D;
    out[idx] = chol_packed_at(sP, i, j);
  }
}

#ifndef UGLAD_TU_NT
__global__ void init_diag_kernel(const float* __restrict__ S, const float* __restrict__ params,
                                 float* __restrict__ theta0, int D, size_t total, int gs) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / ((size_t)D * D);
    const float t = params[(m / gs) * kNParam + P_T];
    const int r = (int)(idx - m * (size_t)D * D);
    const int i = r / D, j = r - i * D;
    theta0[idx] = (i == j) ? 1.0f / (S[idx] + t) : 0.f;
  }
}
#endif

// gt_partial[m] = -<sym(G0), Theta0^2>
template <int NT>
__global__ __launch_bounds__(kThreads) void init_bwd_kernel(const float* __restrict__ theta0,
                                                            const float* __restrict__ G0, float* __restrict__ gt_partial,
                                                            float* __restrict__ gws, int D) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sX, DP * LD, sUnused, 4, gws)
  __shared__ float s_red[8];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t base = (size_t)blockIdx.x * D * D;
  for (int idx0 = 0; idx0 < DP * DP; idx0 += 8 * kThreads) {  // eight loads in flight per thread (clamped addresses)
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = idx0 + q * kThreads + tid;
      const int i = idx / DP, k = idx - i * DP;
      const bool in = (idx < DP * DP) && i < D && k < D;
      const float x = theta0[base + (in ? i * D + k : 0)];
      v[q] = in ? x : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = idx0 + q * kThreads + tid;
      if (idx < DP * DP) sX[(idx / DP) * LD + (idx % DP)] = v[q];
    }
  }
  __syncthreads();
  using T = Tiles<NT, false>;
  f32x16 acc[T::kPerWave];
  gemm_lds<NT, false, false, false>(sX, sX, acc);
  float sum = 0.f;
#pragma unroll
  for (int n = 0; n < T::kPerWave; ++n) {
    const int t = w + kWaves * n;
    if (t < T::kCount) {
      int I, J;
      T::ij(t, I, J);
      const int j = J * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {  // (unconditional loads from clamped addresses: all sixteen in flight)
        const int i = I * 32 + acc_row(e, lane);
        const bool in = i < D && j < D;
        const float gv = G0[base + (in ? j * D + i : 0)];
        sum = fmaf(in ? gv : 0.f, acc[n][e], sum);  // <G0, (Theta0^2)^T>
      }
    }
  }
  sum = block_sum(sum, s_red);
  if (tid == 0) gt_partial[blockIdx.x] = -sum;
}

// Theta_0 = (S + t I)^-1 with respect to S:  gS -= Theta0 sym(G0) Theta0.  T = Theta0 G0 on all tiles, then T Theta0 on the upper tiles,
// subtracted from gS_ij and mirrored into gS_ji (exactly symmetric).  The 42 parameter gradients stay with init_bwd_kernel.
template <int NT>
__global__ __launch_bounds__(kThreads) void init_bwd_gs_kernel(const float* __restrict__ theta0, const float* __restrict__ G0,
                                                               float* __restrict__ gS, float* __restrict__ gws, int D) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sX, DP * LD, sY, DP * LD, gws)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t base = (size_t)blockIdx.x * D * D;
  for (int idx = tid; idx < DP * DP; idx += kThreads) {
    const int i = idx / DP, k = idx - i * DP;
    const bool in = i < D && k < D;
    sX[i * LD + k] = in ? theta0[base + i * D + k] : 0.f;
    sY[i * LD + k] = in ? 0.5f * (G0[base + i * D + k] + G0[base + k * D + i]) : 0.f;
  }
  __syncthreads();
  {
    f32x16 acc[Tiles<NT, false>::kPerWave];
    gemm_lds<NT, false, false, false>(sX, sY, acc);
    __syncthreads();
    store_tiles<NT>(sY, acc);
  }
  __syncthreads();
  using T = Tiles<NT, true>;
  f32x16 acc[T::kPerWave];
  gemm_lds<NT, false, false, true>(sY, sX, acc);
#pragma unroll
  for (int n = 0; n < T::kPerWave; ++n) {
    const int t = w + kWaves * n;
    if (t < T::kCount) {
      int I, J;
      T::ij(t, I, J);
      const int j = J * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = I * 32 + acc_row(e, lane);
        if (i <= j && j < D) {
          const float v = gS[base + i * D + j] - acc[n][e];
          gS[base + i * D + j] = v;
          if (i != j) gS[base + j * D + i] = v;
        }
      }
    }
  }
}

#ifndef UGLAD_TU_NT
// Theta_0 = diag(1 / (S_ii + t)) with respect to S:  gS_ii -= G0_ii Theta0_ii^2.  One thread per diagonal entry.
__global__ void init_bwd_diag_gs_kernel(const float* __restrict__ theta0, const float* __restrict__ G0, float* __restrict__ gS, int D,
                                        size_t total) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / D;
    const size_t at = m * D * D + (idx - m * D) * (D + 1);
    const float d = theta0[at];
    gS[at] -= G0[at] * d * d;
  }
}
#endif

#ifndef UGLAD_TU_NT
__global__ __launch_bounds__(kThreads) void init_bwd_diag_kernel(const float* __restrict__ theta0,
                                                                 const float* __restrict__ G0,
                                                                 float* __restrict__ gt_partial, int D) {
  __shared__ float s_red[8];
  const size_t base = (size_t)blockIdx.x * D * D;
  float sum = 0.f;
  for (int i = threadIdx.x; i < D; i += kThreads) {
    const float d = theta0[base + i * D + i];
    sum = fmaf(G0[base + i * D + i], d * d, sum);
  }
  sum = block_sum(sum, s_red);
  if (threadIdx.x == 0) gt_partial[blockIdx.x] = -sum;
}
#endif

// =============================================================================================== loss
__device__ __forceinline__ float log_cosh(float x) {
  const float a = fabsf(x);
  return a + log1pf(expf(-2.f * a)) - 0.69314718056f;
}

// loss partial + Theta^-1 through the eigendecomposition Theta = V diag(beta) V^T:  logdet = sum log|beta_i| with the sign of
// prod beta_i deciding NaN (det < 0) / -inf (det = 0) as torch.logdet does; Theta^-1 = V diag(1/beta) V^T.
template <int NT>
__global__ __launch_bounds__(kThreads) void loss_fwd_kernel(const float* __restrict__ theta, const float* __restrict__ S,
                                                            int s_batch, const float* __restrict__ struct_theta,
                                                            float* __restrict__ loss_partial,
                                                            float* __restrict__ theta_inv,
                                                            float* __restrict__ tri, int D, const int* __restrict__ only_flagged) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sA, eig_buf0_floats<DP>(), sV, DP * LD, tri)
  __shared__ __attribute__((aligned(16))) EigScratch<DP> ws;
  __shared__ float s_f[DP], s_red[8];
  if (only_flagged && only_flagged[blockIdx.x] == 0) return;  // (the Cholesky kernel has done this matrix)
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const size_t sbase = (size_t)(blockIdx.x % s_batch) * D * D;
  float tr = 0.f;
  for (int idx = tid; idx < D * D; idx += kThreads) {
    const int i = idx / D, j = idx - i * D;
    const float th = theta[base + idx];
    tr = fmaf(S[sbase + j * D + i], th, tr);
    if (struct_theta) {
      const float mask = (1.f - struct_theta[sbase + idx]) - ((i == j) ? 1.f : 0.f);
      tr += log_cosh(th * mask);
    }
  }
  tr = block_sum(tr, s_red);
  symeig_from_tridiagonal<NT>(sA, sV, D, ws, tri + (size_t)blockIdx.x * 3 * DP, theta_inv + base, D);
  float lad = 0.f, neg = 0.f, zero = 0.f;
  if (tid < DP) {
    float f = 0.f;
    if (tid < D) {
      const float be = ws.d[tid];
      f = 1.0f / be;
      lad = logf(fabsf(be));
      neg = (be < 0.f) ? 1.f : 0.f;
      zero = (be == 0.f) ? 1.f : 0.f;
    }
    s_f[tid] = f;
  }
  lad = block_sum(lad, s_red);
  neg = block_sum(neg, s_red);
  zero = block_sum(zero, s_red);
  spectral_to_global<NT>(sA, sV, s_f, theta_inv + base, D, theta + base, 0.f);
  if (tid == 0) {
    float logdet = lad;
    if (((int)neg) & 1) logdet = __builtin_nanf("");
    if (zero > 0.f) logdet = -__builtin_inff();
    loss_partial[blockIdx.x] = -logdet + tr;
  }
}

// ... and the loss partial -logdet(Theta) + tr(S Theta) (+ structure penalty) with Theta^-1 for the backward pass (loss_fwd_kernel's outputs)
template <int NT>
__global__ __launch_bounds__(kThreads, 4) void chol_loss_kernel(const float* __restrict__ theta, const float* __restrict__ S, int s_batch,
                                                             const float* __restrict__ struct_theta, float* __restrict__ loss_partial,
                                                             float* __restrict__ theta_inv, int* __restrict__ flags, int D) {
  __shared__ __attribute__((aligned(16))) float sP[chol_lower_tiles(NT) * kTF];
  __shared__ __attribute__((aligned(16))) float sQ[(chol_offdiag_tiles(NT) > kWaves ? chol_offdiag_tiles(NT) : kWaves) * kTF];  // (>= one tile per wave)
  __shared__ int s_flag;
  __shared__ float s_log[3], s_red[8];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const size_t sbase = (size_t)(blockIdx.x % s_batch) * D * D;
  float tr = 0.f;
  constexpr int kElems = chol_lower_tiles(NT) * 1024;
  for (int idx = tid; idx < kElems; idx += kThreads) {  // identity on the padding (LDS only)
    int i, k;
    chol_packed_coords<NT>(idx, i, k);
    if (i >= D || k >= D) sP[(idx >> 10) * kTF + ((idx >> 5) & 31) * kTS + (idx & 31)] = (i == k) ? 1.f : 0.f;
  }
  // The trace term sum_ij S_ij Theta_ji and the lower tiles of Theta -> LDS from ONE pass over Theta, tile by tile: a wave takes the pair
  // (S_IJ, Theta_JI), both read along their rows (128 contiguous bytes per half wave), and transposes S_IJ through a tile of LDS -- read
  // straight from memory the transposed operand costs a cache line per element (the kernel took 270 us against Theta_0's 160).
  {
    const int lane = tid & 63, w = tid >> 6, c = lane & 31, rh = lane >> 5;
    float* __restrict__ sT = sQ + w * kTF;  // one scratch tile per wave (sQ is idle until W = L^-1)
    for (int t = w; t < NT * NT; t += kWaves) {
      const int I = t / NT, J = t - I * NT;
      float sv[16], th[16];
#pragma unroll
      for (int it = 0; it < 16; ++it) {  // rows 2 it + rh of both tiles, column c: 32 loads in flight per lane
        const int r = 2 * it + rh;
        const int si = 32 * I + r, sj = 32 * J + c;  // S_IJ[r][c]
        const int ti = 32 * J + r, tj = 32 * I + c;  // Theta_JI[r][c]
        const float xs = S[sbase + ((si < D && sj < D) ? si * D + sj : 0)];
        const float xt = theta[base + ((ti < D && tj < D) ? ti * D + tj : 0)];
        sv[it] = (si < D && sj < D) ? xs : 0.f;
        th[it] = (ti < D && tj < D) ? xt : 0.f;
      }
      UGLAD_WAVE_SYNC();  // (the wave's previous tile has been read by all its lanes)
#pragma unroll
      for (int it = 0; it < 16; ++it) sT[(2 * it + rh) * kTS + c] = sv[it];
      UGLAD_WAVE_SYNC();  // a wave's own LDS writes are visible to its own later reads; other waves use other tiles
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        const int r = 2 * it + rh;
        const int ti = 32 * J + r, tj = 32 * I + c;
        if (ti < D && tj < D) {
          tr = fmaf(sT[c * kTS + r], th[it], tr);  // S_IJ[c][r] Theta_JI[r][c]
          if (struct_theta) {
            const float mask = (1.f - struct_theta[sbase + (size_t)ti * D + tj]) - ((ti == tj) ? 1.f : 0.f);
            tr += log_cosh(th[it] * mask);
          }
          if (J >= I) sP[chol_slot(J, I) * kTF + r * kTS + c] = th[it];
        }
      }
    }
  }
  tr = block_sum(tr, s_red);
  __syncthreads();
  float logdet, pivot_ratio;
  bool ok = chol_inverse_packed<NT>(sP, sQ, logdet, pivot_ratio, &s_flag, s_log);
  ok = ok && !(pivot_ratio > kCholNewtonRatio);  // (ill-conditioned: the eigen path with its Newton step, as for Theta_0)
  if (tid == 0) flags[blockIdx.x] = ok ? 0 : 1;
  if (!ok) return;
  if (tid == 0) loss_partial[blockIdx.x] = -logdet + tr;
  float* __restrict__ out = theta_inv + base;
  for (int idx = tid; idx < D * D; idx += kThreads) {
    const int i = idx / D, j = idx - i * D;
    out[idx] = chol_packed_at(sP, i, j);
  }
}

#ifndef UGLAD_TU_NT
__global__ void loss_bwd_kernel(const float* __restrict__ theta, const float* __restrict__ theta_inv,
                                const float* __restrict__ S, int s_batch, const float* __restrict__ struct_theta,
                                const float* __restrict__ g_up, float scale, float* __restrict__ Gout, int D,
                                size_t total) {
  const float gs = g_up[0] * scale;
  const size_t dd = (size_t)D * D;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / dd;
    const int r = (int)(idx - m * dd);
    const int i = r / D, j = r - i * D;
    const size_t sb = (m % s_batch) * dd;
    // Theta^-1 (mirrored by loss_fwd) and S are symmetric: read them in place, coalesced, instead of transposed
    float v = -theta_inv[idx] + S[sb + r];
    if (struct_theta) {
      const float mask = (1.f - struct_theta[sb + r]) - ((i == j) ? 1.f : 0.f);
      v += tanhf(theta[idx] * mask) * mask;
    }
    Gout[idx] = gs * v;
  }
}

// dL/dS of the loss, symmetric part: gS_b = g_up[0] * scale * sum over the matrices m that read S_b of (Theta_m + Theta_m^T) / 2
// (one S broadcast against all M matrices when s_batch = 1).  Overwrites gS (s_batch, D, D); a fixed order of the sum over m.
__global__ void loss_bwd_gs_kernel(const float* __restrict__ theta, const float* __restrict__ g_up, float scale, float* __restrict__ gS,
                                   int s_batch, int M, int D) {
  const float gs = g_up[0] * scale * 0.5f;
  const size_t dd = (size_t)D * D, total = (size_t)s_batch * dd;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t sb = idx / dd;
    const int r = (int)(idx - sb * dd);
    const int i = r / D, j = r - i * D;
    float v = 0.f;
    for (size_t m = sb; m < (size_t)M; m += s_batch) v += theta[m * dd + i * D + j] + theta[m * dd + j * D + i];
    gS[idx] = gs * v;
  }
}

// dL/dS of one step on the paths whose kernels have no dL/dS variant (the many-workgroups backward, csrc/wide_bwd.h, and the matrix
// iteration, csrc/wide_ns.h), behind their unchanged launches: per upper-triangle entry (i, j) the rhoNN / threshold backward of the step
// is evaluated again from G_next, theta_half, S and Z_in -- the S-feature term, and the Z_in-feature term gz that the step's G_out holds
// together with -G_B (G_out = gz - G_B) -- and gS_ij += (gz - sym(G_out))_ij / lam_k + the S-feature term, mirrored into gS_ji.
__global__ __launch_bounds__(256) void cell_gs_step_kernel(const float* __restrict__ Gnext, const float* __restrict__ S,
                                                           const float* __restrict__ Zin, const float* __restrict__ half,
                                                           const float* __restrict__ lam_ptr, const float* __restrict__ params,
                                                           const float* __restrict__ Gout, float* __restrict__ gS, int D, int gs,
                                                           size_t total) {
  const size_t dd = (size_t)D * D;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / dd;
    const int r = (int)(idx - m * dd);
    const int i = r / D, j = r - i * D;
    if (j < i) continue;
    const size_t ij = m * dd + r, ji = m * dd + (size_t)j * D + i;
    const int grp = (int)(m / gs);
    const float* p = params + (size_t)grp * kNParam;
    const float lam = lam_ptr[grp];
    const float gn = (i == j) ? Gnext[ij] : 0.5f * (Gnext[ij] + Gnext[ji]);
    const float x = half[ij];
    RhoAct act;
    rho_forward(p, x, S[ij], Zin[ij], act);
    const bool active = fabsf(x) > act.rho;
    const float sgn = (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f);
    const float g_rho = active ? -sgn * gn : 0.f;
    const float gz = rho_backward_col(p, act, g_rho, 2);
    const float go = (i == j) ? Gout[ij] : 0.5f * (Gout[ij] + Gout[ji]);
    const float v = gS[ij] + (gz - go) / lam + rho_backward_col(p, act, g_rho, 1);
    gS[ij] = v;
    gS[ji] = v;
  }
}

// C_m = A_m B_m for M matrices of D x D (fp32; 64 x 64 output tile per workgroup, 4 x 4 per thread, k in chunks of 16 through LDS): the
// Theta_0 term of dL/dS beyond the one-workgroup kernels' size.
__global__ __launch_bounds__(256) void gs_gemm_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ C, int D) {
  __shared__ float sA[16][65], sB[16][65];
  const size_t base = (size_t)blockIdx.z * D * D;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int k0 = 0; k0 < D; k0 += 16) {
    for (int e = threadIdx.x; e < 1024; e += 256) {
      const int ar = e >> 4, ac = e & 15, gi = i0 + ar, gk = k0 + ac;
      sA[ac][ar] = (gi < D && gk < D) ? A[base + (size_t)gi * D + gk] : 0.f;
      const int br = e >> 6, bc = e & 63, bk = k0 + br, bj = j0 + bc;
      sB[br][bc] = (bk < D && bj < D) ? B[base + (size_t)bk * D + bj] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float a[4], b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a[q] = sA[k][4 * ty + q];
        b[q] = sB[k][4 * tx + q];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = fmaf(a[u], b[v], acc[u][v]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = i0 + 4 * ty + u;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = j0 + 4 * tx + v;
      if (i < D && j < D) C[base + (size_t)i * D + j] = acc[u][v];
    }
  }
}

// gS -= (R + R^T) / 2, elementwise over M matrices (exactly symmetric when gS is)
__global__ void gs_sub_sym_kernel(const float* __restrict__ R, float* __restrict__ gS, int D, size_t total) {
  const size_t dd = (size_t)D * D;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / dd;
    const int r = (int)(idx - m * dd);
    const int i = r / D, j = r - i * D;
    gS[idx] -= 0.5f * (R[idx] + R[m * dd + (size_t)j * D + i]);
  }
}
#endif

// =============================================================================================== lambda / reductions
// one thread per group g < G: lam (.., G), lam_in (.., G, 2), params (G, 42)
#ifndef UGLAD_TU_NT
__global__ void lambda_init_kernel(const float* __restrict__ params, float lambda_init, float* __restrict__ lam_out,
                                   float* __restrict__ lam_in, int G) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < G) {
    lam_in[2 * g] = lambda_init;
    lam_in[2 * g + 1] = 0.f;
    lam_out[g] = lambda_forward(params + (size_t)g * kNParam, lambda_init, 0.f);
  }
}
#endif

#ifndef UGLAD_TU_NT
__global__ void lambda_step_kernel(const float* __restrict__ normF_sum, float inv_M, const float* __restrict__ lam_prev,
                                   const float* __restrict__ params, float* __restrict__ lam_next,
                                   float* __restrict__ lam_in_next, int G) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < G) {
    const float n = normF_sum[g] * inv_M, lp = lam_prev[g];
    lam_in_next[2 * g] = n;
    lam_in_next[2 * g + 1] = lp;
    lam_next[g] = lambda_forward(params + (size_t)g * kNParam, n, lp);
  }
}
#endif

// sum_partials + lambda_step in one launch (the single-process pass: nothing to exchange between the two).  One block per
// group; same summation order as sum_partials_kernel, so the sharded and the fused path see the same bits per rank.
#ifndef UGLAD_TU_NT
__global__ __launch_bounds__(kThreads) void norm_lambda_kernel(const float* __restrict__ partials, int n, float inv_M,
                                                               const float* __restrict__ lam_prev,
                                                               const float* __restrict__ params, float* __restrict__ nf_sum,
                                                               float* __restrict__ lam_next, float* __restrict__ lam_in_next) {
  __shared__ float s_red[8];
  const int g = blockIdx.x;
  partials += (size_t)g * n;
  float v = 0.f;
  for (int i = threadIdx.x; i < n; i += kThreads) v += partials[i];
  v = block_sum(v, s_red);
  if (threadIdx.x == 0) {
    nf_sum[g] = v;
    const float nrm = v * inv_M, lp = lam_prev[g];
    lam_in_next[2 * g] = nrm;
    lam_in_next[2 * g + 1] = lp;
    lam_next[g] = lambda_forward(params + (size_t)g * kNParam, nrm, lp);
  }
}
#endif

#ifndef UGLAD_TU_NT
__global__ void zero_kernel(float* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0.f;
}
#endif

// deterministic: fixed per-thread strides, fixed tree
#ifndef UGLAD_TU_NT
__global__ __launch_bounds__(kThreads) void sum_partials_kernel(const float* __restrict__ partials, int n,
                                                                float* __restrict__ out) {
  __shared__ float s_red[8];
  partials += (size_t)blockIdx.x * n;  // one block per group
  float v = 0.f;
  for (int i = threadIdx.x; i < n; i += kThreads) v += partials[i];
  v = block_sum(v, s_red);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}
#endif

// grad[0] <- sum gt ; grad[1..28] <- column sums of grad_rho_partial ; grad[29..41] <- LambdaNN chain
#ifndef UGLAD_TU_NT
__global__ __launch_bounds__(kThreads) void finish_grads_kernel(const float* __restrict__ gt_partial,
                                                                const float* __restrict__ grad_rho_partial,
                                                                const float* __restrict__ glam_partial,
                                                                const float* __restrict__ lam_in,
                                                                const float* __restrict__ p, float* __restrict__ grad,
                                                                int L, int Mtot, int gs) {
  // one block per group g: matrices [g gs, (g + 1) gs) of the Mtot in the batch; p, grad: (G, 42); lam_in: (L + 1, G, 2)
  __shared__ float s_red[8];
  __shared__ float s_glam[64];
  const int tid = threadIdx.x;
  const int g = blockIdx.x, G = gridDim.x, M = gs;
  gt_partial += (size_t)g * gs;
  grad_rho_partial += (size_t)g * gs * kNRho;
  glam_partial += (size_t)g * gs;
  p += (size_t)g * kNParam;
  grad += (size_t)g * kNParam;
  {
    float v = 0.f;
    for (int i = tid; i < M; i += kThreads) v += gt_partial[i];
    v = block_sum(v, s_red);
    if (tid == 0) grad[P_T] = v;
  }
  for (int q = 0; q < kNRho; ++q) {
    float v = 0.f;
    for (int i = tid; i < M; i += kThreads) v += grad_rho_partial[(size_t)i * kNRho + q];
    v = block_sum(v, s_red);
    if (tid == 0) grad[1 + q] = v;
  }
  float gl[13];
#pragma unroll
  for (int q = 0; q < 13; ++q) gl[q] = 0.f;
  for (int k0 = 0; k0 < L; k0 += 64) {
    const int kn = (L - k0) < 64 ? (L - k0) : 64;
    for (int kk = 0; kk < kn; ++kk) {
      float v = 0.f;
      for (int i = tid; i < M; i += kThreads) v += glam_partial[(size_t)(k0 + kk) * Mtot + i];
      v = block_sum(v, s_red);
      if (tid == 0) s_glam[kk] = v;
    }
    __syncthreads();
    if (tid == 0) {
      for (int kk = 0; kk < kn; ++kk) {
        const float n = lam_in[2 * ((size_t)(k0 + kk) * G + g)], lp = lam_in[2 * ((size_t)(k0 + kk) * G + g) + 1];
        float h[3], o = p[P_LB2];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          h[u] = tanhf(fmaf(p[P_LW1 + 2 * u], n, fmaf(p[P_LW1 + 2 * u + 1], lp, p[P_LB1 + u])));
          o = fmaf(p[P_LW2 + u], h[u], o);
        }
        const float sg = sigmoidf_(o);
        const float go = s_glam[kk] * sg * (1.f - sg);
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          gl[6 + 3 + u] += go * h[u];  // lambda_f.2.weight
          const float ga = go * p[P_LW2 + u] * (1.f - h[u] * h[u]);
          gl[2 * u] += ga * n;       // lambda_f.0.weight[u][0]
          gl[2 * u + 1] += ga * lp;  // lambda_f.0.weight[u][1]
          gl[6 + u] += ga;           // lambda_f.0.bias
        }
        gl[12] += go;  // lambda_f.2.bias
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < 13; ++q) grad[P_LW1 + q] = gl[q];
  }
}
#endif

// =============================================================================================== consensus
#ifndef UGLAD_TU_NT
__global__ void consensus_partial_kernel(const float* __restrict__ theta_K, int K, int DD, float* __restrict__ absmin,
                                         float* __restrict__ signsum) {
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < DD; idx += gridDim.x * blockDim.x) {
    float mn = __builtin_inff(), ss = 0.f;
    for (int k = 0; k < K; ++k) {
      const float v = theta_K[(size_t)k * DD + idx];
      mn = fminf(mn, fabsf(v));
      ss += (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : 0.f);
    }
    absmin[idx] = mn;
    signsum[idx] = ss;
  }
}
#endif

#ifndef UGLAD_TU_NT
__global__ void consensus_combine_kernel(const float* __restrict__ absmin, const float* __restrict__ signsum, int DD,
                                         float* __restrict__ out) {
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < DD; idx += gridDim.x * blockDim.x)
    out[idx] = (signsum[idx] >= 0.f ? 1.f : -1.f) * absmin[idx];
}
#endif

// =============================================================================================== symeig (unit-test exports)
// the LDS-lean solver alone (D <= 128): what uglad_symeig runs there, so that the unit tests of the solver (degenerate,
// clustered, graded spectra) exercise the code path of the forward cell
template <int NT>
__global__ __launch_bounds__(kThreads, NT <= 4 ? 4 : 2) void symeig_lean_kernel(float* __restrict__ U, float* __restrict__ beta,
                                                                  const float* __restrict__ tri, float* __restrict__ Tws, int D) {
  constexpr int DP = NT * 32, LD = DP + 1;
  constexpr bool kGM = DP > 128;
  __shared__ __attribute__((aligned(16))) float sQ_lds[kGM ? 4 : DP * LD];
  float* sQ = kGM ? const_cast<float*>(tri) + (size_t)gridDim.x * kWsPerMatrix<DP> + (size_t)blockIdx.x * big_floats<DP>() : sQ_lds;
  __shared__ __attribute__((aligned(16))) LeanScratch<DP> ws;
  const size_t base = (size_t)blockIdx.x * D * D;
  symeig_lean<NT>(sQ, D, ws, tri + (size_t)blockIdx.x * 3 * DP, U + base, D, Tws + (size_t)blockIdx.x * NT * 1024);
  copy_out_matrix(U + base, sQ, D, LD);
  if (threadIdx.x < D) beta[(size_t)blockIdx.x * D + threadIdx.x] = ws.d[threadIdx.x];
}

#ifdef UGLAD_STAMPS
// diagnostic build only: the solver alone, phase stamps of workgroup m copied to stamps[m*64 ..]
template <int NT>
__global__ __launch_bounds__(kThreads) void symeig_stamp_kernel(float* __restrict__ U, float* __restrict__ beta,
                                                                float* __restrict__ tri, int D,
                                                                unsigned long long* __restrict__ stamps) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sA, eig_buf0_floats<DP>(), sV, DP * LD, tri)
  __shared__ __attribute__((aligned(16))) EigScratch<DP> ws;
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  if (tid < 96) ws.stamp[tid] = 0;
  __syncthreads();
  UGLAD_STAMP(ws, 0);
  symeig_from_tridiagonal<NT>(sA, sV, D, ws, tri + (size_t)blockIdx.x * 3 * DP, U + base, D);
  for (int idx = tid; idx < D * D; idx += kThreads) U[base + idx] = sV[(idx / D) * LD + (idx % D)];
  if (tid < D) beta[(size_t)blockIdx.x * D + tid] = ws.d[tid];
  __syncthreads();
  if (tid < 96) stamps[(size_t)blockIdx.x * 96 + tid] = ws.stamp[tid];
}
#endif

// =============================================================================================== covariance front-end
// What fit() does to a table before the hot path: min-max normalisation of the columns
// (prepare_data.py:597-613, main.py:85), the maximum-likelihood covariance sum_n (x_n - mu)(x_n - mu)^T / N of
// sklearn.empirical_covariance (prepare_data.py:342) and -- in a second launch, once the eigenvalues are known -- the
// reference's repair of a singular matrix (prepare_data.py:347-352).  One workgroup per task: column statistics in a first
// pass over the table, then the table streams through LDS in chunks of 64 centred rows into the upper 32x32 MFMA tiles.
template <int NT>
__global__ __launch_bounds__(kThreads) void cov_kernel(const float* __restrict__ X, int N, int D, int normalize,
                                                       float* __restrict__ S_out) {
  constexpr int DP = NT * 32, LD = DP + 1, CH = 64, G = kThreads / DP;
  __shared__ __attribute__((aligned(16))) float s_x[CH * LD];
  __shared__ float s_mn[DP], s_sc[DP], s_mu[DP];
  __shared__ float s_p[3][G][DP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* Xt = X + (size_t)blockIdx.x * N * D;
  float* So = S_out + (size_t)blockIdx.x * D * D;
  // ---- pass 1: min, max, sum per column (thread = column c, row group g; rows g, g + G, ...)
  {
    const int c = tid % DP, g = tid / DP;
    if (g < G) {
      float mn = 3.4e38f, mx = -3.4e38f, sm = 0.f;
      bool nan = false;
      if (c < D)
        for (int n = g; n < N; n += G) {
          const float v = Xt[(size_t)n * D + c];
          nan = nan || (v != v);
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
          sm += v;
        }
      s_p[0][g][c] = nan ? __builtin_nanf("") : mn;
      s_p[1][g][c] = mx;
      s_p[2][g][c] = sm;
    }
  }
  __syncthreads();
  if (tid < DP) {
    float mn = s_p[0][0][tid], mx = s_p[1][0][tid], sm = s_p[2][0][tid];
    for (int g = 1; g < G; ++g) {
      const float a = s_p[0][g][tid];
      mn = (a != a || mn != mn) ? __builtin_nanf("") : fminf(mn, a);
      mx = fmaxf(mx, s_p[1][g][tid]);
      sm += s_p[2][g][tid];
    }
    const float mean = sm / (float)N;
    if (normalize == 1) {  // (x - min) / (max - min): a constant column gives 0/0 = NaN, as in the reference
      const float sc = 1.0f / (mx - mn);
      s_mn[tid] = mn;
      s_sc[tid] = sc;
      s_mu[tid] = (mean - mn) * sc;
    } else {
      s_mn[tid] = 0.f;
      s_sc[tid] = 1.f;
      s_mu[tid] = mean;
    }
  }
  __syncthreads();
  // ---- pass 2: S = sum over chunks of Xc^T Xc on the upper tiles
  using T = Tiles<NT, true>;
  f32x16 acc[T::kPerWave];
#pragma unroll
  for (int n = 0; n < T::kPerWave; ++n)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;
  for (int r0 = 0; r0 < N; r0 += CH) {
    for (int idx = tid; idx < CH * DP; idx += kThreads) {
      const int r = idx / DP, c = idx - r * DP;
      float v = 0.f;
      if (r0 + r < N && c < D) v = (Xt[(size_t)(r0 + r) * D + c] - s_mn[c]) * s_sc[c] - s_mu[c];
      s_x[r * LD + c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < T::kPerWave; ++n) {
      const int t = w + kWaves * n;
      if (t < T::kCount) {
        int I, J;
        T::ij(t, I, J);
        mfma_tile(s_x + I * 32, 1, LD, s_x + J * 32, LD, 1, CH, acc[n]);
      }
    }
    __syncthreads();
  }
  const float inv_n = 1.0f / (float)N;
#pragma unroll
  for (int n = 0; n < T::kPerWave; ++n) {
    const int t = w + kWaves * n;
    if (t < T::kCount) {
      int I, J;
      T::ij(t, I, J);
      const int j = J * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = I * 32 + acc_row(e, lane);
        if (i <= j && j < D) {
          const float v = acc[n][e] * inv_n;
          So[i * D + j] = v;
          if (i != j) So[j * D + i] = v;
        }
      }
    }
  }
}

// S += (offset - min eig) I where the smallest eigenvalue is <= 1e-6 (beta ascending: beta[0] is the smallest)
#ifndef UGLAD_TU_NT
__global__ void cov_repair_kernel(float* __restrict__ S, const float* __restrict__ beta, int D, float offset) {
  const float mn = beta[(size_t)blockIdx.x * D];
  if (mn <= 1e-6f) {
    float* So = S + (size_t)blockIdx.x * D * D;
    for (int i = threadIdx.x; i < D; i += blockDim.x) So[i * D + i] += offset - mn;
  }
}
#endif

// =============================================================================================== after the path
// ---- N3: conditional Gaussian / MAP estimate given observed coordinates (main.py:1176-1260).  With the precision matrix
// partitioned into unobserved (u) and observed (o) coordinates the reference computes  mean_u - L_uu^-1 L_uo (x_o - mean_o)
// (scipy.linalg.solve), the conditional covariance L_uu^-1 and the density at the MAP point.  Here L_uu stays IN PLACE: the
// masked matrix A (A_ij = P_ij for i, j both unobserved, delta_ij otherwise) has L_uu^-1 as the (u, u) block of its inverse and
// the identity elsewhere, so no gather / scatter is needed and the path's own eigensolver does the solve.
#ifndef UGLAD_TU_NT
__global__ void map_prepare_kernel(const float* __restrict__ P, const float* __restrict__ observed, float* __restrict__ A, int D,
                                   size_t total) {
  const size_t dd = (size_t)D * D;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / dd;
    const int r = (int)(idx - m * dd);
    const int i = r / D, j = r - i * D;
    const bool keep = observed[m * D + i] == 0.f && observed[m * D + j] == 0.f;
    // (the upper-triangle value on both sides: the solver assumes exact symmetry)
    A[idx] = keep ? P[m * dd + (i <= j ? (size_t)i * D + j : (size_t)j * D + i)] : ((i == j) ? 1.f : 0.f);
  }
}
#endif

template <int NT>
__global__ __launch_bounds__(kThreads) void map_solve_kernel(const float* __restrict__ P, const float* __restrict__ mean,
                                                             const float* __restrict__ observed,
                                                             const float* __restrict__ values, const float* __restrict__ A,
                                                             float* __restrict__ full_mean, float* __restrict__ cond_cov,
                                                             float* __restrict__ log_pdf, float* __restrict__ tri, int D,
                                                             int clip01) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sA, eig_buf0_floats<DP>(), sV, DP * LD, tri)
  __shared__ __attribute__((aligned(16))) EigScratch<DP> ws;
  __shared__ float s_f[DP], s_r[DP], s_t[DP], s_y[DP], s_red[8];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const float* Pm = P + base;
  const float* Am = A + base;
  const float* mu = mean + (size_t)blockIdx.x * D;
  const float* ob = observed + (size_t)blockIdx.x * D;
  const float* xv = values + (size_t)blockIdx.x * D;
  // right-hand side r_u = L_uo (x_o - mean_o), zero on the observed coordinates
  if (tid < DP) {
    float r = 0.f;
    if (tid < D && ob[tid] == 0.f) {
      for (int j = 0; j < D; ++j)
        if (ob[j] != 0.f) r = fmaf(Pm[tid <= j ? tid * D + j : j * D + tid], xv[j] - mu[j], r);
    }
    s_r[tid] = r;
  }
  symeig_from_tridiagonal<NT>(sA, sV, D, ws, tri + (size_t)blockIdx.x * 3 * DP, cond_cov + base, D);
  float lad = 0.f, bad = 0.f, nu = 0.f;
  if (tid < DP) {
    float f = 0.f;
    if (tid < D) {
      const float be = ws.d[tid];
      f = 1.0f / be;
      lad = logf(be);  // (NaN for a negative eigenvalue: L_uu not positive definite)
      bad = (be > 0.f) ? 0.f : 1.f;
      nu = (ob[tid] == 0.f) ? 1.f : 0.f;
    }
    s_f[tid] = f;
  }
  lad = block_sum(lad, s_red);
  bad = block_sum(bad, s_red);
  nu = block_sum(nu, s_red);
  // y = A^-1 r = V diag(1/beta) V^T r, then one step of iterative refinement y += A^-1 (r - A y) (A from global memory)
  auto apply_inverse = [&](const float* __restrict__ rhs, float* __restrict__ dst, bool accumulate) {
    if (tid < DP) {
      float t = 0.f;
      for (int i = 0; i < D; ++i) t = fmaf(sV[i * LD + tid], rhs[i], t);
      s_t[tid] = t * s_f[tid];
    }
    __syncthreads();
    if (tid < DP) {
      float y = 0.f;
      if (tid < D)
        for (int k = 0; k < D; ++k) y = fmaf(sV[tid * LD + k], s_t[k], y);
      dst[tid] = accumulate ? dst[tid] + y : y;
    }
    __syncthreads();
  };
  apply_inverse(s_r, s_y, false);
  if (tid < DP) {
    float res = 0.f;
    if (tid < D) {
      res = s_r[tid];
      for (int j = 0; j < D; ++j) res = fmaf(-Am[tid * D + j], s_y[j], res);
    }
    sA[tid] = res;  // (sA is free between the solver and spectral_to_global)
  }
  __syncthreads();
  apply_inverse(sA, s_y, true);
  if (tid < D) {
    float v = (ob[tid] != 0.f) ? xv[tid] : mu[tid] - s_y[tid];
    if (clip01) v = fminf(fmaxf(v, 0.f), 1.f);
    full_mean[(size_t)blockIdx.x * D + tid] = v;
  }
  if (tid == 0 && log_pdf)
    log_pdf[blockIdx.x] = (bad > 0.f) ? __builtin_nanf("") : fmaf(-0.5f * nu, 1.8378770664093453f, 0.5f * lad);
  __syncthreads();
  spectral_to_global<NT>(sA, sV, s_f, cond_cov + base, D, Am, 0.f);  // A^-1: L_uu^-1 on the (u, u) block, identity elsewhere
}

// ---- N4: partial correlations (main.py:796-821): rho_ij = -p_ij / sqrt(p_ii p_jj) from the UPPER triangle, mirrored, 1 on the diagonal
#ifndef UGLAD_TU_NT
__global__ void partial_corr_kernel(const float* __restrict__ P, float* __restrict__ rho, int D, size_t total) {
  const size_t dd = (size_t)D * D;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t m = idx / dd;
    const int r = (int)(idx - m * dd);
    const int i = r / D, j = r - i * D;
    const float* Pm = P + m * dd;
    const int a = i < j ? i : j, b = i < j ? j : i;
    rho[idx] = (i == j) ? 1.f : -Pm[(size_t)a * D + b] / sqrtf(Pm[(size_t)a * D + a] * Pm[(size_t)b * D + b]);
  }
}
#endif

// ---- N4: support-recovery metrics of report_metrics_all (utils/metrics.py:25-108) for one (true, predicted) pair per
// workgroup.  Edges = strict upper triangle; an edge is predicted where the entry is non-zero; scores for the ranking metrics
// are |entry|.  All counting is integer (exact, order-independent): ROC-AUC is the Mann-Whitney statistic with ties at 1/2
// (the trapezoid of sklearn.metrics.roc_curve), average precision is (1/T) sum over true edges of precision at that edge's
// score (sklearn.metrics.average_precision_score: thresholds are the distinct scores).  out[0..10] (double): FDR, TPR, FPR,
// SHD, nnzTrue, nnzPred, precision, recall, Fbeta, aupr, auc -- unrounded (the host rounds to 3 decimals as the reference does).
template <int NT>
__global__ __launch_bounds__(kThreads) void support_metrics_kernel(const float* __restrict__ true_theta,
                                                                   const float* __restrict__ pred_theta,
                                                                   double* __restrict__ out, int D, int beta) {
  constexpr int DP = NT * 32, EMAX = DP * (DP - 1) / 2;
  __shared__ float s_score[EMAX];            // |pred| of edge e
  __shared__ int s_true[EMAX / 32 + 1];       // bit e: the edge exists in the true graph
  __shared__ long long s_cnt[kThreads];
  __shared__ double s_dbl[kThreads];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const int E = D * (D - 1) / 2;
  for (int w = tid; w < EMAX / 32 + 1; w += kThreads) s_true[w] = 0;
  __syncthreads();
  for (int idx = tid; idx < D * D; idx += kThreads) {
    const int i = idx / D, j = idx - i * D;
    if (i < j) {
      const int e = i * D - (i * (i + 1)) / 2 + (j - i - 1);
      s_score[e] = fabsf(pred_theta[base + idx]);
      if (true_theta[base + idx] != 0.f) atomicOr(&s_true[e >> 5], (int)(1u << (e & 31)));
    }
  }
  __syncthreads();
  auto is_true = [&](int e) { return (((unsigned)s_true[e >> 5]) >> (e & 31)) & 1u; };
  // reduce a per-thread integer over the workgroup, in index order
  auto total = [&](long long v) {
    s_cnt[tid] = v;
    __syncthreads();
    long long t = 0;
    if (tid == 0)
      for (int q = 0; q < kThreads; ++q) t += s_cnt[q];
    __syncthreads();
    return t;  // valid on thread 0
  };
  long long tp = 0, np_ = 0, nt = 0;
  for (int e = tid; e < E; e += kThreads) {
    const bool t = is_true(e), p = s_score[e] != 0.f;
    tp += (t && p) ? 1 : 0;
    np_ += p ? 1 : 0;
    nt += t ? 1 : 0;
  }
  const long long TP = total(tp), Pn = total(np_), Tn = total(nt);
  // ranking statistics: one true edge per thread and pass, all E scores swept from LDS (same address on every lane: broadcast)
  long long mw2 = 0;  // sum over true edges of 2 #(false edges with a smaller score) + #(false edges with an equal score)
  double ap = 0.0;
  for (int e = tid; e < E; e += kThreads) {
    if (!is_true(e)) continue;
    const float se = s_score[e];
    int lt = 0, eq = 0, ge_all = 0, ge_pos = 0;
    for (int w0 = 0; w0 < E; w0 += 32) {
      const unsigned bits = (unsigned)s_true[w0 >> 5];
      const int lim = (E - w0) < 32 ? (E - w0) : 32;
      for (int b = 0; b < lim; ++b) {
        const float sf = s_score[w0 + b];
        const bool t = (bits >> b) & 1u;
        lt += (!t && sf < se) ? 1 : 0;
        eq += (!t && sf == se) ? 1 : 0;
        ge_all += (sf >= se) ? 1 : 0;
        ge_pos += (t && sf >= se) ? 1 : 0;
      }
    }
    mw2 += 2LL * lt + eq;
    ap += (double)ge_pos / (double)ge_all;
  }
  const long long MW2 = total(mw2);
  s_dbl[tid] = ap;
  __syncthreads();
  if (tid == 0) {
    double AP = 0.0;
    for (int q = 0; q < kThreads; ++q) AP += s_dbl[q];
    const double dTP = (double)TP, dP = (double)Pn, dT = (double)Tn, dF = (double)E - dT;
    const double FP = dP - dTP, FN = dT - dTP;
    const double b2 = (double)beta * (double)beta;
    double* o = out + (size_t)blockIdx.x * 11;
    o[0] = FP / dP;
    o[1] = dTP / dT;
    o[2] = FP / dF;
    o[3] = FP + FN;
    o[4] = dT;
    o[5] = dP;
    o[6] = dTP / (dTP + FP);
    o[7] = dTP / (dTP + FN);
    o[8] = (1.0 + b2) * dTP / ((1.0 + b2) * dTP + b2 * FN + FP);
    o[9] = (Tn > 0 && dF > 0) ? AP / dT : __builtin_nan("");
    o[10] = (Tn > 0 && dF > 0) ? (double)MW2 / (2.0 * dT * dF) : __builtin_nan("");
  }
}

// the round-1 Jacobi solver, kept as an independent on-device cross-check of the divide & conquer path
template <int NT>
__global__ __launch_bounds__(kThreads) void symeig_jacobi_kernel(const float* __restrict__ A, float* __restrict__ U,
                                                                 float* __restrict__ beta, int D) {
  constexpr int DP = NT * 32, LD = DP + 1;
  __shared__ float sA[DP * LD];
  __shared__ float sV[DP * LD];
  __shared__ float s_t[DP / 2], s_s[DP / 2], s_h[DP / 2], s_red[8];
  __shared__ int s_flag;
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  for (int idx = tid; idx < DP * DP; idx += kThreads) {
    const int i = idx / DP, j = idx - i * DP;
    float v = 0.f;
    if (i < D && j < D) v = A[base + (i < j ? i * D + j : j * D + i)];
    sA[i * LD + j] = v;
    sV[i * LD + j] = (i == j) ? 1.f : 0.f;
  }
  __syncthreads();
  jacobi_eig<DP>(sA, sV, s_t, s_s, s_h, s_red, &s_flag);
  for (int idx = tid; idx < D * D; idx += kThreads) {
    const int i = idx / D, k = idx - i * D;
    U[base + idx] = sV[i * LD + k];
  }
  if (tid < D) beta[(size_t)blockIdx.x * D + tid] = sA[tid * LD + tid];
}

// ---- one translation unit per NT (the build of __graft_entry__.py): compiled with -DUGLAD_TU_NT=k this file emits ONLY the
// kernels templated on NT = k (explicit instantiations; the C ABI below is skipped), compiled with -DUGLAD_TU_HOST it emits
// everything else and merely declares those instantiations.  The units compile in parallel and link into one library.
// Without either macro (emulator and sanitizer builds) the file is one self-contained unit as before.
#define UGLAD_PER_NT_KERNELS(X, NT)                                                                                             \
  X void tridiag_kernel<NT, kThreads>(const float*, const float*, const float*, float*, float*, int, int, const int*);                  \
  X void cell_bwd_kernel<NT>(const float*, const float*, const float*, const float*, const float*, const float*, const float*, \
                             const float*, float*, float*, float*, float*, int, int, int, int, int);                            \
  X void init_inverse_kernel<NT>(const float*, const float*, float*, float*, int, int, const int*);                            \
  X void init_bwd_kernel<NT>(const float*, const float*, float*, float*, int);                                                 \
  X void loss_fwd_kernel<NT>(const float*, const float*, int, const float*, float*, float*, float*, int, const int*);          \
  X void cov_kernel<NT>(const float*, int, int, int, float*);                                                                  \
  X void map_solve_kernel<NT>(const float*, const float*, const float*, const float*, const float*, float*, float*, float*,   \
                              float*, int, int);                                                                                \
  X void support_metrics_kernel<NT>(const float*, const float*, double*, int, int);                                            \
  X void symeig_lean_kernel<NT>(float*, float*, const float*, float*, int);                                                    \
  X void cell_fwd_lean_kernel<NT>(const float*, const float*, const float*, const float*, float*, float*, float*, float*,     \
                                  float*, float*, const float*, float*, int, int, int, int, LamStep);
// the dL/dS variants (uglad_glad_backward_wrt_s) in translation units of their own (-DUGLAD_TU_GS): instantiated next to the kernels above
// they changed how the compiler treated cell_bwd_kernel<3> (80 instead of 78 SGPR spills, scripts/kernel_meta.py)
#define UGLAD_PER_NT_GS(X, NT)                                                                                                  \
  X void cell_bwd_gs_kernel<NT>(const float*, const float*, const float*, const float*, const float*, const float*, const float*, \
                                const float*, float*, float*, float*, float*, int, int, int, int, int, float*);                  \
  X void init_bwd_gs_kernel<NT>(const float*, const float*, float*, float*, int);
#define UGLAD_PER_NT_SMALL(X, NT)                                                                                       \
  X void symeig_jacobi_kernel<NT>(const float*, float*, float*, int);                                                  \
  X void chol_init_kernel<NT>(const float*, const float*, float*, int*, int, int);                                     \
  X void chol_loss_kernel<NT>(const float*, const float*, int, const float*, float*, float*, int*, int);
// D <= 96: the tridiagonalisation with 16 column groups as at D = 128 (128 NT threads) instead of 512 threads -- with 512 the chain wave gathers
// 512 / (DP / 4) partial sums per row, 64 at DP = 32, most of them zeros (profiles/r04_tridiag_small.txt)
#define UGLAD_PER_NT_TRISMALL(X, NT) \
  X void tridiag_kernel<NT, 128 * NT>(const float*, const float*, const float*, float*, float*, int, int, const int*);
// D <= 32: one wave per matrix, the matrix in its registers (tridiag_wave.h)
#define UGLAD_PER_NT_TRIWAVE(X, NT) X void tridiag_wave_kernel<NT>(const float*, const float*, const float*, float*, float*, int, int, const int*);
#define UGLAD_PER_NT_BIG(X, NT)                                                                             \
  X void tridiag_kernel<NT, 1024>(const float*, const float*, const float*, float*, float*, int, int, const int*); \
  X void cell_fwd_back_kernel<NT>(const float*, float*, const float*, float*, float*, int, int);
#ifdef UGLAD_STAMPS
#define UGLAD_PER_NT_DIAG(X, NT) X void symeig_stamp_kernel<NT>(float*, float*, float*, int, unsigned long long*);
#else
#define UGLAD_PER_NT_DIAG(X, NT)
#endif
#if defined(UGLAD_TU_NT) && defined(UGLAD_DEV_ONLY_LEAN)
// development (scripts/spill_check.sh): the forward cell's second stage alone, to read its register allocation in seconds
template __global__ void cell_fwd_lean_kernel<UGLAD_TU_NT>(const float*, const float*, const float*, const float*, float*, float*, float*,
                                                          float*, float*, float*, const float*, float*, int, int, int, int, LamStep);
#elif defined(UGLAD_TU_NT) && defined(UGLAD_DEV_ONLY_TRIDIAG)
template __global__ void tridiag_kernel<UGLAD_TU_NT, kThreads>(const float*, const float*, const float*, float*, float*, int, int, const int*);
#elif defined(UGLAD_TU_NT) && defined(UGLAD_DEV_ONLY_BWD)
template __global__ void cell_bwd_kernel<UGLAD_TU_NT>(const float*, const float*, const float*, const float*, const float*, const float*,
                                                     const float*, const float*, float*, float*, float*, float*, int, int, int, int, int);
#elif defined(UGLAD_TU_NT) && defined(UGLAD_DEV_ONLY_TRIWAVE)
UGLAD_PER_NT_TRIWAVE(template __global__, UGLAD_TU_NT)
#elif defined(UGLAD_TU_NT) && defined(UGLAD_DEV_ONLY_CHOL)
UGLAD_PER_NT_SMALL(template __global__, UGLAD_TU_NT)
#elif defined(UGLAD_TU_NT) && defined(UGLAD_TU_GS)
UGLAD_PER_NT_GS(template __global__, UGLAD_TU_NT)
#elif defined(UGLAD_TU_NT)
UGLAD_PER_NT_KERNELS(template __global__, UGLAD_TU_NT)
UGLAD_PER_NT_DIAG(template __global__, UGLAD_TU_NT)
#if UGLAD_TU_NT <= 4
UGLAD_PER_NT_SMALL(template __global__, UGLAD_TU_NT)
#if UGLAD_TU_NT <= 3
UGLAD_PER_NT_TRISMALL(template __global__, UGLAD_TU_NT)
#endif
#if UGLAD_TU_NT == 1
UGLAD_PER_NT_TRIWAVE(template __global__, UGLAD_TU_NT)
#endif
#else
UGLAD_PER_NT_BIG(template __global__, UGLAD_TU_NT)
#endif
#elif defined(UGLAD_TU_HOST)
#define UGLAD_DECLARE_NT(NT) UGLAD_PER_NT_KERNELS(extern template __global__, NT) UGLAD_PER_NT_DIAG(extern template __global__, NT) \
  UGLAD_PER_NT_GS(extern template __global__, NT)
UGLAD_DECLARE_NT(1) UGLAD_DECLARE_NT(2) UGLAD_DECLARE_NT(3) UGLAD_DECLARE_NT(4)
UGLAD_PER_NT_SMALL(extern template __global__, 1) UGLAD_PER_NT_SMALL(extern template __global__, 2)
UGLAD_PER_NT_SMALL(extern template __global__, 3) UGLAD_PER_NT_SMALL(extern template __global__, 4)
UGLAD_PER_NT_TRISMALL(extern template __global__, 1) UGLAD_PER_NT_TRISMALL(extern template __global__, 2) UGLAD_PER_NT_TRISMALL(extern template __global__, 3)
UGLAD_PER_NT_TRIWAVE(extern template __global__, 1)
UGLAD_DECLARE_NT(5) UGLAD_DECLARE_NT(6) UGLAD_DECLARE_NT(7) UGLAD_DECLARE_NT(8)
UGLAD_PER_NT_BIG(extern template __global__, 5) UGLAD_PER_NT_BIG(extern template __global__, 6)
UGLAD_PER_NT_BIG(extern template __global__, 7) UGLAD_PER_NT_BIG(extern template __global__, 8)
#endif

}  // namespace uglad

#ifndef UGLAD_TU_NT
// =============================================================================================== C ABI
using namespace uglad;

// UGLAD_MAX_NT (default 8): the largest instantiated NT = ceil(D / 32).  Test builds (sanitizer, emulator) lower it to keep their
// compile time down; UGLAD_NO_BIG is the older spelling of UGLAD_MAX_NT=4.
#ifndef UGLAD_MAX_NT
#ifdef UGLAD_NO_BIG
#define UGLAD_MAX_NT 4
#else
#define UGLAD_MAX_NT 8
#endif
#endif
#define UGLAD_MAX_EIG_DIM (32 * UGLAD_MAX_NT)  // the spectral path: eigensolver, LDS / slab-resident kernels templated on NT
#define UGLAD_MAX_DIM (kNsMaxD > UGLAD_MAX_EIG_DIM ? kNsMaxD : UGLAD_MAX_EIG_DIM)  // beyond it the matrix-iteration path (wide_ns.h)
// cond(b^T b + 4/lam I) up to which reference-made goldens sit inside the 1e-4 tolerance on Theta (tests/golden/regime_sweep.json:
// every case up to cond 708 within 1.1e-5 of the fp64 value of its own function; the min-max-normalised fit that runs to convergence,
// tests/golden/fit_direct_converged.npz, reaches 1.03e3 with precision_ 2.0e-5 from the reference; the case at 4.4e3 is 1.04e-4 off:
// DESIGN.md section 2).  Round 3 had 1000 here, BELOW a case its own goldens validate -- that fit warned.
#define UGLAD_VALIDATED_COND 1500.0f

static inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// UGLAD_NT_MASK (test builds only: bit k set = NT = k is instantiated; default all): the sanitizer build compiles just the padded
// sizes its script uses, which halves its compile time.  A size that is masked out is refused like one beyond UGLAD_MAX_DIM.
#ifndef UGLAD_NT_MASK
#define UGLAD_NT_MASK 0x1fe
#endif
#define UGLAD_HAS_NT(k) (((UGLAD_NT_MASK) >> (k)) & 1)
#define CHECK_DIMS_EIG(M, D) /* entry points that exist on the spectral path only */ \
  do {                                                    \
    if ((M) < 1 || (D) < 1 || (D) > UGLAD_MAX_EIG_DIM || !UGLAD_HAS_NT(((D) + 31) / 32)) return UGLAD_E_DIM; \
  } while (0)
#define CHECK_DIMS(M, D) /* the path itself: any D up to UGLAD_MAX_DIM */ \
  do {                                                    \
    if ((M) < 1 || (D) < 1 || (D) > UGLAD_MAX_DIM || ((D) <= UGLAD_MAX_EIG_DIM && !UGLAD_HAS_NT(((D) + 31) / 32))) return UGLAD_E_DIM; \
    if (((D) > UGLAD_MAX_EIG_DIM || ns_wanted(D)) && (M) > kNsMaxBatch) return UGLAD_E_DIM; \
  } while (0)
// (the matrix iteration's launches carry matrix x product, up to three products, in one grid dimension of at most 65535)
constexpr int kNsMaxBatch = 65535 / 3;
static bool ns_wanted(int D);

// dispatch on NT = ceil(D / 32): every padded size has its own instantiation; beyond NT = 4 (D > 128) the kernels keep their
// two D x D buffers in the caller's workspace instead of LDS
#if UGLAD_HAS_NT(1)
#define DISPATCH_NT1(...) case 1: { constexpr int NT = 1; __VA_ARGS__; } break;
#else
#define DISPATCH_NT1(...)
#endif
#if UGLAD_HAS_NT(2)
#define DISPATCH_NT2(...) case 2: { constexpr int NT = 2; __VA_ARGS__; } break;
#else
#define DISPATCH_NT2(...)
#endif
#if UGLAD_HAS_NT(3)
#define DISPATCH_NT3(...) case 3: { constexpr int NT = 3; __VA_ARGS__; } break;
#else
#define DISPATCH_NT3(...)
#endif
#if UGLAD_HAS_NT(4)
#define DISPATCH_NT4(...) case 4: { constexpr int NT = 4; __VA_ARGS__; } break;
#else
#define DISPATCH_NT4(...)
#endif
#if UGLAD_MAX_NT >= 5 && UGLAD_HAS_NT(5)
#define DISPATCH_NT5(...) case 5: { constexpr int NT = 5; __VA_ARGS__; } break;
#else
#define DISPATCH_NT5(...)
#endif
#if UGLAD_MAX_NT >= 6 && UGLAD_HAS_NT(6)
#define DISPATCH_NT6(...) case 6: { constexpr int NT = 6; __VA_ARGS__; } break;
#else
#define DISPATCH_NT6(...)
#endif
#if UGLAD_MAX_NT >= 7 && UGLAD_HAS_NT(7)
#define DISPATCH_NT7(...) case 7: { constexpr int NT = 7; __VA_ARGS__; } break;
#else
#define DISPATCH_NT7(...)
#endif
#if UGLAD_MAX_NT >= 8 && UGLAD_HAS_NT(8)
#define DISPATCH_NT8(...) case 8: { constexpr int NT = 8; __VA_ARGS__; } break;
#else
#define DISPATCH_NT8(...)
#endif
#define DISPATCH_NT(D, ...)          \
  switch (((D) + 31) / 32) {          \
    DISPATCH_NT1(__VA_ARGS__) DISPATCH_NT2(__VA_ARGS__) DISPATCH_NT3(__VA_ARGS__) DISPATCH_NT4(__VA_ARGS__) \
    DISPATCH_NT5(__VA_ARGS__) DISPATCH_NT6(__VA_ARGS__) DISPATCH_NT7(__VA_ARGS__) DISPATCH_NT8(__VA_ARGS__) \
    default: break; /* unreachable: CHECK_DIMS */ \
  }
#define DISPATCH_NT_SMALL(D, ...) /* kernels instantiated for NT <= 4 only */ \
  switch (((D) + 31) / 32) {          \
    DISPATCH_NT1(__VA_ARGS__) DISPATCH_NT2(__VA_ARGS__) DISPATCH_NT3(__VA_ARGS__) DISPATCH_NT4(__VA_ARGS__) \
    default: break; \
  }
static inline int padded_dim(int D) { return ((D + 31) / 32) * 32; }
static inline long long big_floats_rt(int DP) { return 2LL * (((long long)DP * (DP + 1) + 3) & ~3LL); }  // = big_floats<DP>()

static std::atomic<int> g_wide_mode{-2};  // -2: not set (UGLAD_WIDE_BWD in the environment decides, else automatic); -1 auto, 0 never, 1 always

extern "C" {

int uglad_version(void) { return 3; }
float uglad_validated_cond(void) { return UGLAD_VALIDATED_COND; }
int uglad_set_wide_mode(int mode) {
  if (mode < -1 || mode > 1) return UGLAD_E_MODE;
  g_wide_mode.store(mode, std::memory_order_relaxed);
  return 0;
}
int uglad_max_dim(void) { return UGLAD_MAX_DIM; }
int uglad_max_eig_dim(void) { return UGLAD_MAX_EIG_DIM; }

// The matrix-iteration path (wide_ns.h).  Modes: -1 automatic (below), 0 only beyond the eigensolver's size, 1 for every D (tests, A/B
// measurements).  UGLAD_MATRIX_ITERATION=0/1 in the environment presets it when nothing was set.
// Automatic: beyond the eigensolver's size always; and for FEW matrices of 128 < D <= 256, where one workgroup's Householder chain is
// most of the spectral cell while the iteration's products use the whole chip -- measured over a grid of (D, batch), ms per 15-step pass
// spectral vs iteration (profiles/r03_ns_crossover.txt): training D = 256: 1 matrix 16.9 vs 9.4, 6: 17.3 vs 15.4, 8: 17.5 vs 18.6; D = 192:
// 8: 12.5 vs 12.2, 16: 12.7 vs 18.1; D = 160: 8: 11.3 vs 10.0; forward only D = 256: 1: 15.5 vs 4.2, 16: 16.1 vs 9.7, 64: 17.2 vs 27.7.
// Only for UGLAD_SQRT_NS10.
static std::atomic<int> g_ns_mode{-2};
int uglad_set_matrix_iteration(int mode) {
  if (mode < -1 || mode > 1) return UGLAD_E_MODE;
  g_ns_mode.store(mode, std::memory_order_relaxed);
  return 0;
}
static int ns_mode() {
  int mode = g_ns_mode.load(std::memory_order_relaxed);
  if (mode == -2) {
    const char* e = std::getenv("UGLAD_MATRIX_ITERATION");
    const int env_mode = (e && e[0] == '1') ? 1 : ((e && e[0] == '0') ? 0 : -1);
    int expected = -2;
    mode = g_ns_mode.compare_exchange_strong(expected, env_mode, std::memory_order_relaxed) ? env_mode : expected;
  }
  return mode;
}
// forced for this size whatever the batch: by the mode, or because no eigensolver exists
static bool ns_wanted(int D) { return ns_mode() == 1 || D > UGLAD_MAX_EIG_DIM; }
// Theta_0, its gradient and the loss's logdet / inverse on the factorisation of wide_ns.h (L D L^T + Newton steps) instead of the
// eigensolver: wherever there is none, and for the few large matrices the cell itself takes to the matrix-iteration path (one
// 256 x 256 matrix: 0.35 ms against 0.9 ms for the eigen path's tridiagonalisation, merges, back-transformation and products)
static bool ns_path(int M, int D, bool training, int sqrt_mode);
static bool ns_factorisation(int M, int D) {
  return D > UGLAD_MAX_EIG_DIM || (D > 128 && (ns_path(M, D, true, UGLAD_SQRT_NS10) || ns_path(M, D, false, UGLAD_SQRT_NS10)));
}
// the products' all-chunks-in-flight form (wide_ns.h, PRE): D <= 4 k chunks of the 32 x 32 tiling; UGLAD_NS_PREFETCH_ALL=0 in the environment: off (A/B)
static bool ns_prefetch_all(int D) {
  const char* e = std::getenv("UGLAD_NS_PREFETCH_ALL");
  return D <= 4 * NsTile<32>::kK && !(e && e[0] == '0');
}
// the path of a cell call: training = the call saves state for a backward pass (which must take the same path)
static bool ns_path(int M, int D, bool training, int sqrt_mode) {
  if (ns_wanted(D)) return true;
  if (ns_mode() != -1 || sqrt_mode != UGLAD_SQRT_NS10 || D <= 128) return false;
  const long long tiles = (long long)M * wide_tiles(D) * wide_tiles(D);
  return training ? (tiles <= 96 && M <= 8) : tiles <= 256;
}
extern "C" int uglad_cond_is_upper_bound(int M, int D, int training, int sqrt_mode) {
  if (M < 1 || D < 1 || D > UGLAD_MAX_DIM) return UGLAD_E_DIM;
  return ns_path(M, D, training != 0, sqrt_mode) ? 1 : 0;
}
// per matrix: the header every path uses and, behind all headers, this matrix's region: kNsSlabs D x D fp64 slabs and one fp32 slab
// (G_half) -- or, for the factorisations beyond the eigensolver's size, the three padded fp32 slabs of the L D L^T inverse and one more
// D x D for the Newton steps' residual, whichever is larger
struct NsLayout {
  size_t hdr, region;  // floats
  size_t dslab, dregion;  // doubles: one slab, one matrix's region
  float* H;
  float* W;    // region of matrix m: W + m * region
  double* Wd;  // the same as fp64: slab s of matrix m at Wd + m * dregion + s * dslab
  float* Gh;   // the fp32 slab of matrix m: Gh + m * region
};
static NsLayout ns_layout(float* workspace, int M, int D) {
  const int DP = padded_dim(D);
  NsLayout l;
  l.hdr = 3 * (size_t)DP + (size_t)(DP / 32) * 1024;
  // (the header also holds this path's per-tile sums and scalars, wide_ns.h: past D = 1900 they outgrow the size the other paths' layout gives it)
  const size_t need = (size_t)ns_off_dbl(D) + 2 * ((size_t)ns_tiles_max(D) + 4 + (size_t)wide_tiles(D)) + 8;
  if (need > l.hdr) l.hdr = (need + 3) & ~(size_t)3;
  l.dslab = (size_t)D * D;
  l.region = 2 * kNsSlabs * l.dslab + l.dslab;
  const size_t fact = 3 * (size_t)ns_fact_dim(D) * (ns_fact_dim(D) + 1) + l.dslab;
  if (D > 128 && fact > l.region) l.region = fact;  // (D <= 128: Theta_0 and the loss use the LDS Cholesky kernels on every path)
  l.region = (l.region + 3) & ~(size_t)3;  // (16-byte granularity: vector loads of the slabs)
  l.dregion = l.region / 2;
  l.H = workspace;
  l.W = workspace ? workspace + (size_t)M * l.hdr : nullptr;
  l.Wd = reinterpret_cast<double*>(l.W);
  l.Gh = l.W ? l.W + 2 * kNsSlabs * l.dslab : nullptr;
  return l;
}
int uglad_workspace_floats(int M, int D) {
  if (M < 1 || D < 1 || D > UGLAD_MAX_DIM) return UGLAD_E_DIM;
  const int DP = padded_dim(D);
  long long n = 0;
  if (D <= UGLAD_MAX_EIG_DIM) n = (long long)M * (3 * DP + (DP / 32) * 1024) + (DP > 128 ? (long long)M * big_floats_rt(DP) : 0);
  if (ns_path(M, D, true, UGLAD_SQRT_NS10) || ns_path(M, D, false, UGLAD_SQRT_NS10)) {  // (either kind of call may take the matrix-iteration path at this shape)
    const NsLayout l = ns_layout(nullptr, M, D);
    const long long nn = (long long)M * (long long)(l.hdr + l.region);
    if (nn > n) n = nn;
  }
  return n > 2147483647LL ? UGLAD_E_DIM : (int)n;
}

// Groups: the batch may consist of G independent problems of M / G consecutive matrices each, every one with its own 42
// parameters and its own lambda sequence (the folds of CV mode in one launch: uglad_glad_forward_grouped).  The per-step
// entry points keep their single-group meaning; the grouped whole-pass calls set the group count for their duration.
static thread_local int t_groups = 1;
struct GroupScope {
  int saved;
  explicit GroupScope(int g) : saved(t_groups) { t_groups = g; }
  ~GroupScope() { t_groups = saved; }
};
static inline int group_size(int M) { return M / t_groups > 0 ? M / t_groups : 1; }

// the tridiagonalisation launch every eigendecomposition starts with (tridiag.h); R = the D x D slab of each matrix that
// will receive that matrix's final output
#define LAUNCH_TRIDIAG(A0, A1, LAMP, RBASE, TRI) LAUNCH_TRIDIAG_IF(A0, A1, LAMP, RBASE, TRI, (const int*)nullptr)
/* ONLY: per-matrix flags (0 = skip this matrix) or nullptr = all */
// UGLAD_TRIDIAG_SMALL=0 in the environment: 512 threads also for D <= 96 (A/B measurements)
static bool tridiag_small_enabled() {  // (8 column groups, 64 NT threads, measured as well: slower at every size, profiles/r04_tridiag_small.txt)
  static const bool on = [] {
    const char* e = std::getenv("UGLAD_TRIDIAG_SMALL");
    return !(e && e[0] == '0');
  }();
  return on;
}
// UGLAD_TRIDIAG_WAVE=0: the workgroup kernel also for D <= 64 (A/B measurements; read on every call: tests flip it)
static bool tridiag_wave_enabled() {
  const char* e = std::getenv("UGLAD_TRIDIAG_WAVE");
  return !(e && e[0] == '0');
}
#define LAUNCH_TRIDIAG_IF(A0, A1, LAMP, RBASE, TRI, ONLY)                                                                     \
  DISPATCH_NT(D, if constexpr (NT == 1) {                                                                                     \
    if (tridiag_wave_enabled()) { /* one wave per matrix, no barriers (tridiag_wave.h; NT = 2 measured slower) */             \
      hipLaunchKernelGGL((tridiag_wave_kernel<NT>), dim3(M), dim3(64), 0, st, A0, A1, LAMP, RBASE, TRI, D, group_size(M), ONLY); \
      break;                                                                                                                  \
    }                                                                                                                         \
  } if constexpr (NT <= 3) {                                                                                                  \
    if (tridiag_small_enabled()) {                                                                                            \
      hipLaunchKernelGGL((tridiag_kernel<NT, 128 * NT>), dim3(M), dim3(128 * NT), 0, st, A0, A1, LAMP, RBASE, TRI, D,         \
                         group_size(M), ONLY);                                                                                \
      break;                                                                                                                  \
    }                                                                                                                         \
  } if constexpr (NT > 4) {                                                                                                   \
    if (M <= 256) { /* few large matrices: one workgroup per CU anyway, 1024 threads hide the sweep's latency (tridiag.h) */  \
      hipLaunchKernelGGL((tridiag_kernel<NT, 1024>), dim3(M), dim3(1024), 0, st, A0, A1, LAMP, RBASE, TRI, D, group_size(M),  \
                         ONLY);                                                                                               \
      break;                                                                                                                  \
    }                                                                                                                         \
  } hipLaunchKernelGGL((tridiag_kernel<NT, kThreads>), dim3(M), dim3(kThreads), 0, st, A0, A1, LAMP, RBASE, TRI, D,           \
                       group_size(M), ONLY))

// D <= 128: Theta_0 and the loss's logdet / inverse by blocked Cholesky (chol.h); the eigen path follows only for matrices the
// Cholesky kernel flagged (not positive definite, NaN).  UGLAD_CHOLESKY=0 in the environment: the eigen path for all (A/B measurements).
static bool cholesky_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("UGLAD_CHOLESKY");
    return !(e && e[0] == '0');
  }();
  return on;
}
// UGLAD_PERSISTENT_BWD=0: one launch per step of the backward pass also for D <= 128 (read on every call: tests flip it)
static bool persistent_bwd_enabled() {
  const char* e = std::getenv("UGLAD_PERSISTENT_BWD");
  return !(e && e[0] == '0');
}
// the per-matrix flags live at the head of the workspace region the forward cell uses for its triangular factors (idle here)
static int* chol_flags(float* workspace, int M, int D) { return reinterpret_cast<int*>(workspace + (size_t)M * 3 * padded_dim(D)); }

static bool wide_wanted(int M, int D);
static void launch_ns_inverse(const float* A, const float* shift, int shift_stride, float* out, float* logdet_out, float* workspace, int M, int D,
                              hipStream_t st);
static void launch_wide_inverse(const float* A, const float* shift, int shift_stride, float* out, float* workspace, int M, int D,
                                hipStream_t st);

int uglad_init_theta(const float* S, const float* params, int init_diag, float* theta0, float* workspace, int M, int D,
                     uglad_stream_t stream) {
  if (!S || !params || !theta0 || (init_diag == 0 && !workspace)) return UGLAD_E_NULL;
  CHECK_DIMS(M, D);
  hipStream_t st = (hipStream_t)stream;
  if (init_diag == 1) {
    const size_t total = (size_t)M * D * D;
    const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(init_diag_kernel, dim3(grid), dim3(256), 0, st, S, params, theta0, D, total, group_size(M));
  } else if (init_diag == 0 && ns_factorisation(M, D)) {
    launch_ns_inverse(S, params + P_T, kNParam, theta0, nullptr, workspace, M, D, st);
  } else if (init_diag == 0) {
    const int* only = nullptr;
    if (D <= 128 && cholesky_enabled()) {
      int* flags = chol_flags(workspace, M, D);
      DISPATCH_NT_SMALL(D, hipLaunchKernelGGL((chol_init_kernel<NT>), dim3(M), dim3(kThreads), 0, st, S, params, theta0, flags, D,
                                              group_size(M)));
      only = flags;
    }
    LAUNCH_TRIDIAG_IF(S, (const float*)nullptr, (const float*)nullptr, theta0, workspace, only);
    if (wide_wanted(M, D)) {
      launch_wide_inverse(S, params + P_T, kNParam, theta0, workspace, M, D, st);
    } else {
      DISPATCH_NT(D, hipLaunchKernelGGL((init_inverse_kernel<NT>), dim3(M), dim3(kThreads), 0, st, S, params, theta0,
                                        workspace, D, group_size(M), only));
    }
  } else {
    return UGLAD_E_MODE;
  }
  return launch_status();
}

int uglad_init_theta_bwd(const float* theta0, const float* G0, int init_diag, float* gt_partial, float* workspace, int M,
                         int D, uglad_stream_t stream) {
  if (!theta0 || !G0 || !gt_partial || (D > 128 && init_diag == 0 && !workspace)) return UGLAD_E_NULL;
  CHECK_DIMS(M, D);
  hipStream_t st = (hipStream_t)stream;
  if (init_diag == 1) {
    hipLaunchKernelGGL(init_bwd_diag_kernel, dim3(M), dim3(kThreads), 0, st, theta0, G0, gt_partial, D);
  } else if (init_diag == 0 && ns_factorisation(M, D)) {  // gt_partial = -<G0^T, Theta0 Theta0>, one workgroup per tile of the product
    const NsLayout l = ns_layout(workspace, M, D);
    const int nt = wide_tiles(D);
    WideFwd fw{};
    fw.X = G0;
    fw.x_stride = (size_t)D * D;
    hipLaunchKernelGGL((wide_gemm_kernel<false, false, kEpiDotT>), dim3(nt, nt, M), dim3(kWThreads), 0, st, theta0, (size_t)D * D, theta0,
                       (size_t)D * D, (float*)nullptr, (size_t)0, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, l.H,
                       l.hdr, ns_off_tiles(D), D, 0, group_size(M), D, D, D, fw);
    hipLaunchKernelGGL(ns_tile_sum_kernel, dim3((M + 63) / 64), dim3(64), 0, st, (const float*)l.H, l.hdr, gt_partial, -1.f, M, D);
  } else if (init_diag == 0) {
    DISPATCH_NT(D, hipLaunchKernelGGL((init_bwd_kernel<NT>), dim3(M), dim3(kThreads), 0, st, theta0, G0, gt_partial, workspace,
                                      D));
  } else {
    return UGLAD_E_MODE;
  }
  return launch_status();
}

int uglad_lambda_init(const float* params, float lambda_init, float* lam_out, float* lam_in, uglad_stream_t stream) {
  if (!params || !lam_out || !lam_in) return UGLAD_E_NULL;
  hipLaunchKernelGGL(lambda_init_kernel, dim3((t_groups + 63) / 64), dim3(64), 0, (hipStream_t)stream, params, lambda_init,
                     lam_out, lam_in, t_groups);
  return launch_status();
}

// Few, large matrices: many workgroups per matrix (wide_bwd.h) -- the backward cell as six short launches, the forward cell's
// part after the eigen-decomposition as one.  Taken when one workgroup per
// matrix would leave most of the chip idle; UGLAD_WIDE_BWD=0 / 1 in the environment forces the choice for D > 128 (A/B, tests).
static bool wide_wanted(int M, int D) {
  if (D <= 128) return false;
  int mode = g_wide_mode.load(std::memory_order_relaxed);
  if (mode == -2) {  // unset: the environment decides, once -- and never over a value uglad_set_wide_mode() stored meanwhile
    const char* e = std::getenv("UGLAD_WIDE_BWD");
    const int env_mode = e ? (e[0] == '0' ? 0 : 1) : -1;
    int expected = -2;
    mode = g_wide_mode.compare_exchange_strong(expected, env_mode, std::memory_order_relaxed) ? env_mode : expected;
  }
  // measured (scripts/bench_bwd_wide.py): D = 256 wide wins at every batch size (82 vs 775 us at M = 1, 1.6 vs 2.1 ms at M = 512);
  // D = 160: 70 vs 216 us at M = 8, 315 vs 273 us at M = 256
  return mode >= 0 ? mode == 1 : (D > 192 || M <= 128);
}

// Few large matrices: the eigen-decomposition after the single-workgroup front (tridiagonalisation and merges below the last one have
// run; reflectors in the slab R of each matrix): secular roots and eigenvector update of the last merge with many workgroups per
// matrix (wide_fwd.h), back-transformation on two.  Leaves U in the matrix's second slab (row stride DP + 1) and the eigenvalues
// in place of d in its (d, e, tau) record.
static void launch_wide_eig_tail(float* workspace, const float* R, float* U_out, float* beta_out, int M, int D, hipStream_t st) {
  const int DPr = padded_dim(D), ntp = wide_tiles(DPr), LD = DPr + 1;
  const size_t rec = 3 * (size_t)DPr, slab = (size_t)big_floats_rt(DPr), lrec = (size_t)(DPr / 32) * 1024;
  float* Tws = workspace + (size_t)M * 3 * DPr;
  float* Q0 = workspace + (size_t)M * (3 * DPr + (DPr / 32) * 1024);  // eigenvectors before the last merge
  float* Q1 = Q0 + slab / 2;                                            // ... after it, then back-transformed in place: U
  hipLaunchKernelGGL(wide_secular_kernel, dim3((D + kWThreads / 8 - 1) / (kWThreads / 8), M), dim3(kWThreads), 0, st, Tws, lrec,
                     workspace, rec, D, DPr);
  hipLaunchKernelGGL(wide_merge_kernel, dim3(ntp, ntp, M), dim3(kWThreads), 0, st, (const float*)Q0, Q1, slab, (const float*)Tws,
                     lrec, D, DPr, LD);
  switch (DPr / 32) {
#define UGLAD_BACK_CASE(K)                                                                                                   \
  case K:                                                                                                                    \
    hipLaunchKernelGGL((cell_fwd_back_kernel<K>), dim3((K * 2 + kWaves - 1) / kWaves, M), dim3(kThreads), 0, st,            \
                       (const float*)workspace, Tws, R, U_out, beta_out, D, M);                                              \
    break;
#if UGLAD_MAX_NT >= 5 && UGLAD_HAS_NT(5)
    UGLAD_BACK_CASE(5)
#endif
#if UGLAD_MAX_NT >= 6 && UGLAD_HAS_NT(6)
    UGLAD_BACK_CASE(6)
#endif
#if UGLAD_MAX_NT >= 7 && UGLAD_HAS_NT(7)
    UGLAD_BACK_CASE(7)
#endif
#if UGLAD_MAX_NT >= 8 && UGLAD_HAS_NT(8)
    UGLAD_BACK_CASE(8)
#endif
#undef UGLAD_BACK_CASE
    default: break;
  }
}

// The same for a plain symmetric matrix whose tridiagonalisation has just been enqueued (LAUNCH_TRIDIAG(A, ..., out, workspace)), and
// then out = (A + shift I)^-1 = U diag(1 / (beta + shift)) U^T with one Newton step, every product with one workgroup per 64 x 64 tile.
// shift: device scalar per group with stride shift_stride floats, or nullptr.
static void launch_wide_inverse(const float* A, const float* shift, int shift_stride, float* out, float* workspace, int M, int D,
                                hipStream_t st) {
  const int DPr = padded_dim(D), nt = wide_tiles(D), LD = DPr + 1, gs = group_size(M);
  const size_t rec = 3 * (size_t)DPr, slab = (size_t)big_floats_rt(DPr), dd = (size_t)D * D;
  float* Tws = workspace + (size_t)M * 3 * DPr;
  float* Q0 = workspace + (size_t)M * (3 * DPr + (DPr / 32) * 1024);
  float* Q1 = Q0 + slab / 2;
  // front: everything below the last merge, one workgroup per matrix (the cell's kernel in its split mode; it only touches the
  // workspace then, the other pointers just have to be valid)
  DISPATCH_NT(D, hipLaunchKernelGGL((cell_fwd_lean_kernel<NT>), dim3(M), dim3(kThreads), 0, st, A, A, (const float*)workspace,
                                    (const float*)workspace, out, (float*)nullptr, (float*)nullptr, (float*)nullptr, workspace,
                                    (float*)nullptr, (const float*)workspace, Tws, D, UGLAD_SQRT_EXACT, gs, 2, LamStep{}));
  launch_wide_eig_tail(workspace, out, nullptr, nullptr, M, D, st);
  const WideFwd nofw{nullptr, nullptr, nullptr, nullptr};
  const dim3 tiles(nt, nt, M), blk(kWThreads);
  hipLaunchKernelGGL((wide_gemm_kernel<false, true, kEpiInverse>), tiles, blk, 0, st, (const float*)Q1, slab, (const float*)Q1, slab, Q0,
                     slab, (const float*)nullptr, (const float*)workspace, shift, (float*)nullptr, rec, shift_stride, D, 0, gs, LD, LD,
                     LD, nofw);  // X0 = U f U^T -> first slab
  hipLaunchKernelGGL((wide_gemm_kernel<false, false, kEpiResidual>), tiles, blk, 0, st, A, dd, (const float*)Q0, slab, Q1, slab,
                     (const float*)nullptr, (const float*)nullptr, shift, (float*)nullptr, rec, shift_stride, D, 0, gs, D, LD, LD,
                     nofw);  // E = I - (A + shift I) X0 -> second slab (U is dead)
  hipLaunchKernelGGL((wide_gemm_kernel<false, false, kEpiNewton>), tiles, blk, 0, st, (const float*)Q0, slab, (const float*)Q1, slab, out,
                     dd, (const float*)nullptr, (const float*)nullptr, shift, (float*)nullptr, rec, shift_stride, D, 0, gs, LD, LD, D,
                     nofw);  // out = X0 + X0 E
}

static int launch_cell_bwd_wide(const float* G_next, const float* S, const float* Z_in, const float* half, const float* U,
                                const float* beta, const float* lam, const float* params, float* G_out, float* grad_rho_partial,
                                float* glam_partial, float* workspace, int M, int D, int sqrt_mode, hipStream_t st) {
  const int DP = padded_dim(D), nt = wide_tiles(D), nup = kWQ * (nt * (nt + 1) / 2), gs = group_size(M);  // nup: phase-A workgroups per matrix
  const size_t pstride = 3 * (size_t)DP + (size_t)(DP / 32) * 1024;  // = kWsPerMatrix<DP>: the region the forward's d, e, tau, T factors use
  const size_t slab = (size_t)big_floats_rt(DP), dd = (size_t)D * D;
  float* part = workspace;
  float* X0 = workspace + (size_t)M * pstride;
  float* X1 = X0 + slab / 2;
  const dim3 tiles(nt, nt, M), blk(kWThreads);
  const WideFwd nofw{nullptr, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(wide_phase_a_kernel, dim3(nup, M), blk, 0, st, G_next, S, Z_in, half, params, X0, G_out, part, D, gs, slab,
                     pstride);
  hipLaunchKernelGGL((wide_gemm_kernel<true, false, kEpiStore>), tiles, blk, 0, st, U, dd, (const float*)X0, slab, X1, slab,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (size_t)0, 0, D, sqrt_mode,
                     gs, D, D, D, nofw);  // R = U^T G_half
  hipLaunchKernelGGL((wide_gemm_kernel<false, false, kEpiDivDiff>), tiles, blk, 0, st, (const float*)X1, slab, U, dd, X0, slab,
                     (const float*)nullptr, beta, lam, part, pstride, nup * kNRho, D, sqrt_mode, gs, D, D, D, nofw);  // Y = (R U) o F
  hipLaunchKernelGGL((wide_gemm_kernel<false, false, kEpiStore>), tiles, blk, 0, st, U, dd, (const float*)X0, slab, X1, slab,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (size_t)0, 0, D, sqrt_mode,
                     gs, D, D, D, nofw);  // T2 = U Y
  hipLaunchKernelGGL((wide_gemm_kernel<false, true, kEpiGout>), tiles, blk, 0, st, (const float*)X1, slab, U, dd, G_out, dd, S,
                     (const float*)nullptr, lam, part, pstride, nup * kNRho + nt * nt, D, sqrt_mode, gs, D, D, D, nofw);  // G_out -= T2 U^T
  hipLaunchKernelGGL(wide_reduce_kernel, dim3(M, kNRho + 1), dim3(64), 0, st, (const float*)part, pstride, grad_rho_partial, glam_partial, D);
  return launch_status();
}


// ---- the matrix-iteration path (wide_ns.h): launch sequences
static inline dim3 ns_ew_grid(int M, int D) {
  const size_t dd = (size_t)D * D;
  return dim3((unsigned)((dd + 255) / 256 < 256 ? (dd + 255) / 256 : 256), (unsigned)M);
}
// output tile of the products: 64 x 64, or 32 x 32 while the 64 x 64 tiles of the batch would not fill the 256 CUs (one 512 x 512
// matrix: 64 workgroups; 45.8 vs 19.4 us per product, profiles/r03_ns_kernel_stats_d512_tile{64,32}.csv; the two tilings meet at 256
// tiles of 64 x 64: D = 256 with 16 matrices 39.8 vs 39.1 ms per pass, D = 512 with 4: 66.2 vs 69.5, profiles/r03_ns_tile_probe.txt)
static inline int ns_tile(int M, int D) {
  if (const char* e = std::getenv("UGLAD_NS_TILE")) {  // (tests, A/B: read on every call)
    if (e[0] == '3') return 32;
    if (e[0] == '6') return 64;
  }
  return (long long)M * wide_tiles(D) * wide_tiles(D) < 256 ? 32 : 64;
}
static inline int ns_tiles_per_dim(int M, int D) { return ns_tile(M, D) == 32 ? (D + 31) / 32 : wide_tiles(D); }
// one launch of up to three independent products C = alpha op(A) B + beta C + gamma I (fp64; ta: A is read transposed)
struct NsLaunch {
  NsBatch b{};
  NsLaunch& add(const double* A, const double* B, double* C, double alpha, double beta, double gamma, bool ta = false) {
    b.p[b.n++] = NsProd{A, B, C, alpha, beta, gamma, ta ? 1 : 0};
    return *this;
  }
};
static void ns_products(hipStream_t st, const NsLayout& l, int M, int D, const NsLaunch& nl, const float* gamma_div = nullptr, bool frob = false) {
  NsEpi ep{};
  ep.gamma_div = gamma_div;
  ep.hdr = frob ? l.H : nullptr;
  ep.hdr_stride = l.hdr;
  ep.gs = group_size(M);
  // (the tiling follows the batch alone, not the products per launch: per-tile sums and their readers agree on it)
  if (ns_tile(M, D) == 32) {
    const int n32 = (D + 31) / 32;
    if (ns_prefetch_all(D))
      hipLaunchKernelGGL((ns_gemm64_kernel<kNsAffine, 32, true>), dim3(n32, n32, M * nl.b.n), dim3(kWThreads), 0, st, nl.b, l.dregion, D, ep);
    else
      hipLaunchKernelGGL((ns_gemm64_kernel<kNsAffine, 32>), dim3(n32, n32, M * nl.b.n), dim3(kWThreads), 0, st, nl.b, l.dregion, D, ep);
  } else {
    const int nt = wide_tiles(D);
    hipLaunchKernelGGL((ns_gemm64_kernel<kNsAffine, 64>), dim3(nt, nt, M * nl.b.n), dim3(kWThreads), 0, st, nl.b, l.dregion, D, ep);
  }
}

static int launch_cell_fwd_ns(const float* S, const float* Z_in, const float* lam, const float* params, float* Z_out, float* half_out,
                              float* sqrt_out, float* normF_partial, float* cond_max, float* workspace, int M, int D, hipStream_t st) {
  const NsLayout l = ns_layout(workspace, M, D);
  const int nt = wide_tiles(D), gs = group_size(M);
  double* Wb = l.Wd;                  // b
  double* Wy = l.Wd + 1 * l.dslab;    // A -> Y
  double* Wt = l.Wd + 2 * l.dslab;    // T
  double* Wz = l.Wd + 3 * l.dslab;    // Z
  double* Wy2 = l.Wd + 4 * l.dslab;   // the next Y
  double* Wz2 = l.Wd + 5 * l.dslab;   // the next Z
  const dim3 ew = ns_ew_grid(M, D);
  hipLaunchKernelGGL(ns_b_kernel, ew, dim3(256), 0, st, S, Z_in, lam, Wb, l.dregion, D, gs);
  ns_products(st, l, M, D, NsLaunch().add(Wb, Wb, Wy, 1.0, 0.0, 4.0, true), lam, true);  // A = b^T b + 4/lam I, ||A||_F^2 per tile
  if (cond_max) hipLaunchKernelGGL(ns_cond_kernel, dim3(nt, M), dim3(256), 0, st, (const double*)Wy, l.dregion, l.H, l.hdr, D);
  const int ntd = ns_tiles_per_dim(M, D);
  hipLaunchKernelGGL(ns_norm_kernel, dim3(M), dim3(64), 0, st, l.H, l.hdr, lam, cond_max, D, gs, ntd * ntd);
  hipLaunchKernelGGL(ns_start_kernel, ew, dim3(256), 0, st, Wy, Wt, Wz, l.dregion, (const float*)l.H, l.hdr, D);
  ns_products(st, l, M, D, NsLaunch().add(Wy, Wt, Wy2, 1.0, 0.0, 0.0));  // Y1 = Y0 T0  (Z1 = T0 is in place)
  double *Y = Wy2, *Yn = Wy, *Z = Wz, *Zn = Wz2;
  for (int t = 1; t < kNsIters; ++t) {
    ns_products(st, l, M, D, NsLaunch().add(Z, Y, Wt, -0.5, 0.0, 1.5));  // T = (3 I - Z Y) / 2
    if (t + 1 < kNsIters) {
      ns_products(st, l, M, D, NsLaunch().add(Y, Wt, Yn, 1.0, 0.0, 0.0).add(Wt, Z, Zn, 1.0, 0.0, 0.0));  // Y <- Y T ; Z <- T Z
      double* t0 = Y; Y = Yn; Yn = t0;
      t0 = Z; Z = Zn; Zn = t0;
    }
  }
  // the last Y T: theta_half = (sqrt(||A||_F) Y T - b) / 2, rhoNN + threshold, the norm -- upper tiles, mirrored
  NsEpi ep{};
  ep.hdr = l.H;
  ep.hdr_stride = l.hdr;
  ep.gs = gs;
  ep.b = Wb;
  ep.S = S;
  ep.Zin = Z_in;
  ep.params = params;
  ep.lam = lam;
  ep.Zout = Z_out;
  ep.half_out = half_out;
  ep.sqrt_out = sqrt_out;
  const NsLaunch last = NsLaunch().add(Y, Wt, nullptr, 1.0, 0.0, 0.0);
  if (ns_tile(M, D) == 32 && ns_prefetch_all(D))
    hipLaunchKernelGGL((ns_gemm64_kernel<kNsTheta, 32, true>), dim3(ntd, ntd, M), dim3(kWThreads), 0, st, last.b, l.dregion, D, ep);
  else if (ns_tile(M, D) == 32)
    hipLaunchKernelGGL((ns_gemm64_kernel<kNsTheta, 32>), dim3(ntd, ntd, M), dim3(kWThreads), 0, st, last.b, l.dregion, D, ep);
  else
    hipLaunchKernelGGL((ns_gemm64_kernel<kNsTheta, 64>), dim3(nt, nt, M), dim3(kWThreads), 0, st, last.b, l.dregion, D, ep);
  hipLaunchKernelGGL(ns_norm_reduce_kernel, dim3(M), dim3(64), 0, st, (const float*)l.H, l.hdr, ntd, normF_partial, D);
  return launch_status();
}

static int launch_cell_bwd_ns(const float* G_next, const float* S, const float* Z_in, const float* half, const float* sqrtm,
                              const float* lam, const float* params, float* G_out, float* grad_rho_partial, float* glam_partial,
                              float* workspace, int M, int D, hipStream_t st) {
  const NsLayout l = ns_layout(workspace, M, D);
  const int nt = wide_tiles(D), nup = kWQ * (nt * (nt + 1) / 2), gs = group_size(M);
  double* Wb = l.Wd;                  // b
  double* Wa = l.Wd + 1 * l.dslab;    // A
  double* Wp = l.Wd + 2 * l.dslab;    // P
  double* Wq = l.Wd + 3 * l.dslab;    // Q
  double* Wr = l.Wd + 4 * l.dslab;    // R, then Q + Q^T
  double* Wa2 = l.Wd + 5 * l.dslab;   // the next A
  double* Wq2 = l.Wd + 6 * l.dslab;   // the next Q
  const dim3 ew = ns_ew_grid(M, D);
  hipLaunchKernelGGL(wide_phase_a_kernel, dim3(nup, M), dim3(kWThreads), 0, st, G_next, S, Z_in, half, params, l.Gh, G_out, l.H, D, gs, l.region,
                     l.hdr);
  hipLaunchKernelGGL(ns_b_kernel, ew, dim3(256), 0, st, S, Z_in, lam, Wb, l.dregion, D, gs);
  hipLaunchKernelGGL(ns_frob_kernel, dim3(kNsFrobBlocks, M), dim3(256), 0, st, sqrtm, (size_t)D * D, l.H, l.hdr, D);
  hipLaunchKernelGGL(ns_bwd_start_kernel, ew, dim3(256), 0, st, sqrtm, (const float*)l.Gh, l.region, Wa, Wq, l.dregion, (const float*)l.H, l.hdr,
                     D);
  double *A = Wa, *An = Wa2, *Q = Wq, *Qn = Wq2;
  for (int t = 0; t < kNsIters; ++t) {  // torch_sqrtm.py:42-44, three launches per step
    const bool more = t + 1 < kNsIters;
    ns_products(st, l, M, D, NsLaunch().add(A, A, Wp, -1.0, 0.0, 3.0).add(A, Q, Wr, 1.0, 0.0, 0.0, true));  // P = 3 I - A A ; R = A^T Q ...
    NsLaunch second;
    second.add(Q, A, Wr, -1.0, 1.0, 0.0).add(Q, Wp, Qn, 1.0, 0.0, 0.0);  // ... - Q A ; Q' = Q P ...
    if (more) second.add(A, Wp, An, 0.5, 0.0, 0.0);                       // A <- A P / 2
    ns_products(st, l, M, D, second);
    ns_products(st, l, M, D, NsLaunch().add(A, Wr, Qn, -0.5, 0.5, 0.0, true));  // ... - A^T R, halved
    if (more) {
      double* t0 = A; A = An; An = t0;
    }
    double* t0 = Q; Q = Qn; Qn = t0;
  }
  hipLaunchKernelGGL(ns_symm_kernel, ew, dim3(256), 0, st, (const double*)Q, Wr, l.dregion, D);
  NsEpi ep{};
  ep.hdr = l.H;
  ep.hdr_stride = l.hdr;
  ep.gs = gs;
  ep.S = S;
  ep.lam = lam;
  ep.Zout = G_out;
  ep.Gh = l.Gh;
  ep.gh_stride = l.region;
  const int ntd = ns_tiles_per_dim(M, D);
  const NsLaunch last = NsLaunch().add(Wb, Wr, nullptr, 1.0, 0.0, 0.0);
  if (ns_tile(M, D) == 32 && ns_prefetch_all(D))
    hipLaunchKernelGGL((ns_gemm64_kernel<kNsGout, 32, true>), dim3(ntd, ntd, M), dim3(kWThreads), 0, st, last.b, l.dregion, D, ep);
  else if (ns_tile(M, D) == 32)
    hipLaunchKernelGGL((ns_gemm64_kernel<kNsGout, 32>), dim3(ntd, ntd, M), dim3(kWThreads), 0, st, last.b, l.dregion, D, ep);
  else
    hipLaunchKernelGGL((ns_gemm64_kernel<kNsGout, 64>), dim3(nt, nt, M), dim3(kWThreads), 0, st, last.b, l.dregion, D, ep);
  hipLaunchKernelGGL(ns_glam_kernel, dim3(M), dim3(64), 0, st, l.H, l.hdr, ntd * ntd, nup * kNRho, D);
  hipLaunchKernelGGL(wide_reduce_kernel, dim3(M, kNRho + 1), dim3(64), 0, st, (const float*)l.H, l.hdr, grad_rho_partial, glam_partial, D);
  return launch_status();
}

// out = (A + shift I)^-1 (and log det in the header) beyond the eigensolver's size: L D L^T of the padded matrix, one Newton step
static void launch_ns_inverse(const float* A, const float* shift, int shift_stride, float* out, float* logdet_out, float* workspace, int M, int D,
                              hipStream_t st) {
  const NsLayout l = ns_layout(workspace, M, D);
  const int nt = wide_tiles(D), gs = group_size(M), FD = ns_fact_dim(D), LDc = FD + 1;
  float* X1 = l.W;                                           // the factorisation's first slab, dead once it returns (row stride 513)
  float* X0 = l.W + 2 * (size_t)FD * (FD + 1);     // (row stride FD + 1)
  float* E = l.W + 3 * (size_t)FD * (FD + 1);      // residual, row stride D
  // the factorisation: ONE workgroup per matrix up to D = 256 (0.35 ms there), a sequence of launches with the tiles of every phase spread
  // over the chip beyond (ns_ldl_phase_kernel: 5 nt + 1 launches, nt = ceil(D / 32); UGLAD_LDL_LAUNCHES=0 / 1 in the environment forces one or the other)
  const char* ldl_env = std::getenv("UGLAD_LDL_LAUNCHES");  // (read on every call: tests flip it)
  const int forced = ldl_env ? (ldl_env[0] == '0' ? 0 : 1) : -1;
  const int ntl = (D + 31) / 32;
  const bool phases = forced >= 0 ? forced == 1 : ntl >= 9;
  if (!phases) {
    if (FD == kNsFactSmall)
      hipLaunchKernelGGL(ns_ldl_kernel<kNsFactSmall>, dim3(M), dim3(64 * kNsLdlWaves), 0, st, A, shift, shift_stride, l.W, l.region, logdet_out, D, gs);
    else
      hipLaunchKernelGGL(ns_ldl_kernel<kNsMaxD>, dim3(M), dim3(64 * kNsLdlWaves), 0, st, A, shift, shift_stride, l.W, l.region, logdet_out, D, gs);
  } else {
    auto phase = [&](int ph, int jd, int items) {  // `items` tiles (one wave each) or elements (one thread each, capped) of work per matrix
      int wgs = 1;
      if (ph == kLdlInit || ph == kLdlScale || ph == kLdlFinish) {
        wgs = (items + 64 * kLdlWavesPerWg - 1) / (64 * kLdlWavesPerWg);
        if (wgs > 512) wgs = 512;
      } else {
        wgs = (items + kLdlWavesPerWg - 1) / kLdlWavesPerWg;
      }
      if (wgs < 1) wgs = 1;
      if (FD == kNsFactSmall)
        hipLaunchKernelGGL(ns_ldl_phase_kernel<kNsFactSmall>, dim3(wgs, M), dim3(64 * kLdlWavesPerWg), 0, st, ph, jd, A, shift, shift_stride, l.W, l.region,
                           logdet_out, D, gs);
      else
        hipLaunchKernelGGL(ns_ldl_phase_kernel<kNsMaxD>, dim3(wgs, M), dim3(64 * kLdlWavesPerWg), 0, st, ph, jd, A, shift, shift_stride, l.W, l.region,
                           logdet_out, D, gs);
    };
    const int dpl = ntl * 32;
    phase(kLdlInit, 0, dpl * dpl);
    for (int j = 0; j < ntl; ++j) {
      phase(kLdlDiag, j, 1);
      if (j + 1 < ntl) {
        phase(kLdlPanel, j, ntl - 1 - j);
        phase(kLdlTrail, j, (ntl - 1 - j) * (ntl - j) / 2);
      }
    }
    for (int d = 1; d < ntl; ++d) {
      phase(kLdlWSum, d, ntl - d);
      phase(kLdlWMul, d, ntl - d);
    }
    phase(kLdlScale, 0, dpl * dpl);
    phase(kLdlX, 0, ntl * (ntl + 1) / 2);
    phase(kLdlFinish, 0, dpl * dpl);
  }
  const WideFwd nofw{};
  const dim3 tiles(nt, nt, M), blk(kWThreads);
  // two Newton steps X <- X + X (I - A X): without pivoting the factorisation of a strongly indefinite matrix is only a starting point
  // (the reference's Theta_L at D = 512, cond 2e5 with 104 negative eigenvalues: 4e-2 -> 1.8e-3 -> the ~2e-4 of a pivoted LU in fp32)
  for (int step = 0; step < 2; ++step) {
    const float* Xin = step ? X1 : X0;
    float* Xout = step ? out : X1;
    hipLaunchKernelGGL((wide_gemm_kernel<false, false, kEpiResidual>), tiles, blk, 0, st, A, (size_t)D * D, Xin, l.region, E, l.region,
                       (const float*)nullptr, (const float*)nullptr, shift, (float*)nullptr, l.hdr, shift_stride, D, 0, gs, D, LDc, D, nofw);
    hipLaunchKernelGGL((wide_gemm_kernel<false, false, kEpiNewton>), tiles, blk, 0, st, Xin, l.region, (const float*)E, l.region, Xout,
                       step ? (size_t)D * D : l.region, (const float*)nullptr, (const float*)nullptr, shift, (float*)nullptr, l.hdr,
                       shift_stride, D, 0, gs, LDc, D, step ? D : LDc, nofw);
  }
}

// second launch of the forward cell: the lean kernel (eig_lean.h) -- its one big matrix in LDS up to D = 128 (two workgroups
// per CU), in a workspace slab beyond.
static int launch_cell_stage2(const float* S, const float* Z_in, const float* lam, const float* params, float* Z_out,
                              float* half_out, float* U_out, float* beta_out, float* normF_partial, float* cond_max,
                              float* workspace, int M, int D, int sqrt_mode, hipStream_t st, LamStep ls = LamStep{}) {
  const int DPr = padded_dim(D);
  float* Tws = workspace + (size_t)M * 3 * DPr;
  {
    // few large matrices (wide_bwd.h, wide_fwd.h): the single-workgroup kernel stops before the last merge of the divide & conquer
    // (D > 128: there is one); secular roots, eigenvector update, back-transformation and theta_half follow as their own launches
    const int split = wide_wanted(M, D) ? 2 : 0;
    DISPATCH_NT(D, hipLaunchKernelGGL((cell_fwd_lean_kernel<NT>), dim3(M), dim3(kThreads), 0, st, S, Z_in, lam, params, Z_out,
                                      half_out, U_out, beta_out, normF_partial, cond_max, workspace, Tws, D, sqrt_mode, group_size(M), split,
                                      split ? LamStep{} : ls));
    if (split) {
      const int nt = wide_tiles(D), LD = DPr + 1;
      const size_t rec = 3 * (size_t)DPr, slab = (size_t)big_floats_rt(DPr);
      float* Q1 = workspace + (size_t)M * (3 * DPr + (DPr / 32) * 1024) + slab / 2;  // U, row stride DP + 1
      launch_wide_eig_tail(workspace, Z_out, U_out, beta_out, M, D, st);
      // theta_half = (U phi) U^T, rhoNN + threshold and the norm with one workgroup per upper 64 x 64 tile (wide_bwd.h)
      WideFwd fw{Z_in, params, half_out, cond_max};
      hipLaunchKernelGGL((wide_gemm_kernel<false, true, kEpiThetaHalf>), dim3(nt, nt, M), dim3(kWThreads), 0, st, (const float*)Q1, slab,
                         (const float*)Q1, slab, Z_out, (size_t)D * D, S, (const float*)workspace, lam, workspace, rec, DPr, D, sqrt_mode,
                         group_size(M), LD, LD, D, fw);
      hipLaunchKernelGGL(wide_norm_reduce_kernel, dim3((M + 63) / 64), dim3(64), 0, st, (const float*)workspace, rec, DPr,
                         normF_partial, M, D);
    }
  }
  return launch_status();
}

int uglad_cell_fwd(const float* S, const float* Z_in, const float* lam, const float* params, float* Z_out,
                   float* half_out, float* U_out, float* beta_out, float* normF_partial, float* cond_max, float* workspace, int M,
                   int D, int sqrt_mode, uglad_stream_t stream) {
  if (!S || !Z_in || !lam || !params || !Z_out || !normF_partial || !workspace) return UGLAD_E_NULL;
  CHECK_DIMS(M, D);
  if (sqrt_mode != UGLAD_SQRT_EXACT && sqrt_mode != UGLAD_SQRT_NS10) return UGLAD_E_MODE;
  hipStream_t st = (hipStream_t)stream;
  if (ns_path(M, D, half_out != nullptr || U_out != nullptr, sqrt_mode)) {
    if (sqrt_mode != UGLAD_SQRT_NS10) return UGLAD_E_MODE;  // (the iteration IS the ten-step square root)
    return launch_cell_fwd_ns(S, Z_in, lam, params, Z_out, half_out, U_out, normF_partial, cond_max, workspace, M, D, st);
  }
  LAUNCH_TRIDIAG(S, Z_in, lam, Z_out, workspace);
  return launch_cell_stage2(S, Z_in, lam, params, Z_out, half_out, U_out, beta_out, normF_partial, cond_max, workspace, M, D, sqrt_mode,
                            st);
}

int uglad_cell_fwd_stage2(const float* S, const float* Z_in, const float* lam, const float* params, float* Z_out,
                          float* half_out, float* U_out, float* beta_out, float* normF_partial, float* cond_max, float* workspace,
                          int M, int D, int sqrt_mode, uglad_stream_t stream) {
  if (!S || !Z_in || !lam || !params || !Z_out || !normF_partial || !workspace) return UGLAD_E_NULL;
  CHECK_DIMS(M, D);
  if (sqrt_mode != UGLAD_SQRT_EXACT && sqrt_mode != UGLAD_SQRT_NS10) return UGLAD_E_MODE;
  if (ns_wanted(D)) return UGLAD_E_DIM;  // (no tridiagonal stage to follow on the matrix-iteration path: uglad_cell_fwd is one piece there)
  return launch_cell_stage2(S, Z_in, lam, params, Z_out, half_out, U_out, beta_out, normF_partial, cond_max, workspace, M, D,
                            sqrt_mode, (hipStream_t)stream);
}

int uglad_sum_partials(const float* partials, int n, float* out, uglad_stream_t stream) {
  if (!partials || !out) return UGLAD_E_NULL;
  if (n < 1) return UGLAD_E_DIM;
  hipLaunchKernelGGL(sum_partials_kernel, dim3(t_groups), dim3(kThreads), 0, (hipStream_t)stream, partials, group_size(n), out);
  return launch_status();
}

int uglad_lambda_step(const float* normF_sum, float inv_M, const float* lam_prev, const float* params, float* lam_next,
                      float* lam_in_next, uglad_stream_t stream) {
  if (!normF_sum || !lam_prev || !params || !lam_next || !lam_in_next) return UGLAD_E_NULL;
  hipLaunchKernelGGL(lambda_step_kernel, dim3((t_groups + 63) / 64), dim3(64), 0, (hipStream_t)stream, normF_sum, inv_M,
                     lam_prev, params, lam_next, lam_in_next, t_groups);
  return launch_status();
}

int uglad_cell_bwd(const float* G_next, const float* S, const float* Z_in, const float* half, const float* U,
                   const float* beta, const float* lam, const float* params, float* G_out, float* grad_rho_partial,
                   float* glam_partial, float* workspace, int M, int D, int sqrt_mode, uglad_stream_t stream) {
  if (!G_next || !S || !Z_in || !half || !U || !beta || !lam || !params || !G_out || !grad_rho_partial || !glam_partial ||
      (D > 128 && !workspace))
    return UGLAD_E_NULL;
  CHECK_DIMS(M, D);
  if (sqrt_mode != UGLAD_SQRT_EXACT && sqrt_mode != UGLAD_SQRT_NS10) return UGLAD_E_MODE;
  hipStream_t st = (hipStream_t)stream;
  if (ns_path(M, D, true, sqrt_mode)) {  // (as the forward call that saved this step's state)
    if (sqrt_mode != UGLAD_SQRT_NS10) return UGLAD_E_MODE;
    return launch_cell_bwd_ns(G_next, S, Z_in, half, U, lam, params, G_out, grad_rho_partial, glam_partial, workspace, M, D, st);
  }
  if (wide_wanted(M, D)) return launch_cell_bwd_wide(G_next, S, Z_in, half, U, beta, lam, params, G_out, grad_rho_partial,
                                                          glam_partial, workspace, M, D, sqrt_mode, st);
  DISPATCH_NT(D, hipLaunchKernelGGL((cell_bwd_kernel<NT>), dim3(M), dim3(kThreads), 0, st, G_next, S, Z_in, half, U, beta,
                                    lam, params, G_out, grad_rho_partial, glam_partial, workspace, D, sqrt_mode, group_size(M), 1, 0));
  return launch_status();
}

// Steps L-1 .. 0 of the backward pass in one launch (D <= 128, one workgroup per matrix): dL/dZ never leaves LDS between the steps.
// All arrays are the whole-pass ones (step-major, as uglad_glad_backward takes them); G_out receives dL/dZ_0.
static int launch_cell_bwd_all_steps(const float* G_L, const float* S, const float* Z, const float* half, const float* U,
                                     const float* beta, const float* lam, const float* params, float* G_out, float* grad_rho_partial,
                                     float* glam_partial, int L, int M, int D, int sqrt_mode, hipStream_t st, float* gS = nullptr) {
  const size_t mdd = (size_t)M * D * D, last = (size_t)(L - 1);
  if (gS) {
    DISPATCH_NT_SMALL(D, hipLaunchKernelGGL((cell_bwd_gs_kernel<NT>), dim3(M), dim3(kThreads), 0, st, G_L, S, Z + last * mdd,
                                            half + last * mdd, U + last * mdd, beta + last * M * D, lam + last * t_groups, params, G_out,
                                            grad_rho_partial, glam_partial + last * M, nullptr, D, sqrt_mode, group_size(M), L, t_groups,
                                            gS));
    return launch_status();
  }
  DISPATCH_NT_SMALL(D, hipLaunchKernelGGL((cell_bwd_kernel<NT>), dim3(M), dim3(kThreads), 0, st, G_L, S, Z + last * mdd, half + last * mdd,
                                          U + last * mdd, beta + last * M * D, lam + last * t_groups, params, G_out, grad_rho_partial,
                                          glam_partial + last * M, nullptr, D, sqrt_mode, group_size(M), L, t_groups));
  return launch_status();
}

// One step of the backward pass that also accumulates dL/dS into gS: the spectral path's one-workgroup cell (uglad_cell_bwd's last case;
// uglad_glad_backward_wrt_s has refused the passes that take its other two paths).
static int launch_cell_bwd_step_gs(const float* G_next, const float* S, const float* Z_in, const float* half, const float* U,
                                   const float* beta, const float* lam, const float* params, float* G_out, float* grad_rho_partial,
                                   float* glam_partial, float* workspace, int M, int D, int sqrt_mode, float* gS, hipStream_t st) {
  DISPATCH_NT(D, hipLaunchKernelGGL((cell_bwd_gs_kernel<NT>), dim3(M), dim3(kThreads), 0, st, G_next, S, Z_in, half, U, beta, lam, params,
                                    G_out, grad_rho_partial, glam_partial, workspace, D, sqrt_mode, group_size(M), 1, 0, gS));
  return launch_status();
}

int uglad_loss_fwd(const float* theta, const float* S, int s_batch, const float* struct_theta, float* loss_partial,
                   float* theta_inv_out, float* workspace, int M, int D, uglad_stream_t stream) {
  if (!theta || !S || !loss_partial || !theta_inv_out || !workspace) return UGLAD_E_NULL;
  CHECK_DIMS(M, D);
  if (s_batch != 1 && s_batch != M) return UGLAD_E_DIM;
  hipStream_t st = (hipStream_t)stream;
  if (ns_factorisation(M, D)) {
    const NsLayout l = ns_layout(workspace, M, D);
    launch_ns_inverse(theta, nullptr, 0, theta_inv_out, loss_partial, workspace, M, D, st);  // (log det parked in loss_partial)
    hipLaunchKernelGGL(wide_loss_trace_kernel, dim3(wide_tiles(D), M), dim3(kWThreads), 0, st, theta, S, s_batch, struct_theta, l.H, l.hdr,
                       ns_off_tiles(D), D);
    hipLaunchKernelGGL(ns_loss_finish_kernel, dim3((M + 63) / 64), dim3(64), 0, st, (const float*)l.H, l.hdr, ns_off_tiles(D),
                       (const float*)loss_partial, loss_partial, M, D);
    return launch_status();
  }
  const int* only = nullptr;
  if (D <= 128 && cholesky_enabled()) {
    int* flags = chol_flags(workspace, M, D);
    DISPATCH_NT_SMALL(D, hipLaunchKernelGGL((chol_loss_kernel<NT>), dim3(M), dim3(kThreads), 0, st, theta, S, s_batch, struct_theta,
                                            loss_partial, theta_inv_out, flags, D));
    only = flags;
  }
  LAUNCH_TRIDIAG_IF(theta, (const float*)nullptr, (const float*)nullptr, theta_inv_out, workspace, only);
  if (wide_wanted(M, D)) {
    const int DPr = padded_dim(D);
    launch_wide_inverse(theta, nullptr, 0, theta_inv_out, workspace, M, D, st);
    hipLaunchKernelGGL(wide_loss_trace_kernel, dim3(wide_tiles(D), M), dim3(kWThreads), 0, st, theta, S, s_batch, struct_theta, workspace,
                       3 * (size_t)DPr, DPr, D);
    hipLaunchKernelGGL(wide_loss_finish_kernel, dim3((M + 63) / 64), dim3(64), 0, st, (const float*)workspace, 3 * (size_t)DPr, DPr,
                       loss_partial, M, D);
    return launch_status();
  }
  DISPATCH_NT(D, hipLaunchKernelGGL((loss_fwd_kernel<NT>), dim3(M), dim3(kThreads), 0, st, theta, S, s_batch, struct_theta,
                                    loss_partial, theta_inv_out, workspace, D, only));
  return launch_status();
}

int uglad_loss_bwd(const float* theta, const float* theta_inv, const float* S, int s_batch, const float* struct_theta,
                   const float* g_up, float scale, float* G_out, int M, int D, uglad_stream_t stream) {
  if (!theta || !theta_inv || !S || !g_up || !G_out) return UGLAD_E_NULL;
  CHECK_DIMS(M, D);
  if (s_batch != 1 && s_batch != M) return UGLAD_E_DIM;
  const size_t total = (size_t)M * D * D;
  const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(loss_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, theta, theta_inv, S, s_batch,
                     struct_theta, g_up, scale, G_out, D, total);
  return launch_status();
}

int uglad_loss_bwd_wrt_s(const float* theta, const float* theta_inv, const float* S, int s_batch, const float* struct_theta,
                         const float* g_up, float scale, float* G_out, float* gS, int M, int D, uglad_stream_t stream) {
  if (!gS) return UGLAD_E_NULL;
  int rc = uglad_loss_bwd(theta, theta_inv, S, s_batch, struct_theta, g_up, scale, G_out, M, D, stream);
  if (rc) return rc;
  const size_t total = (size_t)s_batch * D * D;
  const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(loss_bwd_gs_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, theta, g_up, scale, gS, s_batch, M, D);
  return launch_status();
}

int uglad_finish_grads(const float* gt_partial, const float* grad_rho_partial, const float* glam_partial,
                       const float* lam_in, const float* params, float* grad, int L, int M, uglad_stream_t stream) {
  if (!gt_partial || !grad_rho_partial || !glam_partial || !lam_in || !params || !grad) return UGLAD_E_NULL;
  if (L < 1 || M < 1) return UGLAD_E_DIM;
  hipLaunchKernelGGL(finish_grads_kernel, dim3(t_groups), dim3(kThreads), 0, (hipStream_t)stream, gt_partial, grad_rho_partial,
                     glam_partial, lam_in, params, grad, L, M, group_size(M));
  return launch_status();
}

// Zero n floats with a kernel, not hipMemsetAsync: captured into a caller's graph (PyTorch's stream capture, ROCm 7.2) the memset NODES of the two
// small zero-fills of a pass did not replay as zero-fills -- the 4-byte one left 5e36 behind, the 112-byte one left every other float
// unzeroed (tests/test_gpu_parity.py::test_a_whole_pass_can_be_captured_into_the_callers_graph failed on exactly these two buffers) --
// while a kernel node replays as launched.
static int zero_floats(float* p, size_t n, hipStream_t st) {
  const int grid = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
  hipLaunchKernelGGL(zero_kernel, dim3(grid), dim3(256), 0, st, p, n);
  return launch_status();
}

// ---- the whole unrolled pass in one call (single-process case: no collective between the norm and the lambda step)
static int enqueue_glad_forward(const float* S, const float* params, float lambda_init, int init_diag, int L, float* Z,
                                int z_slabs, float* half, float* U, float* beta, float* lam, float* lam_in, float* nf_partial,
                                float* nf_sum, float* cond_max, float* workspace, int M, int D, int sqrt_mode,
                                uglad_stream_t stream, int m_global = 0, uglad_allreduce_fn exchange = nullptr,
                                void* exchange_ctx = nullptr) {
  if (!S || !params || !Z || !lam || !lam_in || !nf_partial || !nf_sum || !workspace) return UGLAD_E_NULL;
  CHECK_DIMS(M, D);
  if (L < 1 || z_slabs < 2) return UGLAD_E_DIM;
  const size_t mdd = (size_t)M * D * D;
  int rc = uglad_init_theta(S, params, init_diag, Z, workspace, M, D, stream);
  if (rc) return rc;
  if (cond_max) {  // running maximum over the L steps: starts at 0
    if ((rc = zero_floats(cond_max, (size_t)M, (hipStream_t)stream))) return rc;
  }
  if ((rc = uglad_lambda_init(params, lambda_init, lam, lam_in, stream))) return rc;
  const int G = t_groups;  // lam: (L + 1, G), lam_in: (L + 1, G, 2), nf_sum: (G)
  const float inv_m = 1.0f / (float)(exchange ? m_global : group_size(M));
  // one matrix per group on the eigensolver's one-workgroup kernel: the lambda step rides in the cell's second launch (LamStep)
  const bool fuse_lambda = !exchange && group_size(M) == 1 && D <= UGLAD_MAX_EIG_DIM && !wide_wanted(M, D) &&
                           !ns_path(M, D, half != nullptr || U != nullptr, sqrt_mode) && !std::getenv("UGLAD_NO_FUSED_LAMBDA");
  for (int k = 0; k < L; ++k) {
    const float* zi = Z + (size_t)(k % z_slabs) * mdd;
    float* zo = Z + (size_t)((k + 1) % z_slabs) * mdd;
    if (fuse_lambda) {
      if (sqrt_mode != UGLAD_SQRT_EXACT && sqrt_mode != UGLAD_SQRT_NS10) return UGLAD_E_MODE;
      hipStream_t st = (hipStream_t)stream;
      const float* lamk = lam + (size_t)k * G;
      LAUNCH_TRIDIAG(S, zi, lamk, zo, workspace);
      const LamStep ls{nf_sum, lam + (size_t)(k + 1) * G, lam_in + 2 * (size_t)(k + 1) * G, inv_m};
      if ((rc = launch_cell_stage2(S, zi, lamk, params, zo, half ? half + (size_t)k * mdd : nullptr, U ? U + (size_t)k * mdd : nullptr,
                                   beta ? beta + (size_t)k * M * D : nullptr, nf_partial, cond_max, workspace, M, D, sqrt_mode, st, ls)))
        return rc;
      continue;
    }
    rc = uglad_cell_fwd(S, zi, lam + (size_t)k * G, params, zo, half ? half + (size_t)k * mdd : nullptr,
                        U ? U + (size_t)k * mdd : nullptr, beta ? beta + (size_t)k * M * D : nullptr, nf_partial, cond_max, workspace,
                        M, D, sqrt_mode, stream);
    if (rc) return rc;
    if (exchange) {
      // sharded batch: local sum -> SUM over the ranks (stream-ordered, no host decision) -> LambdaNN on every rank from the same bits
      if ((rc = uglad_sum_partials(nf_partial, M, nf_sum, stream))) return rc;
      if ((rc = exchange(nf_sum, 1, exchange_ctx, stream))) return rc;
      if ((rc = uglad_lambda_step(nf_sum, inv_m, lam + k, params, lam + k + 1, lam_in + 2 * (size_t)(k + 1), stream))) return rc;
      continue;
    }
    // (uglad_sum_partials + uglad_lambda_step as one launch: nothing is exchanged between them in a single-process pass)
    hipLaunchKernelGGL(norm_lambda_kernel, dim3(G), dim3(kThreads), 0, (hipStream_t)stream, nf_partial, group_size(M), inv_m,
                       lam + (size_t)k * G, params, nf_sum, lam + (size_t)(k + 1) * G, lam_in + 2 * (size_t)(k + 1) * G);
    if ((rc = launch_status())) return rc;
  }
  return 0;
}

static int enqueue_glad_backward(const float* G_L, const float* S, const float* params, int init_diag, int L, const float* Z,
                                 const float* half, const float* U, const float* beta, const float* lam, const float* lam_in,
                                 float* gbuf0, float* gbuf1, float* grad_rho_partial, float* glam_partial, float* gt_partial,
                                 float* grad, float* workspace, int M, int D, int sqrt_mode, uglad_stream_t stream,
                                 float* gS = nullptr) {
  if (!G_L || !S || !params || !Z || !half || !U || !beta || !lam || !lam_in || !gbuf0 || !gbuf1 || !grad_rho_partial ||
      !glam_partial || !gt_partial || !grad)
    return UGLAD_E_NULL;
  CHECK_DIMS(M, D);
  if (L < 1) return UGLAD_E_DIM;
  const size_t mdd = (size_t)M * D * D;
  int rc = zero_floats(grad_rho_partial, (size_t)M * UGLAD_NRHO, (hipStream_t)stream);
  if (rc) return rc;
  if (gS && (rc = zero_floats(gS, mdd, (hipStream_t)stream))) return rc;
  const float* cur = G_L;
  if (D <= 128 && !ns_wanted(D) && !wide_wanted(M, D) && persistent_bwd_enabled()) {
    if ((rc = launch_cell_bwd_all_steps(G_L, S, Z, half, U, beta, lam, params, gbuf0, grad_rho_partial, glam_partial, L, M, D, sqrt_mode,
                                        (hipStream_t)stream, gS)))
      return rc;
    cur = gbuf0;
  } else
  for (int k = L - 1; k >= 0; --k) {
    float* out = (k & 1) ? gbuf1 : gbuf0;
    if (gS && (ns_path(M, D, true, sqrt_mode) || wide_wanted(M, D))) {  // no dL/dS variant there: the step as it is, then its dL/dS
      rc = uglad_cell_bwd(cur, S, Z + (size_t)k * mdd, half + (size_t)k * mdd, U + (size_t)k * mdd, beta + (size_t)k * M * D,
                          lam + (size_t)k * t_groups, params, out, grad_rho_partial, glam_partial + (size_t)k * M, workspace, M, D,
                          sqrt_mode, stream);
      if (rc) return rc;
      const int grid = (int)((mdd + 255) / 256 < 4096 ? (mdd + 255) / 256 : 4096);
      hipLaunchKernelGGL(cell_gs_step_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, cur, S, Z + (size_t)k * mdd,
                         half + (size_t)k * mdd, lam + (size_t)k * t_groups, params, (const float*)out, gS, D, group_size(M), mdd);
      rc = launch_status();
    } else if (gS)
      rc = launch_cell_bwd_step_gs(cur, S, Z + (size_t)k * mdd, half + (size_t)k * mdd, U + (size_t)k * mdd, beta + (size_t)k * M * D,
                                   lam + (size_t)k * t_groups, params, out, grad_rho_partial, glam_partial + (size_t)k * M, workspace, M,
                                   D, sqrt_mode, gS, (hipStream_t)stream);
    else
      rc = uglad_cell_bwd(cur, S, Z + (size_t)k * mdd, half + (size_t)k * mdd, U + (size_t)k * mdd, beta + (size_t)k * M * D,
                          lam + (size_t)k * t_groups, params, out, grad_rho_partial, glam_partial + (size_t)k * M, workspace, M, D,
                          sqrt_mode, stream);
    if (rc) return rc;
    cur = out;
  }
  if ((rc = uglad_init_theta_bwd(Z, cur, init_diag, gt_partial, workspace, M, D, stream))) return rc;
  if (gS) {  // the Theta_0 term of dL/dS
    hipStream_t st = (hipStream_t)stream;
    if (init_diag == 1) {
      const size_t total = (size_t)M * D;
      const int grid = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
      hipLaunchKernelGGL(init_bwd_diag_gs_kernel, dim3(grid), dim3(256), 0, st, (const float*)Z, cur, gS, D, total);
    } else if (ns_factorisation(M, D)) {  // beyond the one-workgroup kernels: T = Theta0 G0 into the idle G buffer, R = T Theta0 into G0's
      float* T = (cur == gbuf0) ? gbuf1 : gbuf0;
      float* R = const_cast<float*>(cur);
      const dim3 tiles((D + 63) / 64, (D + 63) / 64, M);
      hipLaunchKernelGGL(gs_gemm_kernel, tiles, dim3(256), 0, st, (const float*)Z, cur, T, D);
      hipLaunchKernelGGL(gs_gemm_kernel, tiles, dim3(256), 0, st, (const float*)T, (const float*)Z, R, D);
      const int grid = (int)((mdd + 255) / 256 < 4096 ? (mdd + 255) / 256 : 4096);
      hipLaunchKernelGGL(gs_sub_sym_kernel, dim3(grid), dim3(256), 0, st, (const float*)R, gS, D, mdd);
    } else {
      DISPATCH_NT(D, hipLaunchKernelGGL((init_bwd_gs_kernel<NT>), dim3(M), dim3(kThreads), 0, st, Z, cur, gS, workspace, D));
    }
    if ((rc = launch_status())) return rc;
  }
  return uglad_finish_grads(gt_partial, grad_rho_partial, glam_partial, lam_in, params, grad, L, M, stream);
}

// (Round 3 removed the hipGraph cache of small passes that lived here: once persistent buffers made it hit -- 4 captures, 436 replays in a
// 220-epoch fit at D = 25 -- the epoch took 1.58 ms with it and 1.51 ms without (profiles/r03_fit_small_graph_probe.txt): a small pass is bound
// by the latency of its dependent kernels, not by their launches.  The entry points neither allocate nor synchronise, so a caller's own
// stream capture of a pass still works.)
int uglad_glad_forward(const float* S, const float* params, float lambda_init, int init_diag, int L, float* Z, int z_slabs,
                       float* half, float* U, float* beta, float* lam, float* lam_in, float* nf_partial, float* nf_sum,
                       float* cond_max, float* workspace, int M, int D, int sqrt_mode, uglad_stream_t stream) {
  return enqueue_glad_forward(S, params, lambda_init, init_diag, L, Z, z_slabs, half, U, beta, lam, lam_in, nf_partial, nf_sum, cond_max,
                              workspace, M, D, sqrt_mode, stream);
}

int uglad_glad_backward(const float* G_L, const float* S, const float* params, int init_diag, int L, const float* Z,
                        const float* half, const float* U, const float* beta, const float* lam, const float* lam_in,
                        float* gbuf0, float* gbuf1, float* grad_rho_partial, float* glam_partial, float* gt_partial,
                        float* grad, float* workspace, int M, int D, int sqrt_mode, uglad_stream_t stream) {
  return enqueue_glad_backward(G_L, S, params, init_diag, L, Z, half, U, beta, lam, lam_in, gbuf0, gbuf1, grad_rho_partial, glam_partial,
                               gt_partial, grad, workspace, M, D, sqrt_mode, stream);
}

int uglad_glad_forward_grouped(const float* S, const float* params, float lambda_init, int init_diag, int L, float* Z,
                               int z_slabs, float* half, float* U, float* beta, float* lam, float* lam_in, float* nf_partial,
                               float* nf_sum, float* cond_max, float* workspace, int M, int D, int groups, int sqrt_mode,
                               uglad_stream_t stream) {
  if (groups < 1 || M < groups || M % groups != 0) return UGLAD_E_DIM;
  GroupScope scope(groups);
  return uglad_glad_forward(S, params, lambda_init, init_diag, L, Z, z_slabs, half, U, beta, lam, lam_in, nf_partial, nf_sum,
                            cond_max, workspace, M, D, sqrt_mode, stream);
}

int uglad_glad_backward_grouped(const float* G_L, const float* S, const float* params, int init_diag, int L, const float* Z,
                                const float* half, const float* U, const float* beta, const float* lam, const float* lam_in,
                                float* gbuf0, float* gbuf1, float* grad_rho_partial, float* glam_partial, float* gt_partial,
                                float* grad, float* workspace, int M, int D, int groups, int sqrt_mode, uglad_stream_t stream) {
  if (groups < 1 || M < groups || M % groups != 0) return UGLAD_E_DIM;
  GroupScope scope(groups);
  return uglad_glad_backward(G_L, S, params, init_diag, L, Z, half, U, beta, lam, lam_in, gbuf0, gbuf1, grad_rho_partial,
                             glam_partial, gt_partial, grad, workspace, M, D, sqrt_mode, stream);
}

int uglad_glad_backward_wrt_s(const float* G_L, const float* S, const float* params, int init_diag, int L, const float* Z,
                              const float* half, const float* U, const float* beta, const float* lam, const float* lam_in,
                              float* gbuf0, float* gbuf1, float* grad_rho_partial, float* glam_partial, float* gt_partial,
                              float* grad, float* workspace, int M, int D, int groups, int sqrt_mode, float* gS, uglad_stream_t stream) {
  if (!gS || (D > 128 && !workspace)) return UGLAD_E_NULL;
  if (groups < 1 || M < groups || M % groups != 0) return UGLAD_E_DIM;
  CHECK_DIMS(M, D);
  if (sqrt_mode != UGLAD_SQRT_EXACT && sqrt_mode != UGLAD_SQRT_NS10) return UGLAD_E_MODE;
  if (init_diag != 0 && init_diag != 1) return UGLAD_E_MODE;
  GroupScope scope(groups);
  return enqueue_glad_backward(G_L, S, params, init_diag, L, Z, half, U, beta, lam, lam_in, gbuf0, gbuf1, grad_rho_partial, glam_partial,
                               gt_partial, grad, workspace, M, D, sqrt_mode, stream, gS);
}

// ---- the sharded pass as ONE call (collective site i)
int uglad_glad_forward_sharded(const float* S, const float* params, float lambda_init, int init_diag, int L, float* Z, int z_slabs,
                               float* half, float* U, float* beta, float* lam, float* lam_in, float* nf_partial, float* nf_sum,
                               float* cond_max, float* workspace, int M, int D, int m_global, int sqrt_mode,
                               uglad_allreduce_fn exchange, void* exchange_ctx, uglad_stream_t stream) {
  if (!exchange) return UGLAD_E_NULL;
  if (m_global < M || t_groups != 1) return UGLAD_E_DIM;
  return enqueue_glad_forward(S, params, lambda_init, init_diag, L, Z, z_slabs, half, U, beta, lam, lam_in, nf_partial, nf_sum, cond_max,
                              workspace, M, D, sqrt_mode, stream, m_global, exchange, exchange_ctx);
}

// ---- RCCL as the exchange: resolved at run time from the RCCL that is already in the process (PyTorch-ROCm's) or, failing that, the
// system's -- libuglad_hip.so itself has no link-time dependency on it.
}  // extern "C"
#ifndef UGLAD_SIMT_EMUL
#include <dlfcn.h>
namespace {
struct RcclApi {
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, uglad_rccl_id, int) = nullptr;  // (ncclUniqueId travels by value: 128 bytes)
  int (*CommDestroy)(void*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;
  bool ok = false;
};
const RcclApi& rccl_api() {
  static const RcclApi api = [] {
    RcclApi a;
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so"})
      if (!h) h = dlopen(name, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);  // the copy PyTorch has loaded, if any
    for (const char* name : {"librccl.so.1", "librccl.so"})
      if (!h) h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (!h) return a;
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(h, "ncclAllReduce"));
    a.CommCount = reinterpret_cast<decltype(a.CommCount)>(dlsym(h, "ncclCommCount"));
    a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllReduce;
    return a;
  }();
  return api;
}
constexpr int kNcclFloat32 = 7, kNcclSum = 0;  // rccl.h: ncclDataType_t / ncclRedOp_t
}  // namespace
#endif
extern "C" {

int uglad_rccl_unique_id(uglad_rccl_id* id_out) {
  if (!id_out) return UGLAD_E_NULL;
#ifndef UGLAD_SIMT_EMUL
  if (!rccl_api().ok) return UGLAD_E_RCCL;
  return rccl_api().GetUniqueId(id_out) == 0 ? 0 : UGLAD_E_RCCL;
#else
  return UGLAD_E_RCCL;
#endif
}

int uglad_rccl_comm_init(const uglad_rccl_id* id, int nranks, int rank, void** comm_out) {
  if (!id || !comm_out) return UGLAD_E_NULL;
  if (nranks < 1 || rank < 0 || rank >= nranks) return UGLAD_E_DIM;
#ifndef UGLAD_SIMT_EMUL
  if (!rccl_api().ok) return UGLAD_E_RCCL;
  return rccl_api().CommInitRank(comm_out, nranks, *id, rank) == 0 ? 0 : UGLAD_E_RCCL;
#else
  return UGLAD_E_RCCL;
#endif
}

int uglad_rccl_comm_destroy(void* comm) {
  if (!comm) return UGLAD_E_NULL;
#ifndef UGLAD_SIMT_EMUL
  if (!rccl_api().ok) return UGLAD_E_RCCL;
  return rccl_api().CommDestroy(comm) == 0 ? 0 : UGLAD_E_RCCL;
#else
  return UGLAD_E_RCCL;
#endif
}

// ncclCommCount: how many ranks the communicator spans -- what a multi-GPU record can show to prove that RCCL saw all of them
int uglad_rccl_comm_count(void* comm, int* nranks_out) {
  if (!comm || !nranks_out) return UGLAD_E_NULL;
#ifndef UGLAD_SIMT_EMUL
  if (!rccl_api().ok || !rccl_api().CommCount) return UGLAD_E_RCCL;
  return rccl_api().CommCount(comm, nranks_out) == 0 ? 0 : UGLAD_E_RCCL;
#else
  return UGLAD_E_RCCL;
#endif
}

// (has the signature of uglad_allreduce_fn: hand its address and the communicator to uglad_glad_forward_sharded)
int uglad_rccl_allreduce_sum(float* buf, int n, void* comm, uglad_stream_t stream) {
  if (!buf || !comm) return UGLAD_E_NULL;
  if (n < 1) return UGLAD_E_DIM;
#ifndef UGLAD_SIMT_EMUL
  if (!rccl_api().ok) return UGLAD_E_RCCL;
  return rccl_api().AllReduce(buf, buf, (size_t)n, kNcclFloat32, kNcclSum, comm, (hipStream_t)stream) == 0 ? 0 : UGLAD_E_RCCL;
#else
  return UGLAD_E_RCCL;
#endif
}

int uglad_consensus_partial(const float* theta_K, int K, int D, float* absmin, float* signsum, uglad_stream_t stream) {
  if (!theta_K || !absmin || !signsum) return UGLAD_E_NULL;
  if (K < 1 || D < 1) return UGLAD_E_DIM;
  const int DD = D * D;
  hipLaunchKernelGGL(consensus_partial_kernel, dim3((DD + 255) / 256), dim3(256), 0, (hipStream_t)stream, theta_K, K, DD,
                     absmin, signsum);
  return launch_status();
}

int uglad_consensus_combine(const float* absmin, const float* signsum, int D, float* out, uglad_stream_t stream) {
  if (!absmin || !signsum || !out) return UGLAD_E_NULL;
  if (D < 1) return UGLAD_E_DIM;
  const int DD = D * D;
  hipLaunchKernelGGL(consensus_combine_kernel, dim3((DD + 255) / 256), dim3(256), 0, (hipStream_t)stream, absmin, signsum,
                     DD, out);
  return launch_status();
}

int uglad_symeig(const float* A, float* U, float* beta, float* workspace, int M, int D, uglad_stream_t stream) {
  if (!A || !U || !beta || !workspace) return UGLAD_E_NULL;
  CHECK_DIMS_EIG(M, D);
  hipStream_t st = (hipStream_t)stream;
  LAUNCH_TRIDIAG(A, (const float*)nullptr, (const float*)nullptr, U, workspace);
  float* Tws = workspace + (size_t)M * 3 * padded_dim(D);
  DISPATCH_NT(D, hipLaunchKernelGGL((symeig_lean_kernel<NT>), dim3(M), dim3(kThreads), 0, st, U, beta, workspace, Tws, D));
  return launch_status();
}

int uglad_covariance(const float* X, int K, int N, int D, int normalize, float eval_offset, float* S_out, float* eig_scratch,
                     float* workspace, uglad_stream_t stream) {
  if (!X || !S_out) return UGLAD_E_NULL;
  CHECK_DIMS_EIG(K, D);
  if (N < 1) return UGLAD_E_DIM;
  if (normalize != 0 && normalize != 1) return UGLAD_E_MODE;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_NT(D, hipLaunchKernelGGL((cov_kernel<NT>), dim3(K), dim3(kThreads), 0, st, X, N, D, normalize, S_out));
  int rc = launch_status();
  if (rc || !eig_scratch) return rc;  // eig_scratch == NULL: no eigenvalue repair
  if (!workspace) return UGLAD_E_NULL;
  float* beta = eig_scratch + (size_t)K * D * D;
  if ((rc = uglad_symeig(S_out, eig_scratch, beta, workspace, K, D, stream))) return rc;
  hipLaunchKernelGGL(cov_repair_kernel, dim3(K), dim3(256), 0, st, S_out, beta, D, eval_offset);
  return launch_status();
}


#ifdef UGLAD_PHASE_EXIT
int uglad_diag_set_exit(int at) {  // (development build: see eig_dc.h)
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_exit_at), &at, sizeof(int));
}
#endif

#ifdef UGLAD_STAMPS
int uglad_diag_tstamps(unsigned long long* host_out, int reset) {
  unsigned long long zero[4] = {0, 0, 0, 0};
  const hipError_t e = hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_tstamps), sizeof(zero));
  if (reset) (void)hipMemcpyToSymbol(HIP_SYMBOL(g_tstamps), zero, sizeof(zero));
  return (int)e;
}

int uglad_diag_twg(unsigned long long* host_out, int n) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_twg), sizeof(unsigned long long) * 3 * (size_t)n);
}

int uglad_diag_cwg(unsigned long long* host_out, int n) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_cwg), sizeof(unsigned long long) * 3 * (size_t)n);
}

int uglad_diag_sec(unsigned long long* host_out) {  // 16 x 8 stamps of the secular solver (eig_lean.h)
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_sec), sizeof(unsigned long long) * 16 * 8);
}

int uglad_diag_lstamps(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_lstamps), sizeof(unsigned long long) * 4 * 96);
}

int uglad_diag_kstamps(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_kstamps), sizeof(unsigned long long) * 32);
}

int uglad_symeig_stamps(const float* A, float* U, float* beta, float* workspace, int M, int D, unsigned long long* stamps,
                        uglad_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  LAUNCH_TRIDIAG(A, (const float*)nullptr, (const float*)nullptr, U, workspace);
  DISPATCH_NT(D, hipLaunchKernelGGL((symeig_stamp_kernel<NT>), dim3(M), dim3(kThreads), 0, st, U, beta,
                                    workspace, D, stamps));
  return launch_status();
}
#endif

int uglad_conditional_mean(const float* precision, const float* mean, const float* observed, const float* values,
                           float* full_mean, float* cond_cov, float* log_pdf, float* scratch, float* workspace, int K, int D,
                           int clip01, uglad_stream_t stream) {
  if (!precision || !mean || !observed || !values || !full_mean || !cond_cov || !scratch || !workspace) return UGLAD_E_NULL;
  CHECK_DIMS_EIG(K, D);
  hipStream_t st = (hipStream_t)stream;
  const int M = K;
  const size_t total = (size_t)K * D * D;
  const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(map_prepare_kernel, dim3(grid), dim3(256), 0, st, precision, observed, scratch, D, total);
  LAUNCH_TRIDIAG(scratch, (const float*)nullptr, (const float*)nullptr, cond_cov, workspace);
  DISPATCH_NT(D, hipLaunchKernelGGL((map_solve_kernel<NT>), dim3(K), dim3(kThreads), 0, st, precision, mean, observed, values,
                                    scratch, full_mean, cond_cov, log_pdf, workspace, D, clip01));
  return launch_status();
}

int uglad_partial_correlations(const float* precision, float* rho, int K, int D, uglad_stream_t stream) {
  if (!precision || !rho) return UGLAD_E_NULL;
  if (K < 1 || D < 1) return UGLAD_E_DIM;
  const size_t total = (size_t)K * D * D;
  const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(partial_corr_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, precision, rho, D, total);
  return launch_status();
}

int uglad_support_metrics(const float* true_theta, const float* pred_theta, double* out, int K, int D, int beta,
                          uglad_stream_t stream) {
  if (!true_theta || !pred_theta || !out) return UGLAD_E_NULL;
  CHECK_DIMS_EIG(K, D);
  if (D < 2) return UGLAD_E_DIM;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_NT(D, hipLaunchKernelGGL((support_metrics_kernel<NT>), dim3(K), dim3(kThreads), 0, st, true_theta, pred_theta, out, D,
                                    beta));
  return launch_status();
}

int uglad_tridiagonalize(const float* A0, const float* A1, const float* lam, float* R, float* workspace, int M, int D,
                         uglad_stream_t stream) {
  if (!A0 || !R || !workspace || (A1 && !lam)) return UGLAD_E_NULL;
  CHECK_DIMS_EIG(M, D);
  hipStream_t st = (hipStream_t)stream;
  LAUNCH_TRIDIAG(A0, A1, lam, R, workspace);
  return launch_status();
}

int uglad_symeig_jacobi(const float* A, float* U, float* beta, int M, int D, uglad_stream_t stream) {
  if (!A || !U || !beta) return UGLAD_E_NULL;
  CHECK_DIMS_EIG(M, D);
  if (D > 128) return UGLAD_E_DIM;  // LDS-resident only
  hipStream_t st = (hipStream_t)stream;
  switch ((D + 31) / 32) {
    case 1: hipLaunchKernelGGL((symeig_jacobi_kernel<1>), dim3(M), dim3(kThreads), 0, st, A, U, beta, D); break;
    case 2: hipLaunchKernelGGL((symeig_jacobi_kernel<2>), dim3(M), dim3(kThreads), 0, st, A, U, beta, D); break;
    case 3: hipLaunchKernelGGL((symeig_jacobi_kernel<3>), dim3(M), dim3(kThreads), 0, st, A, U, beta, D); break;
    default: hipLaunchKernelGGL((symeig_jacobi_kernel<4>), dim3(M), dim3(kThreads), 0, st, A, U, beta, D); break;
  }
  return launch_status();
}

}  // extern "C"
#endif  // !UGLAD_TU_NT
