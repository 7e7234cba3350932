// Theta_0 = (S + t I)^-1 and its gradient: the spectral and the Cholesky kernel, the Newton step both share with the loss and the
// MAP solve (spectral_to_global), and the backward kernels for t and for S.
#pragma once
#include "chol.h"
#include "eig_lean.h"

namespace uglad {

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

// Theta_0 = (S + t I)^-1 through the eigendecomposition of S (the cell's solver, eig_lean.h): V diag(1/(s_i + t)) V^T.  The
// eigenvectors land in the first big buffer (sV), the second (sA) is the scratch of spectral_to_global.
template <int NT>
__global__ __launch_bounds__(kThreads) void init_inverse_kernel(const float* __restrict__ S,
                                                                const float* __restrict__ params,
                                                                float* __restrict__ theta0,
                                                                float* __restrict__ tri, int D, int gs,
                                                                const int* __restrict__ only_flagged) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sV, DP * LD, sA, DP * LD, tri)
  __shared__ __attribute__((aligned(16))) LeanScratch<DP> ws;
  __shared__ float s_f[DP];
  if (only_flagged && only_flagged[blockIdx.x] == 0) return;  // (the Cholesky kernel has done this matrix)
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * D * D;
  const float t = params[(size_t)(blockIdx.x / gs) * kNParam + P_T];
  symeig_lean<NT>(sV, D, ws, tri + (size_t)blockIdx.x * 3 * DP, theta0 + base, D, tfac_behind_flags<DP>(tri, gridDim.x, blockIdx.x));
  __syncthreads();  // (the solver ends with a barrier of its own only if there are reflectors, D > 2)
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

// ---- not templated on NT (INIT_DIAG: Theta_0 = diag(1 / (S_ii + t))): in the host unit only, the per-NT units would define them again
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
#endif  // !UGLAD_TU_NT

}  // namespace uglad
