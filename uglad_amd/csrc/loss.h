// The loss -logdet(Theta) + tr(S Theta) (+ structure penalty) with Theta^-1 for its backward pass, spectral and Cholesky; the
// elementwise backward kernels and the helpers of dL/dS on the paths whose kernels have no dL/dS variant.
#pragma once
#include "theta0.h"

namespace uglad {

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
  UGLAD_BIG_BUFFERS(sV, DP * LD, sA, DP * LD, tri)  // eigenvectors ; scratch of spectral_to_global
  __shared__ __attribute__((aligned(16))) LeanScratch<DP> ws;
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
  symeig_lean<NT>(sV, D, ws, tri + (size_t)blockIdx.x * 3 * DP, theta_inv + base, D, tfac_behind_flags<DP>(tri, gridDim.x, blockIdx.x));
  __syncthreads();  // (the solver ends with a barrier of its own only if there are reflectors, D > 2)
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

// ---- not templated on NT: in the host unit only
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
#endif  // !UGLAD_TU_NT

}  // namespace uglad
