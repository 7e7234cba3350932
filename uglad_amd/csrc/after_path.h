// Around the unrolled path: the two symeig exports of the unit tests, the covariance
// front-end of fit(), and what follows a fit -- MAP solve, partial correlations, support-recovery metrics.
#pragma once
#include "eig_lean.h"
#include "theta0.h"

namespace uglad {

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

// =============================================================================================== after the path
// ---- N3: conditional Gaussian / MAP estimate given observed coordinates (main.py:1176-1260).  With the precision matrix
// partitioned into unobserved (u) and observed (o) coordinates the reference computes  mean_u - L_uu^-1 L_uo (x_o - mean_o)
// (scipy.linalg.solve), the conditional covariance L_uu^-1 and the density at the MAP point.  Here L_uu stays IN PLACE: the
// masked matrix A (A_ij = P_ij for i, j both unobserved, delta_ij otherwise) has L_uu^-1 as the (u, u) block of its inverse and
// the identity elsewhere, so no gather / scatter is needed and the path's own eigensolver does the solve.
// (map_prepare_kernel, at the end of this header, writes A.)
template <int NT>
__global__ __launch_bounds__(kThreads) void map_solve_kernel(const float* __restrict__ P, const float* __restrict__ mean,
                                                             const float* __restrict__ observed,
                                                             const float* __restrict__ values, const float* __restrict__ A,
                                                             float* __restrict__ full_mean, float* __restrict__ cond_cov,
                                                             float* __restrict__ log_pdf, float* __restrict__ tri, int D,
                                                             int clip01) {
  constexpr int DP = NT * 32, LD = DP + 1;
  UGLAD_BIG_BUFFERS(sV, DP * LD, sA, DP * LD, tri)  // eigenvectors ; scratch of spectral_to_global
  __shared__ __attribute__((aligned(16))) LeanScratch<DP> ws;
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
  symeig_lean<NT>(sV, D, ws, tri + (size_t)blockIdx.x * 3 * DP, cond_cov + base, D, tfac_behind_flags<DP>(tri, gridDim.x, blockIdx.x));
  __syncthreads();  // (the solver ends with a barrier of its own only if there are reflectors, D > 2)
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

// ---- not templated on NT: in the host unit only
#ifndef UGLAD_TU_NT
// S += (offset - min eig) I where the smallest eigenvalue is <= 1e-6 (beta ascending: beta[0] is the smallest)
__global__ void cov_repair_kernel(float* __restrict__ S, const float* __restrict__ beta, int D, float offset) {
  const float mn = beta[(size_t)blockIdx.x * D];
  if (mn <= 1e-6f) {
    float* So = S + (size_t)blockIdx.x * D * D;
    for (int i = threadIdx.x; i < D; i += blockDim.x) So[i * D + i] += offset - mn;
  }
}

// ---- N3: the masked matrix A that map_solve_kernel inverts (see there)
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

// ---- N4: partial correlations (main.py:796-821): rho_ij = -p_ij / sqrt(p_ii p_jj) from the UPPER triangle, mirrored, 1 on the diagonal
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
#endif  // !UGLAD_TU_NT

}  // namespace uglad
