// LambdaNN steps, deterministic reductions and the consensus of K estimates: small kernels, none templated on NT, so the whole
// header is for the host unit (the per-NT units would define them again).
#pragma once
#include "glad_device.h"

namespace uglad {

#ifndef UGLAD_TU_NT
// =============================================================================================== lambda / reductions
// one thread per group g < G: lam (.., G), lam_in (.., G, 2), params (G, 42)
__global__ void lambda_init_kernel(const float* __restrict__ params, float lambda_init, float* __restrict__ lam_out,
                                   float* __restrict__ lam_in, int G) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < G) {
    lam_in[2 * g] = lambda_init;
    lam_in[2 * g + 1] = 0.f;
    lam_out[g] = lambda_forward(params + (size_t)g * kNParam, lambda_init, 0.f);
  }
}

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

// sum_partials + lambda_step in one launch (the single-process pass: nothing to exchange between the two).  One block per
// group; same summation order as sum_partials_kernel, so the sharded and the fused path see the same bits per rank.
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

__global__ void zero_kernel(float* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0.f;
}

// deterministic: fixed per-thread strides, fixed tree
__global__ __launch_bounds__(kThreads) void sum_partials_kernel(const float* __restrict__ partials, int n,
                                                                float* __restrict__ out) {
  __shared__ float s_red[8];
  partials += (size_t)blockIdx.x * n;  // one block per group
  float v = 0.f;
  for (int i = threadIdx.x; i < n; i += kThreads) v += partials[i];
  v = block_sum(v, s_red);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// grad[0] <- sum gt ; grad[1..28] <- column sums of grad_rho_partial ; grad[29..41] <- LambdaNN chain
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

// =============================================================================================== consensus
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

__global__ void consensus_combine_kernel(const float* __restrict__ absmin, const float* __restrict__ signsum, int DD,
                                         float* __restrict__ out) {
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < DD; idx += gridDim.x * blockDim.x)
    out[idx] = (signsum[idx] >= 0.f ? 1.f : -1.f) * absmin[idx];
}
#endif  // !UGLAD_TU_NT

}  // namespace uglad
