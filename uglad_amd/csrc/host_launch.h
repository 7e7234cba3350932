// Host layer, part 2: the launch sequences.  Every function takes the Route of its call (host_route.h) and asks nothing else about the path.
#pragma once

// the tridiagonalisation launch every eigendecomposition starts with (tridiag.h); R = the D x D slab of each matrix that will receive
// that matrix's final output; only: per-matrix flags (0 = skip this matrix) or nullptr = all
static void launch_tridiag(const Route& r, hipStream_t st, const float* A0, const float* A1, const float* lam, float* R, float* tri,
                           const int* only = nullptr) {
  const int M = r.M, D = r.D;
  for_nt(D, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    if constexpr (NT == 1) {
      if (r.tridiag == Tridiag::kWave) {
        hipLaunchKernelGGL((tridiag_wave_kernel<NT>), dim3(M), dim3(64), 0, st, A0, A1, lam, R, tri, D, r.gs, only);
        return;
      }
    }
    if constexpr (NT <= 3) {
      if (r.tridiag == Tridiag::kSmall) {
        hipLaunchKernelGGL((tridiag_kernel<NT, 128 * NT>), dim3(M), dim3(128 * NT), 0, st, A0, A1, lam, R, tri, D, r.gs, only);
        return;
      }
    }
    if constexpr (NT > 4) {
      if (r.tridiag == Tridiag::kBig) {
        hipLaunchKernelGGL((tridiag_kernel<NT, 1024>), dim3(M), dim3(1024), 0, st, A0, A1, lam, R, tri, D, r.gs, only);
        return;
      }
    }
    hipLaunchKernelGGL((tridiag_kernel<NT, kThreads>), dim3(M), dim3(kThreads), 0, st, A0, A1, lam, R, tri, D, r.gs, only);
  });
}

// Few large matrices: the eigen-decomposition after the single-workgroup front (tridiagonalisation and merges below the last one have
// run; reflectors in the slab R of each matrix): secular roots and eigenvector update of the last merge with many workgroups per
// matrix (wide_fwd.h), back-transformation on two.  Leaves U in the matrix's second big buffer (row stride DP + 1) and the eigenvalues
// in place of d in its (d, e, tau) record.
static void launch_wide_eig_tail(const Route& r, hipStream_t st, const EigLayout& l, const float* R, float* U_out, float* beta_out) {
  const int M = r.M, D = r.D, ntp = wide_tiles(l.DP);
  hipLaunchKernelGGL(wide_secular_kernel, dim3((D + kWThreads / 8 - 1) / (kWThreads / 8), M), dim3(kWThreads), 0, st, l.T, l.tfac, l.tri, l.rec,
                     D, l.DP);
  hipLaunchKernelGGL(wide_merge_kernel, dim3(ntp, ntp, M), dim3(kWThreads), 0, st, (const float*)l.big0, l.big1, l.slab, (const float*)l.T,
                     l.tfac, D, l.DP, l.LD);
  dispatch_nt<5, 8>(D, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    hipLaunchKernelGGL((cell_fwd_back_kernel<NT>), dim3((NT * 2 + kWaves - 1) / kWaves, M), dim3(kThreads), 0, st, (const float*)l.tri, l.T, R,
                       U_out, beta_out, D, M);
  });
}

// The same for a plain symmetric matrix whose tridiagonalisation has just been enqueued (launch_tridiag(A, ..., out, workspace)), and
// then out = (A + shift I)^-1 = U diag(1 / (beta + shift)) U^T with one Newton step, every product with one workgroup per 64 x 64 tile.
// shift: device scalar per group with stride shift_stride floats, or nullptr.
static void launch_wide_inverse(const Route& r, hipStream_t st, const float* A, const float* shift, int shift_stride, float* out,
                                float* workspace) {
  const int M = r.M, D = r.D, nt = wide_tiles(D), gs = r.gs;
  const EigLayout l = eig_layout(workspace, M, D);
  const int LD = l.LD;
  const size_t rec = l.rec, slab = l.slab, dd = (size_t)D * D;
  float *Q0 = l.big0, *Q1 = l.big1;  // eigenvectors before the last merge | after it, then back-transformed in place: U
  // front: everything below the last merge, one workgroup per matrix (the cell's kernel in its split mode; it only touches the
  // workspace then, the other pointers just have to be valid)
  for_nt(D, [&](auto ntc) {
    hipLaunchKernelGGL((cell_fwd_lean_kernel<decltype(ntc)::value>), dim3(M), dim3(kThreads), 0, st, A, A, (const float*)workspace,
                       (const float*)workspace, out, (float*)nullptr, (float*)nullptr, (float*)nullptr, workspace, (float*)nullptr,
                       (const float*)workspace, l.T, D, UGLAD_SQRT_EXACT, gs, 2, LamStep{});
  });
  launch_wide_eig_tail(r, st, l, out, nullptr, nullptr);
  const WideFwd nofw{nullptr, nullptr, nullptr, nullptr};
  const dim3 tiles(nt, nt, M), blk(kWThreads);
  hipLaunchKernelGGL((wide_gemm_kernel<false, true, kEpiInverse>), tiles, blk, 0, st, (const float*)Q1, slab, (const float*)Q1, slab, Q0,
                     slab, (const float*)nullptr, (const float*)workspace, shift, (float*)nullptr, rec, shift_stride, D, 0, gs, LD, LD,
                     LD, nofw);  // X0 = U f U^T -> first buffer
  hipLaunchKernelGGL((wide_gemm_kernel<false, false, kEpiResidual>), tiles, blk, 0, st, A, dd, (const float*)Q0, slab, Q1, slab,
                     (const float*)nullptr, (const float*)nullptr, shift, (float*)nullptr, rec, shift_stride, D, 0, gs, D, LD, LD,
                     nofw);  // E = I - (A + shift I) X0 -> second buffer (U is dead)
  hipLaunchKernelGGL((wide_gemm_kernel<false, false, kEpiNewton>), tiles, blk, 0, st, (const float*)Q0, slab, (const float*)Q1, slab, out,
                     dd, (const float*)nullptr, (const float*)nullptr, shift, (float*)nullptr, rec, shift_stride, D, 0, gs, LD, LD, D,
                     nofw);  // out = X0 + X0 E
}

// one step of the backward pass: the arrays of that step, as uglad_cell_bwd takes them
struct BwdStep {
  const float *G_next, *S, *Z_in, *half, *U, *beta, *lam, *params;
  float *G_out, *grad_rho_partial, *glam_partial;
};

static int launch_cell_bwd_wide(const Route& r, hipStream_t st, const BwdStep& s, float* workspace) {
  const int M = r.M, D = r.D, nt = wide_tiles(D), nup = kWQ * (nt * (nt + 1) / 2), gs = r.gs, sqrt_mode = r.sqrt_mode;  // nup: phase-A workgroups per matrix
  const EigLayout l = eig_layout(workspace, M, D);
  const size_t pstride = l.hdr, slab = l.slab, dd = (size_t)D * D;  // (partial sums: in the region the forward's d, e, tau, T factors use)
  float *part = workspace, *X0 = l.big0, *X1 = l.big1;
  const float *U = s.U, *lam = s.lam;
  const dim3 tiles(nt, nt, M), blk(kWThreads);
  const WideFwd nofw{nullptr, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(wide_phase_a_kernel, dim3(nup, M), blk, 0, st, s.G_next, s.S, s.Z_in, s.half, s.params, X0, s.G_out, part, D, gs, slab,
                     pstride);
  hipLaunchKernelGGL((wide_gemm_kernel<true, false, kEpiStore>), tiles, blk, 0, st, U, dd, (const float*)X0, slab, X1, slab,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (size_t)0, 0, D, sqrt_mode,
                     gs, D, D, D, nofw);  // R = U^T G_half
  hipLaunchKernelGGL((wide_gemm_kernel<false, false, kEpiDivDiff>), tiles, blk, 0, st, (const float*)X1, slab, U, dd, X0, slab,
                     (const float*)nullptr, s.beta, lam, part, pstride, nup * kNRho, D, sqrt_mode, gs, D, D, D, nofw);  // Y = (R U) o F
  hipLaunchKernelGGL((wide_gemm_kernel<false, false, kEpiStore>), tiles, blk, 0, st, U, dd, (const float*)X0, slab, X1, slab,
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (size_t)0, 0, D, sqrt_mode,
                     gs, D, D, D, nofw);  // T2 = U Y
  hipLaunchKernelGGL((wide_gemm_kernel<false, true, kEpiGout>), tiles, blk, 0, st, (const float*)X1, slab, U, dd, s.G_out, dd, s.S,
                     (const float*)nullptr, lam, part, pstride, nup * kNRho + nt * nt, D, sqrt_mode, gs, D, D, D, nofw);  // G_out -= T2 U^T
  hipLaunchKernelGGL(wide_reduce_kernel, dim3(M, kNRho + 1), dim3(64), 0, st, (const float*)part, pstride, s.grad_rho_partial, s.glam_partial, D);
  return launch_status();
}

// ---- the matrix-iteration path (wide_ns.h)
static inline dim3 ns_ew_grid(int M, int D) {
  const size_t dd = (size_t)D * D;
  return dim3((unsigned)((dd + 255) / 256 < 256 ? (dd + 255) / 256 : 256), (unsigned)M);
}
static inline int ns_tiles_per_dim(const Route& r) { return r.ns_tile == 32 ? (r.D + 31) / 32 : wide_tiles(r.D); }
// one launch of up to three independent products C = alpha op(A) B + beta C + gamma I (fp64; ta: A is read transposed)
struct NsLaunch {
  NsBatch b{};
  NsLaunch& add(const double* A, const double* B, double* C, double alpha, double beta, double gamma, bool ta = false) {
    b.p[b.n++] = NsProd{A, B, C, alpha, beta, gamma, ta ? 1 : 0};
    return *this;
  }
};
// (the tiling follows the batch alone, not the products per launch: per-tile sums and their readers agree on it)
template <int EPI>
static void ns_gemm(const Route& r, hipStream_t st, const NsLayout& l, const NsLaunch& nl, const NsEpi& ep) {
  const int D = r.D, ntd = ns_tiles_per_dim(r);
  const dim3 grid(ntd, ntd, r.M * nl.b.n), blk(kWThreads);
  if (r.ns_tile == 32 && r.ns_prefetch_all) hipLaunchKernelGGL((ns_gemm64_kernel<EPI, 32, true>), grid, blk, 0, st, nl.b, l.dregion, D, ep);
  else if (r.ns_tile == 32) hipLaunchKernelGGL((ns_gemm64_kernel<EPI, 32>), grid, blk, 0, st, nl.b, l.dregion, D, ep);
  else hipLaunchKernelGGL((ns_gemm64_kernel<EPI, 64>), grid, blk, 0, st, nl.b, l.dregion, D, ep);
}
static void ns_products(const Route& r, hipStream_t st, const NsLayout& l, const NsLaunch& nl, const float* gamma_div = nullptr, bool frob = false) {
  NsEpi ep{};
  ep.gamma_div = gamma_div;
  ep.hdr = frob ? l.H : nullptr;
  ep.hdr_stride = l.hdr;
  ep.gs = r.gs;
  ns_gemm<kNsAffine>(r, st, l, nl, ep);
}

static int launch_cell_fwd_ns(const Route& r, hipStream_t st, const float* S, const float* Z_in, const float* lam, const float* params,
                              float* Z_out, float* half_out, float* sqrt_out, float* normF_partial, float* cond_max, float* workspace) {
  const int M = r.M, D = r.D, nt = wide_tiles(D), gs = r.gs;
  const NsLayout l = ns_layout(workspace, M, D);
  double* Wb = l.Wd;                  // b
  double* Wy = l.Wd + 1 * l.dslab;    // A -> Y
  double* Wt = l.Wd + 2 * l.dslab;    // T
  double* Wz = l.Wd + 3 * l.dslab;    // Z
  double* Wy2 = l.Wd + 4 * l.dslab;   // the next Y
  double* Wz2 = l.Wd + 5 * l.dslab;   // the next Z
  const dim3 ew = ns_ew_grid(M, D);
  hipLaunchKernelGGL(ns_b_kernel, ew, dim3(256), 0, st, S, Z_in, lam, Wb, l.dregion, D, gs);
  ns_products(r, st, l, NsLaunch().add(Wb, Wb, Wy, 1.0, 0.0, 4.0, true), lam, true);  // A = b^T b + 4/lam I, ||A||_F^2 per tile
  if (cond_max) hipLaunchKernelGGL(ns_cond_kernel, dim3(nt, M), dim3(256), 0, st, (const double*)Wy, l.dregion, l.H, l.hdr, D);
  const int ntd = ns_tiles_per_dim(r);
  hipLaunchKernelGGL(ns_norm_kernel, dim3(M), dim3(64), 0, st, l.H, l.hdr, lam, cond_max, D, gs, ntd * ntd);
  hipLaunchKernelGGL(ns_start_kernel, ew, dim3(256), 0, st, Wy, Wt, Wz, l.dregion, (const float*)l.H, l.hdr, D);
  ns_products(r, st, l, NsLaunch().add(Wy, Wt, Wy2, 1.0, 0.0, 0.0));  // Y1 = Y0 T0  (Z1 = T0 is in place)
  double *Y = Wy2, *Yn = Wy, *Z = Wz, *Zn = Wz2;
  for (int t = 1; t < kNsIters; ++t) {
    ns_products(r, st, l, NsLaunch().add(Z, Y, Wt, -0.5, 0.0, 1.5));  // T = (3 I - Z Y) / 2
    if (t + 1 < kNsIters) {
      ns_products(r, st, l, NsLaunch().add(Y, Wt, Yn, 1.0, 0.0, 0.0).add(Wt, Z, Zn, 1.0, 0.0, 0.0));  // Y <- Y T ; Z <- T Z
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
  ns_gemm<kNsTheta>(r, st, l, NsLaunch().add(Y, Wt, nullptr, 1.0, 0.0, 0.0), ep);
  hipLaunchKernelGGL(ns_norm_reduce_kernel, dim3(M), dim3(64), 0, st, (const float*)l.H, l.hdr, ntd, normF_partial, D);
  return launch_status();
}

static int launch_cell_bwd_ns(const Route& r, hipStream_t st, const BwdStep& s, float* workspace) {
  const int M = r.M, D = r.D, nt = wide_tiles(D), nup = kWQ * (nt * (nt + 1) / 2), gs = r.gs;
  const NsLayout l = ns_layout(workspace, M, D);
  const float* sqrtm = s.U;  // (this path saves the square root where the spectral path saves U)
  double* Wb = l.Wd;                  // b
  double* Wa = l.Wd + 1 * l.dslab;    // A
  double* Wp = l.Wd + 2 * l.dslab;    // P
  double* Wq = l.Wd + 3 * l.dslab;    // Q
  double* Wr = l.Wd + 4 * l.dslab;    // R, then Q + Q^T
  double* Wa2 = l.Wd + 5 * l.dslab;   // the next A
  double* Wq2 = l.Wd + 6 * l.dslab;   // the next Q
  const dim3 ew = ns_ew_grid(M, D);
  hipLaunchKernelGGL(wide_phase_a_kernel, dim3(nup, M), dim3(kWThreads), 0, st, s.G_next, s.S, s.Z_in, s.half, s.params, l.Gh, s.G_out, l.H, D, gs,
                     l.region, l.hdr);
  hipLaunchKernelGGL(ns_b_kernel, ew, dim3(256), 0, st, s.S, s.Z_in, s.lam, Wb, l.dregion, D, gs);
  hipLaunchKernelGGL(ns_frob_kernel, dim3(kNsFrobBlocks, M), dim3(256), 0, st, sqrtm, (size_t)D * D, l.H, l.hdr, D);
  hipLaunchKernelGGL(ns_bwd_start_kernel, ew, dim3(256), 0, st, sqrtm, (const float*)l.Gh, l.region, Wa, Wq, l.dregion, (const float*)l.H, l.hdr,
                     D);
  double *A = Wa, *An = Wa2, *Q = Wq, *Qn = Wq2;
  for (int t = 0; t < kNsIters; ++t) {  // torch_sqrtm.py:42-44, three launches per step
    const bool more = t + 1 < kNsIters;
    ns_products(r, st, l, NsLaunch().add(A, A, Wp, -1.0, 0.0, 3.0).add(A, Q, Wr, 1.0, 0.0, 0.0, true));  // P = 3 I - A A ; R = A^T Q ...
    NsLaunch second;
    second.add(Q, A, Wr, -1.0, 1.0, 0.0).add(Q, Wp, Qn, 1.0, 0.0, 0.0);  // ... - Q A ; Q' = Q P ...
    if (more) second.add(A, Wp, An, 0.5, 0.0, 0.0);                       // A <- A P / 2
    ns_products(r, st, l, second);
    ns_products(r, st, l, NsLaunch().add(A, Wr, Qn, -0.5, 0.5, 0.0, true));  // ... - A^T R, halved
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
  ep.S = s.S;
  ep.lam = s.lam;
  ep.Zout = s.G_out;
  ep.Gh = l.Gh;
  ep.gh_stride = l.region;
  const int ntd = ns_tiles_per_dim(r);
  ns_gemm<kNsGout>(r, st, l, NsLaunch().add(Wb, Wr, nullptr, 1.0, 0.0, 0.0), ep);
  hipLaunchKernelGGL(ns_glam_kernel, dim3(M), dim3(64), 0, st, l.H, l.hdr, ntd * ntd, nup * kNRho, D);
  hipLaunchKernelGGL(wide_reduce_kernel, dim3(M, kNRho + 1), dim3(64), 0, st, (const float*)l.H, l.hdr, s.grad_rho_partial, s.glam_partial, D);
  return launch_status();
}

// the slab layout of the L D L^T inverse (ldl_wide.h): f(std::integral_constant<int, ns_fact_dim(D)>)
template <class F>
static inline void ldl_layout(int D, F&& f) {
  if (ns_fact_dim(D) == kNsFactSmall) return f(std::integral_constant<int, kNsFactSmall>{});
  f(std::integral_constant<int, kNsMaxD>{});
}

// out = (A + shift I)^-1 (and log det in logdet_out) wherever Route::factor is kLdl: L D L^T of the padded matrix (ldl_wide.h), two Newton steps
static void launch_ns_inverse(const Route& r, hipStream_t st, const float* A, const float* shift, int shift_stride, float* out, float* logdet_out,
                              float* workspace) {
  const int M = r.M, D = r.D, nt = wide_tiles(D), gs = r.gs, FD = ns_fact_dim(D), LDc = FD + 1;
  const NsLayout l = ns_layout(workspace, M, D);
  float* X1 = l.W;                                 // the factorisation's first slab, dead once it returns (row stride FD + 1)
  float* X0 = l.W + 2 * (size_t)FD * (FD + 1);     // (row stride FD + 1)
  float* E = l.W + 3 * (size_t)FD * (FD + 1);      // residual, row stride D
  ldl_layout(D, [&](auto fd) {  // (the kernels are instantiated per slab layout, ns_fact_dim)
    constexpr int kFD = decltype(fd)::value;
    if (!r.ldl_phases) {  // one workgroup per matrix walks the schedule
      hipLaunchKernelGGL(ns_ldl_kernel<kFD>, dim3(M), dim3(64 * kNsLdlWaves), 0, st, A, shift, shift_stride, l.W, l.region, logdet_out, D, gs);
      return;
    }
    // one launch per step: `items` tiles (one wave each) or elements (one thread each, capped) of work per matrix
    ldl_schedule((D + 31) / 32, [&](int ph, int jd, int items) {
      int wgs = 1;
      if (ph == kLdlInit || ph == kLdlScale || ph == kLdlFinish) {
        wgs = (items + 64 * kLdlWavesPerWg - 1) / (64 * kLdlWavesPerWg);
        if (wgs > 512) wgs = 512;
      } else {
        wgs = (items + kLdlWavesPerWg - 1) / kLdlWavesPerWg;
      }
      if (wgs < 1) wgs = 1;
      hipLaunchKernelGGL(ns_ldl_phase_kernel<kFD>, dim3(wgs, M), dim3(64 * kLdlWavesPerWg), 0, st, ph, jd, A, shift, shift_stride, l.W, l.region,
                         logdet_out, D, gs);
    });
  });
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

// ---- the forward cell on the spectral path
// second launch: the lean kernel (eig_lean.h) -- its one big matrix in LDS up to D = 128 (two workgroups per CU), in a workspace buffer beyond.
static int launch_cell_stage2(const Route& r, hipStream_t st, const float* S, const float* Z_in, const float* lam, const float* params,
                              float* Z_out, float* half_out, float* U_out, float* beta_out, float* normF_partial, float* cond_max,
                              float* workspace, const LamStep* ls = nullptr) {
  const int M = r.M, D = r.D, sqrt_mode = r.sqrt_mode;
  const EigLayout l = eig_layout(workspace, M, D);
  // few large matrices (wide_bwd.h, wide_fwd.h): the single-workgroup kernel stops before the last merge of the divide & conquer
  // (D > 128: there is one); secular roots, eigenvector update, back-transformation and theta_half follow as their own launches
  const int split = r.wide ? 2 : 0;
  for_nt(D, [&](auto ntc) {
    hipLaunchKernelGGL((cell_fwd_lean_kernel<decltype(ntc)::value>), dim3(M), dim3(kThreads), 0, st, S, Z_in, lam, params, Z_out, half_out, U_out,
                       beta_out, normF_partial, cond_max, workspace, l.T, D, sqrt_mode, r.gs, split, ls && !split ? *ls : LamStep{});
  });
  if (split) {
    const int nt = wide_tiles(D);
    launch_wide_eig_tail(r, st, l, Z_out, U_out, beta_out);
    // theta_half = (U phi) U^T, rhoNN + threshold and the norm with one workgroup per upper 64 x 64 tile (wide_bwd.h); U: second big buffer
    WideFwd fw{Z_in, params, half_out, cond_max};
    hipLaunchKernelGGL((wide_gemm_kernel<false, true, kEpiThetaHalf>), dim3(nt, nt, M), dim3(kWThreads), 0, st, (const float*)l.big1, l.slab,
                       (const float*)l.big1, l.slab, Z_out, (size_t)D * D, S, (const float*)workspace, lam, workspace, l.rec, l.DP, D, sqrt_mode,
                       r.gs, l.LD, l.LD, D, fw);
    hipLaunchKernelGGL(wide_norm_reduce_kernel, dim3((M + 63) / 64), dim3(64), 0, st, (const float*)workspace, l.rec, l.DP, normF_partial, M, D);
  }
  return launch_status();
}

// the cell on the path the route names; ls: the lambda step that follows it, for the kernel to take along (Route::fuse_lambda)
static int launch_cell_fwd(const Route& r, hipStream_t st, const float* S, const float* Z_in, const float* lam, const float* params, float* Z_out,
                           float* half_out, float* U_out, float* beta_out, float* normF_partial, float* cond_max, float* workspace,
                           const LamStep* ls = nullptr) {
  if (!valid_sqrt(r.sqrt_mode)) return UGLAD_E_MODE;
  if (r.cell == CellPath::kMatrixIteration) {
    if (r.sqrt_mode != UGLAD_SQRT_NS10) return UGLAD_E_MODE;  // (the iteration IS the ten-step square root)
    return launch_cell_fwd_ns(r, st, S, Z_in, lam, params, Z_out, half_out, U_out, normF_partial, cond_max, workspace);
  }
  launch_tridiag(r, st, S, Z_in, lam, Z_out, workspace);
  return launch_cell_stage2(r, st, S, Z_in, lam, params, Z_out, half_out, U_out, beta_out, normF_partial, cond_max, workspace, ls);
}

// ---- the backward cell.  r: the route of a TRAINING call of this shape -- the one the forward call that saved this step's state took.
// gS: also accumulate dL/dS into it (the one-workgroup cell has a variant that does; the other two paths run the step as it is, then its dL/dS)
static int launch_cell_bwd(const Route& r, hipStream_t st, const BwdStep& s, float* workspace, float* gS = nullptr) {
  const int M = r.M, D = r.D;
  if (D > 128 && !workspace) return UGLAD_E_NULL;
  if (!valid_sqrt(r.sqrt_mode)) return UGLAD_E_MODE;
  if (r.cell == CellPath::kOneWorkgroup) {
    for_nt(D, [&](auto ntc) {
      constexpr int NT = decltype(ntc)::value;
      if (gS)
        hipLaunchKernelGGL((cell_bwd_gs_kernel<NT>), dim3(M), dim3(kThreads), 0, st, s.G_next, s.S, s.Z_in, s.half, s.U, s.beta, s.lam, s.params,
                           s.G_out, s.grad_rho_partial, s.glam_partial, workspace, D, r.sqrt_mode, r.gs, 1, 0, gS);
      else
        hipLaunchKernelGGL((cell_bwd_kernel<NT>), dim3(M), dim3(kThreads), 0, st, s.G_next, s.S, s.Z_in, s.half, s.U, s.beta, s.lam, s.params,
                           s.G_out, s.grad_rho_partial, s.glam_partial, workspace, D, r.sqrt_mode, r.gs, 1, 0);
    });
    return launch_status();
  }
  if (r.cell == CellPath::kMatrixIteration && r.sqrt_mode != UGLAD_SQRT_NS10) return UGLAD_E_MODE;
  const int rc = r.cell == CellPath::kMatrixIteration ? launch_cell_bwd_ns(r, st, s, workspace) : launch_cell_bwd_wide(r, st, s, workspace);
  if (rc || !gS) return rc;
  const size_t mdd = (size_t)M * D * D;
  hipLaunchKernelGGL(cell_gs_step_kernel, dim3(blocks256(mdd, 4096)), dim3(256), 0, st, s.G_next, s.S, s.Z_in, s.half, s.lam, s.params,
                     (const float*)s.G_out, gS, D, r.gs, mdd);
  return launch_status();
}

// Steps L-1 .. 0 of the backward pass in one launch (D <= 128, one workgroup per matrix): dL/dZ never leaves LDS between the steps.
// s: the LAST step's arrays of the whole-pass ones (step-major, as uglad_glad_backward takes them); G_out receives dL/dZ_0.
static int launch_cell_bwd_all_steps(const Route& r, hipStream_t st, const BwdStep& s, int L, float* gS) {
  const int M = r.M, D = r.D;
  for_nt_lds(D, [&](auto ntc) {
    constexpr int NT = decltype(ntc)::value;
    if (gS)
      hipLaunchKernelGGL((cell_bwd_gs_kernel<NT>), dim3(M), dim3(kThreads), 0, st, s.G_next, s.S, s.Z_in, s.half, s.U, s.beta, s.lam, s.params,
                         s.G_out, s.grad_rho_partial, s.glam_partial, nullptr, D, r.sqrt_mode, r.gs, L, r.groups, gS);
    else
      hipLaunchKernelGGL((cell_bwd_kernel<NT>), dim3(M), dim3(kThreads), 0, st, s.G_next, s.S, s.Z_in, s.half, s.U, s.beta, s.lam, s.params,
                         s.G_out, s.grad_rho_partial, s.glam_partial, nullptr, D, r.sqrt_mode, r.gs, L, r.groups);
  });
  return launch_status();
}

// ---- Theta_0 = (S + t I)^-1 and the loss's log det / inverse, on the factorisation the route names
// the spectral ones: Cholesky first where the route says so, then the tridiagonalisation (of the flagged matrices only) for `finish` to build on
template <class Chol>
static const int* launch_factor_front(const Route& r, hipStream_t st, const float* A, float* out, float* workspace, Chol&& chol) {
  const int* only = nullptr;
  if (r.factor == Factor::kCholesky) {
    int* flags = eig_layout(workspace, r.M, r.D).flags;
    for_nt_lds(r.D, [&](auto nt) { chol(nt, flags); });
    only = flags;
  }
  launch_tridiag(r, st, A, nullptr, nullptr, out, workspace, only);
  return only;
}

// Zero n floats with a kernel, not hipMemsetAsync: captured into a caller's graph (PyTorch's stream capture, ROCm 7.2) the memset NODES of the two
// small zero-fills of a pass did not replay as zero-fills -- the 4-byte one left 5e36 behind, the 112-byte one left every other float
// unzeroed (tests/test_gpu_parity.py::test_a_whole_pass_can_be_captured_into_the_callers_graph failed on exactly these two buffers) --
// while a kernel node replays as launched.
static int zero_floats(float* p, size_t n, hipStream_t st) {
  hipLaunchKernelGGL(zero_kernel, dim3(blocks256(n, 1024)), dim3(256), 0, st, p, n);
  return launch_status();
}
