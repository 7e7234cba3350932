// Host layer, part 3: the extern "C" entry points of the pass (include/uglad_hip.h).  A public entry point validates its arguments, builds
// the Route of its call (one group, unless it takes a group count) and calls the internal function the whole-pass entry points call too.
#pragma once

// ---- internals: arguments are valid, the route is the caller's
static int init_theta(const Route& r, hipStream_t st, const float* S, const float* params, int init_diag, float* theta0, float* workspace) {
  const int M = r.M, D = r.D;
  if (init_diag == 1) {
    const size_t total = (size_t)M * D * D;
    hipLaunchKernelGGL(init_diag_kernel, dim3(blocks256(total, 2048)), dim3(256), 0, st, S, params, theta0, D, total, r.gs);
  } else if (init_diag != 0) {
    return UGLAD_E_MODE;
  } else if (r.factor == Factor::kLdl) {
    launch_ns_inverse(r, st, S, params + P_T, kNParam, theta0, nullptr, workspace);
  } else {
    const int* only = launch_factor_front(r, st, S, theta0, workspace, [&](auto nt, int* flags) {
      hipLaunchKernelGGL((chol_init_kernel<decltype(nt)::value>), dim3(M), dim3(kThreads), 0, st, S, params, theta0, flags, D, r.gs);
    });
    if (r.factor == Factor::kWideInverse) {
      launch_wide_inverse(r, st, S, params + P_T, kNParam, theta0, workspace);
    } else {
      for_nt(D, [&](auto nt) {
        hipLaunchKernelGGL((init_inverse_kernel<decltype(nt)::value>), dim3(M), dim3(kThreads), 0, st, S, params, theta0, workspace, D, r.gs, only);
      });
    }
  }
  return launch_status();
}

static int init_theta_bwd(const Route& r, hipStream_t st, const float* theta0, const float* G0, int init_diag, float* gt_partial,
                          float* workspace) {
  const int M = r.M, D = r.D;
  if (init_diag == 1) {
    hipLaunchKernelGGL(init_bwd_diag_kernel, dim3(M), dim3(kThreads), 0, st, theta0, G0, gt_partial, D);
  } else if (init_diag != 0) {
    return UGLAD_E_MODE;
  } else if (r.factor == Factor::kLdl) {  // gt_partial = -<G0^T, Theta0 Theta0>, one workgroup per tile of the product
    const NsLayout l = ns_layout(workspace, M, D);
    const int nt = wide_tiles(D);
    WideFwd fw{};
    fw.X = G0;
    fw.x_stride = (size_t)D * D;
    hipLaunchKernelGGL((wide_gemm_kernel<false, false, kEpiDotT>), dim3(nt, nt, M), dim3(kWThreads), 0, st, theta0, (size_t)D * D, theta0,
                       (size_t)D * D, (float*)nullptr, (size_t)0, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, l.H,
                       l.hdr, ns_off_tiles(D), D, 0, r.gs, D, D, D, fw);
    hipLaunchKernelGGL(ns_tile_sum_kernel, dim3((M + 63) / 64), dim3(64), 0, st, (const float*)l.H, l.hdr, gt_partial, -1.f, M, D);
  } else {
    for_nt(D, [&](auto nt) {
      hipLaunchKernelGGL((init_bwd_kernel<decltype(nt)::value>), dim3(M), dim3(kThreads), 0, st, theta0, G0, gt_partial, workspace, D);
    });
  }
  return launch_status();
}

static int lambda_init(int groups, hipStream_t st, const float* params, float lambda_init, float* lam_out, float* lam_in) {
  hipLaunchKernelGGL(lambda_init_kernel, dim3((groups + 63) / 64), dim3(64), 0, st, params, lambda_init, lam_out, lam_in, groups);
  return launch_status();
}
static int sum_partials(int groups, int gs, hipStream_t st, const float* partials, float* out) {
  hipLaunchKernelGGL(sum_partials_kernel, dim3(groups), dim3(kThreads), 0, st, partials, gs, out);
  return launch_status();
}
static int lambda_step(int groups, hipStream_t st, const float* normF_sum, float inv_M, const float* lam_prev, const float* params, float* lam_next,
                       float* lam_in_next) {
  hipLaunchKernelGGL(lambda_step_kernel, dim3((groups + 63) / 64), dim3(64), 0, st, normF_sum, inv_M, lam_prev, params, lam_next, lam_in_next,
                     groups);
  return launch_status();
}
static int finish_grads(int groups, int gs, hipStream_t st, const float* gt_partial, const float* grad_rho_partial, const float* glam_partial,
                        const float* lam_in, const float* params, float* grad, int L, int M) {
  hipLaunchKernelGGL(finish_grads_kernel, dim3(groups), dim3(kThreads), 0, st, gt_partial, grad_rho_partial, glam_partial, lam_in, params, grad, L,
                     M, gs);
  return launch_status();
}

// ---- the whole unrolled pass in one call.  exchange: the sharded batch's SUM over the ranks between the norm and the lambda step
// (m_global matrices in all); without one nothing happens between them and they are one launch, or part of the cell's (Route::fuse_lambda)
static int enqueue_glad_forward(int groups, const float* S, const float* params, float lambda_init_value, int init_diag, int L, float* Z,
                                int z_slabs, float* half, float* U, float* beta, float* lam, float* lam_in, float* nf_partial,
                                float* nf_sum, float* cond_max, float* workspace, int M, int D, int sqrt_mode, hipStream_t st,
                                int m_global = 0, uglad_allreduce_fn exchange = nullptr, void* exchange_ctx = nullptr) {
  if (!S || !params || !Z || !lam || !lam_in || !nf_partial || !nf_sum || !workspace) return UGLAD_E_NULL;
  const Route r = make_route(M, D, groups, half != nullptr || U != nullptr, sqrt_mode);
  int rc = check_dims(r);
  if (rc) return rc;
  if (L < 1 || z_slabs < 2) return UGLAD_E_DIM;
  const size_t mdd = (size_t)M * D * D;
  if ((rc = init_theta(r, st, S, params, init_diag, Z, workspace))) return rc;
  if (cond_max) {  // running maximum over the L steps: starts at 0
    if ((rc = zero_floats(cond_max, (size_t)M, st))) return rc;
  }
  if ((rc = lambda_init(groups, st, params, lambda_init_value, lam, lam_in))) return rc;
  const int G = groups;  // lam: (L + 1, G), lam_in: (L + 1, G, 2), nf_sum: (G)
  const float inv_m = 1.0f / (float)(exchange ? m_global : r.gs);
  const bool fuse_lambda = r.fuse_lambda && !exchange;
  for (int k = 0; k < L; ++k) {
    const float* zi = Z + (size_t)(k % z_slabs) * mdd;
    float* zo = Z + (size_t)((k + 1) % z_slabs) * mdd;
    const float* lamk = lam + (size_t)k * G;
    float *lam_next = lam + (size_t)(k + 1) * G, *lam_in_next = lam_in + 2 * (size_t)(k + 1) * G;
    const LamStep ls{nf_sum, lam_next, lam_in_next, inv_m};
    rc = launch_cell_fwd(r, st, S, zi, lamk, params, zo, half ? half + (size_t)k * mdd : nullptr, U ? U + (size_t)k * mdd : nullptr,
                         beta ? beta + (size_t)k * M * D : nullptr, nf_partial, cond_max, workspace, fuse_lambda ? &ls : nullptr);
    if (rc) return rc;
    if (fuse_lambda) continue;
    if (exchange) {
      // sharded batch: local sum -> SUM over the ranks (stream-ordered, no host decision) -> LambdaNN on every rank from the same bits
      if ((rc = sum_partials(G, r.gs, st, nf_partial, nf_sum))) return rc;
      if ((rc = exchange(nf_sum, 1, exchange_ctx, (uglad_stream_t)st))) return rc;
      if ((rc = lambda_step(G, st, nf_sum, inv_m, lamk, params, lam_next, lam_in_next))) return rc;
      continue;
    }
    // (sum_partials + lambda_step as one launch: nothing is exchanged between them in a single-process pass)
    hipLaunchKernelGGL(norm_lambda_kernel, dim3(G), dim3(kThreads), 0, st, nf_partial, r.gs, inv_m, lamk, params, nf_sum, lam_next, lam_in_next);
    if ((rc = launch_status())) return rc;
  }
  return 0;
}

static int enqueue_glad_backward(int groups, const float* G_L, const float* S, const float* params, int init_diag, int L, const float* Z,
                                 const float* half, const float* U, const float* beta, const float* lam, const float* lam_in,
                                 float* gbuf0, float* gbuf1, float* grad_rho_partial, float* glam_partial, float* gt_partial,
                                 float* grad, float* workspace, int M, int D, int sqrt_mode, hipStream_t st, float* gS = nullptr) {
  if (!G_L || !S || !params || !Z || !half || !U || !beta || !lam || !lam_in || !gbuf0 || !gbuf1 || !grad_rho_partial ||
      !glam_partial || !gt_partial || !grad)
    return UGLAD_E_NULL;
  const Route r = make_route(M, D, groups, true, sqrt_mode);  // (as the forward pass that saved the state)
  int rc = check_dims(r);
  if (rc) return rc;
  if (L < 1) return UGLAD_E_DIM;
  const size_t mdd = (size_t)M * D * D;
  if ((rc = zero_floats(grad_rho_partial, (size_t)M * UGLAD_NRHO, st))) return rc;
  if (gS && (rc = zero_floats(gS, mdd, st))) return rc;
  auto step = [&](int k, const float* G_next, float* G_out) {
    return BwdStep{G_next, S, Z + (size_t)k * mdd, half + (size_t)k * mdd, U + (size_t)k * mdd, beta + (size_t)k * M * D, lam + (size_t)k * groups,
                   params, G_out, grad_rho_partial, glam_partial + (size_t)k * M};
  };
  const float* cur = G_L;
  if (r.persistent_bwd) {
    if ((rc = launch_cell_bwd_all_steps(r, st, step(L - 1, G_L, gbuf0), L, gS))) return rc;
    cur = gbuf0;
  } else {
    for (int k = L - 1; k >= 0; --k) {
      float* out = (k & 1) ? gbuf1 : gbuf0;
      if ((rc = launch_cell_bwd(r, st, step(k, cur, out), workspace, gS))) return rc;
      cur = out;
    }
  }
  if ((rc = init_theta_bwd(r, st, Z, cur, init_diag, gt_partial, workspace))) return rc;
  if (gS) {  // the Theta_0 term of dL/dS
    if (init_diag == 1) {
      const size_t total = (size_t)M * D;
      hipLaunchKernelGGL(init_bwd_diag_gs_kernel, dim3(blocks256(total, 1024)), dim3(256), 0, st, (const float*)Z, cur, gS, D, total);
    } else if (r.factor == Factor::kLdl) {  // beyond the one-workgroup kernels: T = Theta0 G0 into the idle G buffer, R = T Theta0 into G0's
      float* T = (cur == gbuf0) ? gbuf1 : gbuf0;
      float* R = const_cast<float*>(cur);
      const dim3 tiles((D + 63) / 64, (D + 63) / 64, M);
      hipLaunchKernelGGL(gs_gemm_kernel, tiles, dim3(256), 0, st, (const float*)Z, cur, T, D);
      hipLaunchKernelGGL(gs_gemm_kernel, tiles, dim3(256), 0, st, (const float*)T, (const float*)Z, R, D);
      hipLaunchKernelGGL(gs_sub_sym_kernel, dim3(blocks256(mdd, 4096)), dim3(256), 0, st, (const float*)R, gS, D, mdd);
    } else {
      for_nt(D, [&](auto nt) {
        hipLaunchKernelGGL((init_bwd_gs_kernel<decltype(nt)::value>), dim3(M), dim3(kThreads), 0, st, Z, cur, gS, workspace, D);
      });
    }
    if ((rc = launch_status())) return rc;
  }
  return finish_grads(groups, r.gs, st, gt_partial, grad_rho_partial, glam_partial, lam_in, params, grad, L, M);
}

static bool valid_groups(int M, int groups) { return groups >= 1 && M >= groups && M % groups == 0; }

extern "C" {

int uglad_version(void) { return 3; }
float uglad_validated_cond(void) { return UGLAD_VALIDATED_COND; }
int uglad_max_dim(void) { return UGLAD_MAX_DIM; }
int uglad_max_eig_dim(void) { return UGLAD_MAX_EIG_DIM; }
int uglad_set_wide_mode(int mode) {
  if (mode < -1 || mode > 1) return UGLAD_E_MODE;
  g_wide_mode.store(mode, std::memory_order_relaxed);
  return 0;
}
int uglad_set_matrix_iteration(int mode) {
  if (mode < -1 || mode > 1) return UGLAD_E_MODE;
  g_ns_mode.store(mode, std::memory_order_relaxed);
  return 0;
}
int uglad_cond_is_upper_bound(int M, int D, int training, int sqrt_mode) {
  if (M < 1 || D < 1 || D > UGLAD_MAX_DIM) return UGLAD_E_DIM;
  return make_route(M, D, 1, training != 0, sqrt_mode).cell == CellPath::kMatrixIteration ? 1 : 0;
}
int uglad_workspace_floats(int M, int D) {
  if (M < 1 || D < 1 || D > UGLAD_MAX_DIM) return UGLAD_E_DIM;
  size_t n = D <= UGLAD_MAX_EIG_DIM ? eig_layout(nullptr, M, D).total(M) : 0;
  if (make_route(M, D, 1, true, UGLAD_SQRT_NS10).ns_any) {  // (either kind of call may take the matrix-iteration path at this shape)
    const size_t nn = ns_layout(nullptr, M, D).total(M);
    if (nn > n) n = nn;
  }
  return n > 2147483647ULL ? UGLAD_E_DIM : (int)n;
}

int uglad_init_theta(const float* S, const float* params, int init_diag, float* theta0, float* workspace, int M, int D,
                     uglad_stream_t stream) {
  if (!S || !params || !theta0 || (init_diag == 0 && !workspace)) return UGLAD_E_NULL;
  const Route r = make_route(M, D, 1, true, UGLAD_SQRT_NS10);
  if (int rc = check_dims(r)) return rc;
  return init_theta(r, (hipStream_t)stream, S, params, init_diag, theta0, workspace);
}

int uglad_init_theta_bwd(const float* theta0, const float* G0, int init_diag, float* gt_partial, float* workspace, int M,
                         int D, uglad_stream_t stream) {
  if (!theta0 || !G0 || !gt_partial || (D > 128 && init_diag == 0 && !workspace)) return UGLAD_E_NULL;
  const Route r = make_route(M, D, 1, true, UGLAD_SQRT_NS10);
  if (int rc = check_dims(r)) return rc;
  return init_theta_bwd(r, (hipStream_t)stream, theta0, G0, init_diag, gt_partial, workspace);
}

int uglad_lambda_init(const float* params, float lambda_init_value, float* lam_out, float* lam_in, uglad_stream_t stream) {
  if (!params || !lam_out || !lam_in) return UGLAD_E_NULL;
  return lambda_init(1, (hipStream_t)stream, params, lambda_init_value, lam_out, lam_in);
}

int uglad_cell_fwd(const float* S, const float* Z_in, const float* lam, const float* params, float* Z_out,
                   float* half_out, float* U_out, float* beta_out, float* normF_partial, float* cond_max, float* workspace, int M,
                   int D, int sqrt_mode, uglad_stream_t stream) {
  if (!S || !Z_in || !lam || !params || !Z_out || !normF_partial || !workspace) return UGLAD_E_NULL;
  const Route r = make_route(M, D, 1, half_out != nullptr || U_out != nullptr, sqrt_mode);
  if (int rc = check_dims(r)) return rc;
  return launch_cell_fwd(r, (hipStream_t)stream, S, Z_in, lam, params, Z_out, half_out, U_out, beta_out, normF_partial, cond_max, workspace);
}

int uglad_cell_fwd_stage2(const float* S, const float* Z_in, const float* lam, const float* params, float* Z_out,
                          float* half_out, float* U_out, float* beta_out, float* normF_partial, float* cond_max, float* workspace,
                          int M, int D, int sqrt_mode, uglad_stream_t stream) {
  if (!S || !Z_in || !lam || !params || !Z_out || !normF_partial || !workspace) return UGLAD_E_NULL;
  const Route r = make_route(M, D, 1, half_out != nullptr || U_out != nullptr, sqrt_mode);
  if (int rc = check_dims(r)) return rc;
  if (!valid_sqrt(sqrt_mode)) return UGLAD_E_MODE;
  if (r.ns_forced) return UGLAD_E_DIM;  // (no tridiagonal stage to follow on the matrix-iteration path: uglad_cell_fwd is one piece there)
  return launch_cell_stage2(r, (hipStream_t)stream, S, Z_in, lam, params, Z_out, half_out, U_out, beta_out, normF_partial, cond_max, workspace);
}

int uglad_sum_partials(const float* partials, int n, float* out, uglad_stream_t stream) {
  if (!partials || !out) return UGLAD_E_NULL;
  if (n < 1) return UGLAD_E_DIM;
  return sum_partials(1, n, (hipStream_t)stream, partials, out);
}

int uglad_lambda_step(const float* normF_sum, float inv_M, const float* lam_prev, const float* params, float* lam_next,
                      float* lam_in_next, uglad_stream_t stream) {
  if (!normF_sum || !lam_prev || !params || !lam_next || !lam_in_next) return UGLAD_E_NULL;
  return lambda_step(1, (hipStream_t)stream, normF_sum, inv_M, lam_prev, params, lam_next, lam_in_next);
}

int uglad_cell_bwd(const float* G_next, const float* S, const float* Z_in, const float* half, const float* U,
                   const float* beta, const float* lam, const float* params, float* G_out, float* grad_rho_partial,
                   float* glam_partial, float* workspace, int M, int D, int sqrt_mode, uglad_stream_t stream) {
  if (!G_next || !S || !Z_in || !half || !U || !beta || !lam || !params || !G_out || !grad_rho_partial || !glam_partial ||
      (D > 128 && !workspace))
    return UGLAD_E_NULL;
  const Route r = make_route(M, D, 1, true, sqrt_mode);
  if (int rc = check_dims(r)) return rc;
  return launch_cell_bwd(r, (hipStream_t)stream, BwdStep{G_next, S, Z_in, half, U, beta, lam, params, G_out, grad_rho_partial, glam_partial}, workspace);
}

int uglad_loss_fwd(const float* theta, const float* S, int s_batch, const float* struct_theta, float* loss_partial,
                   float* theta_inv_out, float* workspace, int M, int D, uglad_stream_t stream) {
  if (!theta || !S || !loss_partial || !theta_inv_out || !workspace) return UGLAD_E_NULL;
  const Route r = make_route(M, D, 1, true, UGLAD_SQRT_NS10);
  if (int rc = check_dims(r)) return rc;
  if (s_batch != 1 && s_batch != M) return UGLAD_E_DIM;
  hipStream_t st = (hipStream_t)stream;
  if (r.factor == Factor::kLdl) {
    const NsLayout l = ns_layout(workspace, M, D);
    launch_ns_inverse(r, st, theta, nullptr, 0, theta_inv_out, loss_partial, workspace);  // (log det parked in loss_partial)
    hipLaunchKernelGGL(wide_loss_trace_kernel, dim3(wide_tiles(D), M), dim3(kWThreads), 0, st, theta, S, s_batch, struct_theta, l.H, l.hdr,
                       ns_off_tiles(D), D);
    hipLaunchKernelGGL(ns_loss_finish_kernel, dim3((M + 63) / 64), dim3(64), 0, st, (const float*)l.H, l.hdr, ns_off_tiles(D),
                       (const float*)loss_partial, loss_partial, M, D);
    return launch_status();
  }
  const int* only = launch_factor_front(r, st, theta, theta_inv_out, workspace, [&](auto nt, int* flags) {
    hipLaunchKernelGGL((chol_loss_kernel<decltype(nt)::value>), dim3(M), dim3(kThreads), 0, st, theta, S, s_batch, struct_theta, loss_partial,
                       theta_inv_out, flags, D);
  });
  if (r.factor == Factor::kWideInverse) {
    const EigLayout l = eig_layout(workspace, M, D);
    launch_wide_inverse(r, st, theta, nullptr, 0, theta_inv_out, workspace);
    hipLaunchKernelGGL(wide_loss_trace_kernel, dim3(wide_tiles(D), M), dim3(kWThreads), 0, st, theta, S, s_batch, struct_theta, workspace, l.rec,
                       l.DP, D);
    hipLaunchKernelGGL(wide_loss_finish_kernel, dim3((M + 63) / 64), dim3(64), 0, st, (const float*)workspace, l.rec, l.DP, loss_partial, M, D);
    return launch_status();
  }
  for_nt(D, [&](auto nt) {
    hipLaunchKernelGGL((loss_fwd_kernel<decltype(nt)::value>), dim3(M), dim3(kThreads), 0, st, theta, S, s_batch, struct_theta, loss_partial,
                       theta_inv_out, workspace, D, only);
  });
  return launch_status();
}

int uglad_loss_bwd(const float* theta, const float* theta_inv, const float* S, int s_batch, const float* struct_theta,
                   const float* g_up, float scale, float* G_out, int M, int D, uglad_stream_t stream) {
  if (!theta || !theta_inv || !S || !g_up || !G_out) return UGLAD_E_NULL;
  if (int rc = check_dims(make_route(M, D, 1, true, UGLAD_SQRT_NS10))) return rc;
  if (s_batch != 1 && s_batch != M) return UGLAD_E_DIM;
  const size_t total = (size_t)M * D * D;
  hipLaunchKernelGGL(loss_bwd_kernel, dim3(blocks256(total, 2048)), dim3(256), 0, (hipStream_t)stream, theta, theta_inv, S, s_batch,
                     struct_theta, g_up, scale, G_out, D, total);
  return launch_status();
}

int uglad_loss_bwd_wrt_s(const float* theta, const float* theta_inv, const float* S, int s_batch, const float* struct_theta,
                         const float* g_up, float scale, float* G_out, float* gS, int M, int D, uglad_stream_t stream) {
  if (!gS) return UGLAD_E_NULL;
  int rc = uglad_loss_bwd(theta, theta_inv, S, s_batch, struct_theta, g_up, scale, G_out, M, D, stream);
  if (rc) return rc;
  const size_t total = (size_t)s_batch * D * D;
  hipLaunchKernelGGL(loss_bwd_gs_kernel, dim3(blocks256(total, 2048)), dim3(256), 0, (hipStream_t)stream, theta, g_up, scale, gS, s_batch, M, D);
  return launch_status();
}

int uglad_finish_grads(const float* gt_partial, const float* grad_rho_partial, const float* glam_partial,
                       const float* lam_in, const float* params, float* grad, int L, int M, uglad_stream_t stream) {
  if (!gt_partial || !grad_rho_partial || !glam_partial || !lam_in || !params || !grad) return UGLAD_E_NULL;
  if (L < 1 || M < 1) return UGLAD_E_DIM;
  return finish_grads(1, M, (hipStream_t)stream, gt_partial, grad_rho_partial, glam_partial, lam_in, params, grad, L, M);
}

// (Round 3 removed the hipGraph cache of small passes that lived here: once persistent buffers made it hit -- 4 captures, 436 replays in a
// 220-epoch fit at D = 25 -- the epoch took 1.58 ms with it and 1.51 ms without (profiles/r03_fit_small_graph_probe.txt): a small pass is bound
// by the latency of its dependent kernels, not by their launches.  The entry points neither allocate nor synchronise, so a caller's own
// stream capture of a pass still works.)
int uglad_glad_forward(const float* S, const float* params, float lambda_init, int init_diag, int L, float* Z, int z_slabs,
                       float* half, float* U, float* beta, float* lam, float* lam_in, float* nf_partial, float* nf_sum,
                       float* cond_max, float* workspace, int M, int D, int sqrt_mode, uglad_stream_t stream) {
  return enqueue_glad_forward(1, S, params, lambda_init, init_diag, L, Z, z_slabs, half, U, beta, lam, lam_in, nf_partial, nf_sum, cond_max,
                              workspace, M, D, sqrt_mode, (hipStream_t)stream);
}

int uglad_glad_backward(const float* G_L, const float* S, const float* params, int init_diag, int L, const float* Z,
                        const float* half, const float* U, const float* beta, const float* lam, const float* lam_in,
                        float* gbuf0, float* gbuf1, float* grad_rho_partial, float* glam_partial, float* gt_partial,
                        float* grad, float* workspace, int M, int D, int sqrt_mode, uglad_stream_t stream) {
  return enqueue_glad_backward(1, G_L, S, params, init_diag, L, Z, half, U, beta, lam, lam_in, gbuf0, gbuf1, grad_rho_partial, glam_partial,
                               gt_partial, grad, workspace, M, D, sqrt_mode, (hipStream_t)stream);
}

int uglad_glad_forward_grouped(const float* S, const float* params, float lambda_init, int init_diag, int L, float* Z,
                               int z_slabs, float* half, float* U, float* beta, float* lam, float* lam_in, float* nf_partial,
                               float* nf_sum, float* cond_max, float* workspace, int M, int D, int groups, int sqrt_mode,
                               uglad_stream_t stream) {
  if (!valid_groups(M, groups)) return UGLAD_E_DIM;
  return enqueue_glad_forward(groups, S, params, lambda_init, init_diag, L, Z, z_slabs, half, U, beta, lam, lam_in, nf_partial, nf_sum,
                              cond_max, workspace, M, D, sqrt_mode, (hipStream_t)stream);
}

int uglad_glad_backward_grouped(const float* G_L, const float* S, const float* params, int init_diag, int L, const float* Z,
                                const float* half, const float* U, const float* beta, const float* lam, const float* lam_in,
                                float* gbuf0, float* gbuf1, float* grad_rho_partial, float* glam_partial, float* gt_partial,
                                float* grad, float* workspace, int M, int D, int groups, int sqrt_mode, uglad_stream_t stream) {
  if (!valid_groups(M, groups)) return UGLAD_E_DIM;
  return enqueue_glad_backward(groups, G_L, S, params, init_diag, L, Z, half, U, beta, lam, lam_in, gbuf0, gbuf1, grad_rho_partial,
                               glam_partial, gt_partial, grad, workspace, M, D, sqrt_mode, (hipStream_t)stream);
}

int uglad_glad_backward_wrt_s(const float* G_L, const float* S, const float* params, int init_diag, int L, const float* Z,
                              const float* half, const float* U, const float* beta, const float* lam, const float* lam_in,
                              float* gbuf0, float* gbuf1, float* grad_rho_partial, float* glam_partial, float* gt_partial,
                              float* grad, float* workspace, int M, int D, int groups, int sqrt_mode, float* gS, uglad_stream_t stream) {
  if (!gS || (D > 128 && !workspace)) return UGLAD_E_NULL;
  if (!valid_groups(M, groups)) return UGLAD_E_DIM;
  if (int rc = check_dims(make_route(M, D, groups, true, sqrt_mode))) return rc;
  if (!valid_sqrt(sqrt_mode)) return UGLAD_E_MODE;
  if (init_diag != 0 && init_diag != 1) return UGLAD_E_MODE;
  return enqueue_glad_backward(groups, G_L, S, params, init_diag, L, Z, half, U, beta, lam, lam_in, gbuf0, gbuf1, grad_rho_partial,
                               glam_partial, gt_partial, grad, workspace, M, D, sqrt_mode, (hipStream_t)stream, gS);
}

// ---- the sharded pass as ONE call (collective site i)
int uglad_glad_forward_sharded(const float* S, const float* params, float lambda_init, int init_diag, int L, float* Z, int z_slabs,
                               float* half, float* U, float* beta, float* lam, float* lam_in, float* nf_partial, float* nf_sum,
                               float* cond_max, float* workspace, int M, int D, int m_global, int sqrt_mode,
                               uglad_allreduce_fn exchange, void* exchange_ctx, uglad_stream_t stream) {
  if (!exchange) return UGLAD_E_NULL;
  if (m_global < M) return UGLAD_E_DIM;
  return enqueue_glad_forward(1, S, params, lambda_init, init_diag, L, Z, z_slabs, half, U, beta, lam, lam_in, nf_partial, nf_sum, cond_max,
                              workspace, M, D, sqrt_mode, (hipStream_t)stream, m_global, exchange, exchange_ctx);
}

}  // extern "C"
