// Host layer, part 5: the one-workgroup utilities around the pass (consensus, symeig, covariance, conditional mean, metrics) and the diagnostic
// exports of the development builds (UGLAD_PHASE_EXIT, UGLAD_STAMPS).  Their many-workgroup counterparts are in host_wide.h.
#pragma once
// the route of a utility: its batch is one group, and only the tridiagonalisation flavour is asked of it
static Route util_route(int M, int D) { return make_route(M, D, 1, false, UGLAD_SQRT_EXACT); }

extern "C" {

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
  if (int rc = check_dims(util_route(M, D), true)) return rc;
  hipStream_t st = (hipStream_t)stream;
  launch_tridiag(util_route(M, D), st, A, nullptr, nullptr, U, workspace);
  for_nt(D, [&](auto nt) {
    hipLaunchKernelGGL((symeig_lean_kernel<decltype(nt)::value>), dim3(M), dim3(kThreads), 0, st, U, beta, workspace, eig_layout(workspace, M, D).T, D);
  });
  return launch_status();
}

int uglad_covariance(const float* X, int K, int N, int D, int normalize, float eval_offset, float* S_out, float* eig_scratch,
                     float* workspace, uglad_stream_t stream) {
  if (!X || !S_out) return UGLAD_E_NULL;
  if (int rc = check_dims(util_route(K, D), true)) return rc;
  if (N < 1) return UGLAD_E_DIM;
  if (normalize != 0 && normalize != 1) return UGLAD_E_MODE;
  hipStream_t st = (hipStream_t)stream;
  for_nt(D, [&](auto nt) {
    hipLaunchKernelGGL((cov_kernel<decltype(nt)::value>), dim3(K), dim3(kThreads), 0, st, X, N, D, normalize, S_out);
  });
  int rc = launch_status();
  if (rc || !eig_scratch) return rc;  // eig_scratch == NULL: no eigenvalue repair
  if (!workspace) return UGLAD_E_NULL;
  float* beta = eig_scratch + (size_t)K * D * D;
  if ((rc = uglad_symeig(S_out, eig_scratch, beta, workspace, K, D, stream))) return rc;
  hipLaunchKernelGGL(cov_repair_kernel, dim3(K), dim3(256), 0, st, S_out, beta, D, eval_offset);
  return launch_status();
}

#ifdef UGLAD_PHASE_EXIT
int uglad_diag_set_exit(int at) {  // (development build: see glad_device.h)
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
#endif

int uglad_conditional_mean(const float* precision, const float* mean, const float* observed, const float* values,
                           float* full_mean, float* cond_cov, float* log_pdf, float* scratch, float* workspace, int K, int D,
                           int clip01, uglad_stream_t stream) {
  if (!precision || !mean || !observed || !values || !full_mean || !cond_cov || !scratch || !workspace) return UGLAD_E_NULL;
  if (int rc = check_dims(util_route(K, D), true)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int M = K;
  const size_t total = (size_t)K * D * D;
  hipLaunchKernelGGL(map_prepare_kernel, dim3(blocks256(total, 2048)), dim3(256), 0, st, precision, observed, scratch, D, total);
  launch_tridiag(util_route(M, D), st, scratch, nullptr, nullptr, cond_cov, workspace);
  for_nt(D, [&](auto nt) {
    hipLaunchKernelGGL((map_solve_kernel<decltype(nt)::value>), dim3(K), dim3(kThreads), 0, st, precision, mean, observed, values,
                                    scratch, full_mean, cond_cov, log_pdf, workspace, D, clip01);
  });
  return launch_status();
}

int uglad_partial_correlations(const float* precision, float* rho, int K, int D, uglad_stream_t stream) {
  if (!precision || !rho) return UGLAD_E_NULL;
  if (K < 1 || D < 1) return UGLAD_E_DIM;
  const size_t total = (size_t)K * D * D;
  hipLaunchKernelGGL(partial_corr_kernel, dim3(blocks256(total, 2048)), dim3(256), 0, (hipStream_t)stream, precision, rho, D, total);
  return launch_status();
}

int uglad_support_metrics(const float* true_theta, const float* pred_theta, double* out, int K, int D, int beta,
                          uglad_stream_t stream) {
  if (!true_theta || !pred_theta || !out) return UGLAD_E_NULL;
  if (int rc = check_dims(util_route(K, D), true)) return rc;
  if (D < 2) return UGLAD_E_DIM;
  hipStream_t st = (hipStream_t)stream;
  for_nt(D, [&](auto nt) {
    hipLaunchKernelGGL((support_metrics_kernel<decltype(nt)::value>), dim3(K), dim3(kThreads), 0, st, true_theta, pred_theta, out, D,
                                    beta);
  });
  return launch_status();
}

int uglad_tridiagonalize(const float* A0, const float* A1, const float* lam, float* R, float* workspace, int M, int D,
                         uglad_stream_t stream) {
  if (!A0 || !R || !workspace || (A1 && !lam)) return UGLAD_E_NULL;
  if (int rc = check_dims(util_route(M, D), true)) return rc;
  hipStream_t st = (hipStream_t)stream;
  launch_tridiag(util_route(M, D), st, A0, A1, lam, R, workspace);
  return launch_status();
}

int uglad_symeig_jacobi(const float* A, float* U, float* beta, int M, int D, uglad_stream_t stream) {
  if (!A || !U || !beta) return UGLAD_E_NULL;
  if (int rc = check_dims(util_route(M, D), true)) return rc;
  if (D > 128) return UGLAD_E_DIM;  // LDS-resident only
  hipStream_t st = (hipStream_t)stream;
  for_nt_lds(D, [&](auto nt) {
    hipLaunchKernelGGL((symeig_jacobi_kernel<decltype(nt)::value>), dim3(M), dim3(kThreads), 0, st, A, U, beta, D);
  });
  return launch_status();
}

}  // extern "C"
