// Host layer, part 6: the many-workgroup fp64 utilities (chol_wide.h and its clients; sort_wide.h and its clients).  Their workspaces are
// described once, by the view in the kernel header and its factory; here are the checks and the launch chains they share, and the entry points.
#pragma once
// *_workspace_floats: K items of floats_per_item(D) floats, for min_D <= D <= UGLAD_MAX_DIM; a size beyond 2^31 - 1 is refused like a dimension.
// floats_per_item: size_t(int D), called only for a D in range -- a function, or a lambda closed over the entry point's further argument
template <class PerItem>
static int wide_workspace_floats(int K, int D, int min_D, PerItem floats_per_item) {
  if (K < 1 || K > 65535 || D < min_D || D > UGLAD_MAX_DIM) return UGLAD_E_DIM;
  const size_t n = (size_t)K * floats_per_item(D);
  return n > 2147483647ULL ? UGLAD_E_DIM : (int)n;
}
static bool wide_workspace_ok(const float* workspace) { return workspace && !(reinterpret_cast<size_t>(workspace) & 7); }
// the blocked Cholesky of K slabs: update + panel for every block column; a CholwInvView also gets L(j, j)^-T and the log-pivots
template <class View>
static void launch_cholw(hipStream_t st, int K, const View& v) {
  const int nt = v.DP / kT64;
  for (int j = 0; j < nt; ++j) {
    hipLaunchKernelGGL(cholw_update_kernel, dim3(nt - j, K), dim3(kWThreads), 0, st, j, static_cast<const CholwView&>(v));
    hipLaunchKernelGGL(cholw_panel_kernel<View>, dim3(nt - j, K), dim3(kWThreads), 0, st, j, v);
  }
}
// the shift bisection of K slabs and their repair (chol_wide.h): the test at the threshold, then Bracket::kSteps steps; slabs that are done
// (or whose factorisation has broken down) cost empty launches.  out32: the (K, D, D) fp32 matrix whose diagonal the repair rewrites.
// after_reset(): the client's launches between the controller's reset and the first factorisation (a client that bars slabs of its own)
template <class Bracket, class AfterReset>
static void launch_cholw_bisection(hipStream_t st, int K, int D, double eval_offset, const CholwView& v, float* out32, double* min_eig_out,
                                   AfterReset after_reset) {
  constexpr int steps = Bracket::kSteps;
  for (int step = 0; step <= steps; ++step) {
    hipLaunchKernelGGL(cholw_bisect_kernel<Bracket>, dim3(K), dim3(64), 0, st, step - 1, D, v);
    if (step == 0) after_reset();
    launch_cholw(st, K, v);
  }
  hipLaunchKernelGGL(cholw_bisect_kernel<Bracket>, dim3(K), dim3(64), 0, st, steps, D, v);
  hipLaunchKernelGGL(cholw_repair_kernel, dim3((D + 255) / 256, K), dim3(256), 0, st, D, eval_offset, v, out32, min_eig_out);
}
template <class Bracket>
static void launch_cholw_bisection(hipStream_t st, int K, int D, double eval_offset, const CholwView& v, float* out32, double* min_eig_out) {
  launch_cholw_bisection<Bracket>(st, K, D, eval_offset, v, out32, min_eig_out, [] {});
}
// the radix sort of K arrays of keys (sort_wide.h); an even number of passes: the sorted keys end in buffer 0
static void launch_sortw(hipStream_t st, int K, const SortwView& v) {
  const dim3 tiles(v.tiles, K), wg(kWThreads);
  for (int pass = 0; pass < kSortwPasses; ++pass) {
    hipLaunchKernelGGL(sortw_hist_kernel, tiles, wg, 0, st, pass, pass & 1, v);
    hipLaunchKernelGGL(sortw_scan_kernel, dim3(K), wg, 0, st, v);
    hipLaunchKernelGGL(sortw_scatter_kernel, tiles, wg, 0, st, pass, pass & 1, v);
  }
}

// the covariance (centred, / N) of K tables of N rows into the slabs of an EigwView, with their tile flags: the column statistics
// without normalisation, then the Gram product of cov_wide.h; cov_out: (K, D, D) fp64 or NULL
static void launch_eigw_gram(hipStream_t st, const double* X64, int K, int N, int D, const EigwView& v, double* cov_out) {
  const int nt = v.DP / kT64;
  hipLaunchKernelGGL(covw_stats_kernel, dim3(nt, K), dim3(kWThreads), 0, st, X64, N, D, 0, v.chol());
  hipLaunchKernelGGL(covw_gram_kernel<EigwGramSink>, dim3(nt, nt, K), dim3(kWThreads), 0, st, X64, N, D, v, cov_out);
}
// the eigenvalues of K slabs that eigw_prepare_kernel or launch_eigw_gram has filled (eigvals_wide.h): per column the finish of the one
// before and its own reflector, then the strip partials of A v; behind every whole panel the trailing update; bisection; summary
static void launch_eigw(hipStream_t st, int K, int D, double th, const EigwView& v, double* eig_out, double* summary_out) {
  const int nt = v.DP / kT64, nc = (v.DP + kEigwChunk - 1) / kEigwChunk;
  const dim3 slabs(K), wg(kWThreads);
  for (int j = 0; j < D; ++j) {
    if (j > 0 && j % kEigwPanel == 0) {
      hipLaunchKernelGGL(eigw_column_kernel, slabs, wg, 0, st, j - 1, -1, D, v);
      const int T = nt - j / kT64;
      hipLaunchKernelGGL(eigw_update_kernel, dim3(T, T, K), wg, 0, st, j - kEigwPanel, v);
      hipLaunchKernelGGL(eigw_column_kernel, slabs, wg, 0, st, -1, j, D, v);
    } else {
      hipLaunchKernelGGL(eigw_column_kernel, slabs, wg, 0, st, j - 1, j, D, v);
    }
    if (j <= D - 2) hipLaunchKernelGGL(eigw_matvec_kernel, dim3(nc - (j + 1) / kEigwChunk, nt - (j + 1) / kT64, K), wg, 0, st, j, v);
  }
  hipLaunchKernelGGL(eigw_bisect_kernel, dim3((D + kWThreads - 1) / kWThreads, K), wg, 0, st, D, v, eig_out);
  hipLaunchKernelGGL(eigw_summary_kernel, slabs, wg, 0, st, D, th, eig_out, summary_out);
}

extern "C" {

int uglad_eigvalsh_wide_workspace_floats(int K, int D) { return wide_workspace_floats(K, D, 1, eigw_slab_floats); }

int uglad_eigvalsh_wide(const double* A64, int K, int D, double th, double* eig_out, double* summary_out, float* workspace,
                        uglad_stream_t stream) {
  if (!A64 || !eig_out || !summary_out || !wide_workspace_ok(workspace)) return UGLAD_E_NULL;
  if (uglad_eigvalsh_wide_workspace_floats(K, D) < 0) return UGLAD_E_DIM;
  hipStream_t st = (hipStream_t)stream;
  const EigwView v = eigw_view(workspace, D);
  const int nt = v.DP / kT64;
  hipLaunchKernelGGL(eigw_prepare_kernel, dim3(nt, nt, K), dim3(kWThreads), 0, st, A64, D, v);
  launch_eigw(st, K, D, th, v, eig_out, summary_out);
  return launch_status();
}

int uglad_table_spectrum(const double* X64, int K, int N, int D, double th, double* eig_out, double* summary_out, double* cov_out,
                         float* workspace, uglad_stream_t stream) {
  if (!X64 || !eig_out || !summary_out || !wide_workspace_ok(workspace)) return UGLAD_E_NULL;
  if (uglad_eigvalsh_wide_workspace_floats(K, D) < 0 || N < 1) return UGLAD_E_DIM;
  hipStream_t st = (hipStream_t)stream;
  const EigwView v = eigw_view(workspace, D);
  launch_eigw_gram(st, X64, K, N, D, v, cov_out);
  launch_eigw(st, K, D, th, v, eig_out, summary_out);
  return launch_status();
}

int uglad_correlated_features_workspace_floats(int K, int D) { return wide_workspace_floats(K, D, 2, eigw_slab_floats); }

int uglad_correlated_features(const double* S64, int K, int D, int* order, int* counts, int* n_listed, float* workspace,
                              uglad_stream_t stream) {
  if (!S64 || !order || !counts || !n_listed || !wide_workspace_ok(workspace)) return UGLAD_E_NULL;
  if (uglad_correlated_features_workspace_floats(K, D) < 0) return UGLAD_E_DIM;
  hipStream_t st = (hipStream_t)stream;
  const EigwView v = eigw_view(workspace, D);
  const int nt = v.DP / kT64;
  const dim3 tiles(nt, nt, K), wg(kWThreads);
  const double n = (double)D * (double)(D - 1) / 2.0;
  launch_eigw_gram(st, S64, K, D, D, v, nullptr);
  hipLaunchKernelGGL(corrw_init_kernel, dim3(K), wg, 0, st, (int)(0.1 * n), v);  // (the reference's int(0.1 * len))
  for (int pass = 0; pass < kCorrwPasses; ++pass) {
    hipLaunchKernelGGL(corrw_hist_kernel, tiles, wg, 0, st, pass, D, v);
    hipLaunchKernelGGL(corrw_narrow_kernel, dim3(K), wg, 0, st, pass, v);
  }
  hipLaunchKernelGGL(corrw_count_kernel, dim3(D, K), wg, 0, st, D, v, counts);
  hipLaunchKernelGGL(corrw_order_kernel, dim3(K), wg, 0, st, D, (const int*)counts, order, n_listed);
  return launch_status();
}

int uglad_covariance_wide_workspace_floats(int K, int D) { return wide_workspace_floats(K, D, 1, covw_table_floats); }

int uglad_covariance_wide(const double* X, int K, int N, int D, int normalize, double eval_offset, float* S_out, double* min_eig_out,
                          float* workspace, uglad_stream_t stream) {
  if (!X || !S_out || !wide_workspace_ok(workspace)) return UGLAD_E_NULL;
  if (uglad_covariance_wide_workspace_floats(K, D) < 0 || N < 1) return UGLAD_E_DIM;
  if (normalize != 0 && normalize != 1) return UGLAD_E_MODE;
  hipStream_t st = (hipStream_t)stream;
  const CholwView v = covw_view(workspace, D);
  const int nt = v.DP / kT64;
  hipLaunchKernelGGL(covw_stats_kernel, dim3(nt, K), dim3(kWThreads), 0, st, X, N, D, normalize, v);
  hipLaunchKernelGGL(covw_gram_kernel<CovwSink>, dim3(nt, nt, K), dim3(kWThreads), 0, st, X, N, D, v, S_out);
  if (min_eig_out) launch_cholw_bisection<CovwBracket>(st, K, D, eval_offset, v, S_out, min_eig_out);  // (NULL: no repair)
  return launch_status();
}

int uglad_association_max_width(void) { return UGLAD_ASSOC_MAX_WIDTH; }
static_assert(UGLAD_ASSOC_MAX_WIDTH == kAssocMaxWidth, "the header's constant is the kernels'");

int uglad_association_workspace_floats(int K, int D, int W) {
  if (W < D || W > kAssocMaxWidth || W % kT64) return UGLAD_E_DIM;
  return wide_workspace_floats(K, D, 2, [W](int D) { return 2 * assoc_table_doubles(t64_padded(D), W); });
}

int uglad_association(const double* table, int K, int N, int D, const int* col_feature, const int* col_level, const int* feat_offset,
                      const int* feat_width, const int* tile_first, int W, double eval_offset, float* A_out, double* A64_out,
                      double* min_eig_out, float* workspace, uglad_stream_t stream) {
  if (!table || !col_feature || !col_level || !feat_offset || !feat_width || !tile_first || !A_out || !wide_workspace_ok(workspace))
    return UGLAD_E_NULL;
  if (uglad_association_workspace_floats(K, D, W) < 0 || N < 2) return UGLAD_E_DIM;  // (N = 1: the bias correction divides by N - 1)
  hipStream_t st = (hipStream_t)stream;
  const CholwView v = assoc_view(workspace, D, W);
  const AssocMaps m{col_feature, col_level, feat_offset, feat_width, tile_first, W};
  const int wt = W / kT64;
  hipLaunchKernelGGL(assoc_stats_kernel, dim3(wt, K), dim3(kWThreads), 0, st, table, N, D, m, v);
  hipLaunchKernelGGL(assoc_gram_kernel, dim3(wt, wt, K), dim3(kWThreads), 0, st, table, N, D, m, v, A64_out, A_out);
  if (!min_eig_out) return launch_status();  // no repair
  // as uglad_covariance_wide, on the bracket of an indefinite matrix: its lower end from the row sums
  hipLaunchKernelGGL(assoc_rowsum_kernel, dim3((D + 255) / 256, K), dim3(256), 0, st, D, v);
  launch_cholw_bisection<AssocBracket>(st, K, D, eval_offset, v, A_out, min_eig_out);
  return launch_status();
}

// uglad_rank_correlation's arguments: the dimensions first, then the method
static int rank_arguments(int K, int N, int D, int method) {
  if (K < 1 || K > 65535 || D < 2 || D > UGLAD_MAX_DIM || N < 2 || N > kRankMaxN) return UGLAD_E_DIM;
  return method == kRankSpearman || method == kRankKendall || method == kRankScores ? 0 : UGLAD_E_MODE;
}
static_assert(UGLAD_RANK_SPEARMAN == kRankSpearman && UGLAD_RANK_KENDALL == kRankKendall && UGLAD_RANK_SCORES == kRankScores,
              "the header's constants are the kernels'");

int uglad_rank_correlation_workspace_floats(int K, int N, int D, int method) {
  const int rc = rank_arguments(K, N, D, method);
  if (rc != 0) return rc;
  return wide_workspace_floats(K, D, 2, [N, method](int D) { return rank_table_floats(N, D, method); });
}

// Kendall: enough chunks of pairs for about eight workgroups per compute unit, but none below 32 steps of 64 pairs (a chunk ends in T x T
// atomics) and none without a shift of its own
int uglad_rank_correlation_pair_chunks(int K, int N, int D) {
  if (rank_arguments(K, N, D, kRankKendall) != 0) return UGLAD_E_DIM;
  const int T = rank_tile(D), nt = rank_padded_tiles(D) / T;
  const long long groups = (long long)K * (nt * (nt + 1) / 2);
  const long long steps = (long long)N * (N - 1) / 2 / kRankStep + (N - 1) / 2 + 1;  // (the tail of a shift is half a step on average)
  long long chunks = (2048 + groups - 1) / groups;
  if (chunks > steps / 32) chunks = steps / 32;
  if (chunks > N - 1) chunks = N - 1;
  return chunks < 1 ? 1 : (int)chunks;
}

int uglad_rank_correlation(const double* X, int K, int N, int D, int method, int transform, double eval_offset, float* A_out,
                           double* A64_out, double* gram_out, int* info_out, double* min_eig_out, float* workspace, uglad_stream_t stream) {
  if (!X || !A_out || !wide_workspace_ok(workspace)) return UGLAD_E_NULL;
  const int rc = rank_arguments(K, N, D, method);
  if (rc != 0) return rc;
  if (uglad_rank_correlation_workspace_floats(K, N, D, method) < 0) return UGLAD_E_DIM;
  if (transform != 0 && transform != 1) return UGLAD_E_MODE;
  hipStream_t st = (hipStream_t)stream;
  const RankView v = rank_view(workspace, K, N, D);
  const int DP = v.c.DP, nt64 = DP / kT64;
  const dim3 wg(kWThreads);
  hipLaunchKernelGGL(rank_kernel, dim3((N + kWThreads - 1) / kWThreads, D, K), wg, 0, st, X, N, D, method, v, info_out);
  if (method == kRankKendall) {
    const int T = rank_tile(D), nt = v.DT / T;
    const dim3 grid(nt * (nt + 1) / 2, uglad_rank_correlation_pair_chunks(K, N, D), K);
    zero_floats(reinterpret_cast<float*>(v.gram32(0, D)), (size_t)K * v.DT * v.DT, st);  // (int32 zeros are float zeros)
    if (T == kRankTileWide) hipLaunchKernelGGL(rank_kendall_kernel<kRankTileWide / 32>, grid, wg, 0, st, N, D, v);
    else hipLaunchKernelGGL(rank_kendall_kernel<kRankTileNarrow / 32>, grid, wg, 0, st, N, D, v);
  } else {  // the centred sums of the table of c or z, as a covariance's
    hipLaunchKernelGGL(covw_stats_kernel, dim3(nt64, K), wg, 0, st, (const double*)v.table(), N, D, 0, v.c);
    hipLaunchKernelGGL(covw_gram_kernel<RankGramSink>, dim3(nt64, nt64, K), wg, 0, st, (const double*)v.table(), N, D, v.c, (double*)nullptr);
  }
  hipLaunchKernelGGL(rank_finish_kernel, dim3(DP * DP / kWThreads, K), wg, 0, st, D, method, transform, v, A_out, A64_out, gram_out);
  if (!min_eig_out) return launch_status();  // no repair
  hipLaunchKernelGGL(assoc_rowsum_kernel, dim3((D + 255) / 256, K), dim3(256), 0, st, D, v.c);
  launch_cholw_bisection<AssocBracket>(st, K, D, eval_offset, v.c, A_out, min_eig_out);
  return launch_status();
}

int uglad_pairwise_covariance_workspace_floats(int K, int D) { return wide_workspace_floats(K, D, 1, pairw_table_floats); }

int uglad_pairwise_covariance(const double* X, int K, int N, int D, int normalize, int min_pairs, double eval_offset, float* S_out,
                              double* S64_out, int* counts_out, int* info_out, double* min_eig_out, float* workspace, uglad_stream_t stream) {
  if (!X || !S_out || !wide_workspace_ok(workspace)) return UGLAD_E_NULL;
  if (uglad_pairwise_covariance_workspace_floats(K, D) < 0 || N < 1) return UGLAD_E_DIM;
  if ((normalize != 0 && normalize != 1) || min_pairs < 1) return UGLAD_E_MODE;
  hipStream_t st = (hipStream_t)stream;
  const PairwView v = pairw_view(workspace, D);
  const int nt = v.c.DP / kT64;
  const dim3 wg(kWThreads);
  hipLaunchKernelGGL(pairw_stats_kernel, dim3(nt, K), wg, 0, st, X, N, D, normalize, v);
  hipLaunchKernelGGL(pairw_gram_kernel, dim3(nt, nt, K), wg, 0, st, X, N, D, min_pairs, v, PairwOut{S_out, S64_out, counts_out});
  hipLaunchKernelGGL(pairw_info_kernel, dim3(K), wg, 0, st, D, v, info_out);
  if (!min_eig_out) return launch_status();  // no repair
  // as uglad_association, on the bracket of an indefinite matrix; a flagged table (it holds NaN) is barred behind the controller's reset
  hipLaunchKernelGGL(assoc_rowsum_kernel, dim3((D + 255) / 256, K), dim3(256), 0, st, D, v.c);
  launch_cholw_bisection<AssocBracket>(st, K, D, eval_offset, v.c, S_out, min_eig_out,
                                       [&] { hipLaunchKernelGGL(pairw_bar_kernel, dim3(K), dim3(64), 0, st, 0, v, min_eig_out); });
  hipLaunchKernelGGL(pairw_bar_kernel, dim3(K), dim3(64), 0, st, 1, v, min_eig_out);
  return launch_status();
}

int uglad_weighted_covariance_workspace_floats(int R, int D) { return wide_workspace_floats(R, D, 1, wcov_weighting_floats); }

int uglad_weighted_covariance(const double* X, const double* W, int R, int N, int D, double eval_offset, float* S_out, double* S64_out,
                              double* mean_out, int* info_out, double* min_eig_out, float* workspace, uglad_stream_t stream) {
  if (!X || !W || !S_out || !info_out || !wide_workspace_ok(workspace)) return UGLAD_E_NULL;
  if (uglad_weighted_covariance_workspace_floats(R, D) < 0 || N < 1) return UGLAD_E_DIM;
  hipStream_t st = (hipStream_t)stream;
  const WcovView v = wcov_view(workspace, D);
  const WcovOut out{S_out, S64_out, mean_out, info_out};
  const int nt = v.c.DP / kT64, groups = (R + kWcovGroup - 1) / kWcovGroup;
  const dim3 wg(kWThreads);
  hipLaunchKernelGGL(covw_stats_kernel, dim3(nt, 1), wg, 0, st, X, N, D, 0, v.c);  // X as a single table: its column means, shared
  hipLaunchKernelGGL(wcov_stats_kernel, dim3(nt, R), wg, 0, st, X, W, N, D, v, out);
  hipLaunchKernelGGL(wcov_gram_kernel<kWcovGroup>, dim3(nt, nt, groups), wg, 0, st, X, W, R, N, D, v, out);
  if (!min_eig_out) return launch_status();  // no repair
  // as uglad_covariance_wide over K = R slabs; a flagged weighting (it holds NaN) is barred behind the controller's reset
  launch_cholw_bisection<CovwBracket>(st, R, D, eval_offset, v.c, S_out, min_eig_out,
                                      [&] { hipLaunchKernelGGL(wcov_bar_kernel, dim3(R), dim3(64), 0, st, 0, v, min_eig_out); });
  hipLaunchKernelGGL(wcov_bar_kernel, dim3(R), dim3(64), 0, st, 1, v, min_eig_out);
  return launch_status();
}

int uglad_conditional_mean_wide_workspace_floats(int K, int D) { return wide_workspace_floats(K, D, 1, afterw_problem_floats); }

int uglad_conditional_mean_wide(const double* precision, const double* mean, const float* observed, const double* values,
                                double* full_mean, float* cond_cov, double* log_pdf, float* workspace, int K, int D, int clip01,
                                uglad_stream_t stream) {
  if (!precision || !mean || !observed || !values || !full_mean || !wide_workspace_ok(workspace)) return UGLAD_E_NULL;
  if (uglad_conditional_mean_wide_workspace_floats(K, D) < 0) return UGLAD_E_DIM;
  hipStream_t st = (hipStream_t)stream;
  const AfterwView v = afterw_view(workspace, D);
  const AfterwIn in{precision, mean, observed, values};
  const int nt = v.c.DP / kT64;
  const dim3 rows(nt, K), tiles(nt, nt, K), wg(kWThreads);
  hipLaunchKernelGGL(afterw_prepare_kernel, tiles, wg, 0, st, in, D, v);
  hipLaunchKernelGGL(afterw_rhs_kernel, rows, dim3(64), 0, st, observed, D, v);
  launch_cholw(st, K, v.c);
  for (int i = 1; i < nt; ++i) hipLaunchKernelGGL(afterw_subst_kernel, dim3(i, K), wg, 0, st, i, v);
  // y = W^T (W r); y += W^T (W (r - A y))
  using V = AfterwView;
  hipLaunchKernelGGL(afterw_matvec_kernel<false>, rows, wg, 0, st, (int)kAfterwLower, (int)V::kR, (int)V::kT, 0, v);
  hipLaunchKernelGGL(afterw_matvec_kernel<true>, rows, wg, 0, st, (int)kAfterwUpper, (int)V::kT, (int)V::kY, 0, v);
  hipLaunchKernelGGL(afterw_matvec_kernel<false>, rows, wg, 0, st, (int)kAfterwResidual, (int)V::kY, (int)V::kRes, 0, v);
  hipLaunchKernelGGL(afterw_matvec_kernel<false>, rows, wg, 0, st, (int)kAfterwLower, (int)V::kRes, (int)V::kT, 0, v);
  hipLaunchKernelGGL(afterw_matvec_kernel<true>, rows, wg, 0, st, (int)kAfterwUpper, (int)V::kT, (int)V::kY, 1, v);
  if (cond_cov) hipLaunchKernelGGL(afterw_cov_kernel, tiles, wg, 0, st, observed, D, v, cond_cov);
  hipLaunchKernelGGL(afterw_finish_kernel, rows, wg, 0, st, in, D, clip01, v, full_mean, log_pdf);
  return launch_status();
}

int uglad_sample_scores_workspace_floats(int K, int N, int D) {
  if (N < 1) return UGLAD_E_DIM;
  return wide_workspace_floats(K, D, 1, [N](int D) { return scorew_model_floats(N, D); });
}

int uglad_sample_scores(const double* X, int x_batch, const double* precision, const double* mean, double* mahalanobis,
                        double* log_density, double* logdet, float* workspace, int K, int N, int D, uglad_stream_t stream) {
  if (!X || !precision || !mean || !mahalanobis || !wide_workspace_ok(workspace)) return UGLAD_E_NULL;
  if (uglad_sample_scores_workspace_floats(K, N, D) < 0 || (x_batch != 1 && x_batch != K)) return UGLAD_E_DIM;
  hipStream_t st = (hipStream_t)stream;
  const AfterwView v = afterw_view(workspace, D);
  double* parts = scorew_partials(v, K);
  const ScorewIn in{X, mean, x_batch, N, D};
  const int nt = v.c.DP / kT64;
  const dim3 wg(kWThreads);
  hipLaunchKernelGGL(scorew_prepare_kernel, dim3(nt, nt, K), wg, 0, st, precision, D, v);
  hipLaunchKernelGGL(scorew_quad_kernel, dim3((unsigned)((N + (size_t)kT64 - 1) / kT64), nt, K), wg, 0, st, in, v, parts);
  if (log_density || logdet) {  // the factorisation only for those who read it
    launch_cholw(st, K, v.c);
    hipLaunchKernelGGL(scorew_logdet_kernel, dim3(K), wg, 0, st, D, v, logdet);
  }
  hipLaunchKernelGGL(scorew_finish_kernel, dim3((unsigned)((N + (size_t)kWThreads - 1) / kWThreads), K), wg, 0, st, N, D, v, parts, mahalanobis,
                     log_density);
  return launch_status();
}

int uglad_support_metrics_wide_workspace_floats(int K, int D) { return wide_workspace_floats(K, D, 2, mw_pair_floats); }

int uglad_support_metrics_wide(const float* true_theta, const float* pred_theta, double* out, float* workspace, int K, int D, int beta,
                               uglad_stream_t stream) {
  if (!true_theta || !pred_theta || !out || !wide_workspace_ok(workspace)) return UGLAD_E_NULL;
  if (uglad_support_metrics_wide_workspace_floats(K, D) < 0) return UGLAD_E_DIM;
  hipStream_t st = (hipStream_t)stream;
  const MwView v = mw_view(workspace, D);
  const dim3 tiles(v.s.tiles, K), wg(kWThreads);
  hipLaunchKernelGGL(mw_keys_kernel, dim3(v.nt, v.nt, K), wg, 0, st, true_theta, pred_theta, D, v);
  launch_sortw(st, K, v.s);
  hipLaunchKernelGGL(mw_chunk_kernel, tiles, wg, 0, st, v);
  hipLaunchKernelGGL(mw_group_kernel, tiles, wg, 0, st, v);
  hipLaunchKernelGGL(mw_finish_kernel, dim3(K), wg, 0, st, out, beta, v);
  return launch_status();
}

int uglad_graph_wide_workspace_floats(int K, int D) { return wide_workspace_floats(K, D, 2, gw_problem_floats); }

int uglad_graph_wide(const float* values, int from_precision, const int* n_keep, const float* threshold_in, float* threshold,
                     int* edge_count, int* edge_ij, float* edge_w, int* degree, int* triangles2, double* stats, int want_stats, int K, int D,
                     float* workspace, uglad_stream_t stream) {
  if (!values || !n_keep || !threshold || !edge_count || !edge_ij || !edge_w || !degree || !wide_workspace_ok(workspace)) return UGLAD_E_NULL;
  if (uglad_graph_wide_workspace_floats(K, D) < 0) return UGLAD_E_DIM;
  if ((from_precision != 0 && from_precision != 1) || (want_stats != 0 && want_stats != 1)) return UGLAD_E_MODE;
  if (want_stats && (!triangles2 || !stats)) return UGLAD_E_NULL;
  const GwView v = gw_view(workspace, D);
  bool ranked = false;
  for (int k = 0; k < K; ++k) {
    if (n_keep[k] < -1 || n_keep[k] > v.s.E) return UGLAD_E_DIM;
    if (n_keep[k] == -1 && !threshold_in) return UGLAD_E_NULL;
    ranked = ranked || n_keep[k] >= 0;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 tiles(v.nt, v.nt, K), wg(kWThreads);
  if (ranked) {  // (a batch of given thresholds needs no order)
    hipLaunchKernelGGL(gw_keys_kernel, tiles, wg, 0, st, values, from_precision, v);
    launch_sortw(st, K, v.s);
  }
  for (int k0 = 0; k0 < K; k0 += kGwKeepPer) {
    GwKeep keep;
    const int n = K - k0 < kGwKeepPer ? K - k0 : kGwKeepPer;
    for (int q = 0; q < kGwKeepPer; ++q) keep.n[q] = q < n ? n_keep[k0 + q] : -1;
    hipLaunchKernelGGL(gw_threshold_kernel, dim3(n), dim3(64), 0, st, keep, k0, threshold_in, threshold, v);
  }
  hipLaunchKernelGGL(gw_row_kernel, dim3(v.DP, K), wg, 0, st, values, from_precision, degree, v);
  hipLaunchKernelGGL(gw_scan_kernel, dim3(K), wg, 0, st, edge_count, v);
  hipLaunchKernelGGL(gw_edges_kernel, dim3(D, K), wg, 0, st, values, from_precision, edge_ij, edge_w, v);
  if (want_stats) {
    hipLaunchKernelGGL(gw_triangles_kernel, tiles, wg, 0, st, v);
    hipLaunchKernelGGL(gw_rowsum_kernel, dim3((D + kWThreads - 1) / kWThreads, K), wg, 0, st, triangles2, v);
    hipLaunchKernelGGL(gw_finish_kernel, dim3(K), wg, 0, st, degree, triangles2, stats, v);
  }
  return launch_status();
}

int uglad_edge_frequency(const int* edge_count, const int* edge_ij, const float* edge_w, int R, int D, int* count_out, int* positive_out,
                         long long* totals_out, uglad_stream_t stream) {
  if (!edge_count || !edge_ij || !edge_w || !count_out || !positive_out || !totals_out) return UGLAD_E_NULL;
  if (R < 1 || R > 65535 || D < 2 || D > UGLAD_MAX_DIM) return UGLAD_E_DIM;
  hipStream_t st = (hipStream_t)stream;
  const int E = D * (D - 1) / 2;
  int rc;
  if ((rc = zero_floats(reinterpret_cast<float*>(count_out), (size_t)D * D, st))) return rc;  // (int32 zeros are float zeros)
  if ((rc = zero_floats(reinterpret_cast<float*>(positive_out), (size_t)D * D, st))) return rc;
  hipLaunchKernelGGL(gw_frequency_kernel, dim3((E + kWThreads - 1) / kWThreads, R), dim3(kWThreads), 0, st, edge_count, edge_ij, edge_w, E, D,
                     count_out, positive_out);
  hipLaunchKernelGGL(gw_frequency_totals_kernel, dim3(1), dim3(kWThreads), 0, st, (const int*)count_out, R, D, totals_out);
  return launch_status();
}

}  // extern "C"
