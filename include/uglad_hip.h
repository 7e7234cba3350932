/*
 * uglad_hip.h -- C ABI of libuglad_hip.so: the unrolled-GLAD hot path of Harshs27/uGLAD as hand-written
 * gfx950 (MI355X) HIP kernels.
 *
 * The reference has no FFI: its seam is Python-function level.  Each entry point below
 * names the reference code it replaces (paths relative to the reference repo).  INTEGRATION.md shows the
 * ctypes stub a uGLAD maintainer would add to call these from uglad/glad/glad.py and uglad/main.py.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to a caller-owned, contiguous, row-major fp32 buffer; sizes are explicit (the one exception:
 *    uglad_covariance_wide reads its tables, and returns its eigenvalues, in fp64, and uglad_conditional_mean_wide is fp64 but for
 *    its mask and cond_cov);
 *  - `stream` is the hipStream_t the work is enqueued on (pass torch's current stream); nothing synchronises;
 *  - no allocation or free of device memory; the library never keeps a device pointer after returning; entry points that
 *    run the eigensolver take a caller-owned `workspace` of uglad_workspace_floats(M, D) floats;
 *  - process-wide state, all of it host-side: (1) the grouped whole-pass calls set a thread-local group count for their own
 *    duration (restored on return), which the per-step entry points read as 1 otherwise; (2) the kernel-shape switch of
 *    uglad_set_wide_mode().  Nothing else: no cache, no device allocation, no synchronisation -- a caller may capture any
 *    sequence of these calls into a hipGraph of its own;
 *  - return value: 0 ok, <0 argument error (UGLAD_E_*), >0 a hipError_t from the launch;
 *  - scalars that live on the device (lambda_k, the upstream loss gradient) are passed BY POINTER so that the
 *    L-step loop never needs a device->host copy (the reference does one per step: glad.py:147);
 *  - batch index m = 0..M-1 selects matrix m of a (M, D, D) tensor.  D <= uglad_max_dim().
 *
 * Parameter vector `params` (42 floats, the order of GladParams.state_dict(), glad_params.py:13-59):
 *   [0]      theta_init_offset
 *   [1..9]   rho_l1.0.weight (3x3, row = output unit)   [10..12] rho_l1.0.bias
 *   [13..21] rho_l1.2.weight (3x3)                      [22..24] rho_l1.2.bias
 *   [25..27] rho_l1.4.weight (1x3)                      [28]     rho_l1.4.bias
 *   [29..34] lambda_f.0.weight (3x2)                    [35..37] lambda_f.0.bias
 *   [38..40] lambda_f.2.weight (1x3)                    [41]     lambda_f.2.bias
 */
#ifndef UGLAD_HIP_H
#define UGLAD_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* uglad_stream_t; /* hipStream_t */

#define UGLAD_NPARAM 42
#define UGLAD_NRHO 28 /* params[1..28] */

#define UGLAD_E_NULL (-1)  /* a required pointer is NULL */
#define UGLAD_E_DIM (-2)   /* D < 1 or D > uglad_max_dim(), or M < 1 */
#define UGLAD_E_MODE (-3)  /* unknown sqrt mode / init mode */
#define UGLAD_E_RCCL (-4)  /* RCCL is not loadable in this process, or one of its calls failed */

/* How the matrix square root in Theta_{k+1/2} = 1/2(-b + (b^T b + 4/lam I)^{1/2}) is evaluated on the spectrum of b:
 * EXACT: r_i = sqrt(beta_i^2 + 4/lam).
 * NS10 : the value the reference's 10-step Newton-Schulz iteration returns for that eigenvalue, and in the backward
 *        the reference's 10-step approximate Lyapunov operator (torch_sqrtm.py:13-46) -- bit-for-bit the same
 *        spectral function as the reference, at O(D) / O(D^2) cost.  This is the drop-in default. */
#define UGLAD_SQRT_EXACT 0
#define UGLAD_SQRT_NS10 1

int uglad_version(void);
int uglad_max_dim(void);

/* Largest cond_2(b^T b + 4/lam I) (the cond_max diagnostic of uglad_cell_fwd) up to which parity with the reference is validated by
 * reference-made goldens (tests/golden/regime_*.npz, tests/golden/regime_sweep.json): below it the reference's fp32 Newton-Schulz matrix
 * iteration and this library's spectral evaluation of the same iteration agree within the 1e-4 tolerance; beyond it the reference's own
 * arithmetic is no longer a function of the spectrum alone.  fit() / predict() warn when a pass exceeds it. */
float uglad_validated_cond(void);
/* 1 when a cell call of this shape reports the Gershgorin UPPER BOUND max_i sum_j |A_ij| / (4/lam) >= cond(A) in cond_max (the
 * matrix-iteration path, which has no spectrum to read: D > uglad_max_eig_dim(), and few matrices of 128 < D <= 256), 0 when it reports
 * the condition number itself (the spectral path); `training` = the call saves state for a backward pass.  The bound runs 1.3 ... 1.4 x
 * the true value on sample covariances and can reach ~sqrt(D) x: a caller that warns should hold it to a correspondingly larger threshold. */
int uglad_cond_is_upper_bound(int M, int D, int training, int sqrt_mode);

/* Few, large matrices (D > 128): one workgroup per matrix leaves the chip idle (BASELINE config 5 puts ONE 256 x 256 matrix on
 * each GPU), so the backward cell and the forward cell's part after the eigen-decomposition run as several launches with many
 * workgroups per matrix instead (csrc/wide_bwd.h).  mode -1 (default): chosen per call from (M, D); 0: never; 1: whenever D > 128.
 * Process-wide host-side state; UGLAD_WIDE_BWD=0/1 in the environment presets it.  Same results up to the summation order of the
 * products.  Returns 0, or UGLAD_E_MODE. */
int uglad_set_wide_mode(int mode);

/* Beyond the eigensolver's size (uglad_max_eig_dim() = 256 < D <= uglad_max_dim() = 2048 since round 4; 1024 in round 3) the cell is the reference's own matrix
 * iteration -- ten Newton-Schulz steps forward, ten steps of its Lyapunov iteration backward (torch_sqrtm.py:13-46) -- as dense tile
 * products with many workgroups per matrix (csrc/wide_ns.h): 28 + 60 products per step.  Only UGLAD_SQRT_NS10 exists there
 * (UGLAD_E_MODE otherwise); U's slot of the saved tensors carries the square root, beta's stays unused; cond_max receives the
 * Gershgorin UPPER BOUND of the condition number; Theta_0 and the loss's logdet / inverse use an L D L^T factorisation without
 * pivoting (torch.logdet's rules from the signs of D: finite for an even number of negative eigenvalues, NaN for an odd one; a zero
 * pivot gives NaN where a singular matrix gives -inf in torch).  The entry points of the path (init_theta, cell_fwd / cell_bwd, loss_*, glad_forward* / glad_backward*) take every
 * D <= uglad_max_dim(), and so do the covariance front-end through uglad_covariance_wide, the conditional Gaussian through
 * uglad_conditional_mean_wide and the support-recovery metrics through uglad_support_metrics_wide; uglad_symeig, uglad_cell_fwd_stage2,
 * uglad_tridiagonalize, uglad_covariance (the fp32 front-end, whose repair runs the eigensolver), uglad_conditional_mean and
 * uglad_support_metrics stay at uglad_max_eig_dim(); the metrics report beyond it is uglad_support_metrics_wide.  A call on this path takes at most 21845 matrices (UGLAD_E_DIM beyond: matrix x
 * product, up to three products, share one grid dimension).
 * The same path is taken automatically (mode -1, the default) for FEW matrices of 128 < D <= 256 under UGLAD_SQRT_NS10, where one
 * workgroup's Householder chain is most of the spectral cell: training calls (half_out / U_out given) up to 8 matrices and
 * M * ceil(D/64)^2 <= 96, forward-only calls while M * ceil(D/64)^2 <= 256 (one 256 x 256 matrix: 9.4 vs 16.9 ms per 15-step training
 * pass, 4.2 vs 15.5 forward only); uglad_cell_bwd follows the training rule, so it matches the forward call that saved its state.
 * uglad_set_matrix_iteration(0) keeps the spectral path wherever it exists, (1) takes this path for EVERY D (tests, A/B measurements);
 * UGLAD_MATRIX_ITERATION=0/1 in the environment presets it.  Process-wide host-side state; size the workspace after setting it. */
int uglad_max_eig_dim(void);
int uglad_set_matrix_iteration(int mode);

/* Floats of caller-owned device workspace for a batch of M matrices of order D (DP = D rounded up to 32): the tridiagonal
 * form d, e, tau per matrix (3 DP floats), handed from the tridiagonalisation launch to the divide & conquer launch, plus --
 * for 128 < D <= 256, where two D x D fp32 buffers no longer fit the 160 KB of LDS -- two L2-resident DP x (DP+1) slabs per
 * matrix on which the same kernels then work through global pointers; for D > 256 (or every D under uglad_set_matrix_iteration(1))
 * the header and, per matrix, eight D x D fp64 slabs + one fp32 slab, or the three padded F x (F + 1) fp32 slabs + D x D of the
 * factorisation (F = 1024 up to D = 1024, 2048 beyond), whichever is larger (csrc/wide_ns.h).  Every entry point that takes `workspace` accepts a buffer of this size
 * (uglad_cell_bwd and uglad_init_theta_bwd only read it for D > 128 and accept NULL otherwise).  Negative on bad arguments. */
int uglad_workspace_floats(int M, int D);

/* Theta_0.  Replaces glad.py:103-119.  init_diag 0: (S + t I)^-1 -- the reference calls torch.inverse, an LU -- by blocked Cholesky
 * in LDS (D <= 128; a matrix that is not positive definite goes through the eigen path: V diag(1/(s_i + t)) V^T + a Newton step), by
 * the path's eigensolver (128 < D <= 256), by a blocked L D L^T + two Newton steps (D > 256); the result is exactly symmetric and
 * agrees with the LU's to fp32 round-off.  init_diag 1: diag(1/(S_ii + t)).  t = params[0]. */
int uglad_init_theta(const float* S, const float* params, int init_diag, float* theta0, float* workspace, int M, int D,
                     uglad_stream_t stream);

/* d loss / d theta_init_offset, one partial per matrix: gt_partial[m] = -<G0_m, Theta0_m^2> (init_diag 0)
 * or -sum_i G0_ii Theta0_ii^2 (init_diag 1).  Autograd counterpart of glad.py:107-117. */
int uglad_init_theta_bwd(const float* theta0, const float* G0, int init_diag, float* gt_partial, float* workspace, int M,
                         int D, uglad_stream_t stream);

/* lambda_0 = LambdaNN([lambda_init, 0]).  Replaces glad.py:135 (note the reference passes lambda_init in the normF slot).
 * Writes lam_out[0] and the two inputs to lam_in[0..1] (kept for uglad_lambda_bwd). */
int uglad_lambda_init(const float* params, float lambda_init, float* lam_out, float* lam_in, uglad_stream_t stream);

/* One GLAD cell for every matrix of the batch.  Replaces glad.py:139-144 + torch_sqrtm.py:13-29 + glad_params.py:61-81:
 *   b = S/lam - Z_in (symmetric; the upper triangle is read), b = U diag(beta) U^T (batched symmetric eigensolver in LDS),
 *   theta_half = phi(b) assembled as -alpha b + U diag(phi(beta) + alpha beta) U^T (an identity for every alpha; alpha in [0,1] chosen per
 *   matrix to minimise the part that goes through the fp32 eigenvectors, the product on the f32 MFMA, the spectral function in fp64),
 *   Z_out = soft-threshold(theta_half, rhoNN(theta_half, S, Z_in)),  normF_partial[m] = ||Z_out_m - theta_half_m||_F^2.
 * lam points at lambda_k on the device.  half_out / U_out (M,D,D) and beta_out (M,D) may be NULL (inference);
 * when given they are what uglad_cell_bwd needs.  Z_out must not alias Z_in.
 * cond_max (M floats, or NULL): regime diagnostic, cond_max[m] = max(cond_max[m], cond_2(b_m^T b_m + 4/lam I)) -- a RUNNING maximum, so
 * the caller zeroes it before the first step of a pass.  The reference's 10 Newton-Schulz steps (torch_sqrtm.py:13-29) are an accurate
 * square root only while this number is small (hard part 1; validated bound: uglad_validated_cond()). */
int uglad_cell_fwd(const float* S, const float* Z_in, const float* lam, const float* params, float* Z_out,
                   float* half_out, float* U_out, float* beta_out, float* normF_partial, float* cond_max, float* workspace, int M,
                   int D, int sqrt_mode, uglad_stream_t stream);

/* Second launch of uglad_cell_fwd alone (divide & conquer, back-transformation, U phi U^T, rhoNN epilogue), for callers that
 * already ran uglad_tridiagonalize(S, Z_in, lam, Z_out, workspace) on the same stream -- profiling and tests; same arguments
 * as uglad_cell_fwd. */
int uglad_cell_fwd_stage2(const float* S, const float* Z_in, const float* lam, const float* params, float* Z_out,
                          float* half_out, float* U_out, float* beta_out, float* normF_partial, float* cond_max, float* workspace,
                          int M, int D, int sqrt_mode, uglad_stream_t stream);

/* out[0] = sum_i partials[i], summed in index order (deterministic).  Local leg of the per-step normF collective
 * (get_frobenius_norm, glad.py:60-71) and of the loss / gradient reductions. */
int uglad_sum_partials(const float* partials, int n, float* out, uglad_stream_t stream);

/* lambda_{k+1} = LambdaNN([normF_sum * inv_M, lambda_k]).  Replaces glad.py:146-150 + glad_params.py:83-95.
 * normF_sum: device scalar (already summed over the local batch, and all-reduced over ranks when sharded);
 * inv_M = 1 / global batch size (get_frobenius_norm's batch mean).  Writes lam_next[0] and lam_in_next[0..1]. */
int uglad_lambda_step(const float* normF_sum, float inv_M, const float* lam_prev, const float* params, float* lam_next,
                      float* lam_in_next, uglad_stream_t stream);

/* Backward of one cell.  Replaces autograd through glad.py:139-144, torch_sqrtm.py:32-46 and glad_params.py:61-81.
 * G_next = dL/dZ_out.  Writes G_out = dL/dZ_in, ADDS the 28 rhoNN gradients of matrix m to grad_rho_partial[m*28..]
 * (zero it once per backward pass) and WRITES glam_partial[m] = this matrix's contribution to dL/dlambda_k.
 * G_out must not alias G_next.  G_out is symmetric up to rounding (exactly symmetric when one workgroup handles the matrix);
 * only the symmetric part of G_next is used.  For D > 128 the whole workspace is scratch (nothing of a forward call survives). */
int uglad_cell_bwd(const float* G_next, const float* S, const float* Z_in, const float* half, const float* U,
                   const float* beta, const float* lam, const float* params, float* G_out, float* grad_rho_partial,
                   float* glam_partial, float* workspace, int M, int D, int sqrt_mode, uglad_stream_t stream);

/* glasso loss, one partial per matrix.  Replaces main.py:306-311,325-332:
 *   loss_partial[m] = -logdet(Theta_m) + sum_ij S_ij Theta_ji [+ sum_ij log cosh(Theta_ij * ((1 - struct_ij) - delta_ij))].
 * logdet follows torch.logdet: NaN when det < 0, -inf when det = 0.  S holds s_batch matrices (M, or 1 = broadcast,
 * the missing-data call of main.py:620-622); struct (s_batch, D, D) may be NULL.  theta_inv_out (M,D,D) receives
 * Theta^-1 for uglad_loss_bwd.  The caller divides the summed partials by s_batch (main.py:306,315). */
int uglad_loss_fwd(const float* theta, const float* S, int s_batch, const float* struct_theta, float* loss_partial,
                   float* theta_inv_out, float* workspace, int M, int D, uglad_stream_t stream);

/* G = g_up[0] * scale * (-Theta^-T + S^T [+ tanh(Theta o mask) o mask]).  g_up: device scalar (upstream gradient of the
 * loss), scale = 1/s_batch. */
int uglad_loss_bwd(const float* theta, const float* theta_inv, const float* S, int s_batch, const float* struct_theta,
                   const float* g_up, float scale, float* G_out, int M, int D, uglad_stream_t stream);

/* uglad_loss_bwd that also OVERWRITES gS (s_batch, D, D) with dL/dS, symmetric part (the convention of uglad_glad_backward_wrt_s):
 *   gS_b = g_up[0] * scale * sum over the matrices m that read S_b of (Theta_m + Theta_m^T) / 2
 * -- with s_batch == 1 the sum runs over all M matrices (one S broadcast against the batch).  The structure term does not depend on S.
 * G_out is bit-identical to uglad_loss_bwd's. */
int uglad_loss_bwd_wrt_s(const float* theta, const float* theta_inv, const float* S, int s_batch, const float* struct_theta,
                         const float* g_up, float scale, float* G_out, float* gS, int M, int D, uglad_stream_t stream);

/* Finish the 42 parameter gradients of one backward pass (sums over the LOCAL batch; the caller all-reduces them):
 *   grad[0]      = sum_m gt_partial[m]
 *   grad[1..28]  = sum_m grad_rho_partial[m][:]
 *   grad[29..41] = sum_k (sum_m glam_partial[k][m]) * dLambdaNN(lam_in[k])/dparams   (inputs are constants, glad_params.py:94)
 * glam_partial is (L, M); lam_in is (L+1, 2) as written by uglad_lambda_init/_step. */
int uglad_finish_grads(const float* gt_partial, const float* grad_rho_partial, const float* glam_partial,
                       const float* lam_in, const float* params, float* grad, int L, int M, uglad_stream_t stream);

/* The whole unrolled pass of glad.py:103-151 enqueued by ONE call: Theta_0, lambda_0, then L x {uglad_cell_fwd,
 * uglad_sum_partials, uglad_lambda_step} -- for the single-process case (a sharded batch needs the all-reduce between the last
 * two and drives the steps itself).  Z holds z_slabs slabs of (M,D,D): step k reads slab k % z_slabs and writes slab
 * (k+1) % z_slabs (z_slabs = L+1 keeps every Theta_k for the backward pass, 2 is enough for inference).  half/U (L,M,D,D) and
 * beta (L,M,D) may be NULL together.  lam (L+1), lam_in (L+1,2), nf_partial (M), nf_sum (1) as in the per-step calls.  cond_max (M floats
 * or NULL) is zeroed here and receives, per matrix, the maximum over the L steps of cond(b^T b + 4/lam I) (see uglad_cell_fwd). */
int uglad_glad_forward(const float* S, const float* params, float lambda_init, int init_diag, int L, float* Z, int z_slabs,
                       float* half, float* U, float* beta, float* lam, float* lam_in, float* nf_partial, float* nf_sum,
                       float* cond_max, float* workspace, int M, int D, int sqrt_mode, uglad_stream_t stream);

/* Its reverse: L x uglad_cell_bwd (ping-ponging gbuf0/gbuf1, each (M,D,D)), uglad_init_theta_bwd, uglad_finish_grads.
 * G_L = dL/dTheta_L; grad receives the 42 gradients.  grad_rho_partial (M,28) is zeroed here; glam_partial (L,M); gt_partial (M). */
int uglad_glad_backward(const float* G_L, const float* S, const float* params, int init_diag, int L, const float* Z,
                        const float* half, const float* U, const float* beta, const float* lam, const float* lam_in,
                        float* gbuf0, float* gbuf1, float* grad_rho_partial, float* glam_partial, float* gt_partial,
                        float* grad, float* workspace, int M, int D, int sqrt_mode, uglad_stream_t stream);

/* Grouped passes (the folds of CV mode as ONE batch): the M matrices are `groups` independent problems of
 * M / groups consecutive matrices, each with its own parameters and its own lambda sequence.  Same arguments as
 * uglad_glad_forward / uglad_glad_backward with: params (groups, 42); lam (L+1, groups); lam_in (L+1, groups, 2);
 * nf_sum (groups); grad (groups, 42).  groups == 1 is the plain call.  M % groups must be 0. */
int uglad_glad_forward_grouped(const float* S, const float* params, float lambda_init, int init_diag, int L, float* Z,
                               int z_slabs, float* half, float* U, float* beta, float* lam, float* lam_in, float* nf_partial,
                               float* nf_sum, float* cond_max, float* workspace, int M, int D, int groups, int sqrt_mode,
                               uglad_stream_t stream);
int uglad_glad_backward_grouped(const float* G_L, const float* S, const float* params, int init_diag, int L, const float* Z,
                                const float* half, const float* U, const float* beta, const float* lam, const float* lam_in,
                                float* gbuf0, float* gbuf1, float* grad_rho_partial, float* glam_partial, float* gt_partial,
                                float* grad, float* workspace, int M, int D, int groups, int sqrt_mode, uglad_stream_t stream);

/* The gradient with respect to the input covariance.  uglad_glad_backward_grouped (groups == 1: the plain pass) that also OVERWRITES
 * gS (M,D,D) with dL/dS of the whole pass:
 *   sum over the steps k of  G_B,k / lambda_k  (b_k = S / lambda_k - Z_k, glad.py:139)  +  the rhoNN input gradient of the S feature
 *   (glad.py:144, glad_params.py:75)  +  the Theta_0 term: -Theta_0 G_0 Theta_0 (init_diag 0) or -G_0,ii Theta_0,ii^2 (init_diag 1).
 * lambda_k contributes nothing: LambdaNN's inputs are detached (glad_params.py:94).
 * Convention: gS is the SYMMETRIC part (G + G^T) / 2 of the gradient autograd forms for the reference, which treats the D^2 entries of S
 * as independent; gS is exactly symmetric.  Every symmetric parametrisation of S (S = Xc^T Xc / N, ...) sees the same upstream gradient.
 * Theta, the 42 parameter gradients and G_0 come out bit-identical to uglad_glad_backward_grouped's (gbuf0/gbuf1 are scratch).
 * Kernels: on the spectral path's one-workgroup backward a variant of the cell kernel forms the step's terms (all L steps in one launch
 * for D <= 128); on the many-workgroups backward (uglad_set_wide_mode) and the matrix-iteration path (D > uglad_max_eig_dim(), or
 * uglad_set_matrix_iteration) the step runs unchanged and one elementwise kernel behind it forms them again from G_next, G_out and the
 * saved state (gz - sym(G_out) = G_B).  The Theta_0 term beyond the one-workgroup kernels: two tiled fp32 products. */
int uglad_glad_backward_wrt_s(const float* G_L, const float* S, const float* params, int init_diag, int L, const float* Z,
                              const float* half, const float* U, const float* beta, const float* lam, const float* lam_in,
                              float* gbuf0, float* gbuf1, float* grad_rho_partial, float* glam_partial, float* gt_partial,
                              float* grad, float* workspace, int M, int D, int groups, int sqrt_mode, float* gS, uglad_stream_t stream);

/* The unrolled pass of ONE RANK of a batch-sharded run, enqueued by one call (collective site i: the batch mean
 * behind get_frobenius_norm, glad.py:60-71,147, is the only coupling between the matrices of a batch).  As uglad_glad_forward on the M
 * local matrices, except that per step the local sum of nf_partial goes through `exchange` -- SUM over the ranks, in place, enqueued
 * on `stream`, no host synchronisation -- before lambda_{k+1} = LambdaNN([sum / m_global, lambda_k]) is formed, on every rank from the
 * same bits.  m_global = matrices over all ranks (the shards may differ in size).  The backward pass needs no exchange (the reference
 * detaches LambdaNN's inputs, glad_params.py:94): uglad_glad_backward on the local matrices, then one SUM of the 42 gradients per epoch.
 * exchange(buf, n, ctx, stream): 0 = ok; anything else is returned as is.  uglad_rccl_allreduce_sum below is one such function. */
typedef int (*uglad_allreduce_fn)(float* device_buf, int n, void* ctx, uglad_stream_t stream);
int uglad_glad_forward_sharded(const float* S, const float* params, float lambda_init, int init_diag, int L, float* Z, int z_slabs,
                               float* half, float* U, float* beta, float* lam, float* lam_in, float* nf_partial, float* nf_sum,
                               float* cond_max, float* workspace, int M, int D, int m_global, int sqrt_mode,
                               uglad_allreduce_fn exchange, void* exchange_ctx, uglad_stream_t stream);

/* RCCL over xGMI as that exchange: ncclAllReduce(SUM, fp32) issued from the library on the compute stream, one per unroll step, so
 * the 4-byte message costs a link latency and no Python.  The library resolves RCCL at run time (dlopen of the copy PyTorch-ROCm has
 * loaded, else the system's librccl.so); it has no link-time dependency on it.  One process per GPU:
 *   rank 0: uglad_rccl_unique_id(&id); ship the 128 bytes to the other ranks (e.g. torch.distributed.broadcast);
 *   every rank, after hipSetDevice: uglad_rccl_comm_init(&id, nranks, rank, &comm);  ... uglad_rccl_comm_destroy(comm).
 * uglad_rccl_allreduce_sum has the signature of uglad_allreduce_fn (ctx = the communicator).  UGLAD_E_RCCL when RCCL cannot be
 * loaded or a call fails. */
typedef struct { char internal[128]; } uglad_rccl_id; /* = ncclUniqueId */
int uglad_rccl_unique_id(uglad_rccl_id* id_out);
int uglad_rccl_comm_init(const uglad_rccl_id* id, int nranks, int rank, void** comm_out);
int uglad_rccl_comm_destroy(void* comm);
int uglad_rccl_comm_count(void* comm, int* nranks_out); /* ncclCommCount: the ranks the communicator spans */
int uglad_rccl_allreduce_sum(float* device_buf, int n, void* comm, uglad_stream_t stream);

/* Consensus over K precision matrices (main.py:700-716, type="min"), split so that a sharded batch can all-reduce
 * in between: partial -> absmin (D,D) = min_k |Theta_k|, signsum (D,D) = sum_k sign(Theta_k);
 * combine -> out = (signsum >= 0 ? +1 : -1) * absmin. */
int uglad_consensus_partial(const float* theta_K, int K, int D, float* absmin, float* signsum, uglad_stream_t stream);
int uglad_consensus_combine(const float* absmin, const float* signsum, int D, float* out, uglad_stream_t stream);

/* Batched symmetric eigendecomposition A_m = U_m diag(beta_m) U_m^T (A symmetric: both triangles are read; beta ascending):
 * Householder tridiagonalisation + divide & conquer + blocked back-transformation, the solver inside uglad_cell_fwd,
 * exported for unit tests.  U must not alias A (its slab doubles as reflector scratch).  No rescaling of the input: measured
 * on structured matrices (profiles/r04_symeig_sweep.txt) the errors are those of unit scale (<= 2.4e-6) for ||A|| from 1e-9 to
 * 1e18 and grow below (1e-4 at 1e-11: intermediate cubes of pole distances leave the fp32 range); the cell's b = S/lam - Z is O(1).
 * Accuracy (max of eigenvalue error / ||A||_2 and ||A U - U diag beta||_F / ||A||_F; profiles/eigensolver_spectra.txt): <= 5e-6 for
 * separated spectra, but there is no deflation, and a cluster of m (nearly) equal eigenvalues is spread over up to 4 * 2^-24 * m ||A||
 * -- O(D eps ||A||): the bound is 5e-6 + 4 * 2^-24 * D, i.e. 2.0e-5 / 3.6e-5 / 6.6e-5 at D = 64 / 128 / 256.  max |U^T U - I| <= 5e-6
 * either way.  Matrices of low rank (the constant matrix, blocks of ones next to blocks of zeros), whose tridiagonal form decays to
 * 1e-26 of ||A||, meet the 5e-6 bound: couplings below 8 eps ||A|| are dropped rather than merged, and a column whose entries below the
 * sub-diagonal have a norm below 3.2e-18 (absolute) gets no reflector. */
int uglad_symeig(const float* A, float* U, float* beta, float* workspace, int M, int D, uglad_stream_t stream);

/* Covariance front-end of fit() (replaces prepare_data.py:328-356 get_covariance and, with normalize = 1,
 * the min-max normalisation of prepare_data.py:597-613 / main.py:85): X (K,N,D) row-major tables -> S_out (K,D,D) =
 * sum_n (x_n - mean)(x_n - mean)^T / N of the (normalised) columns.  With eig_scratch != NULL (K*D*D + K*D floats) and a
 * workspace of uglad_workspace_floats(K, D) the reference's repair follows: where the smallest eigenvalue is <= 1e-6,
 * S += (eval_offset - min eig) I.  A constant column under normalize = 1 gives NaN, as in the reference. */
int uglad_covariance(const float* X, int K, int N, int D, int normalize, float eval_offset, float* S_out, float* eig_scratch,
                     float* workspace, uglad_stream_t stream);

/* The covariance front-end for every D <= uglad_max_dim() -- what the cell covers -- in fp64 and without an eigensolver (csrc/cov_wide.h).
 * X is a DEVICE pointer to (K, N, D) row-major tables in FP64 (the exception to this header's fp32 convention: the reference's tables
 * are fp64, and with every operation here in fp64 the only rounding left is the store of S_out).  S_out (K, D, D) fp32 receives the
 * covariance of the (normalize = 1: min-max normalised) columns, exactly symmetric; a constant column under normalize = 1 gives NaN,
 * as in the reference.  min_eig_out NULL: no repair.  Otherwise (K doubles) the reference's repair follows: a table whose smallest
 * eigenvalue is <= 1e-6 gets S += (eval_offset - min eig) I and min_eig_out[k] = that eigenvalue, found to ~1e-13 by bisection on
 * "S - sigma I has a Cholesky factorisation" (decided in fp64: error <= D (D + 1) 2^-53 tr S); a table that needs no repair gets
 * min_eig_out[k] = +infinity (its smallest eigenvalue is only known to exceed 1e-6).  Many workgroups per table, 2 + 1 + 25 (2 ceil(D / 64)
 * + 1) + 1 launches, no host readback.  workspace: uglad_covariance_wide_workspace_floats(K, D) floats, 8-byte aligned (UGLAD_E_NULL
 * otherwise), always required: per table two fp64 slabs of order D rounded up to 64, the column statistics and the bisection's state.
 * K <= 65535.  Errors as uglad_covariance; the workspace size is negative (UGLAD_E_DIM) on bad arguments or beyond 2^31 - 1 floats. */
int uglad_covariance_wide_workspace_floats(int K, int D);
int uglad_covariance_wide(const double* X, int K, int N, int D, int normalize, double eval_offset, float* S_out, double* min_eig_out,
                          float* workspace, uglad_stream_t stream);

/* The association matrix of K tables that mix categorical and real columns, and the reference's repair on it (csrc/assoc_wide.h; replaces
 * prepare_data.py:253-285 pairwise_cov_matrix with :177-209 cramers_v -- bias-corrected Cramer's V, Yates' correction on a 2 x 2 table as
 * scipy's chi2_contingency applies it -- for c/c pairs, :212-250 correlation_ratio for c/r pairs and Pearson's r for r/r pairs, and
 * :347-352, the repair of get_covariance).  table is a DEVICE pointer to (K, N, D) row-major FP64 tables, encoded: a categorical column
 * holds level codes 0 .. card - 1, a real column its values.  The five maps are DEVICE int arrays that describe the expanded layout the
 * K tables share (one column per level, one per real column; uglad_amd.utils.prepare_data.encode_mixed_table makes them):
 * col_feature[W] (-1: padding), col_level[W] (>= 0 a level, -1 a real column, -2 padding), feat_offset[D], feat_width[D] -- a feature's
 * expanded columns never straddle a multiple of 64 -- and tile_first[W / 64 + 1], the first feature of every 64 expanded columns (the last
 * entry is D).  W is a multiple of 64, D <= W <= UGLAD_ASSOC_MAX_WIDTH.  A level without a row in a table is ignored there, as pd.crosstab
 * ignores it.  A_out (K, D, D) fp32 receives the matrix, exactly symmetric; A64_out (K, D, D) fp64, optional, the same before the one
 * rounding and ALWAYS unrepaired.  min_eig_out NULL: no repair.  Otherwise (K doubles): a table whose smallest eigenvalue is <= 1e-6 gets
 * A_out += (eval_offset - min eig) I and min_eig_out[k] = that eigenvalue, found by 48 bisection steps on "A - sigma I has a Cholesky
 * factorisation" over [-||A||_inf, 1e-6] (the matrix is indefinite: V and eta are >= 0, r is signed) to ||A||_inf 2^-48; a table that
 * passes at 1e-6 gets +infinity.  Many workgroups per table, 3 + 50 + 49 * 2 ceil(D / 64) + 1 launches, no host readback.  A NaN in a
 * real column gives NaN in that feature's row and column only (without repair).  workspace: uglad_association_workspace_floats(K, D, W)
 * floats, 8-byte aligned (UGLAD_E_NULL otherwise).  2 <= D <= uglad_max_dim(), N >= 2, K <= 65535 (UGLAD_E_DIM otherwise, as for a W
 * that is no multiple of 64 or out of range); the workspace size is negative (UGLAD_E_DIM) on bad arguments or beyond 2^31 - 1 floats. */
#define UGLAD_ASSOC_MAX_WIDTH 16384
int uglad_association_max_width(void);
int uglad_association_workspace_floats(int K, int D, int W);
int uglad_association(const double* table, int K, int N, int D, const int* col_feature, const int* col_level, const int* feat_offset,
                      const int* feat_width, const int* tile_first, int W, double eval_offset, float* A_out, double* A64_out,
                      double* min_eig_out, float* workspace, uglad_stream_t stream);

/* The rank-based correlation matrix of K tables, the front-end of the nonparanormal (Gaussian copula) model, and the repair on it
 * (csrc/rank_wide.h).  X is a DEVICE pointer to (K, N, D) row-major FP64 tables.  Every column is ranked by r2_a = 2 #{b : x_b < x_a} +
 * #{b : x_b = x_a} + 1, twice scipy's rankdata(method="average"), an int32; +-Inf rank like any value.  method:
 *   UGLAD_RANK_SPEARMAN  rho_ij = g_ij / (sqrt(g_ii) sqrt(g_jj)), g = sum_a c_ai c_aj, c = r2 - (N + 1), exact integers; transform = 1
 *                        maps it through 2 sin(pi rho / 6)
 *   UGLAD_RANK_KENDALL   tau-b: tau_ij = G_ij / (sqrt(G_ii) sqrt(G_jj)), G = s^T s over the N (N - 1) / 2 row pairs a < b with
 *                        s = sign(x_a - x_b): G_ij = concordant - discordant pairs, G_ii = pairs not tied in column i, exact integers formed
 *                        on v_mfma_i32_16x16x64_i8; transform = 1 maps it through sin(pi tau / 2)
 *   UGLAD_RANK_SCORES    Pearson's r of the normal scores z = Phi^-1(r2 / (2 (N + 1))), g = their centred sums of products (not divided
 *                        by N); transform is ignored
 * A_out (K, D, D) fp32 receives the matrix, exactly symmetric, its diagonal exactly 1 before the repair; A64_out (K, D, D) fp64, optional,
 * the same before the one rounding and ALWAYS unrepaired; gram_out (K, D, D) fp64, optional, g or G above, exactly symmetric; info_out
 * (K, D) int32, optional: bit 0 set for a column that holds a NaN, bit 1 for a constant column.  Either flag gives NaN in that feature's
 * row and column of the matrix and nowhere else (without repair); a NaN column also in gram_out.  min_eig_out NULL: no repair.
 * Otherwise (K doubles), as uglad_association -- the transforms do not preserve positive semi-definiteness --: a table whose smallest
 * eigenvalue is <= 1e-6 gets A_out += (eval_offset - min eig) I and min_eig_out[k] = that eigenvalue, by 48 bisection steps over
 * [-||A||_inf, 1e-6]; a table that passes at 1e-6 gets +infinity.  Many workgroups per table, no host readback, no allocation; every
 * result is bit-reproducible and does not depend on K, on the table's place in the batch or, for Kendall, on
 * uglad_rank_correlation_pair_chunks(K, N, D), the number of chunks the pairs of a tile of G are dealt over (their int32 partial tiles
 * are combined by integer atomics).  workspace: uglad_rank_correlation_workspace_floats(K, N, D, method) floats, 8-byte aligned
 * (UGLAD_E_NULL otherwise).  2 <= D <= uglad_max_dim(), 2 <= N <= 65536 (where G_ii reaches 2^31), K <= 65535 (UGLAD_E_DIM otherwise);
 * an unknown method or a transform that is not 0 / 1 gives UGLAD_E_MODE; the workspace size is negative on bad arguments (UGLAD_E_DIM,
 * UGLAD_E_MODE) or beyond 2^31 - 1 floats (UGLAD_E_DIM). */
#define UGLAD_RANK_SPEARMAN 0
#define UGLAD_RANK_KENDALL 1
#define UGLAD_RANK_SCORES 2
int uglad_rank_correlation_workspace_floats(int K, int N, int D, int method);
int uglad_rank_correlation_pair_chunks(int K, int N, int D);
int uglad_rank_correlation(const double* X, int K, int N, int D, int method, int transform, double eval_offset, float* A_out,
                           double* A64_out, double* gram_out, int* info_out, double* min_eig_out, float* workspace, uglad_stream_t stream);

/* The available-case (pairwise-complete) covariance of K tables with missing entries, and the repair on it (csrc/pairwise_wide.h; what
 * pandas' DataFrame.cov and R's cov(use = "pairwise.complete.obs") compute, with the reference's divisor).  X is a DEVICE pointer to
 * (K, N, D) row-major FP64 tables; only NaN counts as missing.  With m_ni = 1 where x_ni is observed, y = x (normalize = 0) or
 * y = (x - mn_i) * (1 / (mx_i - mn_i)) over the observed minimum and maximum of column i (normalize = 1), mu_i the mean of the observed
 * y_.i and z_ni = m_ni (y_ni - mu_i):  n_ij = sum_n m_ni m_nj, a_ij = sum_n z_ni m_nj, p_ij = sum_n z_ni z_nj and
 *   cov_ij = p_ij / n_ij - (a_ij / n_ij) (a_ji / n_ij),
 * the covariance of the n_ij rows where both columns are observed, every mean taken over those rows, divided by n_ij (pandas' value times
 * (n_ij - 1) / n_ij).  The shift by mu_i keeps a column offset from cancelling; mu_i is the implementation's rounding of the observed
 * mean ((sum of the observed x / their number - mn_i) * scale), which the result depends on by rounding alone.  Every sum has a fixed
 * order: two calls give the same bits, and they do not depend on K or on the table's place in the batch.  S_out (K, D, D) fp32 receives the
 * matrix, exactly symmetric; S64_out (K, D, D) fp64, optional, the same before the one rounding and ALWAYS unrepaired; counts_out
 * (K, D, D) int32, optional, n_ij; info_out (K, D) int32, optional, per column: bit 1 the column has no observed entry; 2 it is in a pair
 * with n_ij < min_pairs (that entry is NaN; pairs with a column flagged 1, 4 or 8 do not count); 4 normalize = 1 and its observed values
 * are constant (0 / 0, as the reference's NaN); 8 it holds an infinity, which is a value and propagates.  A column flagged 1, 4 or 8 has
 * NaN in its row and column.  min_eig_out NULL: no repair.  Otherwise (K doubles), as uglad_association -- the matrix is in general
 * indefinite, every entry having its own set of rows --: a table whose smallest eigenvalue is <= 1e-6 gets S_out += (eval_offset - min
 * eig) I and min_eig_out[k] = that eigenvalue, by 48 bisection steps over [-||S||_inf, 1e-6]; a table that passes at 1e-6 gets
 * +infinity; a table with any flag set is not repaired and gets NaN, at the cost of empty launches.  Many workgroups per table,
 * 3 + 52 + 49 * 2 ceil(D / 64) + 2 launches, no host readback, no allocation.  workspace: uglad_pairwise_covariance_workspace_floats(K, D)
 * floats, 8-byte aligned (UGLAD_E_NULL otherwise): per table uglad_covariance_wide's slabs and D rounded up to 64, plus 2, int32 of
 * flags.  1 <= D <= uglad_max_dim(), N >= 1, K <= 65535 (UGLAD_E_DIM otherwise); normalize not 0 / 1 or min_pairs < 1 gives UGLAD_E_MODE;
 * the workspace size is negative (UGLAD_E_DIM) on bad arguments or beyond 2^31 - 1 floats. */
int uglad_pairwise_covariance_workspace_floats(int K, int D);
int uglad_pairwise_covariance(const double* X, int K, int N, int D, int normalize, int min_pairs, double eval_offset, float* S_out,
                              double* S64_out, int* counts_out, int* info_out, double* min_eig_out, float* workspace, uglad_stream_t stream);

/* The covariances of ONE table under R weightings of its rows, and the repair on each (csrc/wcov_wide.h; additive: what resampling needs
 * -- a bootstrap resample is a weighting by integer multiplicities, a subsample or a fold one by 0 / 1, a smoothing window one by real
 * weights).  The caller defines X, a DEVICE pointer to the (N, D) row-major FP64 table, and W, a DEVICE pointer to (R, N) FP64 weights;
 * both are only read.  For weighting r, with s = sum_n w_n and mu = sum_n w_n x_n / s:
 *   S = sum_n w_n (x_n - mu) (x_n - mu)^T / s,
 * empirical_covariance of the table with row n repeated w_n times (integer weights), of the row subset (0 / 1), of the table (all ones).
 * There is no normalisation: the caller normalises the table once.  The table is shifted by its unweighted column means c, so that one
 * staged chunk of it serves several weightings, and S = G / s - d d^T with G the weighted Gram matrix of x - c and d = mu - c.  Every sum
 * has a fixed order: two calls give the same bits, and a weighting's bits do not depend on R or on its place in the call.  The entry
 * point defines every element of its outputs: S_out (R, D, D) fp32, exactly symmetric; S64_out (R, D, D) fp64, optional, the same before
 * the one rounding and ALWAYS unrepaired; mean_out (R, D) fp64, optional, mu; info_out (R) int32, per weighting: bit 1 a weight is
 * negative, NaN or infinite; 2 the weights sum to zero.  A flagged weighting is NaN throughout S_out, S64_out and mean_out and leaves
 * the others' bits alone.  A NaN or an infinity in X propagates into that column's row and column of every weighting.  min_eig_out NULL:
 * no repair.  Otherwise (R doubles), as uglad_covariance_wide per weighting: smallest eigenvalue <= 1e-6 gives S_out += (eval_offset -
 * min eig) I and min_eig_out[r] = that eigenvalue; a weighting that passes at 1e-6 gets +infinity; a flagged one is not repaired and
 * gets NaN, at the cost of empty launches.  3 + 25 (2 ceil(D / 64) + 1) + 4 launches, no host readback, no allocation.  workspace:
 * uglad_weighted_covariance_workspace_floats(R, D) floats, 8-byte aligned (UGLAD_E_NULL otherwise), scratch: per weighting
 * uglad_covariance_wide's slabs and D rounded up to 64, plus 2, doubles of its sums.  1 <= D <= uglad_max_dim(), N >= 1, 1 <= R <= 65535
 * (UGLAD_E_DIM otherwise); the workspace size is negative (UGLAD_E_DIM) on bad arguments or beyond 2^31 - 1 floats. */
int uglad_weighted_covariance_workspace_floats(int R, int D);
int uglad_weighted_covariance(const double* X, const double* W, int R, int N, int D, double eval_offset, float* S_out, double* S64_out,
                              double* mean_out, int* info_out, double* min_eig_out, float* workspace, uglad_stream_t stream);

/* First half of the eigensolver on its own (unit tests, profiling): Householder tridiagonalisation of A = A0 (A1 == NULL) or
 * A = A0/lam[0] - A1 (the cell's b = S/lam - Z).  Row k of R_m (M, D, D) receives reflector v_k, the rows without one (D-2, D-1) are
 * zero; workspace receives d, e, tau
 * (3 x 32*ceil(D/32) floats per matrix).  uglad_cell_fwd / uglad_symeig / uglad_init_theta / uglad_loss_fwd launch this
 * kernel themselves before their divide & conquer kernel. */
int uglad_tridiagonalize(const float* A0, const float* A1, const float* lam, float* R, float* workspace, int M, int D,
                         uglad_stream_t stream);

/* After the path: conditional Gaussian given observed coordinates, K independent problems.  Replaces
 * conditional_gaussian_with_probabilities + compute_map_estimate (main.py:1176-1260; scipy.linalg.solve / np.linalg.inv /
 * multivariate_normal.pdf on the host) with the path's own eigensolver on the masked precision matrix.
 *   precision (K,D,D) symmetric (upper triangle read); mean (K,D); observed (K,D): non-zero where the coordinate is observed;
 *   values (K,D): read at the observed coordinates.
 *   full_mean (K,D): values at the observed coordinates, mean_u - L_uu^-1 L_uo (x_o - mean_o) elsewhere; clip01 != 0 clamps
 *                    it to [0,1] (compute_map_estimate, main.py:1260);
 *   cond_cov (K,D,D): L_uu^-1 on the (unobserved, unobserved) block, identity on the observed coordinates (required: its slab
 *                    doubles as the solver's reflector scratch);
 *   log_pdf (K) or NULL: log N(map; map, L_uu^-1) = -n_u/2 log(2 pi) + 1/2 logdet L_uu (NaN unless L_uu is positive definite);
 *   scratch: K*D*D floats; workspace: uglad_workspace_floats(K, D). */
int uglad_conditional_mean(const float* precision, const float* mean, const float* observed, const float* values,
                           float* full_mean, float* cond_cov, float* log_pdf, float* scratch, float* workspace, int K, int D,
                           int clip01, uglad_stream_t stream);

/* The same conditional Gaussian for every D <= uglad_max_dim() -- what the cell covers -- in fp64 and without the eigensolver
 * (csrc/after_wide.h; replaces conditional_gaussian_with_probabilities + compute_map_estimate, main.py:1176-1260): the masked precision
 * matrix (P on the (unobserved, unobserved) block, identity elsewhere) is factored by the blocked Cholesky of uglad_covariance_wide, many
 * workgroups per problem; L^-1 by block forward substitution gives the solve (with one step of refinement), the inverse and the
 * log-determinant.  precision, mean, values, full_mean and log_pdf are FP64 DEVICE pointers (as for uglad_covariance_wide: the only
 * rounding left is the fp32 store of cond_cov); observed is fp32, non-zero where the coordinate is observed.
 *   cond_cov (K,D,D) fp32 or NULL: exactly symmetric; NULL skips the product (compute_map_estimate needs none);
 *   log_pdf (K) or NULL.
 * L_uu not positive definite (a pivot <= 0 or NaN): log_pdf = NaN, the unobserved entries of full_mean and the (u, u) block of cond_cov
 * are NaN, observed entries pass through, the other problems of the batch are unaffected (the reference's multivariate_normal.pdf
 * raises there).  3 ceil(D / 64) + 8 launches in one chain, no host readback.  workspace:
 * uglad_conditional_mean_wide_workspace_floats(K, D) floats, 8-byte aligned (UGLAD_E_NULL otherwise).  K <= 65535.  Errors as
 * uglad_covariance_wide; the workspace size is negative (UGLAD_E_DIM) on bad arguments or beyond 2^31 - 1 floats. */
int uglad_conditional_mean_wide_workspace_floats(int K, int D);
int uglad_conditional_mean_wide(const double* precision, const double* mean, const float* observed, const double* values,
                                double* full_mean, float* cond_cov, double* log_pdf, float* workspace, int K, int D, int clip01,
                                uglad_stream_t stream);

/* Scoring rows against K fitted models, every 1 <= D <= uglad_max_dim(), fp64 throughout, many workgroups per model (csrc/score_wide.h):
 * what sklearn's covariance estimators offer as mahalanobis(X) and score_samples(X), which the reference lacks.  With
 * P = (precision + precision^T) / 2 (formed in fp64) and xc = x - mean:
 *   mahalanobis (K, N)           q = xc^T P xc, the SQUARED distance (as sklearn returns it); required;
 *   log_density (K, N) or NULL   (logdet P - D log 2 pi - q) / 2;
 *   logdet (K) or NULL           from the log-pivots of the blocked Cholesky of uglad_conditional_mean_wide.
 * X is (x_batch, N, D) with x_batch = K, or 1 for one table scored by every model; precision (K, D, D), mean (K, D); all FP64 DEVICE
 * pointers.  A row's two numbers depend on that row and the model alone, bit for bit: not on N, on the row's position, on K or on the
 * model's place in the batch -- so a table may be scored in chunks of rows.  A NaN in a row stays in that row.  P not positive definite (a
 * pivot <= 0 or NaN): logdet and every log_density of that model are NaN, its mahalanobis values are still returned, the other models are
 * unaffected.  The factorisation is skipped when log_density and logdet are both NULL.  At most 2 ceil(D / 64) + 4 launches in one chain,
 * no host readback.  workspace: uglad_sample_scores_workspace_floats(K, N, D) floats (a problem of uglad_conditional_mean_wide per model and
 * ceil(D / 64) partial sums per model and row), 8-byte aligned (UGLAD_E_NULL otherwise).  K <= 65535, N >= 1, x_batch in {1, K}
 * (UGLAD_E_DIM otherwise).  Errors as uglad_conditional_mean_wide; the workspace size is negative (UGLAD_E_DIM) on bad arguments or beyond
 * 2^31 - 1 floats, which a large N reaches: score such a table in chunks of rows. */
int uglad_sample_scores_workspace_floats(int K, int N, int D);
int uglad_sample_scores(const double* X, int x_batch, const double* precision, const double* mean, double* mahalanobis,
                        double* log_density, double* logdet, float* workspace, int K, int N, int D, uglad_stream_t stream);

/* After the path.  Partial correlations rho_ij = -p_ij / sqrt(p_ii p_jj) from the upper triangle, mirrored,
 * ones on the diagonal (get_partial_correlations, main.py:796-821), K matrices at once. */
int uglad_partial_correlations(const float* precision, float* rho, int K, int D, uglad_stream_t stream);

/* Support-recovery metrics of report_metrics_all (utils/metrics.py:25-108) for K (true, predicted) pairs: out (K, 11) DOUBLES on
 * the device = FDR, TPR, FPR, SHD, nnzTrue, nnzPred, precision, recall, Fbeta, aupr, auc, unrounded (the reference rounds to 3
 * decimals).  Integer counting throughout; AUC / AUPR as sklearn defines them (ties included).  2 <= D <= uglad_max_eig_dim(). */
int uglad_support_metrics(const float* true_theta, const float* pred_theta, double* out, int K, int D, int beta,
                          uglad_stream_t stream);

/* The same 11 numbers for every 2 <= D <= uglad_max_dim() -- what the cell covers -- with many workgroups per pair (csrc/metrics_wide.h).
 * uglad_support_metrics sweeps all E = D (D - 1) / 2 scores once per true edge from the LDS of one workgroup; here each pair's edges are
 * sorted by score -- one 32-bit key per edge, ((bits(|pred|)) << 1) | label, a radix sort of 8 passes of 4 bits -- and the ranking metrics
 * are prefix counts over the sorted keys: O(E) work per pass whatever the labels.  Same inputs, same definitions, all counting in
 * integers; `!= 0` is decided on the bit pattern ((bits & 0x7fffffff) != 0: denormals and -0.0 as in numpy).  Every entry but aupr is
 * bit-equal to uglad_support_metrics where both exist; aupr sums its T terms in another (fixed) order.  Results do not depend on K or on
 * the pair's place in the batch.  NaN scores (sklearn raises on them) order by their bit pattern, above every finite score: the call
 * terminates and returns what that order gives.  4 + 3 * 8 launches in one chain, no host readback.  workspace:
 * uglad_support_metrics_wide_workspace_floats(K, D) floats (two key buffers of E words and the sort's tables per pair), 8-byte aligned
 * (UGLAD_E_NULL otherwise).  K <= 65535.  Errors as uglad_conditional_mean_wide; the workspace size is negative (UGLAD_E_DIM) on bad
 * arguments (D < 2 among them) or beyond 2^31 - 1 floats. */
int uglad_support_metrics_wide_workspace_floats(int K, int D);
int uglad_support_metrics_wide(const float* true_theta, const float* pred_theta, double* out, float* workspace, int K, int D, int beta,
                               uglad_stream_t stream);

/* The recovered graph of K precision (from_precision = 1) or partial-correlation (0) matrices, every 2 <= D <= uglad_max_dim(), many
 * workgroups per problem (csrc/graph_wide.h): what graph_from_partial_correlations (main.py:825-946, called by viz_graph_from_precision,
 * main.py:985-1005) builds edge by edge in a Python double loop, and the first six columns of compute_graph_statistics (main.py:1263-1300).
 * Edges are the strict upper triangle in row-major order, E = D (D - 1) / 2, values read at [i][j], i < j; from a precision matrix
 * rho_ij = -P[i][j] / sqrtf(P[i][i] * P[j][j]) in three correctly rounded fp32 operations (main.py:818-820 on a float32 precision_).
 * Threshold per problem: n_keep[k] (HOST array; Python's int(sparsity * E), main.py:865) gives th = s[E - n_keep] with s = |rho| ascending,
 * s[0] for n_keep = 0 (main.py:867: rho_upper[-0]); n_keep[k] = -1 takes threshold_in[k] (device; may be NULL when no entry is -1).  Edge
 * (i, j) is kept iff rho_ij > th or rho_ij < -th (main.py:874, 892); NaN is never an edge and a NaN threshold keeps nothing.
 * Outputs (device): threshold (K); edge_count (K) = m; edge_ij (K, E, 2) int32 and edge_w (K, E) fp32, the first m entries of a problem in
 * the reference's order, the rest undefined (sign: w > th is "+"); degree (K, D) int32; with want_stats = 1 also triangles2 (K, D) int32,
 * t_i = twice the triangles at node i, and stats (K, 6) DOUBLES = num_nodes, num_edges, avg_degree, density, avg_clustering, transitivity
 * by the operations networkx performs on exact integers (one fp64 division each; the c_i summed in node order) -- with want_stats = 0 both
 * may be NULL and the triangle product is not launched.  Results do not depend on K or on the problem's place in the batch.  One chain of
 * at most 32 + ceil(K / 64) launches, no host readback.  workspace: uglad_graph_wide_workspace_floats(K, D) floats, 8-byte aligned
 * (UGLAD_E_NULL otherwise).  K <= 65535.  UGLAD_E_DIM for a dimension or an n_keep outside [-1, E], UGLAD_E_MODE for a flag that is not
 * 0 / 1, all checked before any launch; the workspace size is negative (UGLAD_E_DIM) on bad arguments or beyond 2^31 - 1 floats. */
int uglad_graph_wide_workspace_floats(int K, int D);
int uglad_graph_wide(const float* values, int from_precision, const int* n_keep, const float* threshold_in, float* threshold,
                     int* edge_count, int* edge_ij, float* edge_w, int* degree, int* triangles2, double* stats, int want_stats, int K, int D,
                     float* workspace, uglad_stream_t stream);

/* How often every edge comes back over R recovered graphs (csrc/graph_wide.h; the selection frequencies of stability selection, StARS'
 * instability).  The inputs are what uglad_graph_wide leaves for K = R problems of dimension D, defined by that call and only read here:
 * edge_count (R), edge_ij (R, E, 2), edge_w (R, E), E = D (D - 1) / 2; only the first edge_count[r] entries of list r are read.  The entry
 * point defines every element of its outputs and zeroes them itself: count_out (D, D) int32, count_out[i][j] = count_out[j][i] = the
 * number of lists that hold edge {i, j}, zero on the diagonal; positive_out (D, D) int32, the same count over the edges with weight > 0;
 * totals_out (2) 64-bit integers = {sum_{i < j} c_ij, sum_{i < j} c_ij (R - c_ij)}, exact.  Integer atomics only: the output does not
 * depend on the order of the additions.  No workspace; 4 launches, no host readback.  2 <= D <= uglad_max_dim(), 1 <= R <= 65535
 * (UGLAD_E_DIM otherwise); a NULL pointer gives UGLAD_E_NULL. */
int uglad_edge_frequency(const int* edge_count, const int* edge_ij, const float* edge_w, int R, int D, int* count_out, int* positive_out,
                         long long* totals_out, uglad_stream_t stream);

/* All eigenvalues of K symmetric matrices, every 1 <= D <= uglad_max_dim(), values only, fp64 throughout, many workgroups per matrix
 * (csrc/eigvals_wide.h): a blocked Householder tridiagonalisation (panels of 64, the trailing updates on the fp64 MFMA) and Sturm-count
 * bisection with a fixed number of steps.  A64 (K, D, D) FP64 DEVICE pointer; the matrix solved is its symmetric part (A + A^T) / 2.
 *   eig_out (K, D)       the eigenvalues, ASCENDING
 *   summary_out (K, 6)   min eig, max eig, min |eig|, max |eig|, con = max |eig| / min |eig| (eigen_val_condition_num,
 *                        prepare_data.py:310-325), and the number of eigenvalues < th, as a double
 * A matrix with a NaN or Inf entry comes back as NaN in all D places (its count is 0); the others of the batch are not touched.  Results
 * are bit-reproducible and do not depend on K or on the matrix's place in the batch.  One chain of 2 D + D / 64 + 3 launches, no host
 * readback.  workspace: uglad_eigvalsh_wide_workspace_floats(K, D) floats, 8-byte aligned (UGLAD_E_NULL otherwise).  K <= 65535.
 * UGLAD_E_NULL / UGLAD_E_DIM as for uglad_covariance_wide; the workspace size is negative (UGLAD_E_DIM) on bad arguments or beyond
 * 2^31 - 1 floats. */
int uglad_eigvalsh_wide_workspace_floats(int K, int D);
int uglad_eigvalsh_wide(const double* A64, int K, int D, double th, double* eig_out, double* summary_out, float* workspace,
                        uglad_stream_t stream);

/* The same for the empirical covariance (centred, / N) of K tables X64 (K, N, D) FP64, N >= 1: analyse_condition_number
 * (prepare_data.py:569-594) without the table leaving the device.  The covariance is formed by the Gram product of
 * uglad_covariance_wide straight into the solver's slab; cov_out (K, D, D) FP64 or NULL also receives it, exactly symmetric.
 * workspace: uglad_eigvalsh_wide_workspace_floats(K, D). */
int uglad_table_spectrum(const double* X64, int K, int N, int D, double th, double* eig_out, double* summary_out, double* cov_out,
                         float* workspace, uglad_stream_t stream);

/* get_highly_correlated_features (prepare_data.py:519-550) for K covariance matrices S64 (K, D, D) FP64, every 2 <= D <= uglad_max_dim()
 * (csrc/corr_wide.h): cov2 = the covariance of S's rows (/ D, centred) with a zero diagonal; th = the element at index int(0.1 n) of the
 * n = D (D - 1) / 2 upper-triangle |cov2| in descending order, found exactly by a radix select on the fp64 bit patterns; counts (K, D)
 * int32 = the entries of a row of |cov2| that are >= th; order (K, D) int32 = the features by count descending, ties by index ascending;
 * n_listed (K) int32 = the features with a non-zero count: order[k][:n_listed[k]] is the reference's list.  One chain of 21 launches, no
 * host readback.  workspace: uglad_correlated_features_workspace_floats(K, D) floats, 8-byte aligned.  Errors as uglad_eigvalsh_wide. */
int uglad_correlated_features_workspace_floats(int K, int D);
int uglad_correlated_features(const double* S64, int K, int D, int* order, int* counts, int* n_listed, float* workspace,
                              uglad_stream_t stream);

/* The same decomposition by two-sided cyclic Jacobi (round-robin ordering, Rutishauser rotations): slower, independent of
 * the divide & conquer solver; beta comes back unsorted.  Cross-check only. */
int uglad_symeig_jacobi(const float* A, float* U, float* beta, int M, int D, uglad_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* UGLAD_HIP_H */
