// Host layer, part 1 of 6 (glad_kernels.hip, the manifest of the library, includes them in this order after the kernel headers and its
// instantiation lists -- in the host unit and the single-unit build, not in the per-NT units; none of them holds device code):
//   host_route.h   build limits, the run-time switches, the dispatch on NT, Route (which kernels a call launches), workspace layouts
//   host_launch.h  the launch sequence of every path
//   host_api.h     the extern "C" entry points of the pass: validate, build a Route, call host_launch.h
//   host_rccl.h    RCCL as the exchange of the sharded pass
//   host_extra.h   the one-workgroup utilities (symeig, covariance, conditional mean, ...) and the diagnostic exports
//   host_wide.h    the many-workgroup fp64 utilities: their shared checks and launch chains, their entry points
#pragma once
#include <type_traits>
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
#define UGLAD_MAX_DIM (kNsMaxD > UGLAD_MAX_EIG_DIM ? kNsMaxD : UGLAD_MAX_EIG_DIM)  // beyond the eigensolver: the matrix-iteration path (wide_ns.h, ldl_wide.h)
// cond(b^T b + 4/lam I) up to which reference-made goldens sit inside the 1e-4 tolerance on Theta (tests/golden/regime_sweep.json:
// every case up to cond 708 within 1.1e-5 of the fp64 value of its own function; the min-max-normalised fit that runs to convergence,
// tests/golden/fit_direct_converged.npz, reaches 1.03e3 with precision_ 2.0e-5 from the reference; the case at 4.4e3 is 1.04e-4 off:
// DESIGN.md section 2).  Round 3 had 1000 here, BELOW a case its own goldens validate -- that fit warned.
#define UGLAD_VALIDATED_COND 1500.0f
// UGLAD_NT_MASK (test builds only: bit k set = NT = k is instantiated; default all): the sanitizer build compiles just the padded
// sizes its script uses, which halves its compile time.  A size that is masked out is refused like one beyond UGLAD_MAX_DIM.
#ifndef UGLAD_NT_MASK
#define UGLAD_NT_MASK 0x1fe
#endif
constexpr bool has_nt(int k) { return k >= 1 && k <= UGLAD_MAX_NT && (((UGLAD_NT_MASK) >> k) & 1); }
constexpr int nt_of(int D) { return (D + 31) / 32; }
constexpr int padded_dim(int D) { return nt_of(D) * 32; }
// (the matrix iteration's launches carry matrix x product, up to three products, in one grid dimension of at most 65535)
constexpr int kNsMaxBatch = 65535 / 3;

// grid of a grid-stride kernel over n elements: blocks of 256 threads, at most cap
static inline unsigned blocks256(size_t n, unsigned cap) { return (unsigned)((n + 255) / 256 < cap ? (n + 255) / 256 : cap); }
static inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// Dispatch on NT = ceil(D / 32): every padded size has its own instantiation; beyond NT = 4 (D > 128) the kernels keep their two D x D
// buffers in the caller's workspace instead of LDS.  Calls f(std::integral_constant<int, NT>) if NT lies in Lo..Hi and this build has it;
// a size the build leaves out is never named (the host unit only declares the instantiations that exist), and the entry points have refused it.
template <int Lo, int Hi, class F>
static inline void dispatch_nt(int D, F&& f) {
  if constexpr (Lo <= Hi) {
    if constexpr (has_nt(Lo)) {
      if (nt_of(D) == Lo) return f(std::integral_constant<int, Lo>{});
    }
    dispatch_nt<Lo + 1, Hi>(D, f);
  }
}
template <class F>
static inline void for_nt(int D, F&& f) { dispatch_nt<1, 8>(D, f); }
template <class F>
static inline void for_nt_lds(int D, F&& f) { dispatch_nt<1, 4>(D, f); }  // kernels instantiated for NT <= 4 only

// ---- the run-time switches: every one is an integer in the environment, read on every call (tests flip them); unset or not a number = default
enum Switch { kSwTridiagWave, kSwTridiagSmall, kSwNoFusedLambda, kSwCholesky, kSwPersistentBwd, kSwWideBwd, kSwMatrixIteration, kSwNsTile,
              kSwNsPrefetchAll, kSwLdlLaunches };
constexpr int kAuto = -1;
constexpr struct { const char* name; int dflt; const char* selects; } kSwitches[] = {
    {"UGLAD_TRIDIAG_WAVE", 1, "0: the workgroup tridiagonalisation also for D <= 32 (tridiag_wave.h; A/B measurements)"},
    {"UGLAD_TRIDIAG_SMALL", 1, "0: 512 threads also for D <= 96 (profiles/r04_tridiag_small.txt)"},
    {"UGLAD_NO_FUSED_LAMBDA", 0, "1: one matrix per group: the lambda step as its own launch instead of inside the cell's second launch"},
    {"UGLAD_CHOLESKY", 1, "0: D <= 128: Theta_0 and the loss's logdet / inverse on the eigen path for every matrix"},
    {"UGLAD_PERSISTENT_BWD", 1, "0: one launch per step of the backward pass also for D <= 128"},
    {"UGLAD_WIDE_BWD", kAuto, "0 / 1: D > 128: one / many workgroups per matrix; uglad_set_wide_mode() wins"},
    {"UGLAD_MATRIX_ITERATION", kAuto, "0: the matrix iteration only beyond the eigensolver's size, 1: for every D; uglad_set_matrix_iteration() wins"},
    {"UGLAD_NS_TILE", kAuto, "32 / 64: output tile of the fp64 products (default: by the batch)"},
    {"UGLAD_NS_PREFETCH_ALL", 1, "0: the 32 x 32 products without all k-chunks in flight"},
    {"UGLAD_LDL_LAUNCHES", kAuto, "0 / 1: L D L^T as one workgroup per matrix / as a sequence of chip-wide launches (default: by size)"},
};
static int switch_value(Switch s) {
  const char* e = std::getenv(kSwitches[s].name);
  return e && e[0] >= '0' && e[0] <= '9' ? std::atoi(e) : kSwitches[s].dflt;
}
static bool switch_on(Switch s) { return switch_value(s) != 0; }
// the two that also have a setter: kUnset = the environment decides, on every call; a value set through the API wins
constexpr int kUnset = -2;
static std::atomic<int> g_wide_mode{kUnset}, g_ns_mode{kUnset};  // -1 automatic, 0 never, 1 always
static int mode_of(const std::atomic<int>& set, Switch s) {
  const int mode = set.load(std::memory_order_relaxed);
  if (mode != kUnset) return mode;
  const int env = switch_value(s);
  return env < 0 ? kAuto : (env ? 1 : 0);
}

// ---- the route of a call: built once per entry point from the shape and the switches; every launcher takes it
enum class CellPath { kOneWorkgroup, kWide, kMatrixIteration };  // one workgroup per matrix | many (wide_*.h) | wide_ns.h
enum class Factor { kCholesky, kEigen, kWideInverse, kLdl };     // Theta_0, its gradient and the loss's logdet / inverse
enum class Tridiag { kWave, kSmall, kDefault, kBig };             // tridiag_wave_kernel | 128 NT threads | kThreads | 1024
struct Route {
  int M, D, groups, gs;  // gs: matrices per group (every group with its own 42 parameters and lambda sequence: the folds of CV mode in one launch)
  int sqrt_mode;
  CellPath cell;      // the forward cell of this kind of call (training or not); the backward cell of a training call
  bool ns_forced;     // ... by the mode or because no eigensolver exists at this size, whatever the batch
  bool wide;          // the spectral path with many workgroups per matrix (also when `cell` is the matrix iteration: Theta_0, stage 2)
  Factor factor;
  bool persistent_bwd;  // steps L-1 .. 0 of the backward pass in one launch
  bool fuse_lambda;     // the lambda step rides in the cell's second launch (LamStep); not with an exchange between norm and step
  Tridiag tridiag;
  int ns_tile;          // 32 | 64: output tile of the fp64 products
  bool ns_prefetch_all, ldl_phases;
  bool ns_any;          // a training or a forward-only call of this shape takes the matrix iteration: the workspace must hold its layout
};

// The matrix-iteration path (wide_ns.h).  Modes: -1 automatic (below), 0 only beyond the eigensolver's size, 1 for every D (tests, A/B
// measurements).
// Automatic: beyond the eigensolver's size always; and for FEW matrices of 128 < D <= 256, where one workgroup's Householder chain is
// most of the spectral cell while the iteration's products use the whole chip -- measured over a grid of (D, batch), ms per 15-step pass
// spectral vs iteration (profiles/r03_ns_crossover.txt): training D = 256: 1 matrix 16.9 vs 9.4, 6: 17.3 vs 15.4, 8: 17.5 vs 18.6; D = 192:
// 8: 12.5 vs 12.2, 16: 12.7 vs 18.1; D = 160: 8: 11.3 vs 10.0; forward only D = 256: 1: 15.5 vs 4.2, 16: 16.1 vs 9.7, 64: 17.2 vs 27.7.
// Only for UGLAD_SQRT_NS10.  training = the call saves state for a backward pass (which takes the same path: it asks with training = true).
static bool ns_cell(int ns_mode, int M, int D, bool training, int sqrt_mode) {
  if (ns_mode == 1 || D > UGLAD_MAX_EIG_DIM) return true;
  if (ns_mode != kAuto || sqrt_mode != UGLAD_SQRT_NS10 || D <= 128) return false;
  const long long tiles = (long long)M * wide_tiles(D) * wide_tiles(D);
  return training ? (tiles <= 96 && M <= 8) : tiles <= 256;
}

static Route make_route(int M, int D, int groups, bool training, int sqrt_mode) {
  Route r{};
  r.M = M, r.D = D, r.groups = groups, r.sqrt_mode = sqrt_mode;
  r.gs = M / groups > 0 ? M / groups : 1;
  const int nt = nt_of(D), ns_mode = mode_of(g_ns_mode, kSwMatrixIteration), wide_mode = mode_of(g_wide_mode, kSwWideBwd);
  const long long tiles = (long long)M * wide_tiles(D) * wide_tiles(D);
  r.ns_forced = ns_mode == 1 || D > UGLAD_MAX_EIG_DIM;
  r.ns_any = ns_cell(ns_mode, M, D, true, UGLAD_SQRT_NS10) || ns_cell(ns_mode, M, D, false, UGLAD_SQRT_NS10);
  // Few, large matrices: many workgroups per matrix (wide_bwd.h) -- the backward cell as six short launches, the forward cell's part after
  // the eigen-decomposition as one.  Taken when one workgroup per matrix would leave most of the chip idle; measured
  // (scripts/bench_bwd_wide.py): D = 256 wide wins at every batch size (82 vs 775 us at M = 1, 1.6 vs 2.1 ms at M = 512);
  // D = 160: 70 vs 216 us at M = 8, 315 vs 273 us at M = 256
  r.wide = D > 128 && (wide_mode >= 0 ? wide_mode == 1 : (D > 192 || M <= 128));
  r.cell = ns_cell(ns_mode, M, D, training, sqrt_mode) ? CellPath::kMatrixIteration : (r.wide ? CellPath::kWide : CellPath::kOneWorkgroup);
  // Theta_0 and the loss on the factorisation of ldl_wide.h (L D L^T + Newton steps) instead of the eigensolver: wherever there is none, and for
  // the few large matrices the cell itself takes to the matrix-iteration path (one 256 x 256 matrix: 0.35 ms against 0.9 ms for the eigen
  // path's tridiagonalisation, merges, back-transformation and products).  D <= 128: blocked Cholesky (chol.h); the eigen path follows only
  // for matrices the Cholesky kernel flagged (not positive definite, NaN).
  if (D > UGLAD_MAX_EIG_DIM || (D > 128 && r.ns_any)) r.factor = Factor::kLdl;
  else if (r.wide) r.factor = Factor::kWideInverse;
  else r.factor = D <= 128 && switch_on(kSwCholesky) ? Factor::kCholesky : Factor::kEigen;
  r.persistent_bwd = D <= 128 && !r.ns_forced && switch_on(kSwPersistentBwd);
  r.fuse_lambda = r.gs == 1 && r.cell == CellPath::kOneWorkgroup && !switch_on(kSwNoFusedLambda);
  // the tridiagonalisation every eigendecomposition starts with (tridiag.h).  D <= 32: one wave per matrix, no barriers (tridiag_wave.h;
  // NT = 2 measured slower); D <= 96: 16 column groups as at D = 128 (8 column groups, 64 NT threads, measured as well: slower at every
  // size, profiles/r04_tridiag_small.txt); D > 128 and few matrices: one workgroup per CU anyway, 1024 threads hide the sweep's latency
  if (nt == 1 && switch_on(kSwTridiagWave)) r.tridiag = Tridiag::kWave;
  else if (nt <= 3 && switch_on(kSwTridiagSmall)) r.tridiag = Tridiag::kSmall;
  else r.tridiag = nt > 4 && M <= 256 ? Tridiag::kBig : Tridiag::kDefault;
  // output tile of the products: 64 x 64, or 32 x 32 while the 64 x 64 tiles of the batch would not fill the 256 CUs (one 512 x 512
  // matrix: 64 workgroups; 45.8 vs 19.4 us per product, profiles/r03_ns_kernel_stats_d512_tile{64,32}.csv; the two tilings meet at 256
  // tiles of 64 x 64: D = 256 with 16 matrices 39.8 vs 39.1 ms per pass, D = 512 with 4: 66.2 vs 69.5, profiles/r03_ns_tile_probe.txt)
  const int tile = switch_value(kSwNsTile);
  r.ns_tile = tile == 32 || tile == 64 ? tile : (tiles < 256 ? 32 : 64);
  // the products' all-chunks-in-flight form (wide_ns.h, PRE): D <= 4 k chunks of the 32 x 32 tiling
  r.ns_prefetch_all = D <= 4 * NsTile<32>::kK && switch_on(kSwNsPrefetchAll);
  // L D L^T (ldl_wide.h: one schedule of phases, two kernels that walk it): ONE workgroup per matrix up to D = 256 (ns_ldl_kernel, 0.35 ms
  // there), one launch per step with the tiles of the step spread over the chip beyond (ns_ldl_phase_kernel: 5 nt launches, nt = ceil(D / 32))
  const int ldl = switch_value(kSwLdlLaunches);
  r.ldl_phases = ldl >= 0 ? ldl != 0 : nt >= 9;
  return r;
}

// what every entry point checks first.  eig_only: entry points that exist on the spectral path only; else any D up to UGLAD_MAX_DIM
static int check_dims(const Route& r, bool eig_only = false) {
  if (r.M < 1 || r.D < 1 || r.D > (eig_only ? UGLAD_MAX_EIG_DIM : UGLAD_MAX_DIM)) return UGLAD_E_DIM;
  if (r.D <= UGLAD_MAX_EIG_DIM && !((UGLAD_NT_MASK >> nt_of(r.D)) & 1)) return UGLAD_E_DIM;
  return !eig_only && r.ns_forced && r.M > kNsMaxBatch ? UGLAD_E_DIM : 0;
}
static bool valid_sqrt(int sqrt_mode) { return sqrt_mode == UGLAD_SQRT_EXACT || sqrt_mode == UGLAD_SQRT_NS10; }

// ---- workspace of the spectral path: M (d, e, tau) records | M x DP / 32 triangular factors of the back-transformation (32 x 32 each; their
// head doubles as the Cholesky kernels' per-matrix flags; the eigen kernels that run behind them pack their factors past the flags,
// tfac_behind_flags) | beyond D = 128, M x two big buffers.  The kernels' own description of it: kWsPerMatrix<DP>, big_floats<DP>() (glad_device.h).
constexpr size_t eig_hdr_floats(int DP) { return 3 * (size_t)DP + (size_t)(DP / 32) * 1024; }
constexpr size_t eig_slab_floats(int DP) { return 2 * (((size_t)DP * (DP + 1) + 3) & ~(size_t)3); }
template <int... NT>
constexpr bool eig_layout_matches_the_kernels(std::integer_sequence<int, NT...>) {
  return ((eig_hdr_floats(32 * (NT + 1)) == (size_t)kWsPerMatrix<32 * (NT + 1)> && eig_slab_floats(32 * (NT + 1)) == (size_t)big_floats<32 * (NT + 1)>()) && ...);
}
static_assert(eig_layout_matches_the_kernels(std::make_integer_sequence<int, 8>{}), "EigLayout and glad_device.h describe different workspaces");
struct EigLayout {
  int DP, LD;                  // padded size; row stride of the big buffers
  size_t rec, tfac, hdr, slab;  // floats per matrix: the record, the T factors, both (the wide backward's partial sums reuse them), the big buffers
  float* tri;    // record of matrix m: tri + m * rec
  float* T;      // T factors of matrix m: T + m * tfac
  int* flags;
  float* big0;   // first big buffer of matrix m: big0 + m * slab
  float* big1;   // second
  size_t total(int M) const { return (size_t)M * (hdr + (DP > 128 ? slab : 0)); }
};
static EigLayout eig_layout(float* workspace, int M, int D) {
  EigLayout l{};
  l.DP = padded_dim(D), l.LD = l.DP + 1;
  l.rec = 3 * (size_t)l.DP, l.hdr = eig_hdr_floats(l.DP), l.tfac = l.hdr - l.rec, l.slab = eig_slab_floats(l.DP);
  if (!workspace) return l;  // (sizes only: uglad_workspace_floats)
  l.tri = workspace;
  l.T = workspace + (size_t)M * l.rec;
  l.flags = reinterpret_cast<int*>(l.T);
  l.big0 = workspace + (size_t)M * l.hdr;
  l.big1 = l.big0 + l.slab / 2;
  return l;
}

// ---- workspace of the matrix-iteration path, per matrix: the header every path uses and, behind all headers, this matrix's region: kNsSlabs
// D x D fp64 slabs and one fp32 slab (G_half) -- or, for the factorisations beyond the eigensolver's size, the three padded fp32 slabs of the
// L D L^T inverse and one more D x D for the Newton steps' residual, whichever is larger
struct NsLayout {
  size_t hdr, region;  // floats
  size_t dslab, dregion;  // doubles: one slab, one matrix's region
  float* H;
  float* W;    // region of matrix m: W + m * region
  double* Wd;  // the same as fp64: slab s of matrix m at Wd + m * dregion + s * dslab
  float* Gh;   // the fp32 slab of matrix m: Gh + m * region
  size_t total(int M) const { return (size_t)M * (hdr + region); }
};
static NsLayout ns_layout(float* workspace, int M, int D) {
  NsLayout l;
  l.hdr = eig_hdr_floats(padded_dim(D));
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
