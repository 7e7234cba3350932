"""The L D L^T inverse beyond the eigensolver (csrc/ldl_wide.h) in its two kernel forms: shapes, inputs and checks shared by the GPU test
(test_ldl_forms.py), its CPU twin on the emulator (test_ldl_forms_emulated.py) and the generator of the golden (golden/make_ldl_goldens.py).
`lib` is the HipLib under test, `dev` where its tensors live.

A CASE is (entry point, M, D, input):
  "init": lib.init_theta of synthetic_covariance_batch(M, D, 4 D, seed=D) with golden/params_trained.npz -> Theta_0 = (S + t I)^-1
  "loss": lib.loss_fwd of Q diag(w) Q^T, w = linspace(0.5, 5, D), S = I -> the loss (-logdet + trace) and the inverse; the inputs
          "spd"    as it stands
          "neg2"   two negative eigenvalues: finite logdet, finite inverse
          "neg3"   three: NaN loss (torch.logdet of a negative determinant), finite inverse
          "pivot0" A[0, 0] = 0: the first pivot is zero, NaN everywhere (the not-ok path)
A FORM is the value of UGLAD_LDL_LAUNCHES: "0" one workgroup per matrix (ns_ldl_kernel), "1" one launch per phase (ns_ldl_phase_kernel), None unset
(host_route.h decides: launches from nt = ceil(D / 32) = 9).

The second half of the file is what test_ldl_hard.py and scripts/ldl_probe.py --hard share: hard_matrix (ill-conditioned, indefinite, scaled, graded
and shifted inputs from a seed), run_on (one call on any input) and reference64 (the fp64 reference and the two error bounds, from the input alone)."""
import os
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCH = "UGLAD_LDL_LAUNCHES"
LOSS_INPUTS = ("spd", "neg2", "neg3", "pivot0")
# (entry, M, D, input) -- why this shape
GPU_CASES = [
    ("init", 1, 129, None),    # nt = 5, ragged last tile, first size on this path
    ("init", 3, 150, None),    # a batch: slab stride, blockIdx -> matrix
    ("init", 1, 160, None),    # D = padded size exactly
    ("init", 1, 256, None),    # config 5's own route (default: one workgroup)
    ("init", 1, 288, None),    # first size past the crossover (default: launches)
    ("init", 1, 577, None),    # nt = 19 > 16 waves: the one-workgroup walk wraps its tile loops; dp^2 > 512 * 256: the capped element grids wrap
    ("init", 1, 1025, None),   # the 2048 x 2049 layout (FD = 2048), nt = 33
] + [("loss", 1, 200, k) for k in LOSS_INPUTS]  # sign count, logdet rules, the not-ok path
DEFAULT_TOO = (256, 288)  # the sizes on either side of the crossover also run with the switch unset
# the emulator build's eigensolver ends at D = 160 and every work-item is a fiber: 161 and 170 stand in for 129 .. 160, 1025 is GPU-only
EMUL_CASES = [("init", 1, 161, None), ("init", 2, 170, None)] + [("loss", 1, 200, k) for k in LOSS_INPUTS] + [("init", 1, 577, None)]
FULL_UP_TO = 160  # the golden keeps the outputs themselves up to this D, a CRC32 per matrix beyond


def case_id(case):
    entry, M, D, kind = case
    return f"{entry}_M{M}_D{D}" + (f"_{kind}" if kind else "")


def forms(case):
    return ("0", "1") + ((None,) if case[2] in DEFAULT_TOO else ())


def form_id(form):
    return {"0": "one_workgroup", "1": "launches", None: "default"}[form]


def expected_launches(case, form):
    """(kernel instantiation, number of its launches) host_launch.h sends this case to.  The schedule of nt block columns has 5 nt steps:
    Init, nt Diag, nt - 1 Panel and Trail each, nt - 1 WSum and WMul each, Scale, X, Finish."""
    D = case[2]
    nt, fd = (D + 31) // 32, 1024 if D <= 1024 else 2048
    launches = form == "1" if form is not None else nt >= 9
    return (f"uglad::ns_ldl_phase_kernel<{fd}>", 5 * nt) if launches else (f"uglad::ns_ldl_kernel<{fd}>", 1)


_cache = {}


def packed_params():
    """((42,) float32 tensor the kernels read, t = theta_init_offset) of golden/params_trained.npz."""
    if "params" not in _cache:
        import uglad_amd

        pz = np.load(os.path.join(HERE, "golden", "params_trained.npz"))
        m = uglad_amd.GladParams(1.0)
        m.load_state_dict({k: torch.from_numpy(np.array(pz[k])) for k in pz.files})
        _cache["params"] = (m.packed().detach().contiguous(), float(m.state_dict()["theta_init_offset"].item()))
    return _cache["params"]


def matrices(case):
    """(M, D, D) float32: what the entry point is given.  Computed once per case and left unchanged."""
    if case not in _cache:
        entry, M, D, kind = case
        if entry == "init":
            from uglad_amd.utils.prepare_data import synthetic_covariance_batch

            a = synthetic_covariance_batch(M, D, 4 * D, seed=D)
        else:
            Q, _ = np.linalg.qr(np.random.default_rng(1).standard_normal((D, D)))
            w = np.linspace(0.5, 5.0, D)
            negatives = {"neg2": 2, "neg3": 3}.get(kind, 0)
            w[:negatives] = [-1.0, -3.0, -0.7][:negatives]
            a = ((Q * w) @ Q.T)[None]
            if kind == "pivot0":
                a[0, 0, 0] = 0.0
        _cache[case] = np.ascontiguousarray(a, dtype=np.float32)
        _cache[case].setflags(write=False)
    return _cache[case]


def factored(case):
    """(M, D, D) float64: the matrices the kernels invert, from the fp32 inputs."""
    A = matrices(case).astype(np.float64)
    return A + packed_params()[1] * np.eye(case[2]) if case[0] == "init" else A


def run(lib, dev, case, form):
    """(X (M, D, D), loss (M,) or None) of one call under one form, as numpy float32."""
    return run_on(lib, dev, case[0], matrices(case), form, s_identity=True)


def run_on(lib, dev, entry, A, form, s_identity=False):
    """The same for any (M, D, D) float32 input.  "loss" with S = 0 unless s_identity, so that the loss IS -logdet (its trace term is an exact 0)."""
    M, D, _ = A.shape
    saved = os.environ.pop(SWITCH, None)  # (the host layer reads its switches on every call)
    if form is not None:
        os.environ[SWITCH] = form
    try:
        A = torch.from_numpy(np.array(A, dtype=np.float32)).to(dev)
        X = torch.zeros_like(A)
        wsp = lib.workspace(M, D, A)
        loss = None
        if entry == "init":
            lib.init_theta(A, packed_params()[0].to(dev), 0, X, wsp)
        else:
            loss = torch.zeros(M, dtype=torch.float32, device=dev)
            S = torch.eye(D, dtype=torch.float32, device=dev) if s_identity else torch.zeros(D, D, dtype=torch.float32, device=dev)
            lib.loss_fwd(A, S[None].contiguous(), None, loss, X, wsp)
        if dev != "cpu":
            torch.cuda.synchronize()
        return X.cpu().numpy().copy(), None if loss is None else loss.cpu().numpy().copy()
    finally:
        os.environ.pop(SWITCH, None)
        if saved is not None:
            os.environ[SWITCH] = saved


def crc_per_matrix(X):
    return np.array([zlib.crc32(np.ascontiguousarray(x).tobytes()) for x in X], dtype=np.uint32)


def same_bits(a, b):
    """Equal bits where finite, NaN in the same places (NaN payloads are not compared)."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.where(na, np.float32(0), a).tobytes() == np.where(nb, np.float32(0), b).tobytes()


def canonical(X):
    """X with every NaN replaced by the one quiet NaN, so that a CRC32 compares bits where finite and NaN-ness elsewhere."""
    X = np.array(X, dtype=np.float32)
    X[np.isnan(X)] = np.float32(np.nan)
    return X


def logdet_of(case, loss):
    """The device's log-determinant out of its loss: loss = -logdet + trace(A S), S = I (the trace in fp64 from the fp32 input)."""
    return np.trace(factored(case), axis1=1, axis2=2) - loss.astype(np.float64)


def slogdet(case):
    """fp64 log|det|, NaN for a negative determinant (torch.logdet's rule)."""
    sign, val = np.linalg.slogdet(factored(case))
    return np.where(sign > 0, val, np.nan)


def forward_errors(case, X, loss):
    """Per matrix (||X - X64||_F / ||X64||_F, |logdet - slogdet|) against numpy fp64; NaN where the device or the reference has none."""
    A = factored(case)
    with np.errstate(all="ignore"):
        ref = np.linalg.inv(A)
        ex = np.array([np.linalg.norm(x.astype(np.float64) - r) / np.linalg.norm(r) for x, r in zip(X, ref)])
        el = np.abs(logdet_of(case, loss) - slogdet(case)) if loss is not None else np.full(len(X), np.nan)
    return np.stack([ex, el], axis=1)


def backward_errors(case, X, loss):
    """Per matrix (||A X - I||_F / sqrt(D), |logdet - slogdet|) in fp64; NaN where not finite."""
    A, D = factored(case), case[2]
    with np.errstate(all="ignore"):
        rx = np.array([np.linalg.norm(a @ x.astype(np.float64) - np.eye(D)) / np.sqrt(D) for a, x in zip(A, X)])
        rl = np.abs(logdet_of(case, loss) - slogdet(case)) if loss is not None else np.full(len(X), np.nan)
    return np.stack([rx, rl], axis=1)


def within_twice(got, parent):
    """got <= 2 parent wherever the parent is finite; NaN exactly where the parent has NaN."""
    got, parent = np.asarray(got, dtype=np.float64), np.asarray(parent, dtype=np.float64)
    nan = np.isnan(parent)
    return np.array_equal(np.isnan(got), nan) and bool(np.all(got[~nan] <= 2 * parent[~nan]))


# ---------------------------------------------------------------------------------------------------------------------
# Hard matrices (test_ldl_hard.py, scripts/ldl_probe.py --hard): inputs from a seed, references and bounds in numpy fp64 from the input alone.
U32 = 2.0 ** -24  # unit roundoff of fp32
# "loss" kinds -> lib.loss_fwd with S = 0; Q diag(w) Q^T with a random orthogonal Q unless said otherwise
SPD_KINDS = ("spd_1e2", "spd_1e3", "spd_1e4", "spd_1e5")               # w = logspace(0, -k)
FLIP_KINDS = ("flip2_1e2", "flip40_1e2", "flip80_1e3", "flip40_1e4")   # ... with that many random signs flipped
SCALED_KINDS = ("scaled_down", "scaled_up")                           # w = linspace(.5, 5) * 1e-3 | * 1e3
A00_KINDS = ("a00_1e-2", "a00_1e-4", "a00_1e-6")                       # w = linspace(.5, 5), w[:3] = (-1, -3, .5), then A[0, 0] := that: a tiny first pivot
SHIFTED_KINDS = ("shifted", "shifted_pos")                             # "init" kinds -> lib.init_theta with the trained t < 0 (see hard_matrix)
FAMILIES = SPD_KINDS + FLIP_KINDS + SCALED_KINDS + A00_KINDS + ("graded",) + SHIFTED_KINDS  # every finite kind of the error table
NOT_FINITE_KINDS = ("neg3", "pivot0")                                  # NaN loss, finite inverse | NaN throughout
# where bound 2 must itself be small to say anything (test_ldl_hard.py asserts it is below LOGDET_CAP there); the rest have element growth
LOGDET_CAPPED = SPD_KINDS + SCALED_KINDS + ("graded", "flip2_1e2", "a00_1e-2", "a00_1e-4", "shifted_pos")
LOGDET_CAP = 0.1
SPD_SHORTCUT_BEYOND = 577  # beyond this D the bounds of an spd input take sqrt(a_ii a_jj) for (|L| |d| |L|^T)_ij: no Python factorisation


def logdet_capped(kind, D):
    """Whether bound 2 must be below LOGDET_CAP for this input.  The bound grows like D cond(A): at cond 1e5 it is 6.8e-2 at D = 129, 9.2e-2 at
    161 and 5.6e-1 at 577 whatever the device does, so that one kind is capped up to 161 only (beyond, the inequality alone is asserted)."""
    return kind in LOGDET_CAPPED and (kind != "spd_1e5" or D <= 161)
SIGN_AT = (5, 40, 70, 100, 128)  # test 7: rows of the negative pivots, one per 32-block 0 .. 4
BATCH_KINDS = (("spd_1e2", 0), ("pivot0", 0), ("flip40_1e2", 0), ("neg3", 0), ("spd_1e2", 1))  # test 6: (kind, seed offset) of the M = 5 call


def entry_of(kind):
    return "init" if kind in SHIFTED_KINDS else "loss"


def _orthogonal(D, seed):
    key = ("Q", D, seed)
    if key not in _cache:
        _cache[key] = np.linalg.qr(np.random.default_rng(seed).standard_normal((D, D)))[0]
    return _cache[key]


def hard_matrix(kind, D, seed):
    """(D, D) float32, read-only, computed once: the input of kind `kind` (the tuples above; "sign<k>": test 7's matrix with k negative pivots)."""
    key = ("hard", kind, D, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng([seed, D, zlib.crc32(kind.encode())])
    lin = np.linspace(0.5, 5.0, D)
    if kind.startswith("sign"):
        # exactly T diag(w) T^T with T unit lower triangular and well conditioned: the unpivoted pivots ARE w, the negative ones at SIGN_AT
        w = rng.permutation(lin)
        w[list(SIGN_AT[:int(kind[4:])])] *= -1.0
        T = np.eye(D) + np.tril(rng.standard_normal((D, D)), -1) * (0.3 / np.sqrt(D))
        a = (T * w) @ T.T
    else:
        Q = _orthogonal(D, seed)
        if kind in SPD_KINDS + FLIP_KINDS:
            flips, cond = kind.split("_")
            w = np.logspace(0.0, -float(cond[2:]), D)
            if flips != "spd":
                w[rng.choice(D, int(flips[4:]), replace=False)] *= -1.0
        elif kind in SCALED_KINDS:
            w = lin * (1e-3 if kind == "scaled_down" else 1e3)
        elif kind in A00_KINDS or kind in NOT_FINITE_KINDS:
            w = lin.copy()
            w[:3] = (-1.0, -3.0, -0.7) if kind == "neg3" else (-1.0, -3.0, 0.5) if kind in A00_KINDS else w[:3]
        elif kind == "graded":
            w = lin
        elif kind in SHIFTED_KINDS:
            # a covariance whose smallest eigenvalues (1e-4: a repair offset) lie below |t| = 7.35e-4: S + t I is indefinite with ten tiny negative
            # eigenvalues; "_pos": every eigenvalue of S >= 1e-2, S + t I positive
            w = np.logspace(0.0, -3.0 if kind == "shifted" else -2.0, D)
            if kind == "shifted":
                w[-10:] = 1e-4
        else:
            raise ValueError(kind)
        a = (Q * w) @ Q.T
        if kind in A00_KINDS:
            # lowering A[0, 0] is a negative rank-one change: it adds a third negative eigenvalue, det < 0 and no log-determinant to compare,
            # wherever (A^-1)_00 > 1 / (A_00 - that).  Then w[1] = +3: one negative eigenvalue before, two after
            a[0, 0] = float(kind[4:])
            if np.linalg.slogdet(a)[0] < 0:
                w[1] = 3.0
                a = (Q * w) @ Q.T
                a[0, 0] = float(kind[4:])
        elif kind == "pivot0":
            a[0, 0] = 0.0
        elif kind == "graded":
            s = rng.permutation(np.logspace(-1.5, 1.5, D))
            a = a * np.outer(s, s)
    a = np.ascontiguousarray((a + a.T) / 2, dtype=np.float32)
    a.setflags(write=False)
    _cache[key] = a
    return a


def inverted(kind, a32):
    """(D, D) float64: the matrix the device inverts, from the fp32 input (plus the fp32 t on the diagonal for an "init" kind, as factored())."""
    A = np.asarray(a32, dtype=np.float64)
    return A + packed_params()[1] * np.eye(len(A)) if entry_of(kind) == "init" else A


def shifted32(a32):
    """(D, D) float32: a32 + t on the diagonal in fp32, what kLdlInit forms -- through "loss" it gives the log-determinant "init" does not return."""
    a = np.array(a32, dtype=np.float32)
    a[np.diag_indices(len(a))] += np.float32(packed_params()[1])
    return a


def ldl64(A, nb=64):
    """(L, d) of the unpivoted A = L diag(d) L^T in fp64: rank-1 updates inside a panel of nb columns, one product per panel behind it."""
    A = np.array(A, dtype=np.float64)
    n = len(A)
    L, d = np.eye(n), np.empty(n)
    with np.errstate(all="ignore"):
        for j in range(0, n, nb):
            e = min(j + nb, n)
            for k in range(j, e):
                d[k] = A[k, k]
                L[k + 1:, k] = A[k + 1:, k] / d[k]
                A[k + 1:, k + 1:e] -= np.outer(L[k + 1:, k], A[k, k + 1:e])
            A[e:, e:] -= (L[e:, j:e] * d[j:e]) @ L[e:, j:e].T
    return L, d


def pivots64(A, spd=False):
    """d alone; spd: from Cholesky, no Python loop."""
    return np.diag(np.linalg.cholesky(A)) ** 2 if spd else ldl64(A)[1]


def sum_term(d):
    """u sqrt(D) max_k |sum_{i<=k} ln |d_i||: what the fp32 running sum of the log-pivots can lose."""
    return float(U32 * np.sqrt(len(d)) * np.abs(np.cumsum(np.log(np.abs(d)))).max())


def reference64(A, spd=False):
    """Everything the bounds need, in fp64 from A alone: X = A^-1, d = the unpivoted pivots, G >= |L| |d| |L|^T (spd: sqrt(a_ii a_jj), which bounds
    it, and d from Cholesky: no Python loop), growth = max G / max |A|, logdet = log|det A| or NaN for det < 0, and the two bounds at c = 1:
      inv_unit  u || |X| |A| |X| ||_F / ||X||_F       first-order error of one fp32 evaluation of X + X (I - A X) at the fixed point
      sum_term  u sqrt(D) max_k |sum_{i<=k} ln |d_i||  the fp32 running sum of the log-pivots
      ld_bound  u sum_ij |X|_ij G_ij + sum_term + ulp32(logdet) / 2: tr(A^-1 dA) under an unpivoted factorisation's backward error |dA| <= u G."""
    D = len(A)
    X = np.linalg.inv(A)
    if spd:
        d = pivots64(A, spd=True)
        G = np.sqrt(np.outer(np.diag(A), np.diag(A)))
    else:
        L, d = ldl64(A)
        G = (np.abs(L) * np.abs(d)) @ np.abs(L).T
    aX = np.abs(X)
    sign, logdet = np.linalg.slogdet(A)
    logdet = logdet if sign > 0 else np.nan
    half_ulp = 0.5 * float(np.spacing(np.float32(abs(logdet)))) if np.isfinite(logdet) else 0.0
    return {"X": X, "d": d, "growth": G.max() / np.abs(A).max(), "logdet": logdet, "sum_term": sum_term(d),
            "inv_unit": U32 * np.linalg.norm(aX @ np.abs(A) @ aX) / np.linalg.norm(X), "ld_bound": U32 * np.sum(aX * G) + sum_term(d) + half_ulp}


def hard_reference(kind, D, seed):
    """reference64 of the matrix the device inverts for hard_matrix(kind, D, seed); once per input, shared and left unchanged."""
    key = ("ref", kind, D, seed)
    if key not in _cache:
        _cache[key] = reference64(inverted(kind, hard_matrix(kind, D, seed)), spd=D > SPD_SHORTCUT_BEYOND and kind in SPD_KINDS + SCALED_KINDS)
    return _cache[key]


def inverse_error(X, ref):
    """||X - X64||_F / ||X64||_F"""
    return float(np.linalg.norm(np.asarray(X, dtype=np.float64) - ref["X"]) / np.linalg.norm(ref["X"]))


def residual(A, X):
    """||A X - I||_F / sqrt(D) in fp64"""
    return float(np.linalg.norm(A @ np.asarray(X, dtype=np.float64) - np.eye(len(A))) / np.sqrt(len(A)))


def torch32(A):
    """(inverse, log-determinant) of the reference's own arithmetic: torch.linalg.inv and torch.logdet on the CPU in fp32 on the fp32 rounding of A."""
    a = torch.from_numpy(np.asarray(A, dtype=np.float32).copy())
    return torch.linalg.inv(a).numpy(), float(torch.logdet(a))
