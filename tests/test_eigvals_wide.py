"""All eigenvalues of a wide symmetric matrix on the device (uglad_eigvalsh_wide, uglad_table_spectrum; csrc/eigvals_wide.h): blocked
Householder tridiagonalisation in fp64, then Sturm-count bisection with a fixed number of steps.  CPU: the unmodified kernel sources on the
SIMT emulator.  GPU: the same checkers on the device, with D = 288, 1100 and 2048 added.  The oracle is np.linalg.eigvalsh in fp64 on the
symmetric part of the input.

THE BOUND, fixed here before any run (EPS = 2^-53, the unit roundoff of fp64):

    |lambda_i - lambda_i_ref| <= C D^2 EPS ||A||_F,   C = 24.

Derivation.  The tridiagonal T the device reaches is exactly orthogonally similar to A + E: D - 2 reflectors applied from both sides are
2 (D - 2) Householder applications, each with a backward error of gamma~_D ||A||_F (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., Lemma 19.3; gamma~_D = c D EPS with c a small integer, at most 10 in the lemma's proof), so
||E||_F <= 2 (D - 2) 10 D EPS ||A||_F < 20 D^2 EPS ||A||_F -- the blocked (dlatrd) form applies the same reflectors, accumulated as
V W^T + W V^T, and obeys the same bound (Higham section 19.5).  By Weyl's theorem every eigenvalue moves by at most ||E||_2 <= ||E||_F.
Forming (A + A^T) / 2 costs one rounding per entry (<= EPS ||A||_F).  Bisection returns the midpoint of a bracket narrower than
2^-60 ||T|| around a point where the computed Sturm count changes, and that count is the exact count of a tridiagonal within a few ulp of
T (Demmel, Applied Numerical Linear Algebra, section 5.3.4; dstebz: 2 D EPS ||T|| + pivmin): <= 3 D EPS ||A||_F here.  The oracle itself
is LAPACK's, good to a modest multiple of D EPS ||A||_2.  20 D^2 + 1 + 3 D + (oracle) <= 24 D^2 for every D >= 1 with room for the
oracle.  The measured errors are printed before they are asserted; they sit two to five orders of magnitude below the bound
(profiles/table_probe.txt records them for the large shapes).  The trace: |sum lambda - tr A| <= D times that bound.

Matrices of the shape grid: sample covariances (np.cov, bias=1) of random((N, D)) tables with N = 2 D and with N = D / 2; the second kind
is singular, with D - N + 1 eigenvalues at rounding level and of either sign.  The tile and panel edge is 64: the grid crosses it and
ends in a ragged last panel; D = 1100 crosses the 1024 boundary of the Cholesky layer's slab layouts, D = 2048 is the largest."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

EPS = 2.0 ** -53
C_BOUND = 24.0


def bound(A):
    """C D^2 EPS ||sym(A)||_F per matrix of a (K, D, D) batch."""
    S = 0.5 * (A + np.swapaxes(A, -1, -2))
    return C_BOUND * A.shape[-1] ** 2 * EPS * np.sqrt((S * S).sum(axis=(-1, -2)))


def oracle(A):
    return np.stack([np.linalg.eigvalsh(0.5 * (a + a.T)) for a in A])


def run(A, th=0.0):
    """(eig (K, D), summary (K, 6)) as numpy, from whatever library is installed (the emulator's on the CPU, the device's on the GPU)."""
    from uglad_amd.utils import prepare_data

    eig, summary = prepare_data.eigvalsh_device(np.array(A), th=th, return_summary=True)
    assert eig.dtype == np.float64 and summary.dtype == np.float64 and eig.shape == A.shape[:-1] and summary.shape == (len(A), 6)
    return eig, summary


def check_summary(eig, summary, th):
    """The summary is what numpy computes from the device's OWN eigenvalues, exactly."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = np.abs(eig)
        want = np.stack([eig.min(1), eig.max(1), a.min(1), a.max(1), a.max(1) / a.min(1), (eig < th).sum(1).astype(np.float64)], axis=1)
    assert np.array_equal(summary, want, equal_nan=True), (summary, want)


def check(A, label, th=None):
    """Eigenvalues of a (K, D, D) batch against the oracle; every figure printed before it is asserted.  th: where to count (default: the
    middle of the widest gap of slab 0's spectrum, where the count must equal the oracle's)."""
    K, D, _ = A.shape
    ref, b = oracle(A), bound(A)
    in_gap = th is None
    if in_gap:
        gaps = np.diff(ref[0]) if D > 1 else np.array([1.0])
        g = int(np.argmax(gaps))
        th = float(ref[0][g] + 0.5 * gaps[g]) if D > 1 else float(ref[0][0] - 1.0)
    eig, summary = run(A, th)
    err = np.abs(eig - ref).max(axis=1)
    tr = np.abs(eig.sum(1) - np.trace(A, axis1=1, axis2=2))
    for k in range(K):
        print(f"{label}[{k}] D {D}: max |dlambda| {err[k]:.2e} (bound {b[k]:.2e}), |sum - trace| {tr[k]:.2e} (bound {D * b[k]:.2e})")
    assert (np.diff(eig, axis=1) >= 0).all(), "ascending"
    assert (err <= b).all(), (err, b)
    assert (tr <= D * b).all(), (tr, D * b)
    check_summary(eig, summary, th)
    if in_gap and D > 1 and gaps[g] > 4 * b[0]:
        assert summary[0, 5] == (ref[0] < th).sum()
    return eig, summary


@functools.lru_cache(maxsize=None)
def covariances(K, D, N, seed):
    A = np.stack([np.cov(t.T, bias=1).reshape(D, D) for t in np.random.default_rng(seed).random((K, N, D))])
    A.setflags(write=False)
    return A


# ============================================================================================ 1. the shape grid
GRID_D = [1, 2, 3, 25, 63, 64, 65, 130]


def check_grid(D, Ks=(1, 3)):
    for N in (2 * D, max(D // 2, 1)):
        A = covariances(3, D, N, seed=10 * D + N)
        whole = None
        for K in Ks:
            got = check(A[:K], f"cov n{N} K{K}")
            if whole is not None:  # K = 3 after K = 1: slab 0 has the bits of the single call
                assert np.array_equal(got[0][0], whole[0][0], equal_nan=True) and np.array_equal(got[1][0], whole[1][0], equal_nan=True)
            whole = got


@pytest.mark.parametrize("D", GRID_D)
def test_emulated_shape_grid(emul, D):
    check_grid(D)


@pytest.mark.gpu
@pytest.mark.parametrize("D", GRID_D + [288, 1100])
def test_gpu_shape_grid(D):
    check_grid(D)


@pytest.mark.gpu
def test_gpu_largest_dimension():
    """D = 2048, K = 1, N = 2 D: 32 panels, 32 strips, the largest slab (32 MiB)."""
    check(covariances(1, 2048, 4096, seed=2048), "cov d2048")


# ============================================================================================ 2. special matrices
def special_matrices(D, seed=5):
    rng = np.random.default_rng(seed + D)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    u = rng.standard_normal(D)
    u /= np.linalg.norm(u)
    B = rng.standard_normal((D, D))
    sym = np.cov(rng.random((2 * D, D)).T, bias=1)
    off = rng.standard_normal(D - 1)
    return {
        "diagonal": np.diag(rng.standard_normal(D)),
        "tridiagonal": np.diag(rng.standard_normal(D)) + np.diag(off, 1) + np.diag(off, -1),
        "identity": np.eye(D),
        "I + 5 u u^T": np.eye(D) + 5.0 * np.outer(u, u),
        "zero": np.zeros((D, D)),
        "graded": (Q * np.geomspace(1e-12, 1.0, D)) @ Q.T,
        "asymmetric 1e-5": sym + 1e-5 * (B - B.T),
    }


def check_special(D):
    for name, A in special_matrices(D).items():
        eig, _ = check(A[None], name)
        if name in ("identity", "zero"):
            assert np.array_equal(eig[0], np.full(D, 1.0 if name == "identity" else 0.0))


@pytest.mark.parametrize("D", [65, 130])
def test_emulated_special_matrices(emul, D):
    check_special(D)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [65, 130])
def test_gpu_special_matrices(D):
    check_special(D)


# ============================================================================================ 3. the bitwise properties
def check_bitwise(D=65):
    A = covariances(3, D, 2 * D, seed=77)
    whole = run(A, 0.01)
    again = run(A, 0.01)
    for a, b in zip(whole, again):
        assert np.array_equal(a, b)
    for k in range(3):
        solo = run(A[k:k + 1], 0.01)
        assert np.array_equal(solo[0][0], whole[0][k]) and np.array_equal(solo[1][0], whole[1][k])


def test_emulated_bitwise_properties(emul):
    check_bitwise()


@pytest.mark.gpu
def test_gpu_bitwise_properties():
    check_bitwise()
    check_bitwise(D=288)


# ============================================================================================ 4. a NaN in one slab
def check_nonfinite(D=70):
    A = np.array(covariances(3, D, 2 * D, seed=78))
    clean = run(A, 0.01)
    for poison in (np.nan, np.inf):
        B = A.copy()
        B[1, D // 3, D - 2] = poison  # one entry, off the diagonal, one triangle only
        eig, summary = run(B, 0.01)  # (returns: no loop of the solver depends on the data)
        assert np.isnan(eig[1]).all() and np.isnan(summary[1, :5]).all() and summary[1, 5] == 0
        for k in (0, 2):
            assert np.array_equal(eig[k], clean[0][k]) and np.array_equal(summary[k], clean[1][k])


def test_emulated_nan_stays_in_its_slab(emul):
    check_nonfinite()


@pytest.mark.gpu
def test_gpu_nan_stays_in_its_slab():
    check_nonfinite()


# ============================================================================================ 5. the table entry
def check_table_spectrum(lib, device, K=2, N=50, D=70):
    """uglad_table_spectrum: the covariance it forms is numpy's to rounding, and its eigenvalues are those of that covariance."""
    X = np.random.default_rng(3).random((K, N, D))
    Xd = torch.from_numpy(X).to(device)
    eig, summary, cov = lib.table_spectrum(Xd, th=0.01, want_cov=True)
    eig2, summary2, none = lib.table_spectrum(Xd, th=0.01)
    assert none is None and torch.equal(eig, eig2) and torch.equal(summary, summary2)
    cov, eig, summary = cov.cpu().numpy(), eig.cpu().numpy(), summary.cpu().numpy()
    S = np.stack([np.cov(x.T, bias=1) for x in X])
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    e_cov = np.abs(cov - S).max()
    ref, b = oracle(cov), bound(cov)
    err = np.abs(eig - ref).max(axis=1)
    b_cov = 8 * (N + 2) * EPS
    print(f"table N {N} D {D}: covariance {e_cov:.2e} (bound {b_cov:.2e}), max |dlambda| {err.max():.2e} (bound {b.min():.2e})")
    # entries in [0, 1]: the mean (N EPS), so every centred term (N + 1) EPS twice, and the dot product of N terms of magnitude <= 1 over N
    # ((N + 2) EPS): below 4 (N + 2) EPS on either side
    assert e_cov <= b_cov
    assert (err <= b).all()
    check_summary(eig, summary, 0.01)
    eig3, _ = lib.eigvalsh_wide(torch.from_numpy(cov).to(device), th=0.01)
    assert np.array_equal(eig3.cpu().numpy(), eig)  # the same slab, the same bits


def test_emulated_table_spectrum(emul):
    check_table_spectrum(emul, "cpu")


@pytest.mark.gpu
def test_gpu_table_spectrum():
    from uglad_amd import _lib

    check_table_spectrum(_lib.get_lib(), "cuda")
    check_table_spectrum(_lib.get_lib(), "cuda", K=1, N=150, D=300)


# ============================================================================================ 6. the C entry
def check_c_entry(lib, device):
    from uglad_amd._lib import UgladError

    size = lib._dll.uglad_eigvalsh_wide_workspace_floats
    assert size(0, 8) == -2 and size(65536, 8) == -2 and size(1, 0) == -2 and size(1, lib.max_dim + 1) == -2 and size(1, -1) == -2
    assert lib.max_dim == 2048 and size(1, 2049) == -2
    for K in (1, 2, 5):
        sizes = [size(K, D) for D in (1, 2, 63, 64, 65, 128, 129, 1024, 1025, 2048)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and size(K + 1, 64) > size(K, 64)  # monotone in D and in K
    assert size(1, 64) == size(1, 1) and size(1, 65) > size(1, 64)  # whole tiles
    assert size(100, 2048) > 0 and size(200, 2048) == -2  # beyond 2^31 - 1 floats

    K, D = 2, 8
    A = torch.eye(D, dtype=torch.float64, device=device).repeat(K, 1, 1) * 3.0
    X = torch.zeros(K, 5, D, dtype=torch.float64, device=device)
    eig = torch.zeros(K, D, dtype=torch.float64, device=device)
    summary = torch.zeros(K, 6, dtype=torch.float64, device=device)
    wsp = torch.empty(size(K, D) + 2, dtype=torch.float32, device=device)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    odd = ctypes.c_void_p(wsp.data_ptr() + (4 if wsp.data_ptr() % 8 == 0 else 8))
    assert odd.value % 8 == 4

    def call(A_=A, eig_=eig, summary_=summary, w=lib._p(wsp), K_=K, D_=D):
        lib._call("uglad_eigvalsh_wide", vp(A_), K_, D_, 1.0, vp(eig_), vp(summary_), w)

    def call_table(X_=X, eig_=eig, summary_=summary, cov_=None, w=lib._p(wsp), K_=K, N_=5, D_=D):
        lib._call("uglad_table_spectrum", vp(X_), K_, N_, D_, 1.0, vp(eig_), vp(summary_), vp(cov_), w)

    for fn, first in ((call, "A_"), (call_table, "X_")):
        for kw in ({first: None}, dict(eig_=None), dict(summary_=None), dict(w=None), dict(w=odd)):
            with pytest.raises(UgladError, match="NULL"):
                fn(**kw)
        for kw in (dict(D_=0), dict(D_=2049), dict(K_=0), dict(D_=-3)):
            with pytest.raises(UgladError, match="dimension"):
                fn(**kw)
    with pytest.raises(UgladError, match="dimension"):
        call_table(N_=0)
    call()
    if device != "cpu":
        torch.cuda.synchronize()
    assert torch.equal(eig, torch.full((K, D), 3.0, dtype=torch.float64, device=device))
    assert torch.equal(summary, torch.tensor([[3.0, 3.0, 3.0, 3.0, 1.0, 0.0]] * K, dtype=torch.float64, device=device))
    call_table()  # a constant table: the zero covariance
    if device != "cpu":
        torch.cuda.synchronize()
    assert torch.equal(eig, torch.zeros(K, D, dtype=torch.float64, device=device))
    with pytest.raises(UgladError):  # fp32 belongs elsewhere
        lib.eigvalsh_wide(A.float())
    with pytest.raises(UgladError):
        lib.eigvalsh_wide(A[:, :, :4].contiguous())


def test_emulated_c_entry_error_codes_and_workspace_sizes(emul):
    check_c_entry(emul, "cpu")


@pytest.mark.gpu
def test_gpu_c_entry_error_codes_and_workspace_sizes():
    from uglad_amd import _lib

    check_c_entry(_lib.get_lib(), "cuda")


# ============================================================================================ 7. the Python surface
def check_python_surface(device):
    from uglad_amd.utils import prepare_data

    A = np.array(covariances(2, 25, 50, seed=9))
    ref = oracle(A)
    one = prepare_data.eigvalsh_device(A[0])
    assert isinstance(one, np.ndarray) and one.shape == (25,) and (np.abs(one - ref[0]) <= bound(A)[0]).all()
    t = prepare_data.eigvalsh_device(torch.from_numpy(A).to(device))
    assert torch.is_tensor(t) and t.shape == (2, 25) and np.array_equal(t[0].cpu().numpy(), one)
    with pytest.raises(ValueError):
        prepare_data.eigvalsh_device(np.zeros((3, 4)))
    X = np.random.default_rng(4).random((40, 12))
    S_h, eig_h, con_h = prepare_data.analyse_condition_number(X, "", VERBOSE=False)
    S_d, eig_d, con_d = prepare_data.analyse_condition_number(X, "", VERBOSE=False, device=True)
    assert isinstance(eig_d, list) and eig_d == sorted(eig_d) and isinstance(con_d, float)
    b = bound(S_h[None])[0]
    assert np.abs(S_d - S_h).max() <= 8 * 42 * EPS and np.abs(np.array(eig_d) - np.sort(eig_h)).max() <= b
    assert abs(con_d - con_h) <= con_h * 4 * b / min(eig_h)  # both ends of the quotient within b on either side


def test_emulated_python_surface(emul, capsys):
    check_python_surface("cpu")
    assert capsys.readouterr().out == ""  # VERBOSE=False prints nothing on either path


@pytest.mark.gpu
def test_gpu_python_surface():
    check_python_surface("cuda")
