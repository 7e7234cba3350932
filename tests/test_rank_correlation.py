"""The rank-based correlation matrices of the nonparanormal front-end (uglad_rank_correlation, csrc/rank_wide.h; the host layer in
uglad_amd/utils/prepare_data.py), against goldens made with scipy (tests/golden/make_rank_goldens.py: kendalltau per pair, spearmanr, the
correlation of norm.ppf(rankdata / (N + 1)), eigvalsh and the repair) and against the package's host formulation.  CPU: the host
formulation, and the unmodified kernel sources on the SIMT emulator.  GPU: the same shapes, every golden, a launch of many pair chunks,
flagged columns in a batch, fit_copula.

Tolerances, none of them measured on the code under test:
  integer Grams   exact equality (Kendall's s^T s, Spearman's sum of c c: exact integers in fp64 on both sides).
  rho, tau        |device - oracle| <= 2^-50 before the transform: two square roots, a product and a division of exact integers, each
                  correctly rounded, on values <= 1 (under 2 ulp of 1), with margin.
  after the sine  <= 2^-48: pi / 2 times that, plus the two sines' own few ulp.
  goldens         the same bounds plus the d_ref of that case and method in tests/golden/rank_deviation.json, d_ref = the deviation of
                  the host formulation from scipy as the generator measured it.
  scores          SCORE_BOUND = 256 x the largest scores d_ref of rank_deviation.json (the multiple test_association.py gives the
                  reference's own rounding); it must stay below 1e-12.  Their Gram matrix (centred sums, not / N): the same relative
                  bound at the scale of the sums, |device - oracle| <= SCORE_BOUND x the largest diagonal entry.
  min eig         |device - golden| <= ||A||_inf 2^-40 (the bisection's bracket ends at ||A||_inf 2^-48).
  fp32            every entry of the fp32 output within one fp32 ulp of the float32 rounding of the golden's repaired matrix."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from uglad_amd.utils import prepare_data as pd_

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ["n37_d7", "n130_d70", "n257_d129", "n300_d288"]
METHODS = list(pd_.RANK_METHODS)
with open(os.path.join(GOLDEN, "rank_deviation.json")) as _f:
    DEVIATION = json.load(_f)
RHO_BOUND = 2.0 ** -50
SIN_BOUND = 2.0 ** -48
SCORE_BOUND = 256 * max(v["scores"]["d_ref"] for v in DEVIATION.values())

_cache = {}


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def golden_table(name):
    if name not in _cache:
        g = np.load(os.path.join(GOLDEN, f"rank_{name}.npz"))
        _cache[name] = frozen(g["table"].astype(np.float64), float(g["offset"]))
    return _cache[name]


def golden(name, method):
    """(table fp64, untransformed coefficient, transformed matrix, min eig, offset, repaired) of a golden, loaded once, never modified."""
    if (name, method) not in _cache:
        X, offset = golden_table(name)
        g = np.load(os.path.join(GOLDEN, f"rank_{name}_{method}.npz"))
        D = X.shape[1]
        iu = np.triu_indices(D)
        C = np.zeros((D, D))
        C[iu] = g["coef_triu"]
        C.T[iu] = g["coef_triu"]
        A = {"kendall": np.sin(np.pi * C / 2.0), "spearman": 2.0 * np.sin(np.pi * C / 6.0), "scores": C.copy()}[method]
        C[np.diag_indices(D)] = A[np.diag_indices(D)] = 1.0
        R = A.copy()
        R[np.diag_indices(D)] = g["repaired_diag"]
        _cache[name, method] = frozen(X, C, A, float(g["min_eig"]), offset, R)
    return _cache[name, method]


def oracle(X, method):
    """(gram, untransformed, transformed) of the host formulation for one table, computed once per table and method."""
    key = ("oracle", X.shape, X.tobytes(), method)
    if key not in _cache:
        _cache[key] = frozen(pd_.rank_gram_host(X, method), pd_.rank_correlation_host(X, method, transform=False),
                             pd_.rank_correlation_host(X, method, transform=True))
    return _cache[key]


def run(lib, tables, method, device, **kw):
    """RankCorrelation of a HipLib call as numpy arrays (None stays None)."""
    out = lib.rank_correlation(torch.from_numpy(np.array(tables, dtype=np.float64)).to(device), method, **kw)
    if device != "cpu":
        torch.cuda.synchronize()
    return type(out)(*[None if a is None else a.cpu().numpy() for a in out])


def bounds(method):
    return (SCORE_BOUND, SCORE_BOUND) if method == "scores" else (RHO_BOUND, SIN_BOUND)


def tied_table(N, D, seed):
    """Standard-normal columns driven by three latent factors, every third column rounded to halves: ties."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, 3)) @ rng.standard_normal((3, D)) + rng.standard_normal((N, D))
    X[:, ::3] = np.round(X[:, ::3] * 2.0) / 2.0
    return X


# (N, D, K): one pair and one MFMA with 63 zero-padded k | one tile, ragged, a batch | two feature tiles of 64: an off-diagonal tile and a
# ragged second one | D > 128: the 128 x 128 tile of the wide route, two of them, the second ragged
SHAPES = [(2, 2, 1), (37, 7, 2), (130, 70, 1), (12, 130, 1)]


def shape_tables(N, D, K):
    if (N, D) == (2, 2):
        return np.array([[[0.5, 3.0], [1.5, -2.0]]])
    return np.stack([tied_table(N, D, 100 * N + D + k) for k in range(K)])


def check_shape(lib, device, N, D, K, method):
    tables = shape_tables(N, D, K)
    plain = run(lib, tables, method, device, transform=False, repair=False, want_f64=True, want_gram=True)
    mapped = run(lib, tables, method, device, transform=True, repair=False, want_f64=True)
    b_plain, b_mapped = bounds(method)
    assert plain.min_eig is None and plain.info.shape == (K, D) and not plain.info.any()
    for k in range(K):
        g, C, A = oracle(tables[k], method)
        d_plain, d_mapped = np.abs(plain.A64[k] - C).max(), np.abs(mapped.A64[k] - A).max()
        print(f"({N}, {D}, {K}) {method} table {k}: |device - host formulation| {d_plain:.2e} (bound {b_plain:.2e}), mapped {d_mapped:.2e} "
              f"(bound {b_mapped:.2e}); Gram {np.abs(plain.gram[k] - g).max():.2e}")
        if method != "scores":
            assert np.array_equal(plain.gram[k], g)  # exact integers
        else:  # the centred sums of the scores: the correlation's bound at the scale of the sums, sqrt(g_ii g_jj) <= max g_ii
            assert np.abs(plain.gram[k] - g).max() <= SCORE_BOUND * np.diag(g).max()
        for M in (plain.A64[k], mapped.A64[k], plain.gram[k], plain.A[k], mapped.A[k]):
            assert np.array_equal(M, M.T)  # the mirror is a copy
        assert (np.diag(plain.A64[k]) == 1.0).all() and (np.diag(mapped.A64[k]) == 1.0).all()
        assert d_plain <= b_plain and d_mapped <= b_mapped
        assert np.array_equal(plain.A[k], plain.A64[k].astype(np.float32)) and np.array_equal(mapped.A[k], mapped.A64[k].astype(np.float32))
    if (N, D) == (2, 2) and method == "kendall":  # one pair, discordant: G = [[1, -1], [-1, 1]] and its roots are exact
        assert np.array_equal(plain.gram[0], [[1.0, -1.0], [-1.0, 1.0]]) and np.array_equal(plain.A64[0], [[1.0, -1.0], [-1.0, 1.0]])


def permutation_table(N, D):
    """Column j is a permutation of 0 .. N - 1 of its own, drawn from seed j: a different known pattern per column."""
    return np.stack([np.random.default_rng(j).permutation(N) for j in range(D)], axis=1).astype(np.float64)


def integer_kendall_gram(X):
    """G = s^T s in int64, pair by pair in numpy integers: no BLAS, no float."""
    X = np.asarray(X)
    N, D = X.shape
    G = np.zeros((D, D), dtype=np.int64)
    for a in range(N - 1):
        s = np.sign(X[a] - X[a + 1:]).astype(np.int64)
        G += s.T @ s
    return G


def check_asymmetric(lib, device, N, D, tile):
    """A table whose Gram matrix differs from what a swapped row / column inside an off-diagonal tile, or a wrong C/D map, would store."""
    X = permutation_table(N, D)
    G = integer_kendall_gram(X)
    block = G[:tile, tile:]  # the off-diagonal tile as far as D reaches
    w = block.shape[1]
    assert not np.array_equal(block[:w, :w], block[:w, :w].T)  # a transposed tile would be another matrix
    assert len({tuple(r) for r in block}) == tile  # ... and so would one with two rows swapped or repeated
    out = run(lib, X[None], "kendall", device, transform=False, repair=False, want_gram=True, want_f64=True)
    assert np.array_equal(out.gram[0], G.astype(np.float64))
    r2 = pd_.doubled_midranks(X)
    c = r2 - (N + 1)
    out = run(lib, X[None], "spearman", device, transform=False, repair=False, want_gram=True)
    assert np.array_equal(r2, 2 * X.astype(np.int64) + 2) and np.array_equal(out.gram[0], (c.T @ c).astype(np.float64))


# ============================================================================================ CPU: the kernels on the emulator
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_d%d_k%d" % s)
def test_emulated_shapes_match_the_host_formulation(emul, shape, method):
    check_shape(emul, "cpu", *shape, method)


@pytest.mark.parametrize("N,D,tile", [(71, 70, 64), (41, 140, 128)])
def test_emulated_asymmetric_table_has_the_exact_integer_gram(emul, N, D, tile):
    check_asymmetric(emul, "cpu", N, D, tile)


def check_golden(lib, name, method, device):
    """A golden through the device entry: the coefficient, the mapped matrix, the repair's eigenvalue and the fp32 output."""
    X, C, A, min_eig, offset, R = golden(name, method)
    d_ref = DEVIATION[name][method]["d_ref"]
    b_plain, b_mapped = bounds(method)
    plain = run(lib, X[None], method, device, transform=False, repair=False, want_f64=True)
    out = run(lib, X[None], method, device, transform=True, eval_offset=offset, repair=True, want_f64=True)
    d_plain, d_mapped = np.abs(plain.A64[0] - C).max(), np.abs(out.A64[0] - A).max()
    norm = float(np.abs(A).sum(axis=1).max())
    print(f"{name} {method}: |device - scipy| {d_plain:.2e} (bound {b_plain + d_ref:.2e}), mapped {d_mapped:.2e} (bound "
          f"{b_mapped + d_ref:.2e}); min eig {min_eig!r}, device {out.min_eig[0]!r}, bound {norm * 2.0 ** -40:.2e}")
    assert np.array_equal(out.A64[0], out.A64[0].T) and np.array_equal(out.A[0], out.A[0].T)
    assert d_plain <= b_plain + d_ref and d_mapped <= b_mapped + d_ref
    if min_eig <= 1e-6:
        assert abs(out.min_eig[0] - min_eig) <= norm * 2.0 ** -40
    else:
        assert np.isposinf(out.min_eig[0])  # passed the test at 1e-6: never computed, not repaired
        assert np.array_equal(out.A[0], out.A64[0].astype(np.float32))
    R32 = R.astype(np.float32)
    assert (np.abs(out.A[0].astype(np.float64) - R32.astype(np.float64)) <= np.spacing(np.abs(R32)).astype(np.float64)).all()


@pytest.mark.parametrize("method", METHODS)
def test_emulated_golden_matrix_repair_and_fp32_output(emul, method):
    check_golden(emul, "n37_d7", method, "cpu")


# ============================================================================================ CPU: host layer
def test_bounds_are_derived_and_goldens_are_small():
    assert sorted(DEVIATION) == sorted(NAMES)
    assert SCORE_BOUND < 1e-12
    for name in NAMES:
        assert golden_table(name)[0].shape == (DEVIATION[name]["N"], DEVIATION[name]["D"])
        for suffix in [""] + ["_" + m for m in METHODS]:
            assert os.path.getsize(os.path.join(GOLDEN, f"rank_{name}{suffix}.npz")) < 1 << 20
    eigs = [golden(n, m)[3] for n in NAMES for m in METHODS]
    assert any(e <= 1e-6 for e in eigs) and any(e > 1e-6 for e in eigs)  # a case that needs the repair and one that does not
    X, C, *_ = golden("n37_d7", "kendall")
    assert abs(C[1, 4] + 1.0) <= 1e-15 and (np.unique(X[:, 0]).size < 37)  # |tau| = 1; ties


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", NAMES)
def test_host_formulation_matches_the_scipy_goldens(name, method):
    X, C, A, *_ = golden(name, method)
    g, plain, mapped = oracle(X, method)
    b_plain, b_mapped = bounds(method)
    d_plain, d_mapped = np.abs(plain - C).max(), np.abs(mapped - A).max()
    print(f"{name} {method}: host formulation, |. - scipy| {d_plain:.2e}, mapped {d_mapped:.2e} (recorded d_ref "
          f"{DEVIATION[name][method]['d_ref']:.2e})")
    assert d_plain <= b_plain and d_mapped <= b_mapped
    assert np.array_equal(mapped, mapped.T) and (np.diag(mapped) == 1.0).all()
    if method != "scores":
        assert np.array_equal(g, np.round(g)) and np.abs(g).max() < 2.0 ** 53


def test_host_formulation_ranks_flags_and_arguments():
    X = np.array([[1.0, 5.0, 2.0], [1.0, 5.0, np.nan], [0.0, 5.0, 1.0], [np.inf, 5.0, -np.inf]])
    r2 = pd_.doubled_midranks(X)
    assert np.array_equal(r2[:, 0], [5, 5, 2, 8]) and np.array_equal(r2[:, 1], [5, 5, 5, 5])  # twice rankdata(average); +-Inf rank
    A = pd_.rank_correlation_host(X, "kendall")
    assert np.isnan(A[1]).all() and np.isnan(A[:, 2]).all() and A[0, 0] == 1.0  # constant and NaN columns
    with pytest.raises(ValueError, match="pearson"):
        pd_.rank_correlation_host(X, "pearson")


def test_emulated_c_entry_error_codes(emul):
    from uglad_amd._lib import UgladError

    dll = emul._dll
    size, chunks = dll.uglad_rank_correlation_workspace_floats, dll.uglad_rank_correlation_pair_chunks
    slab = 2 * (2 * 64 * 64 + 3 * 64 + 8 + 32) + 2  # (+ 2: the block behind the slabs starts at a multiple of 16 bytes)
    assert size(1, 37, 7, 0) == size(1, 37, 7, 2) == slab + 2 * 37 * 7
    assert size(1, 37, 7, 1) == slab + 7 * 128 + 64 * 64 and size(3, 37, 7, 1) == 3 * size(1, 37, 7, 1)
    assert size(1, 1, 7, 1) == -2 and size(1, 37, 1, 1) == -2 and size(1, 65537, 7, 1) == -2 and size(0, 37, 7, 1) == -2
    assert size(1, 37, emul.max_dim + 1, 1) == -2 and size(65536, 37, 7, 1) == -2
    assert size(1, 37, 7, 3) == -3 and size(1, 37, 7, -1) == -3
    assert size(1, 65536, 7, 1) > 0 and size(60, 65536, 2048, 0) == -2  # beyond 2^31 - 1 floats
    assert chunks(1, 2, 2) == 1 and chunks(1, 1, 7) == -2 and 2 <= chunks(1, 1025, 70) <= 1024
    N, D = 37, 7
    X = torch.from_numpy(tied_table(N, D, 1))
    A = torch.empty(1, D, D)
    wsp = torch.empty(size(1, N, D, 1) + 2, dtype=torch.float32)
    assert wsp.data_ptr() % 8 == 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(X_p=p(X), N_=N, D_=D, method=1, transform=1, A_p=p(A), wsp_p=p(wsp)):
        emul._call("uglad_rank_correlation", X_p, 1, N_, D_, method, transform, 0.1, A_p, None, None, None, None, wsp_p)

    call()  # (the arguments are good)
    for bad in (dict(X_p=None), dict(A_p=None), dict(wsp_p=None), dict(wsp_p=ctypes.c_void_p(wsp.data_ptr() + 4))):  # NULL, misaligned
        with pytest.raises(UgladError, match="NULL"):
            call(**bad)
    for bad in (dict(N_=1), dict(D_=1), dict(N_=65537), dict(D_=emul.max_dim + 1)):
        with pytest.raises(UgladError, match="dimension"):
            call(**bad)
    for bad in (dict(method=3), dict(method=-1), dict(transform=2)):
        with pytest.raises(UgladError, match="mode"):
            call(**bad)
    with pytest.raises(UgladError):
        emul.rank_correlation(torch.zeros(1, 4, D), "kendall")  # fp32 tables are refused
    with pytest.raises(UgladError, match="pearson"):
        emul.rank_correlation(X[None], "pearson")


def flagged_tables(X):
    """Three copies of a table: a NaN in column 5 of the first, column 9 of the second constant, the third as it is."""
    tables = np.stack([X, X, X])
    tables[0, 11, 5] = np.nan
    tables[1, :, 9] = 2.5
    return tables


def check_flagged(lib, device, X, method):
    D = X.shape[1]
    tables = flagged_tables(X)
    out = run(lib, tables, method, device, repair=False, want_f64=True, want_gram=True)
    alone = run(lib, tables[2:], method, device, repair=False, want_f64=True, want_gram=True)
    for k, (j, bit) in enumerate([(5, 1), (9, 2)]):
        nan = np.zeros((D, D), dtype=bool)
        nan[j, :] = nan[:, j] = True
        assert np.array_equal(np.isnan(out.A64[k]), nan) and np.array_equal(np.isnan(out.A[k]), nan)  # exactly that row and column
        assert np.array_equal(out.A64[k][~nan], out.A64[2][~nan])
        expect = np.zeros(D, dtype=np.int32)
        expect[j] = bit
        assert np.array_equal(out.info[k], expect)
    assert not out.info[2].any()
    for a, b in zip(out, alone):  # the third table's bits are those of a K = 1 call
        assert (a is None and b is None) or np.array_equal(a[2], b[0], equal_nan=True)


@pytest.mark.parametrize("method", METHODS)
def test_emulated_flagged_columns_stay_in_their_row_and_column(emul, method):
    check_flagged(emul, "cpu", tied_table(37, 12, 5), method)


# ============================================================================================ GPU
def gpu_lib():
    from uglad_amd import _lib

    return _lib.get_lib()


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_d%d_k%d" % s)
def test_gpu_shapes_match_the_host_formulation(shape, method):
    check_shape(gpu_lib(), "cuda", *shape, method)


@pytest.mark.gpu
@pytest.mark.parametrize("N,D,tile", [(71, 70, 64), (41, 140, 128)])
def test_gpu_asymmetric_table_has_the_exact_integer_gram(N, D, tile):
    check_asymmetric(gpu_lib(), "cuda", N, D, tile)


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", NAMES)
def test_gpu_goldens_matrix_repair_and_fp32_output(name, method):
    check_golden(gpu_lib(), name, method, "cuda")


@pytest.mark.gpu
def test_gpu_many_pair_chunks_give_the_exact_gram():
    """(1025, 70): the launch deals the pairs of every tile over at least two chunks, whose int32 partial tiles meet in atomics."""
    lib = gpu_lib()
    assert lib.rank_pair_chunks(1, 1025, 70) >= 2
    X = tied_table(1025, 70, 9)
    out = run(lib, X[None], "kendall", "cuda", transform=False, repair=False, want_gram=True, want_f64=True)
    g, C, _ = oracle(X, "kendall")
    assert np.array_equal(out.gram[0], g) and np.abs(out.A64[0] - C).max() <= RHO_BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_gpu_flagged_columns_stay_in_their_row_and_column(method):
    check_flagged(gpu_lib(), "cuda", golden_table("n257_d129")[0], method)


@pytest.mark.gpu
def test_gpu_two_calls_give_identical_bits():
    lib = gpu_lib()
    X = golden_table("n257_d129")[0]
    for method in METHODS:
        first = run(lib, X[None], method, "cuda", repair=True, want_f64=True, want_gram=True)
        second = run(lib, X[None], method, "cuda", repair=True, want_f64=True, want_gram=True)
        for a, b in zip(first, second):
            assert np.array_equal(a, b)


@pytest.mark.gpu
def test_gpu_rank_correlation_takes_an_array_or_a_list():
    import uglad_amd

    X, C, A, min_eig, offset, R = golden("n130_d70", "kendall")
    one, mn = uglad_amd.rank_correlation(X, method="kendall", eval_offset=offset)
    many, mns = uglad_amd.rank_correlation([X, X[::-1].copy()], method="kendall", eval_offset=offset)
    assert one.is_cuda and one.dtype == torch.float32 and one.shape == (70, 70) and many.shape == (2, 70, 70) and mns.shape == (2,)
    assert torch.equal(one, many[0]) and torch.equal(one, many[1]) and mn == mns[0] == mns[1]  # (the order of the rows does not matter)
    assert abs(mn - min_eig) <= np.abs(A).sum(axis=1).max() * 2.0 ** -40
    plain, none = uglad_amd.rank_correlation(X, method="spearman", transform=False, repair=False)
    assert none is None and np.abs(plain.cpu().numpy() - golden("n130_d70", "spearman")[1]).max() < 1e-6
    bad = X.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        uglad_amd.rank_correlation(bad)


@pytest.mark.gpu
def test_gpu_fit_copula_trains_on_the_repaired_rank_correlation_matrix(tmp_path):
    import pandas as pd

    import uglad_amd
    from uglad_amd import main

    X, C, A, min_eig, offset, R = golden("n130_d70", "kendall")
    names = [f"gene{i}" for i in range(70)]
    df = pd.DataFrame(np.exp(X), columns=names)  # a monotone transform of every column: the ranks, and so the fit, do not see it
    torch.manual_seed(0)
    est = uglad_amd.uGLAD_GL()
    est.fit_copula(df, method="kendall", eval_offset=offset, epochs=20, L=6, verbose=False)
    P = est.precision_
    assert P.shape == (70, 70) and np.isfinite(P).all()
    assert np.abs(est.covariance_ - A).max() <= SIN_BOUND + DEVIATION["n130_d70"]["kendall"]["d_ref"] and est.covariance_.dtype == np.float64
    assert abs(est.copula_min_eig_ - min_eig) <= np.abs(A).sum(axis=1).max() * 2.0 ** -40
    assert est.node_names_ == names and np.allclose(est.location_, np.exp(X).mean(axis=0), rtol=1e-12)
    assert est.data_min_ is None and est.data_range_ is None and est.model_glad is not None and np.isfinite(est.cond_max_)
    torch.manual_seed(0)
    Sb = torch.from_numpy(R.astype(np.float32))[None].cuda()
    ref, _, _ = main.run_uGLAD_direct(None, eval_offset=offset, EPOCHS=20, L=6, VERBOSE=False, Sb=Sb)
    ref = ref[0].detach().cpu().numpy().astype(np.float64)
    err = float(np.linalg.norm(P - ref) / np.linalg.norm(ref))
    _, loss = uglad_amd.forward_uGLAD(Sb, est.model_glad, L=6, INIT_DIAG=0)
    print(f"fit_copula against run_uGLAD_direct on the golden's repaired matrix: rel-Frobenius {err:.2e}; loss {float(loss.detach()):.4f}")
    assert np.isfinite(float(loss.detach())) and err < 1e-4  # (the project's contract for a fit, tests/test_gpu_parity.py)
    out = est.predict(S=R.copy())
    assert out.shape == (70, 70) and np.isfinite(out).all()
    graph = est.recovered_graph()
    assert graph.edges.ndim == 2 and graph.edges.shape[1] == 2  # (20 epochs may leave no edge above the threshold: the list may be empty)
    main.save_uGLAD_model(est, str(tmp_path / "copula"))
    back = main.load_uGLAD_model(str(tmp_path / "copula"))
    assert np.array_equal(back.precision_, P) and np.array_equal(back.predict(S=R.copy()), out)
    with pytest.raises(ValueError, match="gene3"):
        est.fit_copula(df.assign(gene3=1.0), epochs=1, verbose=False)
