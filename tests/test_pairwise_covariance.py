"""The pairwise-complete covariance of tables with missing entries (uglad_pairwise_covariance, csrc/pairwise_wide.h; the host formulation
in uglad_amd/utils/prepare_data.py), against pandas' DataFrame.cov and the package's host formulation.  CPU: the host formulation, the
unmodified kernel sources on the SIMT emulator, the Python surface as far as it needs no training.  GPU: the same checks at the same shapes,
a ragged multi-tile batch, fit_pairwise with and without the fold ensemble.

Tolerances, none of them measured on the code under test:
  counts          exact equality.
  the matrix      with q_i = sum_n z_ni^2, Cauchy-Schwarz gives |p_ij| <= sqrt(q_i q_j) and |a_ij a_ji| / n_ij <= sqrt(q_i q_j); either
                  side's dot products err by at most about (N + c) 2^-53 of that:  |device - host| <= 4 (N + 8) 2^-53 sqrt(q_i q_j) / n_ij
                  per entry.  The same bound holds the host formulation to pandas' cov times (n_ij - 1) / n_ij.
  fp32            the fp32 output is the float32 rounding of the device's own fp64 matrix, bit for bit, and within one fp32 ulp of the
                  float32 rounding of the host matrix.
  min eig         |device - eigvalsh(host matrix)| <= ||A||_inf 2^-40 (the bisection's bracket ends at ||A||_inf 2^-48;
                  test_rank_correlation.py's bound for the same bracket).
  repaired diag   diag + offset - min eig to that bound, plus the one fp32 rounding of the stored value.
Every unflagged table asserts min n_ij >= min_pairs, so that a changed seed cannot turn a numeric case into a flag case unnoticed."""
import ctypes

import numpy as np
import pytest
import torch

from uglad_amd.utils import prepare_data as pd_

OFFSET = 0.1
_cache = {}


def frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def missing_table(N, D, p, seed):
    """Three latent factors plus noise plus 50, cells dropped independently with probability p by a seeded generator."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, 3)) @ rng.standard_normal((3, D)) + rng.standard_normal((N, D)) + 50.0
    X[rng.random((N, D)) < p] = np.nan
    return X


# (N, D, K) -> the missing fraction: one MFMA, a pair at n = 2 (min_pairs = 1) | ragged, one tile, a batch; positive definite: no repair |
# two feature tiles, an off-diagonal tile, five k-chunks with a ragged last one; indefinite | N < D, three tiles; indefinite
SHAPES = {(3, 2, 1): None, (37, 7, 2): 0.2, (130, 70, 1): 0.25, (40, 130, 1): 0.3}
INDEFINITE = [(130, 70, 1), (40, 130, 1)]
RAGGED_BATCH = (70, 200, 3)  # (GPU) four tiles of 64, the last one ragged, three k-chunks, three tables


def shape_tables(N, D, K):
    key = ("tables", N, D, K)
    if key not in _cache:
        if (N, D) == (3, 2):
            tables = np.array([[[1.0, 2.0], [3.0, np.nan], [5.0, 1.0]]])
        else:
            p = SHAPES.get((N, D, K), 0.25)
            tables = np.stack([missing_table(N, D, p, 100 * N + D + k) for k in range(K)])
        _cache[key], = frozen(tables)
    return _cache[key]


def min_pairs_of(N, D):
    return 1 if (N, D) == (3, 2) else 2


def oracle(X, normalize, min_pairs=2):
    """(cov, counts, bound) of the host formulation for one table, computed once and never modified."""
    key = ("oracle", X.shape, X.tobytes(), bool(normalize), min_pairs)
    if key not in _cache:
        cov, counts = pd_.pairwise_covariance_host(X, normalize=normalize, min_pairs=min_pairs)
        seen = ~np.isnan(X)
        with np.errstate(all="ignore"):
            y = X
            if normalize:
                mn, scale = pd_.observed_min_scale(X)
                y = (X - mn) * scale
            z = np.where(seen, y - np.where(seen, y, 0.0).sum(axis=0) / seen.sum(axis=0), 0.0)
            q = (z * z).sum(axis=0)
            bound = 4.0 * (X.shape[0] + 8) * 2.0 ** -53 * np.sqrt(np.outer(q, q)) / counts
        _cache[key] = frozen(cov, counts, bound)
    return _cache[key]


def run(lib, tables, device, **kw):
    """PairwiseCovariance of a HipLib call as numpy arrays (None stays None)."""
    out = lib.pairwise_covariance(torch.from_numpy(np.array(tables, dtype=np.float64)).to(device), **kw)
    if device != "cpu":
        torch.cuda.synchronize()
    return type(out)(*[None if a is None else a.cpu().numpy() for a in out])


def same_bits(a, b):
    return (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes())


def within_one_fp32_ulp(S32, host64):
    h = host64.astype(np.float32)
    return (np.abs(S32.astype(np.float64) - h.astype(np.float64)) <= np.spacing(np.abs(h)).astype(np.float64)).all()


# ============================================================================================ the checks, for either device
def check_shape(lib, device, N, D, K, normalize):
    tables, mp = shape_tables(N, D, K), min_pairs_of(N, D)
    out = run(lib, tables, device, normalize=normalize, min_pairs=mp, repair=False, want_f64=True, want_counts=True)
    again = run(lib, tables, device, normalize=normalize, min_pairs=mp, repair=False, want_f64=True, want_counts=True)
    assert out.min_eig is None and out.info.shape == (K, D) and out.info.dtype == np.int32 and not out.info.any()
    assert all(same_bits(a, b) for a, b in zip(out, again))  # two calls, the same bits
    for k in range(K):
        cov, counts, bound = oracle(tables[k], normalize, mp)
        assert counts.min() >= mp and not np.isnan(cov).any()
        ratio = float((np.abs(out.S64[k] - cov) / bound).max())
        print(f"({N}, {D}, {K}) normalize={int(normalize)} table {k}: |device - host formulation| is {ratio:.3f} of the bound; min n_ij {counts.min()}")
        assert np.array_equal(out.counts[k], counts) and out.counts.dtype == np.int32
        assert ratio <= 1.0
        assert np.array_equal(out.S64[k], out.S64[k].T) and np.array_equal(out.S[k], out.S[k].T)  # the mirror is a copy
        assert np.array_equal(out.S[k], out.S64[k].astype(np.float32)) and within_one_fp32_ulp(out.S[k], cov)
    if (N, D) == (3, 2) and not normalize:  # by hand: column 0 over rows {0, 1, 2}, the pair and column 1 over rows {0, 2}
        assert np.array_equal(out.counts[0], [[3, 2], [2, 2]])
        assert np.allclose(out.S64[0], [[8.0 / 3.0, -1.0], [-1.0, 0.25]], rtol=0, atol=1e-15)


def complete_table(N, D, seed):
    return missing_table(N, D, 0.0, seed)


def check_complete_table(lib, device):
    """A table without NaN: the plain covariance, and uglad_covariance_wide's repair decision and eigenvalue on a rank-deficient table."""
    N, D = 40, 70  # N < D: rank-deficient, min eig ~ 0, repaired by both front-ends
    X = complete_table(N, D, 7)
    out = run(lib, X[None], device, eval_offset=OFFSET, repair=True, want_f64=True, want_counts=True)
    cov, counts, bound = oracle(X, False)
    plain = np.cov(X.T, bias=True)
    assert (out.counts[0] == N).all() and not out.info.any()
    assert (np.abs(out.S64[0] - plain) <= bound).all() and (np.abs(out.S64[0] - cov) <= bound).all()
    Xd = torch.from_numpy(X[None].copy()).to(device)
    S_w, mn_w, repaired_w = lib.covariance_wide(Xd, normalize=False, eval_offset=OFFSET, repair=True, return_min_eig=True)
    norm = float(np.abs(plain).sum(axis=1).max())
    print(f"complete ({N}, {D}): min eig {out.min_eig[0]!r}, covariance_wide {float(mn_w[0])!r}, bound {norm * 2.0 ** -40:.2e}")
    assert bool(repaired_w[0]) and np.isfinite(out.min_eig[0])  # the same decision
    assert abs(out.min_eig[0] - float(mn_w[0])) <= norm * 2.0 ** -40
    assert abs(out.min_eig[0] - np.linalg.eigvalsh(plain)[0]) <= norm * 2.0 ** -40


def flag_cases():
    """[(normalize, min_pairs, tables (3, N, D) with a clean middle one, expected info (3, D))]"""
    if "flags" in _cache:
        return _cache["flags"]
    N, D = 37, 12
    base = missing_table(N, D, 0.2, 5)
    out = []
    # an all-NaN column | clean | two columns never observed together
    t = np.stack([base, base, base])
    t[0, :, 3] = np.nan
    t[2, 0::2, 1] = np.nan
    t[2, 1::2, 4] = np.nan
    info = np.zeros((3, D), dtype=np.int32)
    info[0, 3] = 1
    info[2, [1, 4]] = 2
    out.append((False, 2, t, info))
    # min_pairs = 5 with one pair at 4 | clean | the same pair in both its columns' other tile position
    t = np.stack([base, base, base])
    both = np.nonzero(~np.isnan(base[:, 2]) & ~np.isnan(base[:, 7]))[0]
    t[0, both[4:], 2] = np.nan  # columns 2 and 7 are observed together in exactly 4 rows
    both = np.nonzero(~np.isnan(base[:, 0]) & ~np.isnan(base[:, 11]))[0]
    t[2, both[4:], 11] = np.nan
    info = np.zeros((3, D), dtype=np.int32)
    info[0, [2, 7]] = 2
    info[2, [0, 11]] = 2
    out.append((False, 5, t, info))
    # normalize = 1: a constant observed column | clean | a column that holds an infinity
    t = np.stack([base, base, base])
    t[0, ~np.isnan(base[:, 6]), 6] = 2.5
    t[2, np.nonzero(~np.isnan(base[:, 9]))[0][1], 9] = np.inf
    info = np.zeros((3, D), dtype=np.int32)
    info[0, 6] = 4
    info[2, 9] = 8
    out.append((True, 2, t, info))
    _cache["flags"] = [(nz, mp, frozen(t)[0], frozen(i)[0]) for nz, mp, t, i in out]
    return _cache["flags"]


def check_flags(lib, device, case):
    normalize, min_pairs, tables, info = flag_cases()[case]
    D = tables.shape[2]
    kw = dict(normalize=normalize, min_pairs=min_pairs, eval_offset=OFFSET, repair=True, want_f64=True, want_counts=True)
    out = run(lib, tables, device, **kw)
    alone = run(lib, tables[1:2], device, **kw)
    assert np.array_equal(out.info, info)
    for k in range(3):
        cov, counts, bound = oracle(tables[k], normalize, min_pairs)
        dead = (info[k] & (1 | 4 | 8)) != 0
        nan = dead[:, None] | dead[None, :] | (counts < min_pairs)
        if case == 1 and k != 1:
            assert counts[counts < min_pairs].tolist() == [4, 4]  # the one pair, and its mirror
        assert np.array_equal(np.isnan(cov), nan)  # the host formulation gives NaN in the same places by its arithmetic alone
        assert np.array_equal(np.isnan(out.S64[k]), nan) and np.array_equal(np.isnan(out.S[k]), nan)  # NaN exactly in the flagged entries
        assert np.array_equal(out.counts[k], counts)
        assert (np.abs(out.S64[k] - cov)[~nan] <= bound[~nan]).all()
        assert np.isnan(out.min_eig[k]) == bool(info[k].any())  # a flagged table is not repaired
        if info[k].any():
            assert np.array_equal(out.S[k], out.S64[k].astype(np.float32), equal_nan=True)
    cov, counts, _ = oracle(tables[1], normalize, min_pairs)
    assert counts.min() >= min_pairs and not np.isnan(out.min_eig[1])
    for a, b in zip(out, alone):  # the clean table's every output is what a K = 1 call gives, bit for bit
        assert same_bits(a[1], b[0])


def check_repair(lib, device, N, D, K, normalize):
    tables = shape_tables(N, D, K)
    out = run(lib, tables, device, normalize=normalize, eval_offset=OFFSET, repair=True, want_f64=True)
    plain = run(lib, tables, device, normalize=normalize, repair=False, want_f64=True)
    for k in range(K):
        cov, counts, _ = oracle(tables[k], normalize)
        eig = float(np.linalg.eigvalsh(cov)[0])
        norm = float(np.abs(cov).sum(axis=1).max())
        print(f"({N}, {D}, {K}) normalize={int(normalize)} table {k}: min eig {eig!r}, device {out.min_eig[k]!r}, bound {norm * 2.0 ** -40:.2e}")
        assert same_bits(out.S64[k], plain.S64[k])  # S64 is never repaired
        off = ~np.eye(D, dtype=bool)
        assert np.array_equal(out.S[k][off], plain.S[k][off])  # the repair leaves the off-diagonals alone
        if eig <= 1e-6:
            assert abs(out.min_eig[k] - eig) <= norm * 2.0 ** -40
            want = np.diag(cov) + OFFSET - eig
            assert (np.abs(np.diag(out.S[k]).astype(np.float64) - want) <= norm * 2.0 ** -40 + np.spacing(want.astype(np.float32))).all()
        else:
            assert np.isposinf(out.min_eig[k]) and same_bits(out.S[k], plain.S[k])  # passed at 1e-6: never computed, not repaired


# ============================================================================================ CPU: the host formulation
@pytest.mark.parametrize("N,D,p", [(37, 7, 0.2), (130, 70, 0.25), (40, 130, 0.3), (300, 288, 0.25)])
def test_host_formulation_matches_pandas(N, D, p):
    import pandas as pd

    X = missing_table(N, D, p, 100 * N + D)
    cov, counts, bound = oracle(X, False)
    assert counts.min() >= 2
    ref = pd.DataFrame(X).cov().to_numpy() * (counts - 1) / counts
    ratio = float((np.abs(cov - ref) / bound).max())
    print(f"({N}, {D}): |host formulation - pandas (n - 1) / n| is {ratio:.3f} of the bound")
    assert ratio <= 1.0 and np.array_equal(cov, cov.T)
    assert np.array_equal(counts, (~np.isnan(X)).astype(np.int64).T @ (~np.isnan(X)).astype(np.int64))


def test_host_formulation_normalises_over_the_observed_entries_and_checks_its_arguments():
    X = missing_table(37, 7, 0.2, 3)
    mn, mx = np.nanmin(X, axis=0), np.nanmax(X, axis=0)
    cov, counts, bound = oracle(X, True)
    ref, _ = pd_.pairwise_covariance_host((X - mn) / (mx - mn))
    assert (np.abs(cov - ref) <= 4 * bound).all()  # (a division against the product with the reciprocal: an ulp of y per cell)
    few, _ = pd_.pairwise_covariance_host(X, min_pairs=int(counts.min()) + 1)
    assert np.array_equal(np.isnan(few), counts < counts.min() + 1)
    with pytest.raises(ValueError):
        pd_.pairwise_covariance_host(X[None])
    with pytest.raises(ValueError, match="min_pairs"):
        pd_.pairwise_covariance_host(X, min_pairs=0)


# ============================================================================================ CPU: the kernels on the emulator
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "n%d_d%d_k%d" % s)
def test_emulated_shapes_match_the_host_formulation(emul, shape, normalize):
    check_shape(emul, "cpu", *shape, normalize)


def test_emulated_complete_table_is_the_plain_covariance_with_its_repair(emul):
    check_complete_table(emul, "cpu")


@pytest.mark.parametrize("case", [0, 1, 2], ids=["empty_and_disjoint", "few_pairs", "constant_and_infinite"])
def test_emulated_flags_stay_with_their_table_and_entries(emul, case):
    check_flags(emul, "cpu", case)


@pytest.mark.parametrize("shape", INDEFINITE + [(37, 7, 2)], ids=lambda s: "n%d_d%d_k%d" % s)
def test_emulated_repair_of_an_indefinite_matrix(emul, shape):
    check_repair(emul, "cpu", *shape, normalize=True)


def test_emulated_c_entry_error_codes(emul):
    from uglad_amd._lib import UgladError

    size = emul._dll.uglad_pairwise_covariance_workspace_floats
    slab = 2 * (2 * 64 * 64 + 3 * 64 + 8)
    assert size(1, 7) == size(1, 64) == slab + 64 + 2 and size(3, 7) == 3 * size(1, 7)  # the Cholesky slab and DP + 2 int32 of flags
    assert size(1, 0) == -2 and size(1, emul.max_dim + 1) == -2 and size(0, 7) == -2 and size(65536, 7) == -2 and size(1, emul.max_dim) > 0
    N, D = 9, 7
    X = torch.from_numpy(missing_table(N, D, 0.1, 1))
    S = torch.empty(1, D, D)
    wsp = torch.empty(size(1, D) + 2, dtype=torch.float32)
    assert wsp.data_ptr() % 8 == 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(X_p=p(X), N_=N, D_=D, normalize=0, min_pairs=2, S_p=p(S), wsp_p=p(wsp)):
        emul._call("uglad_pairwise_covariance", X_p, 1, N_, D_, normalize, min_pairs, 0.1, S_p, None, None, None, None, wsp_p)

    call()  # (the arguments are good)
    for bad in (dict(X_p=None), dict(S_p=None), dict(wsp_p=None), dict(wsp_p=ctypes.c_void_p(wsp.data_ptr() + 4))):  # NULL, misaligned
        with pytest.raises(UgladError, match="NULL"):
            call(**bad)
    for bad in (dict(D_=0), dict(D_=emul.max_dim + 1), dict(N_=0)):
        with pytest.raises(UgladError, match="dimension"):
            call(**bad)
    for bad in (dict(normalize=2), dict(normalize=-1), dict(min_pairs=0)):
        with pytest.raises(UgladError, match="mode"):
            call(**bad)
    with pytest.raises(UgladError):
        emul.pairwise_covariance(torch.zeros(1, 4, D))  # fp32 tables are refused


def named_table():
    import pandas as pd

    X = missing_table(37, 7, 0.2, 3707)
    return X, pd.DataFrame(X, columns=[f"gene{i}" for i in range(7)])


def test_emulated_python_surface_shapes_and_the_flagged_column_by_name(emul):
    """inputs.pairwise_covariance for one table and for a list; fit_pairwise raises before any training on a flagged column."""
    import uglad_amd

    X, df = named_table()
    S, mn, counts = uglad_amd.pairwise_covariance(df, normalize=True, eval_offset=OFFSET)
    many, mns, cs = uglad_amd.pairwise_covariance([X, X[::-1].copy()], normalize=True, eval_offset=OFFSET)
    assert S.shape == (7, 7) and S.dtype == torch.float32 and isinstance(mn, float) and counts.shape == (7, 7) and counts.dtype == torch.int32
    assert many.shape == (2, 7, 7) and mns.shape == (2,) and mns.dtype == np.float64 and cs.shape == (2, 7, 7)
    assert torch.equal(S, many[0]) and mn == mns[0] and torch.equal(counts, cs[1])  # (the counts do not depend on the order of the rows)
    assert np.array_equal(counts.numpy(), oracle(X, True)[1])
    plain, none, _ = uglad_amd.pairwise_covariance(X, repair=False)
    assert none is None and (np.abs(plain.numpy() - oracle(X, False)[0]) <= 1e-5).all()
    assert uglad_amd.main.pairwise_covariance is uglad_amd.pairwise_covariance
    with pytest.raises(ValueError, match="one shape"):
        uglad_amd.pairwise_covariance(np.zeros(5))
    with pytest.warns(RuntimeWarning, match=r"table 0 .*\['gene3'\]: no observed entry"):  # a flagged table does not raise here: it warns
        bad, bad_mn, _ = uglad_amd.pairwise_covariance(df.assign(gene3=np.nan))
    assert np.isnan(bad_mn) and torch.isnan(bad[3]).all() and not torch.isnan(bad[0, :3]).any()
    est = uglad_amd.uGLAD_GL()
    with pytest.raises(ValueError, match=r"gene3.*no observed entry"):
        est.fit_pairwise(df.assign(gene3=np.nan), epochs=1, verbose=False)
    with pytest.raises(ValueError, match=r"gene5.*constant"):
        est.fit_pairwise(df.assign(gene5=np.where(df["gene5"].isna(), np.nan, 1.0)), epochs=1, verbose=False)
    with pytest.raises(ValueError, match=r"\['gene0', 'gene1'\].*fewer than min_pairs"):
        est.fit_pairwise(df.assign(gene0=df["gene0"].where(np.arange(37) % 2 == 0), gene1=df["gene1"].where(np.arange(37) % 2 == 1)),
                         epochs=1, verbose=False)
    with pytest.raises(ValueError, match="one"):
        est.fit_pairwise([X, X], epochs=1, verbose=False)
    assert est.precision_ is None


# ============================================================================================ GPU
def gpu_lib():
    from uglad_amd import _lib

    return _lib.get_lib()


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalize"])
@pytest.mark.parametrize("shape", list(SHAPES) + [RAGGED_BATCH], ids=lambda s: "n%d_d%d_k%d" % s)
def test_gpu_shapes_match_the_host_formulation(shape, normalize):
    check_shape(gpu_lib(), "cuda", *shape, normalize)


@pytest.mark.gpu
def test_gpu_complete_table_is_the_plain_covariance_with_its_repair():
    check_complete_table(gpu_lib(), "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1, 2], ids=["empty_and_disjoint", "few_pairs", "constant_and_infinite"])
def test_gpu_flags_stay_with_their_table_and_entries(case):
    check_flags(gpu_lib(), "cuda", case)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", INDEFINITE + [(37, 7, 2), RAGGED_BATCH], ids=lambda s: "n%d_d%d_k%d" % s)
def test_gpu_repair_of_an_indefinite_matrix(shape):
    check_repair(gpu_lib(), "cuda", *shape, normalize=True)


FIT = dict(epochs=20, verbose=False)


def fit_table():
    import pandas as pd

    X = missing_table(200, 20, 0.15, 2020)
    return X, pd.DataFrame(X, columns=[f"gene{i}" for i in range(20)])


@pytest.mark.gpu
def test_gpu_fit_pairwise_trains_on_the_repaired_pairwise_matrix(tmp_path):
    import uglad_amd
    from uglad_amd import main

    X, df = fit_table()
    cov, counts, bound = oracle(X, True)
    assert counts.min() >= 2
    torch.manual_seed(0)
    est = uglad_amd.uGLAD_GL()
    est.fit_pairwise(df, eval_offset=OFFSET, **FIT)
    P = est.precision_
    assert P.shape == (20, 20) and np.isfinite(P).all()
    assert np.abs(P - P.T).max() <= 1e-5 * np.abs(P).max()  # (symmetric up to the fp32 rounding of the path's products)
    assert est.covariance_.dtype == np.float64 and (np.abs(est.covariance_ - cov) <= bound).all()
    assert np.array_equal(est.pairwise_counts_, counts) and est.node_names_ == list(df.columns) and np.isfinite(est.cond_max_)
    eig = float(np.linalg.eigvalsh(cov)[0])
    assert (np.isposinf(est.pairwise_min_eig_) if eig > 1e-6 else abs(est.pairwise_min_eig_ - eig) <= np.abs(cov).sum(axis=1).max() * 2.0 ** -40)
    mn, mx = np.nanmin(X, axis=0), np.nanmax(X, axis=0)
    assert np.array_equal(est.data_min_, mn) and np.array_equal(est.data_range_, mx - mn)
    assert np.allclose(est.location_, np.nanmean((X - mn) / (mx - mn), axis=0), rtol=1e-12, atol=0)
    # plumbing: the same bits as direct-mode training on the matrix pairwise_covariance returns
    A, mn_eig, _ = uglad_amd.pairwise_covariance(df, normalize=True, eval_offset=OFFSET)
    assert mn_eig == est.pairwise_min_eig_
    torch.manual_seed(0)
    ref, _, _ = main.run_uGLAD_direct(None, eval_offset=OFFSET, EPOCHS=20, VERBOSE=False, Sb=A[None])
    assert np.array_equal(P, ref[0].detach().cpu().numpy())
    scores = est.score_samples(X)
    assert np.array_equal(np.isnan(scores), np.isnan(X).any(axis=1)) and np.isnan(scores).any() and not np.isnan(scores).all()
    out = est.predict(S=cov + (OFFSET - min(eig, 0.0)) * np.eye(20))
    assert out.shape == (20, 20) and np.isfinite(out).all()
    assert est.recovered_graph().edges.shape[1] == 2
    main.save_uGLAD_model(est, str(tmp_path / "pairwise"))
    back = main.load_uGLAD_model(str(tmp_path / "pairwise"))
    assert np.array_equal(back.precision_, P) and np.array_equal(back.pairwise_counts_, counts)
    with pytest.raises(ValueError, match="gene3"):
        est.fit_pairwise(df.assign(gene3=np.nan), epochs=1, verbose=False)


@pytest.mark.gpu
def test_gpu_fit_pairwise_fold_ensemble_is_the_hand_made_sequence():
    import uglad_amd
    from uglad_amd import main
    from uglad_amd.dist import Collective

    X, df = fit_table()
    torch.manual_seed(0)
    est = uglad_amd.uGLAD_GL()
    est.fit_pairwise(df, eval_offset=OFFSET, k_fold=3, **FIT)
    P = est.precision_
    assert P.shape == (20, 20) and np.isfinite(P).all()
    # by hand: the row folds with their NaN kept, one call per group of one shape, one shared model against the full matrix, consensus
    lib = gpu_lib()
    kw = dict(normalize=True, min_pairs=2, eval_offset=OFFSET, repair=True)
    full = lib.pairwise_covariance(torch.from_numpy(X[None].copy()).cuda(), **kw)
    folds = [X[train] for train, _ in main._kfold_indices(200, 3)]
    assert sorted(len(f) for f in folds) == [133, 133, 134]
    S_K = torch.empty(3, 20, 20, dtype=torch.float32, device="cuda")
    first = lib.pairwise_covariance(torch.from_numpy(np.stack(folds[:2])).cuda(), **kw)
    last = lib.pairwise_covariance(torch.from_numpy(folds[2][None].copy()).cuda(), **kw)
    assert not first.info.any() and not last.info.any() and not full.info.any()
    S_K[:2], S_K[2] = first.S, last.S[0]
    torch.manual_seed(0)
    one = Collective()
    theta, _ = main._train_sharded(S_K, one, 3, 20, 0.002, 0, 15, False, None, loss_Sb=full.S)
    ref = main.get_final_precision_from_batch(theta, type="min", collective=one)
    assert np.array_equal(P, ref[0].cpu().numpy())
    with pytest.raises(ValueError, match="k_fold"):
        est.fit_pairwise(df, k_fold=1, **FIT)
