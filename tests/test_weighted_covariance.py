"""The covariances of one table under R weightings of its rows (uglad_weighted_covariance, csrc/wcov_wide.h; the host formulation in
uglad_amd/utils/prepare_data.py), against the host formulation -- centred directly at every weighted mean -- and, for integer weights,
against numpy's covariance of the materialised resample.  CPU: the host helpers, the unmodified kernel sources on the SIMT emulator, the
Python surface.  GPU: the same checks at the same shapes and a ragged multi-tile call.  Every table column carries an offset of +50, so
that a lost centring shows.

Tolerances, none of them measured on the code under test:
  the matrix      with c the UNWEIGHTED column means and q_i = sum_n w_n (x_ni - c_i)^2, Cauchy-Schwarz bounds both the weighted Gram sum
                  and the centre's product d_i d_j s by sqrt(q_i q_j); either side's dot products err by at most about (N + c) 2^-53 of
                  that:  |device - host| <= 4 (N + 8) 2^-53 sqrt(q_i q_j) / s per entry (test_pairwise_covariance.py's bound with the
                  shifted second moments).  For integer weights the same bound holds against np.cov(np.repeat(X, w, 0), bias=True), N
                  there the materialised row count.
  the mean        |device - host| <= (N + 8) 2^-53 max |x| per entry: a weighted mean of N values of that size.
  fp32            the fp32 output is the float32 rounding of the device's own fp64 matrix, bit for bit.
  min eig         test_covariance_wide.py's min_eig_bound: D (D + 1) 2^-53 tr S + 1.2e-13.
  repaired diag   diag + offset - min eig to that bound, plus the one fp32 rounding of the stored value.
Every repair case asserts that the host's smallest eigenvalue is not within the bound of the threshold, so that a changed seed cannot
flip a decision unnoticed."""
import ctypes

import numpy as np
import pytest
import torch

import buffer_contract as bc
import buffer_contract_cases as cases_
from test_covariance_wide import min_eig_bound
from uglad_amd.utils import prepare_data as pd_

OFFSET = 0.1
_cache = {}


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def table(N, D, seed):
    """Three latent factors plus noise plus 50."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, 3)) @ rng.standard_normal((3, D)) + rng.standard_normal((N, D)) + 50.0


def window(N, centre, width):
    """Real weights: a Gaussian window over the rows."""
    n = np.arange(N, dtype=np.float64)
    return np.exp(-0.5 * ((n - centre) / width) ** 2)


def mixed_weights(N, R, seed):
    """Weighting r is a bootstrap resample (r = 0 mod 3), a half subsample (1) or a Gaussian window (2)."""
    rng = np.random.default_rng(seed)
    W = np.empty((R, N))
    for r in range(R):
        if r % 3 == 0:
            W[r] = pd_.resample_weights(N, 1, "bootstrap", rng=rng)[0]
        elif r % 3 == 1:
            W[r] = pd_.resample_weights(N, 1, "subsample", fraction=0.5, rng=rng)[0]
        else:
            W[r] = window(N, rng.uniform(0, N), N / 4.0)
    return W


# (N, D, R): one MFMA | one ragged tile, two row chunks with a ragged one, a full group and a group of one | two feature tiles with an
# off-diagonal one, five row chunks, a group of two | N < D, three tiles, singular
SHAPES = [(3, 2, 2), (37, 7, 5), (130, 70, 6), (40, 130, 3)]
RAGGED = (70, 200, 9)  # (GPU) four tiles with a ragged last one, three groups with a remainder of one
BY_HAND = (np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 0.0]]), np.array([[1.0, 0.0, 2.0], [1.0, 1.0, 1.0]]))


def shape_inputs(N, D, R):
    key = ("inputs", N, D, R)
    if key not in _cache:
        _cache[key] = frozen(*BY_HAND) if (N, D) == (3, 2) else frozen(table(N, D, 100 * N + D), mixed_weights(N, R, 7 * N + D))
    return _cache[key]


def oracle(X, W):
    """(S (R, D, D), mean (R, D), bound (R, D, D)) of the host formulation, computed once and never modified."""
    key = ("oracle", X.shape, X.tobytes(), W.tobytes())
    if key not in _cache:
        S, mean = pd_.weighted_covariance_host(X, W)
        Z = X - X.mean(axis=0)
        q = W @ (Z * Z)  # (R, D)
        bound = 4.0 * (X.shape[0] + 8) * 2.0 ** -53 * np.sqrt(q[:, :, None] * q[:, None, :]) / W.sum(axis=1)[:, None, None]
        _cache[key] = frozen(S, mean, bound)
    return _cache[key]


def run(lib, X, W, device, **kw):
    """WeightedCovariance of a HipLib call as numpy arrays (None stays None)."""
    out = lib.weighted_covariance(torch.from_numpy(np.array(X, dtype=np.float64)).to(device),
                                  torch.from_numpy(np.array(W, dtype=np.float64)).to(device), **kw)
    if device != "cpu":
        torch.cuda.synchronize()
    return type(out)(*[None if a is None else a.cpu().numpy() for a in out])


def same_bits(a, b):
    return (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes())


ALL = dict(repair=False, want_f64=True, want_mean=True)


# ============================================================================================ the checks, for either device
def check_shape(lib, device, N, D, R):
    X, W = shape_inputs(N, D, R)
    out = run(lib, X, W, device, **ALL)
    again = run(lib, X, W, device, **ALL)
    assert out.min_eig is None and out.info.shape == (R,) and out.info.dtype == np.int32 and not out.info.any()
    assert out.S.shape == (R, D, D) and out.S.dtype == np.float32 and out.S64.dtype == np.float64 and out.mean.shape == (R, D)
    assert all(same_bits(a, b) for a, b in zip(out, again))  # two calls, the same bits
    S, mean, bound = oracle(X, W)
    for r in range(R):
        ratio = float((np.abs(out.S64[r] - S[r]) / bound[r]).max())
        print(f"({N}, {D}, {R}) weighting {r}: |device - host formulation| is {ratio:.3f} of the bound")
        assert ratio <= 1.0
        if (W[r] == np.rint(W[r])).all():  # a resample: numpy's covariance of the materialised table
            w = W[r].astype(np.int64)
            ref = np.cov(np.repeat(X, w, axis=0).T, bias=True).reshape(D, D)
            ratio = float((np.abs(out.S64[r] - ref) / (bound[r] * (w.sum() + 8) / (N + 8))).max())
            print(f"({N}, {D}, {R}) weighting {r}: |device - np.cov of the {w.sum()} materialised rows| is {ratio:.3f} of the bound")
            assert ratio <= 1.0
        assert (np.abs(out.mean[r] - mean[r]) <= (N + 8) * 2.0 ** -53 * np.abs(X).max()).all()
        assert np.array_equal(out.S64[r], out.S64[r].T) and np.array_equal(out.S[r], out.S[r].T)  # the mirror is a copy
        assert np.array_equal(out.S[r], out.S64[r].astype(np.float32))
    if (N, D) == (3, 2):  # by hand: rows {0, 2, 2} and the whole table
        assert np.allclose(out.S64[0], [[32.0 / 9.0, -16.0 / 9.0], [-16.0 / 9.0, 8.0 / 9.0]], rtol=0, atol=1e-14)
        assert np.allclose(out.S64[1], [[8.0 / 3.0, -4.0 / 3.0], [-4.0 / 3.0, 8.0 / 3.0]], rtol=0, atol=1e-14)
        assert np.allclose(out.mean, [[11.0 / 3.0, 2.0 / 3.0], [3.0, 2.0]], rtol=0, atol=1e-14)


def check_independence(lib, device):
    """A weighting's bits do not depend on R, on its place in the call, or on its place in its group."""
    N, D = 37, 7
    X, W = shape_inputs(N, D, 5)
    for r in (0, 1, 2):  # a bootstrap resample, a subsample, a window
        alone = run(lib, X, W[r:r + 1], device, eval_offset=OFFSET, repair=True, want_f64=True, want_mean=True)
        many_W = np.roll(W, 1, axis=0).copy()
        many_W[[0, 3, 4]] = W[r]
        many = run(lib, X, many_W, device, eval_offset=OFFSET, repair=True, want_f64=True, want_mean=True)
        for at in (0, 3, 4):
            assert all(same_bits(a[at], b[0]) for a, b in zip(many, alone)), (r, at)


def flag_cases(N, R):
    """[(weights with one bad weighting, its place, its flag word)]"""
    W = shape_inputs(N, 7, R)[1]
    out = []
    for at, flag, spoil in ((1, 1, lambda w: w.__setitem__(3, -1.0)), (2, 1, lambda w: w.__setitem__(5, np.nan)),
                            (4, 1, lambda w: w.__setitem__(0, np.inf)), (3, 2, lambda w: w.fill(0.0))):
        bad = W.copy()
        spoil(bad[at])
        out.append((bad, at, flag))
    return out


def check_flags(lib, device):
    N, D, R = 37, 7, 5
    X, _ = shape_inputs(N, D, R)
    kw = dict(eval_offset=OFFSET, repair=True, want_f64=True, want_mean=True)
    for W, at, flag in flag_cases(N, R):
        out = run(lib, X, W, device, **kw)
        others = [r for r in range(R) if r != at]
        without = run(lib, X, W[others], device, **kw)
        want = np.zeros(R, dtype=np.int32)
        want[at] = flag
        assert np.array_equal(out.info, want)
        assert np.isnan(out.S[at]).all() and np.isnan(out.S64[at]).all() and np.isnan(out.mean[at]).all() and np.isnan(out.min_eig[at])
        for a, b in zip(out, without):  # the other four have the bits of the call without the flagged one
            assert same_bits(a[others], b)
        assert not np.isnan(out.S[others]).any() and not np.isnan(out.min_eig[others]).any()


def check_repair(lib, device, X, W, expect):
    """expect: per weighting, whether the host repairs it."""
    R, D = W.shape[0], X.shape[1]
    out = run(lib, X, W, device, eval_offset=OFFSET, repair=True, want_f64=True)
    plain = run(lib, X, W, device, repair=False, want_f64=True)
    assert plain.min_eig is None and np.array_equal(plain.S, plain.S64.astype(np.float32))  # without min_eig_out nothing is repaired
    S, _, _ = oracle(X, W)
    for r in range(R):
        eig = float(np.linalg.eigvalsh(S[r])[0])
        tol = min_eig_bound(S[r])
        print(f"({X.shape[0]}, {D}) weighting {r}: host min eig {eig!r}, device {out.min_eig[r]!r}, bound {tol:.2e}")
        assert abs(eig - 1e-6) > tol and (eig <= 1e-6) == expect[r]  # (the decision is not within the bound of the threshold)
        assert same_bits(out.S64[r], plain.S64[r])  # S64 is never repaired
        off = ~np.eye(D, dtype=bool)
        assert np.array_equal(out.S[r][off], plain.S[r][off])  # the repair leaves the off-diagonals alone
        if eig <= 1e-6:
            assert abs(out.min_eig[r] - eig) <= tol
            want = np.diag(S[r]) + OFFSET - eig
            assert (np.abs(np.diag(out.S[r]).astype(np.float64) - want) <= tol + np.spacing(want.astype(np.float32))).all()
        else:
            assert np.isposinf(out.min_eig[r]) and same_bits(out.S[r], plain.S[r])  # passed at 1e-6: never computed, not repaired


def repair_cases():
    """A singular call (N < D: every weighting repaired) and a positive-definite one (every weight positive, or 104 of 130 rows kept)."""
    X, W = shape_inputs(40, 130, 3)
    N = 130
    pd_W = np.stack([np.ones(N), window(N, 50.0, N / 2.0), pd_.resample_weights(N, 1, "subsample", fraction=0.8, rng=3)[0]])
    return [(X, W, [True] * 3), (shape_inputs(130, 70, 6)[0], frozen(pd_W)[0], [False] * 3)]


def bc_weighted(N, D, R, device):
    def make(rng, dev):
        return {"X": cases_._t(table(N, D, 11), dev), "W": cases_._t(mixed_weights(N, R, 13), dev)}

    def call(inp):
        return cases_._lib().weighted_covariance(inp["X"], inp["W"], eval_offset=OFFSET, repair=True, want_f64=True, want_mean=True)._asdict()

    return cases_.Case("weighted_covariance", f"N{N}_D{D}_R{R}", make, call, "repair", device=device)


def bc_frequency(D, R, device):
    def make(rng, dev):
        return {"P": cases_._t(cases_._spd64(rng, R, D).astype(np.float32), dev)}

    def call(inp):
        lib = cases_._lib()
        g = lib.graph_wide(inp["P"], n_keep=max(1, D * (D - 1) // 20), from_precision=True, want_stats=False)
        return {**g._asdict(), **lib.edge_frequency(g, D)._asdict()}

    return cases_.Case("edge_frequency", f"D{D}_R{R}", make, call, exempt={"edge_ij": "graph_wide.edges", "edge_w": "graph_wide.edges"},
                       device=device)


# ============================================================================================ CPU: the host helpers
def test_resample_weights_are_seeded_integer_valued_and_sum_as_their_scheme_says():
    N, R = 37, 6
    boot = pd_.resample_weights(N, R, "bootstrap", rng=5)
    sub = pd_.resample_weights(N, R, "subsample", fraction=0.3, rng=5)
    assert boot.shape == sub.shape == (R, N) and boot.dtype == sub.dtype == np.float64
    assert np.array_equal(boot, np.rint(boot)) and (boot >= 0).all() and (boot.sum(axis=1) == N).all()
    assert set(np.unique(sub)) == {0.0, 1.0} and (sub.sum(axis=1) == int(np.floor(0.3 * N))).all()
    assert np.array_equal(boot, pd_.resample_weights(N, R, "bootstrap", rng=5))
    assert np.array_equal(sub, pd_.resample_weights(N, R, "subsample", fraction=0.3, rng=5))
    assert not np.array_equal(sub, pd_.resample_weights(N, R, "subsample", fraction=0.3, rng=6))
    assert len({w.tobytes() for w in sub}) == R  # the resamples of one call differ
    assert pd_.resample_weights(N, R).sum(axis=1).tolist() == [N // 2] * R  # the default: half subsamples
    with pytest.raises(ValueError, match="scheme"):
        pd_.resample_weights(N, R, "jackknife")
    with pytest.raises(ValueError, match="fraction"):
        pd_.resample_weights(N, R, "subsample", fraction=0.01)


@pytest.mark.parametrize("N,D", [(37, 7), (130, 70), (40, 130)])
def test_host_formulation_is_the_covariance_of_the_materialised_resample(N, D):
    X = table(N, D, 100 * N + D)
    S, mean = pd_.weighted_covariance_host(X, np.ones((1, N)))
    ref = pd_.empirical_covariance(X)
    assert np.abs(S[0] - ref).max() <= 1e-14 * np.abs(ref).max() and np.abs(mean[0] - X.mean(axis=0)).max() <= 1e-14 * 51
    W = mixed_weights(N, 3, 1)
    S, mean, bound = oracle(X, W)
    for r in (0, 1):
        w = W[r].astype(np.int64)
        ref = np.cov(np.repeat(X, w, axis=0).T, bias=True)
        ratio = float((np.abs(S[r] - ref) / (bound[r] * (w.sum() + 8) / (N + 8))).max())
        print(f"({N}, {D}) weighting {r}: |host formulation - np.cov of the materialised rows| is {ratio:.3f} of the bound")
        assert ratio <= 1.0 and np.array_equal(S[r], S[r].T)
    with pytest.raises(ValueError):
        pd_.weighted_covariance_host(X, np.ones((2, N + 1)))


# ============================================================================================ CPU: the kernels on the emulator
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_d%d_r%d" % s)
def test_emulated_shapes_match_the_host_formulation(emul, shape):
    check_shape(emul, "cpu", *shape)


def test_emulated_weighting_does_not_depend_on_its_place(emul):
    check_independence(emul, "cpu")


def test_emulated_flags_stay_with_their_weighting(emul):
    check_flags(emul, "cpu")


@pytest.mark.parametrize("case", [0, 1], ids=["singular_n40_d130", "positive_definite_n130_d70"])
def test_emulated_repair_takes_the_hosts_decision(emul, case):
    check_repair(emul, "cpu", *repair_cases()[case])


def test_emulated_c_entry_error_codes(emul):
    from uglad_amd._lib import UgladError

    size = emul._dll.uglad_weighted_covariance_workspace_floats
    slab = 2 * (2 * 64 * 64 + 3 * 64 + 8)
    assert size(1, 7) == size(1, 64) == slab + 2 * (64 + 2) and size(3, 7) == 3 * size(1, 7)  # the Cholesky slab, d and two words of sums
    assert size(1, 0) == -2 and size(1, emul.max_dim + 1) == -2 and size(0, 7) == -2 and size(65536, 7) == -2 and size(1, emul.max_dim) > 0
    assert size(65535, emul.max_dim) == -2  # beyond 2^31 - 1 floats
    N, D, R = 9, 7, 2
    X, W = torch.from_numpy(table(N, D, 1)), torch.from_numpy(mixed_weights(N, R, 1))
    S, info = torch.empty(R, D, D), torch.empty(R, dtype=torch.int32)
    wsp = torch.empty(size(R, D) + 2, dtype=torch.float32)
    assert wsp.data_ptr() % 8 == 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(X_p=p(X), W_p=p(W), R_=R, N_=N, D_=D, S_p=p(S), info_p=p(info), wsp_p=p(wsp)):
        emul._call("uglad_weighted_covariance", X_p, W_p, R_, N_, D_, 0.1, S_p, None, None, info_p, None, wsp_p)

    call()  # (the arguments are good)
    for bad in (dict(X_p=None), dict(W_p=None), dict(S_p=None), dict(info_p=None), dict(wsp_p=None),
                dict(wsp_p=ctypes.c_void_p(wsp.data_ptr() + 4))):  # NULL, misaligned
        with pytest.raises(UgladError, match="NULL"):
            call(**bad)
    for bad in (dict(D_=0), dict(D_=emul.max_dim + 1), dict(N_=0), dict(R_=0), dict(R_=65536)):
        with pytest.raises(UgladError, match="dimension"):
            call(**bad)
    with pytest.raises(UgladError):
        emul.weighted_covariance(X.float(), W)  # an fp32 table is refused
    with pytest.raises(UgladError, match="rows"):
        emul.weighted_covariance(X, W[:, :-1].contiguous())


def test_emulated_buffer_contract(emul):
    bc.run_case(bc_weighted(37, 7, 5, "cpu"))
    bc.run_case(bc_frequency(7, 5, "cpu"))


def test_emulated_python_surface(emul):
    import pandas as pd

    import uglad_amd

    X, W = shape_inputs(37, 7, 5)
    S, mn, mean = uglad_amd.weighted_covariance(pd.DataFrame(X), W, eval_offset=OFFSET)
    assert S.shape == (5, 7, 7) and S.dtype == torch.float32 and mn.shape == (5,) and mn.dtype == np.float64 and mean.shape == (5, 7)
    host, host_mean, bound = oracle(X, W)
    assert np.isposinf(mn).all() and (np.abs(S.numpy() - host) <= bound + np.spacing(np.abs(host).astype(np.float32))).all()
    plain, none, _ = uglad_amd.weighted_covariance(X, W, repair=False)
    assert none is None and torch.equal(plain, S)
    assert uglad_amd.main.weighted_covariance is uglad_amd.weighted_covariance
    bad = X.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        uglad_amd.weighted_covariance(bad, W)
    with pytest.raises(ValueError, match=r"\(R, N\)"):
        uglad_amd.weighted_covariance(X, W[0])
    zero = W.copy()
    zero[2] = 0.0
    with pytest.warns(RuntimeWarning, match=r"weighting 2 .*the weights sum to zero"):  # a flagged weighting does not raise here: it warns
        S2, mn2, _ = uglad_amd.weighted_covariance(X, zero)
    assert np.isnan(mn2[2]) and torch.isnan(S2[2]).all() and torch.equal(S2[[0, 1, 3, 4]], S[[0, 1, 3, 4]])


# ============================================================================================ GPU
def gpu_lib():
    from uglad_amd import _lib

    return _lib.get_lib()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES + [RAGGED], ids=lambda s: "n%d_d%d_r%d" % s)
def test_gpu_shapes_match_the_host_formulation(shape):
    check_shape(gpu_lib(), "cuda", *shape)


@pytest.mark.gpu
def test_gpu_weighting_does_not_depend_on_its_place():
    check_independence(gpu_lib(), "cuda")


@pytest.mark.gpu
def test_gpu_flags_stay_with_their_weighting():
    check_flags(gpu_lib(), "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1], ids=["singular_n40_d130", "positive_definite_n130_d70"])
def test_gpu_repair_takes_the_hosts_decision(case):
    check_repair(gpu_lib(), "cuda", *repair_cases()[case])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(37, 7, 5), RAGGED], ids=lambda s: "n%d_d%d_r%d" % s)
def test_gpu_buffer_contract(shape):
    gpu_lib()
    bc.run_case(bc_weighted(*shape, "cuda"))
    bc.run_case(bc_frequency(shape[1], shape[2], "cuda"))
