"""Per-sample scores on the device (uglad_sample_scores, csrc/score_wide.h): the squared Mahalanobis distance q = xc^T P xc and the Gaussian
log-density (logdet P - D log 2 pi - q) / 2 of every row under every model, P = (Theta + Theta^T) / 2, xc = x - mu, fp64 throughout; and
what stands on them: main.sample_scores, uGLAD_GL / uGLAD_multitask .mahalanobis / .score_samples / .score with the data_min_ /
data_range_ that fit() now keeps.  CPU: the unmodified kernel sources on the SIMT emulator.  GPU: the same checkers on the device, with
D = 288 and D = 2048 added.  The oracle is the numpy fp64 restatement below.

Tolerances, derived from the arithmetic, none measured on the code under test (EPS = 2^-53):
  q            per row |q - q_ref| <= 4 (D + 2) EPS |xc|^T |P| |xc|      the dot-product bound for about 2 D + 2 roundings on each side
  logdet       <= D^2 c EPS, c = cond(P) computed here by numpy          the rule of tests/test_after_path_wide.py for a sum of D
                                                                         logarithms of pivots; the models built here keep c <= 100
  log-density  half the sum of the two
The built models are random orthogonal bases with the spectrum geomspace(1, 50, D) plus an antisymmetric part of 1e-5 (a converged
precision_ is asymmetric at that level), so the symmetrisation is exercised.  (At D = 1 that is P = 1 exactly: logdet = 0 and D log 2 pi
are exact there, which is what lets the log-density bound -- it has no term for the roundings of the final subtraction -- hold at c = 1.)
The tile edge is 64 and the k chunk 32: the grid below crosses both."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
EPS = 2.0 ** -53
LOG2PI = float(np.log(2.0 * np.pi))


# ============================================================================================ the oracle and the inputs
def oracle(theta, mu, X):
    """fp64 numpy: (q, log-density, logdet, bound of q per row, bound of logdet, bound of the log-density per row, cond(P));
    logdet and the log-density are NaN where P is not positive definite."""
    D = len(mu)
    P = 0.5 * (theta + theta.T)
    Xc = X - mu
    with np.errstate(invalid="ignore"):
        q = ((Xc @ P) * Xc).sum(1)
        scale = ((np.abs(Xc) @ np.abs(P)) * np.abs(Xc)).sum(1)
    pd = np.linalg.eigvalsh(P).min() > 0
    logdet = float(np.linalg.slogdet(P)[1]) if pd else np.nan
    c = float(np.linalg.cond(P))
    b_q = 4.0 * (D + 2) * EPS * scale
    b_det = D * D * c * EPS
    return q, 0.5 * (logdet - D * LOG2PI - q), logdet, b_q, b_det, 0.5 * (b_q + b_det), c


@functools.lru_cache(maxsize=None)
def models(K, D, seed):
    """K precision matrices with the spectrum geomspace(1, 50, D) in random bases, asymmetric at 1e-5, and K locations."""
    rng = np.random.default_rng(seed)
    theta = np.empty((K, D, D))
    for k in range(K):
        Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
        B = rng.standard_normal((D, D))
        theta[k] = (Q * np.geomspace(1.0, 50.0, D)) @ Q.T + 1e-5 * (B - B.T)
    mu = 0.4 + 0.2 * rng.random((K, D))
    theta.setflags(write=False), mu.setflags(write=False)
    return theta, mu


def tables(K, N, D, seed):
    return np.random.default_rng(seed).random((K, N, D))


def run(theta, mu, X, **kw):
    """main.sample_scores on whatever library is installed (the emulator's on the CPU, the device's on the GPU)."""
    from uglad_amd import main

    got = main.sample_scores(theta, mu, X, **kw)
    assert all(np.asarray(a).dtype == np.float64 for a in got)
    return got


def check(got, theta, mu, X, label="", max_cond=100.0):
    """The three outputs of K models against the oracle, every figure printed before it is asserted.  X (K, N, D) or (N, D)."""
    K, D = mu.shape
    if np.ndim(got.logdet) == 0:  # (a single (D, D) model comes back without the batch dimension)
        got = type(got)(got.mahalanobis[None], got.log_density[None], np.array([got.logdet]))
    for k in range(K):
        Xk = X if X.ndim == 2 else X[k]
        q, dens, logdet, b_q, b_det, b_dens, c = oracle(theta[k], mu[k], Xk)
        e_q, e_dens, e_det = np.abs(got.mahalanobis[k] - q), np.abs(got.log_density[k] - dens), abs(got.logdet[k] - logdet)
        print(f"{label}[{k}] D {D} N {len(Xk)} cond {c:.1f}: q {e_q.max():.2e} (bound {b_q[np.argmax(e_q - b_q)]:.2e}), logdet {e_det:.2e} "
              f"(bound {b_det:.2e}), log-density {e_dens.max():.2e} (bound {b_dens[np.argmax(e_dens - b_dens)]:.2e})")
        assert c <= max_cond
        assert got.mahalanobis[k].shape == (len(Xk),) and (e_q <= b_q).all(), (k, e_q.max())
        assert e_det <= b_det, (k, e_det)
        assert (e_dens <= b_dens).all(), (k, e_dens.max())


# ============================================================================================ 1. the shape grid
GRID_D = [1, 2, 25, 63, 64, 65, 130]
GRID_N = [1, 63, 64, 65, 130]


def check_grid(D):
    theta, mu = models(3, D, seed=100 + D)
    for N in GRID_N:
        X = tables(3, N, D, seed=1000 * D + N)
        check(run(theta, mu, X), theta, mu, X, f"K3 n{N}")
        check(run(theta[:1], mu[:1], X[:1]), theta[:1], mu[:1], X[:1], f"K1 n{N}")


def check_one_table_for_every_model(D=65, N=65):
    """x_batch = 1: the table is read once for all three models -- the bits of the same table passed three times."""
    theta, mu = models(3, D, seed=100 + D)
    X = tables(1, N, D, seed=77)
    once, thrice = run(theta, mu, X[0]), run(theta, mu, np.repeat(X, 3, axis=0))
    check(once, theta, mu, X[0], "x_batch 1")
    for a, b in zip(once, thrice):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("D", GRID_D)
def test_emulated_shape_grid(emul, D):
    check_grid(D)


def test_emulated_one_table_for_every_model(emul):
    check_one_table_for_every_model()


@pytest.mark.gpu
@pytest.mark.parametrize("D", GRID_D + [288])
def test_gpu_shape_grid(D):
    check_grid(D)


@pytest.mark.gpu
def test_gpu_one_table_for_every_model():
    check_one_table_for_every_model()


@pytest.mark.gpu
def test_gpu_full_triangle_at_the_largest_dimension():
    """D = 2048, N = 130, K = 2: T = 32 block columns, the full triangle of weighted tiles and 32 partials per row."""
    theta, mu = models(2, 2048, seed=2048)
    X = tables(2, 130, 2048, seed=2049)
    check(run(theta, mu, X), theta, mu, X, "d2048")


# ============================================================================================ 2. numbers the reference made
def check_reference_fit(name):
    """A fit of the reference: mean_n q_n = tr(S Theta) and score = (logdet - D log 2 pi - tr(S Theta)) / 2, S = covariance_."""
    from uglad_amd.utils import prepare_data

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    X = np.array(prepare_data.process_table(g["X"], NORM="min_max", VERBOSE=False))  # as fit() normalises
    theta, mu, S = g["precision_"].astype(np.float64), g["location_"], g["covariance_"]
    D = len(mu)
    got = run(theta, mu, X)
    check(got, theta[None], mu[None], X, name, max_cond=np.inf)  # (the reference's model: its condition number is what it is)
    _, _, logdet, b_q, b_det, b_dens, _ = oracle(theta, mu, X)
    tr = float(np.trace(S @ theta))
    e_tr = abs(got.mahalanobis.mean() - tr)
    e_score = abs(got.log_density.mean() - 0.5 * (logdet - D * LOG2PI - tr))
    print(f"{name}: |mean q - tr(S Theta)| {e_tr:.2e} (bound {b_q.max():.2e}), score {e_score:.2e} (bound {b_dens.max():.2e})")
    assert e_tr <= b_q.max() and e_score <= b_dens.max()


REFERENCE_FITS = ["fit_direct_d25", "fit_direct_d25_converged"]


@pytest.mark.parametrize("name", REFERENCE_FITS)
def test_emulated_reference_fits(emul, name):
    check_reference_fit(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REFERENCE_FITS)
def test_gpu_reference_fits(name):
    check_reference_fit(name)


# ============================================================================================ 3. the bitwise property
def check_bitwise(D=70, N=130):
    theta, mu = models(2, D, seed=100 + D)
    X = tables(2, N, D, seed=31)
    whole = run(theta, mu, X)
    perm = np.random.default_rng(32).permutation(N)
    shuffled = run(theta, mu, X[:, perm])
    assert np.array_equal(shuffled.mahalanobis, whole.mahalanobis[:, perm]) and np.array_equal(shuffled.log_density, whole.log_density[:, perm])
    head = run(theta, mu, X[:, :70])  # another N, another grid
    assert np.array_equal(head.mahalanobis, whole.mahalanobis[:, :70]) and np.array_equal(head.log_density, whole.log_density[:, :70])
    solo = run(theta[1], mu[1], X[1])  # another K, another place in the batch
    assert np.array_equal(solo.mahalanobis, whole.mahalanobis[1]) and np.array_equal(solo.log_density, whole.log_density[1])
    for other in (run(theta, mu, X, row_chunk=64), run(theta, mu, X)):  # chunks of rows; a second run
        for a, b in zip(other, whole):
            assert np.array_equal(a, b)


def test_emulated_bitwise_property(emul):
    check_bitwise()


@pytest.mark.gpu
def test_gpu_bitwise_property():
    check_bitwise()


# ============================================================================================ 4. not positive definite
def check_not_positive_definite(D=65, N=70):
    theta, mu = (np.array(a) for a in models(2, D, seed=100 + D))
    w, Q = np.linalg.eigh(0.5 * (theta[0] + theta[0].T))
    w[D // 2] = -w[D // 2]  # one negative eigenvalue; |P| and the conditioning of q stay as they were
    theta[0] = (Q * w) @ Q.T
    X = tables(2, N, D, seed=41)
    got = run(theta, mu, X)
    q, _, logdet, b_q, _, _, _ = oracle(theta[0], mu[0], X[0])
    assert np.isnan(logdet) and np.isnan(got.logdet[0]) and np.isnan(got.log_density[0]).all()
    e_q = np.abs(got.mahalanobis[0] - q)
    print(f"indefinite model: q {e_q.max():.2e} (bound {b_q[np.argmax(e_q - b_q)]:.2e})")
    assert (e_q <= b_q).all()
    healthy = run(theta[1:], mu[1:], X[1:])
    check(healthy, theta[1:], mu[1:], X[1:], "healthy")
    assert np.array_equal(got.mahalanobis[1], healthy.mahalanobis[0]) and np.array_equal(got.log_density[1], healthy.log_density[0])
    assert got.logdet[1] == healthy.logdet[0]


def test_emulated_not_positive_definite_next_to_a_healthy_model(emul):
    check_not_positive_definite()


@pytest.mark.gpu
def test_gpu_not_positive_definite_next_to_a_healthy_model():
    check_not_positive_definite()


# ============================================================================================ 5. a NaN in one row
def check_nan_row(D=65, N=70, bad=37):
    theta, mu = models(2, D, seed=100 + D)
    X = tables(2, N, D, seed=51)
    clean = run(theta, mu, X)
    X[:, bad, D - 1] = np.nan
    got = run(theta, mu, X)
    rest = np.arange(N) != bad
    assert np.isnan(got.mahalanobis[:, bad]).all() and np.isnan(got.log_density[:, bad]).all()
    assert np.array_equal(got.mahalanobis[:, rest], clean.mahalanobis[:, rest]) and np.array_equal(got.log_density[:, rest], clean.log_density[:, rest])
    assert np.array_equal(got.logdet, clean.logdet)


def test_emulated_nan_stays_in_its_row(emul):
    check_nan_row()


@pytest.mark.gpu
def test_gpu_nan_stays_in_its_row():
    check_nan_row()


# ============================================================================================ 6. the C entry
def check_c_entry(lib, device):
    from uglad_amd._lib import UgladError

    size = lib._dll.uglad_sample_scores_workspace_floats
    DP = lambda D: (D + 63) // 64 * 64  # noqa: E731
    problem = lib._dll.uglad_conditional_mean_wide_workspace_floats
    for K, N, D in ((1, 1, 1), (2, 65, 70), (3, 130, 130)):
        assert size(K, N, D) == K * problem(1, D) + 2 * K * (DP(D) // 64) * DP(N)  # a conditional-mean problem and T partials per row, per model
    assert size(0, 8, 8) == -2 and size(65536, 8, 8) == -2 and size(1, 0, 8) == -2 and size(1, -1, 8) == -2
    assert size(1, 8, 0) == -2 and size(1, 8, lib.max_dim + 1) == -2
    assert size(1, 2 ** 31 - 1, 8) == -2 and size(1, 2 ** 30, 64) == -2  # beyond 2^31 - 1 floats through N
    assert size(1, 2 ** 29, 64) > 0

    K, N, D = 2, 5, 8
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=device)  # noqa: E731
    X, P, m, q, dens, det = z(K, N, D), torch.eye(D, dtype=torch.float64, device=device).repeat(K, 1, 1), z(K, D), z(K, N), z(K, N), z(K)
    wsp = torch.empty(size(K, N, D) + 2, dtype=torch.float32, device=device)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    odd = ctypes.c_void_p(wsp.data_ptr() + (4 if wsp.data_ptr() % 8 == 0 else 8))
    assert odd.value % 8 == 4

    def call(X_=X, xb=K, P_=P, m_=m, q_=q, dens_=dens, det_=det, w=lib._p(wsp), K_=K, N_=N, D_=D):
        lib._call("uglad_sample_scores", vp(X_), xb, vp(P_), vp(m_), vp(q_), vp(dens_), vp(det_), w, K_, N_, D_)

    for kw in (dict(X_=None), dict(P_=None), dict(m_=None), dict(q_=None), dict(w=None), dict(w=odd)):
        with pytest.raises(UgladError, match="NULL"):
            call(**kw)
    for kw in (dict(D_=0), dict(D_=lib.max_dim + 1), dict(N_=0), dict(K_=0), dict(xb=0), dict(xb=3), dict(xb=K + 1)):
        with pytest.raises(UgladError, match="dimension"):
            call(**kw)
    X[:] = 1.0
    call(dens_=None, det_=None)  # neither: the factorisation is skipped
    call(dens_=None)
    call(det_=None)
    call(xb=1)
    if device != "cpu":
        torch.cuda.synchronize()
    assert torch.equal(q, torch.full((K, N), float(D), dtype=torch.float64, device=device)) and torch.equal(det, z(K))
    assert torch.equal(dens, torch.full((K, N), 0.5 * (0.0 - D * 1.8378770664093453 - D), dtype=torch.float64, device=device))
    with pytest.raises(UgladError):  # fp32 belongs elsewhere
        lib.sample_scores(X.float(), P, m)
    with pytest.raises(UgladError):
        lib.sample_scores(X[:, :, :4].contiguous(), P, m)
    q2, dens2, det2 = lib.sample_scores(X, P, m, want_density=False)
    assert dens2 is None and det2 is None and torch.equal(q2, q)


def test_emulated_c_entry_error_codes_and_workspace_sizes(emul):
    check_c_entry(emul, "cpu")


@pytest.mark.gpu
def test_gpu_c_entry_error_codes_and_workspace_sizes():
    from uglad_amd import _lib

    check_c_entry(_lib.get_lib(), "cuda")


# ============================================================================================ 7. the estimators
def raw_table(N=40, D=5, seed=7, shift=0.0):
    """A table in units of its own: columns of different offsets and scales, one constant column (which process_table drops)."""
    rng = np.random.default_rng(seed)
    L = np.tril(rng.standard_normal((D, D))) * 0.4 + np.eye(D)
    X = rng.standard_normal((N, D)) @ L.T * np.array([1.0, 20.0, 0.3, 5.0, 100.0])[:D] + np.array([0.0, -50.0, 3.0, 10.0, 1e3])[:D] + shift
    return np.insert(X, 2, 4.25, axis=1)


def check_estimator(tmp_path):
    import uglad_amd
    from uglad_amd import main
    from uglad_amd.utils import prepare_data

    raw = raw_table()
    kept = np.delete(raw, 2, axis=1)  # the D columns fit() keeps
    est = uglad_amd.uGLAD_GL()
    for call in (est.mahalanobis, est.score_samples, est.score):
        with pytest.raises(ValueError, match=r"call fit\(\) first"):
            call(kept)
    torch.manual_seed(0)
    est.fit(raw, epochs=2, L=2, verbose=False, mode="direct")
    D = 5
    assert est.precision_.shape == (D, D) and est.data_min_.shape == est.data_range_.shape == (D,)
    assert est.data_min_.dtype == est.data_range_.dtype == np.float64
    normalised = np.array(prepare_data.process_table(raw, NORM="min_max", VERBOSE=False))
    assert np.array_equal((kept - est.data_min_) / est.data_range_, normalised)  # bit for bit
    assert np.array_equal(est.data_min_, kept.min(0)) and np.array_equal(est.data_range_, kept.max(0) - kept.min(0))

    direct = main.sample_scores(est.precision_, est.location_, normalised)
    assert direct.mahalanobis.shape == (40,) and np.ndim(direct.logdet) == 0
    assert np.array_equal(est.score_samples(kept), direct.log_density) and np.array_equal(est.mahalanobis(kept), direct.mahalanobis)
    assert np.array_equal(est.score_samples(normalised, normalized=True), direct.log_density)
    assert est.score(kept) == float(np.mean(est.score_samples(kept)))
    # new rows, outside the training range: no row is dropped, nothing is re-normalised by the new table's own range
    fresh = np.delete(raw_table(N=7, seed=8, shift=2.0), 2, axis=1)
    fresh[3] = 0.0  # (process_table would drop an all-zero row)
    assert np.array_equal(est.score_samples(fresh), main.sample_scores(est.precision_, est.location_, (fresh - est.data_min_) / est.data_range_).log_density)
    fresh[5, 1] = np.nan
    holed = est.score_samples(fresh)
    assert np.isnan(holed[5]) and np.isfinite(np.delete(holed, 5)).all() and np.isnan(est.mahalanobis(fresh)[5])
    for bad in (raw, kept[:, :4], kept[0]):  # the dropped column still there; a column short; one dimension
        with pytest.raises(ValueError):
            est.score_samples(bad)
    with pytest.raises(ValueError, match="max_dim"):
        n = main._lib.get_lib().max_dim + 1
        main.sample_scores(np.broadcast_to(np.float64(0.0), (n, n)), np.zeros(n), np.zeros((1, n)))

    # sklearn where it imports: an extra cross-check, never the binding one
    try:
        from sklearn.covariance import EmpiricalCovariance
    except ImportError:
        EmpiricalCovariance = None
    if EmpiricalCovariance is not None:
        sk = EmpiricalCovariance()
        P = 0.5 * (est.precision_.astype(np.float64) + est.precision_.astype(np.float64).T)
        sk.location_, sk.precision_, sk.covariance_ = est.location_, P, np.linalg.inv(P)
        np.testing.assert_allclose(est.mahalanobis(kept), sk.mahalanobis(normalised), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(est.score(kept), sk.score(normalised), rtol=1e-10, atol=1e-12)

    # save / load: the new attributes travel through __dict__
    path = str(tmp_path / "model.pkl")
    uglad_amd.save_uGLAD_model(est, path)
    back = uglad_amd.load_uGLAD_model(path)
    assert np.array_equal(back.data_min_, est.data_min_) and np.array_equal(back.data_range_, est.data_range_)
    assert np.array_equal(back.score_samples(kept), est.score_samples(kept)) and np.array_equal(back.mahalanobis(kept), est.mahalanobis(kept))

    # after fit_mixed the location holds NaN for the categorical columns: the estimator says why it cannot score
    import pandas as pd

    rng = np.random.default_rng(9)
    df = pd.DataFrame({"a": rng.standard_normal(40), "b": rng.integers(0, 3, 40), "c": rng.standard_normal(40), "d": rng.integers(0, 2, 40)})
    mixed = uglad_amd.uGLAD_GL()
    mixed.fit_mixed(df, {"a": "r", "b": "c", "c": "r", "d": "c"}, epochs=1, L=2, verbose=False)
    assert np.isnan(mixed.location_).sum() == 2 and mixed.data_min_ is None and mixed.data_range_ is None
    for call in (mixed.mahalanobis, mixed.score_samples, mixed.score):
        with pytest.raises(ValueError, match="fit_mixed"):
            call(df.to_numpy(dtype=np.float64))


def check_multitask(tmp_path):
    import uglad_amd
    from uglad_amd import main

    raws = [raw_table(seed=11), raw_table(seed=12, shift=5.0)]
    kept = [np.delete(r, 2, axis=1) for r in raws]
    est = uglad_amd.uGLAD_multitask()
    with pytest.raises(ValueError, match=r"call fit\(\) first"):
        est.score_samples(kept[0])
    torch.manual_seed(0)
    est.fit(raws, epochs=2, L=2, verbose=False)
    K, D, N = 2, 5, 40
    assert est.location_.shape == est.data_min_.shape == est.data_range_.shape == (K, D)
    for k in range(K):
        assert np.array_equal(est.data_min_[k], kept[k].min(0)) and np.array_equal(est.data_range_[k], kept[k].max(0) - kept[k].min(0))
    one = est.score_samples(kept[0])  # one table: every task maps it with its own range
    assert one.shape == (K, N) and est.mahalanobis(kept[0]).shape == (K, N) and np.argmax(one, axis=0).shape == (N,)
    for k in range(K):
        ref = main.sample_scores(est.precision_[k], est.location_[k], (kept[0] - est.data_min_[k]) / est.data_range_[k])
        assert np.array_equal(one[k], ref.log_density) and np.array_equal(est.mahalanobis(kept[0])[k], ref.mahalanobis)
    pairs = est.score_samples(kept)  # K tables: pairwise
    assert pairs.shape == (K, N) and np.array_equal(pairs[0], one[0])
    assert np.array_equal(pairs[1], main.sample_scores(est.precision_[1], est.location_[1], (kept[1] - est.data_min_[1]) / est.data_range_[1]).log_density)
    ragged = est.score_samples([kept[0], kept[1][:13]])  # of different lengths: a list
    assert np.array_equal(ragged[0], pairs[0]) and np.array_equal(ragged[1], pairs[1][:13])
    assert np.array_equal(est.score(kept), pairs.mean(axis=1))
    with pytest.raises(ValueError):
        est.score_samples([kept[0]] * 3)
    path = str(tmp_path / "multitask.pkl")
    uglad_amd.save_uGLAD_model(est, path)
    back = uglad_amd.load_uGLAD_model(path)
    assert isinstance(back, uglad_amd.uGLAD_multitask) and np.array_equal(back.score_samples(kept[0]), one)


def test_emulated_estimator_surface(emul, tmp_path):
    check_estimator(tmp_path)


def test_emulated_multitask_surface(emul, tmp_path):
    check_multitask(tmp_path)


@pytest.mark.gpu
def test_gpu_estimator_surface(tmp_path):
    check_estimator(tmp_path)


@pytest.mark.gpu
def test_gpu_multitask_surface(tmp_path):
    check_multitask(tmp_path)
