"""Edge frequencies over R recovered graphs (uglad_edge_frequency, csrc/graph_wide.h; after.edge_frequency) against a numpy recount from
recovered_graph run on every matrix separately -- integers, compared exactly --, and uGLAD_GL.fit_stability.  CPU: the unmodified kernel
sources on the SIMT emulator.  GPU: the same checks, and the fit."""
import numpy as np
import pytest
import torch

import buffer_contract_cases as cases_

_cache = {}


def precisions(D, R):
    """R seeded symmetric positive-definite matrices, float32."""
    if (D, R) not in _cache:
        P = cases_._spd64(np.random.default_rng(1000 * D + R), R, D).astype(np.float32)
        P.setflags(write=False)
        _cache[(D, R)] = P
    return _cache[(D, R)]


def recount(P, sparsity):
    """(count (D, D), positive (D, D), totals) from one recovered_graph call per matrix, in Python integers."""
    import uglad_amd

    R, D, _ = P.shape
    count, positive = np.zeros((D, D), dtype=np.int64), np.zeros((D, D), dtype=np.int64)
    for r in range(R):
        g = uglad_amd.recovered_graph(P[r], sparsity=sparsity, stats=False)
        i, j = g.edges[:, 0], g.edges[:, 1]
        assert (i < j).all()
        count[i, j] += 1
        count[j, i] += 1
        pos = g.weights > 0
        positive[i[pos], j[pos]] += 1
        positive[j[pos], i[pos]] += 1
    upper = [int(c) for c in count[np.triu_indices(D, 1)]]
    return count, positive, [sum(upper), sum(c * (R - c) for c in upper)]


def device_counts(lib, P, sparsity, device):
    from uglad_amd import after

    D = P.shape[-1]
    g = lib.graph_wide(torch.from_numpy(P.copy()).to(device), n_keep=after._n_keep(sparsity, D), from_precision=True, want_stats=False)
    out = lib.edge_frequency(g, D)
    if device != "cpu":
        torch.cuda.synchronize()
    return [a.cpu().numpy() for a in out]


def check_counts(lib, device, D, sparsity, R=4):
    from uglad_amd import after

    P = precisions(D, R)
    count, positive, totals = device_counts(lib, P, sparsity, device)
    again = device_counts(lib, P, sparsity, device)
    want_count, want_positive, want_totals = recount(P, sparsity)
    assert count.dtype == positive.dtype == np.int32 and totals.dtype == np.int64 and count.shape == positive.shape == (D, D)
    assert np.array_equal(count, want_count) and np.array_equal(positive, want_positive) and totals.tolist() == want_totals
    assert want_totals[0] > 0 and 0 < positive.sum() < count.sum()  # (there are edges, and both signs occur)
    assert not np.diag(count).any() and not np.diag(positive).any() and np.array_equal(count, count.T) and np.array_equal(positive, positive.T)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((count, positive, totals), again))  # two calls, the same bits
    E = D * (D - 1) // 2
    freq, sign, instability = after.edge_frequency(P, sparsity=sparsity)
    assert freq.dtype == np.float64 and np.array_equal(freq, want_count / R) and np.array_equal(sign, want_positive / R)
    assert instability == 2 * want_totals[1] / (R * R * E) and 0 < instability <= 0.5
    # R identical matrices: every edge in all of them or in none, no instability at all
    same = np.repeat(P[:1], R, axis=0)
    count, positive, totals = device_counts(lib, same, sparsity, device)
    assert set(np.unique(count)) == {0, R} and totals.tolist() == [R * int((np.triu(count, 1) == R).sum()), 0]
    assert after.edge_frequency(same, sparsity=sparsity)[2] == 0.0


SIZES = [(5, 0.3), (70, 0.1)]  # one row block | two tiles of the plane, ten blocks of 256 edges


@pytest.mark.parametrize("D,sparsity", SIZES, ids=["d5", "d70"])
def test_emulated_edge_counts_are_the_recount(emul, D, sparsity):
    check_counts(emul, "cpu", D, sparsity)


def test_emulated_c_entry_error_codes(emul):
    import ctypes

    from uglad_amd._lib import UgladError

    D, R = 5, 2
    g = emul.graph_wide(torch.from_numpy(precisions(D, 4)[:R].copy()), n_keep=3, want_stats=False)
    count, positive, totals = torch.empty(D, D, dtype=torch.int32), torch.empty(D, D, dtype=torch.int32), torch.empty(2, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(c_p=p(g.edge_count), ij_p=p(g.edge_ij), w_p=p(g.edge_w), R_=R, D_=D, count_p=p(count), pos_p=p(positive), tot_p=p(totals)):
        emul._call("uglad_edge_frequency", c_p, ij_p, w_p, R_, D_, count_p, pos_p, tot_p)

    call()  # (the arguments are good)
    assert int(totals[0]) == int(g.edge_count.sum()) > 0
    for bad in ("c_p", "ij_p", "w_p", "count_p", "pos_p", "tot_p"):
        with pytest.raises(UgladError, match="NULL"):
            call(**{bad: None})
    for bad in (dict(D_=1), dict(D_=emul.max_dim + 1), dict(R_=0), dict(R_=65536)):
        with pytest.raises(UgladError, match="dimension"):
            call(**bad)
    with pytest.raises(UgladError, match="edge lists"):
        emul.edge_frequency(g, D + 1)


def test_stable_edges_sorts_by_frequency_then_index():
    import uglad_amd

    est = uglad_amd.uGLAD_GL()
    with pytest.raises(ValueError, match="fit_stability"):
        est.stable_edges()
    f = np.zeros((4, 4))
    for (i, j), v in {(0, 1): 0.5, (0, 3): 1.0, (1, 2): 1.0, (2, 3): 0.25}.items():
        f[i, j] = f[j, i] = v
    est.edge_frequency_ = f
    assert est.stable_edges() == [(0, 3, 1.0), (1, 2, 1.0)]
    assert est.stable_edges(0.5) == [(0, 3, 1.0), (1, 2, 1.0), (0, 1, 0.5)]
    assert est.stable_edges(0.0) == [(0, 3, 1.0), (1, 2, 1.0), (0, 1, 0.5), (2, 3, 0.25)]  # an edge no resample holds is no edge


# ============================================================================================ GPU
def gpu_lib():
    from uglad_amd import _lib

    return _lib.get_lib()


@pytest.mark.gpu
@pytest.mark.parametrize("D,sparsity", SIZES, ids=["d5", "d70"])
def test_gpu_edge_counts_are_the_recount(D, sparsity):
    check_counts(gpu_lib(), "cuda", D, sparsity)


FIT = dict(n_resamples=6, epochs=20, L=15, verbose=False)


@pytest.mark.gpu
def test_gpu_fit_stability(tmp_path):
    import uglad_amd
    from uglad_amd import main
    from uglad_amd.utils import prepare_data as pd_

    D, N, R = 20, 200, 6
    Xb, true_theta = pd_.get_data(D, [0.1, 0.2], N, rng=2020)
    X = Xb[0]
    torch.manual_seed(0)
    est = uglad_amd.uGLAD_GL()
    est.fit_stability(X, seed=3, true_theta=true_theta[0], **FIT)
    assert est.precision_.shape == (D, D) and est.precision_resamples_.shape == (R, D, D) and np.isfinite(est.precision_resamples_).all()
    assert est.edge_frequency_.shape == est.edge_sign_frequency_.shape == (D, D) and est.edge_frequency_.dtype == np.float64
    assert est.resample_weights_.shape == (R, N) and est.resample_min_eig_.shape == (R,) and est.covariance_.shape == (D, D)
    assert np.array_equal(est.resample_weights_, pd_.resample_weights(N, R, "subsample", 0.5, rng=3))
    f = est.edge_frequency_
    assert (f >= 0).all() and (f <= 1).all() and np.array_equal(f, f.T) and not np.diag(f).any()
    assert (est.edge_sign_frequency_ <= f).all()
    count, positive, totals = recount(est.precision_resamples_, 0.1)
    assert np.array_equal(f, count / R) and np.array_equal(est.edge_sign_frequency_, positive / R)
    assert est.instability_ == 2 * totals[1] / (R * R * (D * (D - 1) // 2))
    listed = est.stable_edges(0.0)
    i, j = np.triu_indices(D, 1)
    assert sorted((a, b) for a, b, _ in listed) == sorted(zip(i[count[i, j] > 0].tolist(), j[count[i, j] > 0].tolist()))
    assert all(v == f[a, b] for a, b, v in listed) and [v for _, _, v in listed] == sorted((v for _, _, v in listed), reverse=True)
    assert all(v >= 0.8 for _, _, v in est.stable_edges()) and len(est.stable_edges()) <= len(listed)
    # the same seed, the same bits; another seed, other resamples
    torch.manual_seed(0)
    again = uglad_amd.uGLAD_GL()
    again.fit_stability(X, seed=3, **FIT)
    assert np.array_equal(again.precision_, est.precision_) and np.array_equal(again.precision_resamples_, est.precision_resamples_)
    assert np.array_equal(again.edge_frequency_, f) and again.instability_ == est.instability_
    torch.manual_seed(0)
    other = uglad_amd.uGLAD_GL()
    other.fit_stability(X, seed=4, scheme="bootstrap", **FIT)
    assert not np.array_equal(other.resample_weights_, est.resample_weights_) and (other.resample_weights_.sum(axis=1) == N).all()
    # afterwards: what a fit leaves works
    assert est.predict(X).shape == (D, D) and est.recovered_graph().edges.shape[1] == 2
    assert est.mahalanobis(X).shape == (N,) and np.isfinite(est.score(X)) and np.isfinite(est.cond_max_)
    assert est.node_names_ == [f"node_{k}" for k in range(D)] and est.location_.shape == (D,)
    main.save_uGLAD_model(est, str(tmp_path / "stability"))
    back = main.load_uGLAD_model(str(tmp_path / "stability"))
    assert np.array_equal(back.precision_, est.precision_) and np.array_equal(back.edge_frequency_, f)
    assert back.instability_ == est.instability_ and back.stable_edges(0.5) == est.stable_edges(0.5)
    assert np.array_equal(back.predict(X), est.predict(X))
