"""The support-recovery metrics for every D the cell covers (uglad_support_metrics_wide, csrc/metrics_wide.h): the edges of every pair sorted by
score on the device, the ranking metrics as prefix counts over the sorted keys.  CPU: the unmodified kernel sources on the SIMT emulator (the
entry point takes every 2 <= D <= max_dim) against a fp64 numpy checker, which is itself pinned against oracle.after_path.support_metrics (an
O(T E) loop: small cases only) wherever the case is small.  GPU: a golden made by the real reference's report_metrics_all
(tests/golden/make_widemetrics_goldens.py), the oracle, the checker at D = 2048, batch independence and fit().

The sort works on tiles of 2048 keys per workgroup (256 threads x 8 keys); E = D (D - 1) / 2 is no multiple of it for any D used here.

Tolerance: the entries FDR ... Fbeta (0-8) and auc (10) come from integer counts through identical IEEE operations: bit-equal (NaN == NaN).
aupr sums T non-negative quotients, each side in its own order: such a sum carries a relative error <= (T - 1) 2^-53 plus 2^-53 for the
quotient, so two of them differ by at most max(T, 1) 2^-52, relative, no absolute term."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import after_path as oap

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TILE = 2048


def checker(true_theta, pred_theta, beta=1):
    """The 11 numbers of oap.support_metrics from np.unique over the scores, cumulative counts and exact integers: O(E log E)."""
    T, G = np.asarray(true_theta), np.asarray(pred_theta)
    iu = np.triu_indices(G.shape[-1], 1)
    t, p, s = T[iu] != 0, G[iu] != 0, np.abs(G[iu])
    E, nT, nP, TP = t.size, int(t.sum()), int(p.sum()), int((t & p).sum())
    nF, FP, FN = E - nT, nP - TP, nT - TP
    _, inv = np.unique(s, return_inverse=True)  # (ascending distinct scores)
    inv = inv.reshape(-1)
    pos, neg = np.bincount(inv[t], minlength=inv.max() + 1).astype(np.int64), np.bincount(inv[~t], minlength=inv.max() + 1).astype(np.int64)
    neg_below, pos_ge, all_ge = np.cumsum(neg) - neg, nT - (np.cumsum(pos) - pos), E - (np.cumsum(pos + neg) - (pos + neg))
    mw2 = int(np.sum(pos * (2 * neg_below + neg)))
    ap = float(np.sum(pos * (pos_ge.astype(np.float64) / all_ge.astype(np.float64))))
    b2 = float(beta) ** 2
    f = np.float64
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([f(FP) / f(nP), f(TP) / f(nT), f(FP) / f(nF), f(FP + FN), f(nT), f(nP), f(TP) / f(TP + FP), f(TP) / f(TP + FN),
                         f((1 + b2) * TP) / f((1 + b2) * TP + b2 * FN + FP),
                         ap / nT if nT > 0 and nF > 0 else np.nan, mw2 / (2.0 * nT * nF) if nT > 0 and nF > 0 else np.nan])


def assert_metrics(got, ref, label=""):
    n_true = max(float(ref[4]), 1.0)
    err = abs(got[9] - ref[9]) / abs(ref[9]) if np.isfinite(ref[9]) and ref[9] != 0 else 0.0
    print(f"{label}: T {int(ref[4])} P {int(ref[5])} auc {got[10]!r} aupr {got[9]!r} (relative error {err:.2e}, bound {n_true * 2.0 ** -52:.2e})")
    keep = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10]
    np.testing.assert_array_equal(got[keep], ref[keep], err_msg=label)
    np.testing.assert_allclose(got[9], ref[9], rtol=n_true * 2.0 ** -52, atol=0, equal_nan=True, err_msg=label)


def reference(T, G, small=True):
    """The checker's numbers per pair; on small cases the checker is pinned against the oracle's loop first."""
    out = []
    for k in range(len(T)):
        ref = checker(T[k], G[k])
        if small:
            assert_metrics(ref, oap.support_metrics(T[k], G[k]), f"checker vs oracle [{k}]")
        out.append(ref)
    return np.array(out)


def pairs(K, D, seed, density=0.2, decimals=1, keep=0.5):
    """K (true, predicted) pairs, different per pair: tied scores (rounded to `decimals`), exact zeros, both labels in the tie groups."""
    rng = np.random.default_rng(seed)
    T, G = np.zeros((K, D, D), dtype=np.float32), np.zeros((K, D, D), dtype=np.float32)
    for k in range(K):
        t = np.triu(rng.random((D, D)) < density * (1.0 + 0.5 * k / K), 1)
        T[k] = (t + t.T) * rng.standard_normal((D, D)) + np.eye(D)
        s = np.triu(np.round(rng.random((D, D)), decimals) * (rng.random((D, D)) < keep), 1)
        G[k] = s + s.T + np.eye(D)
    return T, G


def run_wide(lib, T, G, device="cpu", **kw):
    out = lib.support_metrics_wide(torch.from_numpy(T).to(device), torch.from_numpy(G).to(device), **kw)
    if device != "cpu":
        torch.cuda.synchronize()
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(T), 11)
    return out.cpu().numpy()


def check(lib, T, G, device="cpu", small=True, label=""):
    got, ref = run_wide(lib, T, G, device), reference(T, G, small)
    for k in range(len(T)):
        assert_metrics(got[k], ref[k], f"{label}[{k}]")
    return got


# ============================================================================================ CPU: the kernels on the emulator
def test_emulated_batch_stride_ragged_tail_and_ties(emul):
    """(K = 2, D = 92): E = 4186 = 2 tiles of 2048 and a ragged one of 90: three workgroups per pass.  Scores rounded to one decimal: eleven
    tie groups that hold both labels, the group of exact zeros spans a tile boundary."""
    T, G = pairs(2, 92, seed=71)
    assert (92 * 91 // 2) % TILE != 0 and -(-(92 * 91 // 2) // TILE) == 3
    got = check(emul, T, G, label="d92")
    assert not np.array_equal(got[0], got[1]) and np.isfinite(got).all()


def test_emulated_every_radix_digit_decides_an_order(emul):
    """Scores from 1e-30 to 1e30 (every exponent digit), pairs one unit in the last place apart (the lowest digit), one fp32 denormal (non-zero:
    predicted, whatever the flush mode) and one -0.0 (zero: not predicted)."""
    D = 92
    rng = np.random.default_rng(72)
    T, _ = pairs(1, D, seed=73)
    s = (10.0 ** rng.uniform(-30, 30, size=(D, D))).astype(np.float32)
    s[:, 1::2] = np.nextafter(s[:, 0:-1:2], np.float32(np.inf))  # neighbours in a row: one ulp apart
    s = np.triu(s * np.where(rng.random((D, D)) < 0.5, 1, -1).astype(np.float32), 1)
    s[0, 1] = np.float32(1e-41)
    s[0, 2] = np.float32(-0.0)
    s[1, 2] = -np.float32(1e-41)
    assert s[0, 1] != 0 and abs(s[0, 1]) < np.finfo(np.float32).tiny and np.signbit(s[0, 2])
    G = (s + s.T + np.eye(D, dtype=np.float32))[None]
    T[0, 0, 1] = T[0, 1, 0] = 1.0  # the denormals: one true edge, one false
    T[0, 1, 2] = T[0, 2, 1] = 0.0
    iu = np.triu_indices(D, 1)
    bits = np.abs(G[0][iu]).view(np.uint32).astype(np.uint64) << np.uint64(1)
    for digit in range(8):  # some pair of keys differs in this digit and agrees in every higher one
        hi = np.unique(bits >> np.uint64(4 * digit))
        assert len(np.unique(hi >> np.uint64(4))) < len(hi), digit
    got = check(emul, T, G, label="digits")
    assert got[0][5] == np.count_nonzero(G[0][iu]) == D * (D - 1) // 2 - 1  # the denormals count as predicted, -0.0 does not


@pytest.mark.parametrize("D", [37, 70])
def test_emulated_edge_cases(emul, D):
    """The cases of test_after_path._check_metrics_edges and one more: every edge true (F = 0)."""
    T, G = pairs(6, D, seed=D)
    G[1] = np.eye(D)   # nothing predicted: FDR, precision = 0 / 0
    G[2] = 1.0         # everything predicted with ONE score: AUC = 1 / 2
    T[3] = np.eye(D)   # no true edge: the ranking metrics are undefined
    T[4] = 1.0         # every edge true: no false edge, the ranking metrics are undefined
    got = check(emul, T, G, label=f"edges d{D}")
    assert np.isnan(got[1][0]) and np.isnan(got[1][6]) and got[2][10] == 0.5
    assert np.isnan(got[3][9]) and np.isnan(got[3][10]) and np.isnan(got[4][9]) and np.isnan(got[4][10]) and got[4][4] == D * (D - 1) // 2


@pytest.mark.parametrize("D", [2, 3, 37])
def test_emulated_takes_every_size_from_two(emul, D):
    """D = 2: one edge; D below the 64 x 64 tile of the key kernel."""
    T, G = pairs(4, D, seed=80 + D, density=0.5)
    check(emul, T, G, label=f"d{D}")


@pytest.mark.parametrize("D", [37, 130])
def test_emulated_agrees_with_the_one_workgroup_kernel(emul, D):
    """Where both entry points exist: bit-equal but for aupr (the order of its T terms)."""
    T, G = pairs(2, D, seed=90 + D)
    small = emul.support_metrics(torch.from_numpy(T), torch.from_numpy(G)).numpy()
    wide = run_wide(emul, T, G)
    for k in range(2):
        assert_metrics(wide[k], small[k], f"wide vs one workgroup d{D}[{k}]")
    wide2 = run_wide(emul, T, G, beta=2)
    small2 = emul.support_metrics(torch.from_numpy(T), torch.from_numpy(G), beta=2).numpy()
    assert np.array_equal(wide2[:, 8], small2[:, 8]) and not np.array_equal(wide2[:, 8], wide[:, 8])


def test_emulated_pair_does_not_depend_on_its_batch(emul):
    T, G = pairs(3, 92, seed=74)
    G[2, 0, 5] = G[2, 5, 0] = np.float32("nan")  # a neighbour with a NaN score: terminates, the others are untouched
    batch = run_wide(emul, T, G)
    solo = run_wide(emul, T[1:2], G[1:2])
    assert np.array_equal(batch[1], solo[0])
    assert_metrics(batch[1], checker(T[1], G[1]), "pair 1")


def test_emulated_argument_errors(emul):
    from uglad_amd._lib import UgladError

    with pytest.raises(UgladError):  # fp64 input
        emul.support_metrics_wide(torch.zeros(1, 8, 8, dtype=torch.float64), torch.zeros(1, 8, 8))
    with pytest.raises(UgladError):
        emul.support_metrics_wide(torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, dtype=torch.float64))
    with pytest.raises(UgladError):  # shapes
        emul.support_metrics_wide(torch.zeros(1, 8, 8), torch.zeros(2, 8, 8))
    D = emul.max_dim + 1
    with pytest.raises(UgladError, match="dimension"):
        emul.support_metrics_wide(torch.empty(1, D, D), torch.empty(1, D, D))
    with pytest.raises(UgladError, match="dimension"):
        emul.support_metrics_wide(torch.zeros(1, 1, 1), torch.zeros(1, 1, 1))
    size = emul._dll.uglad_support_metrics_wide_workspace_floats
    assert size(0, 8) < 0 and size(1, 0) < 0 and size(1, 1) < 0 and size(1, emul.max_dim + 1) < 0 and size(65536, 8) < 0 and size(-1, -1) < 0
    assert size(1024, emul.max_dim) < 0  # beyond 2^31 - 1 floats
    assert size(1, 2) > 0 and size(1, emul.max_dim) > 2 * (emul.max_dim * (emul.max_dim - 1) // 2) and size(2, 70) == 2 * size(1, 70)
    assert size(1, 70) % 2 == 0
    t, p = torch.zeros(1, 8, 8), torch.zeros(1, 8, 8)
    out = torch.zeros(1, 11, dtype=torch.float64)
    wsp = torch.empty(size(1, 8) + 2, dtype=torch.float32)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    odd = ctypes.c_void_p(wsp.data_ptr() + (4 if wsp.data_ptr() % 8 == 0 else 8))  # 4 mod 8: a float's alignment, not a double's
    assert odd.value % 8 == 4
    for bad_wsp in (None, odd):  # missing / misaligned workspace
        with pytest.raises(UgladError, match="NULL"):
            emul._call("uglad_support_metrics_wide", vp(t), vp(p), vp(out), bad_wsp, 1, 8, 1)
    for args in ((None, vp(p), vp(out)), (vp(t), None, vp(out)), (vp(t), vp(p), None)):
        with pytest.raises(UgladError, match="NULL"):
            emul._call("uglad_support_metrics_wide", *args, emul._p(wsp), 1, 8, 1)
    for K, D in ((0, 8), (1, 1), (1, emul.max_dim + 1)):
        with pytest.raises(UgladError, match="dimension"):
            emul._call("uglad_support_metrics_wide", vp(t), vp(p), vp(out), emul._p(wsp), K, D, 1)


def no_host(*a, **k):
    raise AssertionError("the host formulation ran for a D the device covers")


def test_emulated_routing_needs_no_host(emul, monkeypatch):
    """main's routing (the library's eigensolver limit lowered so that D = 70 counts as wide): the report stays on the device."""
    from uglad_amd import main

    monkeypatch.setattr("uglad_amd.after.report_metrics_all", no_host)
    monkeypatch.setattr(emul, "max_eig_dim", 32)
    T, G = pairs(2, 70, seed=75)
    got = main.device_report_metrics(T, G)
    ref = reference(T, G)
    assert len(got) == 2
    for k in range(2):
        assert tuple(got[k]) == oap.METRIC_KEYS
        np.testing.assert_array_equal(np.array([got[k][key] for key in oap.METRIC_KEYS]), np.array([round(float(x), 3) for x in ref[k]]))
    one = main.device_report_metrics(T[0], G[0])  # a single pair
    assert one == got[:1]
    # the smaller sizes keep the one-workgroup kernel
    monkeypatch.setattr(emul, "support_metrics_wide", no_host)
    T, G = pairs(1, 20, seed=76)
    assert tuple(main.device_report_metrics(T, G)[0]) == oap.METRIC_KEYS


# ============================================================================================ the golden of the real reference
@functools.lru_cache(maxsize=None)
def load_golden():
    path = os.path.join(GOLDEN, "widemetrics_k2_d288.npz")
    assert os.path.getsize(path) < 1 << 20
    g = np.load(path)
    return g["true_theta"], g["pred_theta"], g["metrics"]


def _check_golden():
    """Exact equality of the reference's 3-decimal values: the generator asserts that no unrounded value sits on a rounding boundary."""
    from uglad_amd import main

    T, G, metrics = load_golden()
    assert T.dtype == G.dtype == np.float32 and T.shape == G.shape == (2, 288, 288) and metrics.shape == (2, 11)
    assert np.isfinite(metrics).all()
    got = main.device_report_metrics(T, G)
    for k in range(2):
        assert tuple(got[k]) == oap.METRIC_KEYS
        np.testing.assert_array_equal(np.array([got[k][key] for key in oap.METRIC_KEYS]), metrics[k])


def test_emulated_matches_the_reference_golden(emul, monkeypatch):
    """The golden through main's routing on the emulator (its build's eigensolver stops at D = 160, so D = 288 is wide there too)."""
    from uglad_amd import main

    monkeypatch.setattr("uglad_amd.after.report_metrics_all", no_host)
    _check_golden()


# ============================================================================================ GPU
@pytest.mark.gpu
def test_gpu_matches_the_reference_golden(monkeypatch):
    from uglad_amd import main

    monkeypatch.setattr("uglad_amd.after.report_metrics_all", no_host)
    _check_golden()


@pytest.mark.gpu
def test_gpu_against_the_oracle():
    """(K = 2, D = 300): 22 tiles per pair, the last one ragged; not a multiple of 64 either."""
    from uglad_amd import _lib

    T, G = pairs(2, 300, seed=81, density=0.05, decimals=2, keep=0.2)
    check(_lib.get_lib(), T, G, "cuda", label="d300")


@pytest.mark.gpu
def test_gpu_largest_size_dense_truth():
    """(K = 1, D = 2048): E = 2 096 128 edges, half of them true, scores rounded to 3 decimals (a thousand tie groups with both labels) --
    the case a kernel with a (true edges) x (edges) term cannot finish in seconds.  Against the checker (the oracle's loop cannot either)."""
    from uglad_amd import _lib

    T, G = pairs(1, 2048, seed=82, density=0.5, decimals=3, keep=0.7)
    got = check(_lib.get_lib(), T, G, "cuda", small=False, label="d2048")
    assert 1.0e6 < got[0][4] < 1.1e6


@pytest.mark.gpu
def test_gpu_pair_does_not_depend_on_its_batch():
    from uglad_amd import _lib

    lib = _lib.get_lib()
    T, G = pairs(3, 513, seed=83, decimals=2)
    batch = run_wide(lib, T, G, "cuda")
    solo = run_wide(lib, T[1:2], G[1:2], "cuda")
    assert np.array_equal(batch[1], solo[0])
    assert_metrics(batch[1], checker(T[1], G[1]), "pair 1 of d513")


@pytest.mark.gpu
def test_gpu_fit_at_288_reports_from_the_device(monkeypatch):
    """fit(X, true_theta=...) as in test_after_path.test_gpu_fit_beyond_256_reports_metrics, with the host formulation taken away."""
    import uglad_amd
    from uglad_amd import main
    from uglad_amd.utils.metrics import report_metrics_all
    from uglad_amd.utils.prepare_data import get_data

    monkeypatch.setattr("uglad_amd.after.report_metrics_all", no_host)
    X, P = get_data(288, (0.02, 0.04), 600, 1, eig_offset=1.0, rng=11)
    est = uglad_amd.uGLAD_GL()
    res = est.fit(X[0], true_theta=P[0], epochs=2, lr=0.01, L=3, verbose=False)
    ref = report_metrics_all(P[0], est.precision_)
    assert list(res) == list(ref)
    np.testing.assert_array_equal(np.array(list(res.values())), np.array(list(ref.values())))
