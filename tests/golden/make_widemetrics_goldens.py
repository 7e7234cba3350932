#!/usr/bin/env python3
"""Golden vector for the support-recovery metrics beyond D = 256 (uglad_support_metrics_wide), made by the REAL reference on CPU (build
container only): report_metrics_all of the reference's uglad/utils/metrics.py:25-108 (sklearn's roc_curve / auc / average_precision_score
behind it), imported the way make_goldens.py imports the reference (a stub for the absent `pyvis`).  The first argument is the checkout
of the reference (Harshs27/uGLAD):

    python tests/golden/make_widemetrics_goldens.py <reference checkout>

widemetrics_k2_d288.npz: true_theta, pred_theta (2, 288, 288) float32 -- exactly what the device reads -- and metrics (2, 11) float64, the
reference's 3-decimal values in the order FDR, TPR, FPR, SHD, nnzTrue, nnzPred, precision, recall, Fbeta, aupr, auc.  The predictions are
the truth plus noise, thresholded to exact zeros as the soft threshold leaves them and rounded to two decimals: tied scores under both labels.
Asserted here, so that the test may ask for exact equality of the rounded values: both ranking metrics are finite, at least one tie group
holds both labels, and no unrounded metric x 1000 lies within 1e-6 of a rounding boundary.  Data only, no reference source."""
import os
import sys
import types

sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "uglad")):
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.abspath(sys.argv[1]))
os.environ.setdefault("MPLBACKEND", "Agg")
pv = types.ModuleType("pyvis")
pv.network = types.ModuleType("pyvis.network")
pv.network.Network = object
sys.modules["pyvis"] = pv
sys.modules["pyvis.network"] = pv.network

import numpy as np  # noqa: E402

from uglad import main as uG  # noqa: E402  (the reference)
from uglad.utils.metrics import get_auc  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
METRIC_KEYS = ("FDR", "TPR", "FPR", "SHD", "nnzTrue", "nnzPred", "precision", "recall", "Fbeta", "aupr", "auc")
K, D = 2, 288


def unrounded(true, pred):
    """The same 11 numbers before the reference rounds them: its own get_auc and the counts of its formulas."""
    iu = np.triu_indices(D, 1)
    t, p, s = true[iu] != 0, pred[iu] != 0, np.abs(pred[iu])
    auc, aupr = get_auc(t.astype(int), s)
    TP, FP, FN = float(np.sum(t & p)), float(np.sum(~t & p)), float(np.sum(t & ~p))
    T, P = float(t.sum()), float(p.sum())
    return np.array([FP / P, TP / T, FP / (t.size - T), FP + FN, T, P, TP / (TP + FP), TP / (TP + FN), 2 * TP / (2 * TP + FN + FP), aupr, auc]), t, s


true_K, pred_K, met_K = [], [], []
for k in range(K):
    rng = np.random.default_rng(28810 + k)
    t = np.triu(rng.random((D, D)) < 0.04 + 0.02 * k, 1) * rng.uniform(0.2, 0.9, size=(D, D)) * np.where(rng.random((D, D)) < 0.5, 1.0, -1.0)
    true = (t + t.T + np.eye(D)).astype(np.float32)
    noise = np.triu((0.25 + 0.1 * k) * rng.standard_normal((D, D)), 1)
    pred = np.round(t + noise, 2)
    pred[np.abs(pred) < 0.35] = 0.0  # exact zeros, as the soft threshold leaves them
    pred = (pred + pred.T + np.eye(D)).astype(np.float32)
    m = uG.report_metrics_all(true, pred)
    row = np.array([m[key] for key in METRIC_KEYS], dtype=np.float64)
    raw, labels, scores = unrounded(true, pred)
    assert np.isfinite(row[9]) and np.isfinite(row[10])
    assert np.array_equal(np.array([round(float(x), 3) for x in raw]), row), (raw, row)
    frac = np.abs(raw * 1000.0 - np.floor(raw * 1000.0) - 0.5)
    assert frac.min() > 1e-6, frac  # no value on a rounding boundary
    mixed = sum(1 for u in np.unique(scores) if labels[scores == u].any() and not labels[scores == u].all())
    assert mixed >= 1
    print(f"pair {k}: {dict(zip(METRIC_KEYS, row))}; distinct scores {len(np.unique(scores))}, tie groups with both labels {mixed}, "
          f"closest to a rounding boundary {frac.min():.1e}")
    true_K.append(true), pred_K.append(pred), met_K.append(row)

path = os.path.join(OUT, "widemetrics_k2_d288.npz")
np.savez_compressed(path, true_theta=np.array(true_K), pred_theta=np.array(pred_K), metrics=np.array(met_K))
print("bytes", os.path.getsize(path))
assert os.path.getsize(path) < 1 << 20
