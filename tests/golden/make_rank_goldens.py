#!/usr/bin/env python3
"""Golden vectors for the rank-based correlation matrices of the nonparanormal front-end (uglad_rank_correlation, csrc/rank_wide.h), made
with scipy on the CPU (build container only; reads nothing of the reference, which has no such option):

    python tests/golden/make_rank_goldens.py

Per case tests/golden/rank_<name>.npz holds
  table      (N, D) float32: standard-normal columns driven by three latent factors, every third column rounded to halves so that ties
             occur; drawn, rounded to float32 and only then used as float64, so the file loses nothing.  In the first case column 4 is
             -exp(column 1): a decreasing transform of it, tau = rho = -1
  offset     the eval_offset of the repair
and, split by method so that every file stays under the repository's 1 MiB limit, tests/golden/rank_<name>_<method>.npz holds
  coef_triu  the upper triangle (np.triu_indices(D) order) of the UNTRANSFORMED coefficient, float64: scipy.stats.kendalltau per pair
             (tau-b), scipy.stats.spearmanr, or np.corrcoef of the normal scores scipy.stats.norm.ppf(rankdata / (N + 1))
  min_eig    the smallest np.linalg.eigvalsh eigenvalue of the TRANSFORMED matrix -- sin(pi tau / 2), 2 sin(pi rho / 6), the scores'
             as it is -- with its diagonal set to exactly 1
  repaired_diag   the diagonal of that matrix after the repair A += (offset - min eig) I where min eig <= 1e-6; ones otherwise
and tests/golden/rank_deviation.json records per case and method d_ref = max |host formulation - scipy| over the entries of the
untransformed and of the transformed matrix (uglad_amd.utils.prepare_data.rank_correlation_host against the above), and min_eig."""
import json
import os
import sys
import time

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(OUT, "..", "..")))
import numpy as np  # noqa: E402
import scipy.stats as ss  # noqa: E402

from uglad_amd.utils import prepare_data as host  # noqa: E402  (the package's host formulation)

CASES = {"n37_d7": (37, 7, 11), "n130_d70": (130, 70, 12), "n257_d129": (257, 129, 13), "n300_d288": (300, 288, 14)}
OFFSET = 0.1


def draw(N, D, seed, monotone):
    rng = np.random.default_rng(seed)
    load = rng.standard_normal((3, D))
    X = rng.standard_normal((N, 3)) @ load + rng.standard_normal((N, D))
    X /= np.sqrt((load * load).sum(axis=0) + 1.0)  # unit variance
    X[:, ::3] = np.round(X[:, ::3] * 2.0) / 2.0
    if monotone:
        X[:, 4] = -np.exp(X[:, 1])
    return X.astype(np.float32)


def transformed(C, method):
    A = {"kendall": np.sin(np.pi * C / 2.0), "spearman": 2.0 * np.sin(np.pi * C / 6.0), "scores": C.copy()}[method]
    A[np.diag_indices_from(A)] = 1.0
    return A


def scipy_coefficient(X, method):
    N, D = X.shape
    if method == "spearman":
        return np.asarray(ss.spearmanr(X).statistic)
    if method == "scores":
        return np.corrcoef(ss.norm.ppf(ss.rankdata(X, axis=0) / (N + 1.0)).T)
    C = np.eye(D)
    for i in range(D):
        for j in range(i + 1, D):
            C[i, j] = C[j, i] = ss.kendalltau(X[:, i], X[:, j]).statistic
    return C


record, repaired_any, passed_any = {}, False, False
for name, (N, D, seed) in CASES.items():
    table = draw(N, D, seed, monotone=name == "n37_d7")
    X = table.astype(np.float64)
    np.savez_compressed(os.path.join(OUT, f"rank_{name}.npz"), table=table, offset=np.float64(OFFSET))
    record[name] = {"N": N, "D": D}
    iu = np.triu_indices(D)
    for method in host.RANK_METHODS:
        t0 = time.time()
        C = scipy_coefficient(X, method)
        seconds = time.time() - t0
        assert np.isfinite(C).all() and np.abs(C - C.T).max() <= 2.0 ** -52
        C = np.triu(C) + np.triu(C, 1).T  # (np.corrcoef's two triangles can differ in the last bit; the upper one is what is kept)
        A = transformed(C, method)
        min_eig = float(np.linalg.eigvalsh(A).min())
        diag = np.ones(D) + ((OFFSET - min_eig) if min_eig <= 1e-6 else 0.0)
        repaired_any, passed_any = repaired_any or min_eig <= 1e-6, passed_any or min_eig > 1e-6
        assert not 1e-7 < min_eig < 1e-5, "a golden must not sit at the repair's threshold"
        d_ref = max(float(np.abs(host.rank_correlation_host(X, method, transform=False) - np.where(np.eye(D) > 0, 1.0, C)).max()),
                    float(np.abs(host.rank_correlation_host(X, method, transform=True) - A).max()))
        if name == "n37_d7" and method != "scores":
            assert abs(C[1, 4] + 1.0) <= 1e-15, C[1, 4]
        path = os.path.join(OUT, f"rank_{name}_{method}.npz")
        np.savez_compressed(path, coef_triu=C[iu], min_eig=np.float64(min_eig), repaired_diag=diag)
        assert os.path.getsize(path) < 1 << 20 and os.path.getsize(os.path.join(OUT, f"rank_{name}.npz")) < 1 << 20
        record[name][method] = {"d_ref": d_ref, "min_eig": min_eig, "scipy_seconds": round(seconds, 2)}
        print(f"{name} {method}: min eig {min_eig:.3e}, d_ref {d_ref:.2e}, scipy {seconds:.1f} s, {os.path.getsize(path)} bytes", flush=True)
assert repaired_any and passed_any, "the goldens must hold a case that needs the repair and one that does not"
with open(os.path.join(OUT, "rank_deviation.json"), "w") as f:
    json.dump(record, f, indent=1, sort_keys=True)
    f.write("\n")
