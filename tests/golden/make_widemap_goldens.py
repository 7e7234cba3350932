#!/usr/bin/env python3
"""Golden vectors for the conditional Gaussian / MAP estimate beyond D = 256 (uglad_conditional_mean_wide), made by the REAL reference on
CPU (build container only): conditional_gaussian_with_probabilities and compute_map_estimate of the reference's uglad/main.py:1176-1260,
imported the way make_goldens.py imports them (a stub for the absent `pyvis`, which only an annotation and the viz functions touch).  The
first argument is the checkout of the reference (Harshs27/uGLAD):

    python tests/golden/make_widemap_goldens.py <reference checkout>

Stored per case: precision_triu and cond_cov_triu (fp64, the upper triangles in the order of np.triu_indices) -- a full 288 x 288 fp64 pair
would put the file past the repository's 1 MiB limit; mean, observed_idx, observed_values; full_mean, map_clipped and log_pdf = the LOG of
the density the reference returns.  The precision matrix is symmetric to the bit (asserted).  The reference's conditional covariance is
np.linalg.inv of a symmetric matrix, which LAPACK's LU does not return symmetric to the bit: its asymmetry is asserted to stay below
1e-13 of its norm (six orders below the fp32 tolerance it is compared at) and stored as cond_cov_asym; the triangle kept is the upper one.
Data only, no reference source."""
import contextlib
import io
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

OUT = os.path.dirname(os.path.abspath(__file__))


def capture(name, precision, mean, observed_idx, observed_values):
    D = len(mean)
    assert np.array_equal(precision, precision.T)
    full_mean, cond_cov, pdf = uG.conditional_gaussian_with_probabilities(precision, mean, list(observed_idx), observed_values)
    asym = float(np.abs(cond_cov - cond_cov.T).max() / np.linalg.norm(cond_cov))
    assert asym < 1e-13, asym
    names = [f"n{i}" for i in range(D)]
    fitted = types.SimpleNamespace(precision_=precision, location_=mean, node_names_=names)
    with contextlib.redirect_stdout(io.StringIO()):
        clipped = np.asarray(uG.compute_map_estimate({names[i]: float(v) for i, v in zip(observed_idx, observed_values)}, fitted))
    iu, ju = np.triu_indices(D), np.triu_indices(cond_cov.shape[0])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, precision_triu=precision[iu], cond_cov_triu=cond_cov[ju], cond_cov_asym=np.float64(asym),
                        mean=mean, observed_idx=np.asarray(observed_idx, dtype=np.int64), observed_values=observed_values,
                        full_mean=full_mean, map_clipped=clipped, log_pdf=np.float64(np.log(pdf)))
    un = [i for i in range(D) if i not in set(observed_idx)]
    print(name, "D", D, "observed", len(observed_idx), "cond(L_uu) %.1f" % np.linalg.cond(precision[np.ix_(un, un)]),
          "log pdf %.3f" % np.log(pdf), "asymmetry of the reference's inverse %.1e" % asym, "clipped entries",
          int(np.sum(clipped != full_mean)), "bytes", os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


# D = 288: 4.5 tiles of 64; a dense, well conditioned precision matrix, 96 observed
rng = np.random.default_rng(28801)
D = 288
A = rng.standard_normal((D, D))
P = A @ A.T / D
P = 0.5 * (P + P.T) + 0.5 * np.eye(D)
obs = sorted(rng.choice(D, size=96, replace=False).tolist())
capture("widemap_d288", P, rng.random(D), obs, rng.random(96))

# D = 320, a multiple of 64: sparse and diagonally dominant like a fitted precision matrix, 40 observed
rng = np.random.default_rng(32001)
D = 320
t = np.triu(rng.random((D, D)) < 0.03, 1) * rng.uniform(-0.6, 0.6, size=(D, D))
P = t + t.T
P = P + np.diag(np.abs(P).sum(1) * 1.1 + 0.2)
obs = sorted(rng.choice(D, size=40, replace=False).tolist())
capture("widemap_d320_sparse", P, rng.random(D), obs, rng.random(40))
