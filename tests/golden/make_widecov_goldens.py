#!/usr/bin/env python3
"""Golden vectors for the covariance front-end beyond D = 256 (uglad_covariance_wide), made by the REAL reference on CPU (build
container only) exactly as make_cov_goldens.py makes the cov_* ones: tables X -> normalize_table(min_max) -> get_covariance(offset) of
the reference's uglad/utils/prepare_data.py.  The first argument is the checkout of the reference (Harshs27/uGLAD):

    python tests/golden/make_widecov_goldens.py <reference checkout>

The files are named widecov_*.npz so that the cov_*.npz glob of tests/test_covariance_frontend.py (the D <= 256 entry point) does not
pick them up.  Stored per case: X (K,N,D) fp32 raw tables, S_triu (K, D (D + 1) / 2) fp64 = the upper triangle, in the order of np.triu_indices(D), of
the matrix exactly as the reference returns it (every case is repaired: its smallest eigenvalue is <= 1e-6), offset.  The reference's
matrices are symmetric to the bit (asserted below), so the triangle loses nothing, and a full 288 x 288 x 2 fp64 array would put the file
past the repository's 1 MiB limit; no S_raw / Xn for the same reason.  Data only, no reference source."""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "uglad")):
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.abspath(sys.argv[1]))
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
from sklearn import covariance  # noqa: E402

from uglad.utils import prepare_data as ref  # noqa: E402  (the reference)

OUT = os.path.dirname(os.path.abspath(__file__))


def make(name, K, N, D, seed, offset=0.1, rank=None):
    rng = np.random.default_rng(seed)
    Xs = []
    for _ in range(K):
        A = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
        X = rng.standard_normal((N, D)) @ A
        if rank is not None:  # columns beyond `rank` are combinations of the first ones: a singular covariance
            X[:, rank:] = X[:, :rank] @ rng.standard_normal((rank, D - rank))
        X = X * rng.uniform(0.5, 20.0, size=D) + rng.uniform(-5, 5, size=D)  # columns on very different scales
        Xs.append(X.astype(np.float32))
    X = np.stack(Xs)
    Xn = np.stack([np.array(ref.normalize_table(pd.DataFrame(x.astype(np.float64)), "min_max")) for x in X])
    S_raw = np.stack([covariance.empirical_covariance(x, assume_centered=False) for x in Xn])
    with contextlib.redirect_stdout(io.StringIO()):
        S = ref.get_covariance(Xn, offset=offset)
    assert np.array_equal(S, np.swapaxes(S, 1, 2))
    iu = np.triu_indices(D)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), X=X, S_triu=S[:, iu[0], iu[1]], offset=np.float64(offset))
    rep = [bool(np.abs(S[k] - S_raw[k]).max() > 0) for k in range(K)]
    print(name, X.shape, "repaired:", rep, "min eig before:", [float(np.linalg.eigvalsh(s).min()) for s in S_raw])


make("widecov_k2_n40_d288_singular", 2, 40, 288, 21)          # D = 4.5 tiles of 64, two tables: the batch stride
make("widecov_k1_n97_d320", 1, 97, 320, 22, offset=0.25)      # D a multiple of 64, ragged N
make("widecov_k1_n400_d300_rank250", 1, 400, 300, 23, rank=250)  # D not a multiple of 4
