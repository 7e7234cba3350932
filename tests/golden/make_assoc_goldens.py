#!/usr/bin/env python3
"""Golden vectors for the mixed-type association matrix (uglad_association, csrc/assoc_wide.h), made by the REAL reference on CPU (build
container only; needs scipy and pandas, which the reference imports).  The first argument is the checkout of the reference
(Harshs27/uGLAD):

    python tests/golden/make_assoc_goldens.py <reference checkout>

Per case tests/golden/assoc_<name>.npz holds
  table      (N, D) float32: the ENCODED table -- 'c' columns hold the level codes 0 .. card - 1 in pd.factorize order, 'r' columns the
             values (drawn, rounded to float32 and only then given to the reference as float64, so the file loses nothing)
  kinds      (D,) 'c' | 'r';  cards (D,) levels of the categoricals, 0 for real columns;  names (D,) the column names
  A_triu     the upper triangle (np.triu_indices(D) order) of the reference's pairwise_cov_matrix output, float64 (symmetric to the
             bit: asserted below; the full D = 288 matrix twice would pass the repository's 1 MiB limit)
  min_eig    min of the real parts of np.linalg.eigvals(A), as the reference's get_covariance computes it (prepare_data.py:345-348)
  offset     the eval_offset of the repair
  repaired_diag   the diagonal of the matrix after the reference's repair A += (offset - min eig) I where min eig <= 1e-6 (its
             off-diagonal is A's: asserted below); equal to A's diagonal for the case that needs no repair
and tests/golden/assoc_deviation.json records per case d_ref = max |host formulation - reference| over the entries (the package's
vectorised uglad_amd.utils.prepare_data.pairwise_cov_matrix against the reference's loop over scipy calls), and the same with the
entries that involve a categorical squared (d_ref_squared), the quantity tests/test_association.py compares.
Data only, no reference source."""
import contextlib
import io
import json
import os
import sys
import time

sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "uglad")):
    raise SystemExit(__doc__)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(OUT, "..", "..")))
sys.path.insert(0, os.path.abspath(sys.argv[1]))
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from uglad.utils import prepare_data as ref  # noqa: E402  (the reference)
from uglad_amd.utils import prepare_data as host  # noqa: E402  (the package's host formulation)


def mixed_table(N, D, cards, seed, factors=4):
    """Columns driven by a few latent factors plus noise; column i is categorical where cards[i] > 0, cut at the quantiles of its own
    values into cards[i] levels of (roughly) equal size.  Level codes in order of first appearance, as pd.factorize gives them."""
    rng = np.random.default_rng(seed)
    lat = rng.standard_normal((N, factors))
    table = np.empty((N, D), dtype=np.float32)
    for i in range(D):
        v = lat @ rng.standard_normal(factors) * rng.uniform(0.2, 1.0) + rng.standard_normal(N)
        if cards[i]:
            cuts = np.quantile(v, np.linspace(0, 1, cards[i] + 1)[1:-1])
            codes, levels = pd.factorize(np.digitize(v, cuts))
            assert len(levels) == cards[i]
            table[:, i] = codes
        else:
            table[:, i] = v * rng.uniform(0.5, 20.0) + rng.uniform(-5, 5)
    return table


def make(name, table, cards, offset=0.1):
    N, D = table.shape
    cards = np.asarray(cards, dtype=np.int32)
    kinds = np.where(cards > 0, "c", "r")
    names = [f"f{i}" for i in range(D)]
    df = pd.DataFrame({n: (table[:, i].astype(np.int64) if cards[i] else table[:, i].astype(np.float64)) for i, n in enumerate(names)})
    dtype = dict(zip(names, kinds))
    t0 = time.time()
    with contextlib.redirect_stdout(io.StringIO()):
        A = np.array(ref.pairwise_cov_matrix(df, dtype))
    t_ref = time.time() - t0
    assert np.array_equal(A, A.T)
    min_eig = min(v.real for v in np.linalg.eigvals(A))
    R = A.copy()
    if min_eig <= 1e-6:
        R += np.eye(D) * (offset - min_eig)
    off = ~np.eye(D, dtype=bool)
    assert np.array_equal(R[off], A[off])
    mine = host.pairwise_cov_matrix(df, dtype)
    assert list(mine.index) == names
    enc, maps = host.encode_mixed_table(df, dtype)
    assert np.array_equal(enc, table.astype(np.float64)) and np.array_equal(maps.cards, cards)
    H = np.array(mine)
    anycat = (kinds[:, None] == "c") | (kinds[None, :] == "c")
    d_ref = float(np.abs(H - A).max())
    d_sq = float(np.abs(np.where(anycat, H * H, H) - np.where(anycat, A * A, A)).max())
    iu = np.triu_indices(D)
    path = os.path.join(OUT, f"assoc_{name}.npz")
    np.savez_compressed(path, table=table, kinds=kinds, cards=cards, names=np.array(names), A_triu=A[iu], min_eig=np.float64(min_eig),
                        offset=np.float64(offset), repaired_diag=np.diagonal(R).copy())
    print(f"{name}: N {N} D {D} W {maps.W}; reference {t_ref:.1f} s; min eig {min_eig:.4f}; repaired {bool(min_eig <= 1e-6)}; "
          f"d_ref {d_ref:.2e} (squared {d_sq:.2e}); {os.path.getsize(path)} bytes", flush=True)
    assert os.path.getsize(path) < 1 << 20
    return {"d_ref": d_ref, "d_ref_squared": d_sq, "N": N, "D": D, "W": maps.W, "reference_seconds": round(t_ref, 2)}


def cards_for(D, seed, lo, hi, binary=()):
    rng = np.random.default_rng(seed)
    cards = np.where(rng.random(D) < 0.5, rng.integers(lo, hi + 1, size=D), 0)
    for i in binary:
        cards[i] = 2
    return cards


record = {}
c12 = cards_for(12, 1, 3, 8, binary=(0, 5))  # two binary columns: their pair is 2 x 2 (Yates)
record["n97_d12"] = make("n97_d12", mixed_table(97, 12, c12, 101), c12)
c40 = cards_for(40, 2, 2, 8)
record["n400_d40"] = make("n400_d40", mixed_table(400, 40, c40, 102), c40)
c288 = cards_for(288, 3, 2, 12)
record["n300_d288"] = make("n300_d288", mixed_table(300, 288, c288, 103, factors=12), c288)
# all real, N > D, weakly coupled columns: Pearson's matrix is positive definite, no repair
call = np.zeros(20, dtype=np.int64)
record["allreal_n200_d20"] = make("allreal_n200_d20", mixed_table(200, 20, call, 104), call)
assert float(np.load(os.path.join(OUT, "assoc_allreal_n200_d20.npz"))["min_eig"]) > 1e-6
with open(os.path.join(OUT, "assoc_deviation.json"), "w") as f:
    json.dump(record, f, indent=1, sort_keys=True)
    f.write("\n")
