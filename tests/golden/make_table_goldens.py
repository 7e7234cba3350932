#!/usr/bin/env python3
"""Golden vectors for process_table's conditioning loop (uglad_table_spectrum + uglad_correlated_features, csrc/eigvals_wide.h and
csrc/corr_wide.h; tests/test_table_conditioning.py), made by the REAL reference on CPU (build container only; needs pandas and sklearn,
which the reference imports).  The first argument is the checkout of the reference (Harshs27/uGLAD):

    python tests/golden/make_table_goldens.py <reference checkout>

Per case tests/golden/table_cond_<name>.npz holds
  table       (N, D) float32: independent uniform(0, 1) columns, and groups of columns that are linear combinations of two or three of
              them plus normal noise of standard deviation 1e-4 (drawn, rounded to float32 and only then given to the reference as
              float64, so the file loses nothing); the columns are named 0 .. D - 1
  cond_num, eigval_th   the arguments of process_table (NORM="no", MIN_VARIANCE=0)
  kept        the column names the reference's process_table keeps
  round_cols, round_con, round_below   per covariance the reference analysed from "Processed" on: its number of columns, its condition
              number (eigen_val_condition_num: np.linalg.eigvals) and the number of its eigenvalues below eigval_th
  round_gap_lo, round_gap_hi   per round the largest eigenvalue below and the smallest above eigval_th (np.linalg.eigvalsh)
The margins the test relies on are asserted here: every eigenvalue of every round is < 1e-5 or > 1e-2, cond_num is at least 10 x away
from every round's condition number, and where that number is below 1e12 the reference's own value agrees with eigvalsh's to 2.5e-7 (a quarter of
the 1e-6 the test allows the device: both errors are a few ulp of ||S|| against the smallest eigenvalue).
Data only, no reference source."""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "uglad")):
    raise SystemExit(__doc__)
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(OUT, "..", "..")))
sys.path.insert(0, os.path.abspath(sys.argv[1]))
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

from uglad.utils import prepare_data as ref  # noqa: E402  (the reference)
from uglad_amd.utils import prepare_data as host  # noqa: E402  (the package's host restatement)

COND_NUM, EIGVAL_TH = 1e4, 1e-3


def collinear_table(N, D, groups, seed):
    """D - sum(groups) independent uniform(0, 1) columns; every group adds that many columns, each a combination of two or three columns
    of the group's own three base columns with coefficients of magnitude 0.6 .. 1 plus N(0, 1e-4^2) noise.  Columns shuffled."""
    rng = np.random.default_rng(seed)
    n_base = D - sum(groups)
    base = rng.uniform(0.0, 1.0, size=(N, n_base))
    cols = [base]
    for g, size in enumerate(groups):
        own = base[:, 3 * g:3 * g + 3]
        for _ in range(size):
            c = rng.uniform(0.6, 1.0, size=3) * rng.choice([-1.0, 1.0], size=3)
            if rng.random() < 0.5:
                c[rng.integers(3)] = 0.0
            cols.append((own @ c + 1e-4 * rng.standard_normal(N))[:, None])
    table = np.concatenate(cols, axis=1)[:, rng.permutation(D)]
    return table.astype(np.float32)


def make(name, table):
    N, D = table.shape
    df = pd.DataFrame(table.astype(np.float64))
    seen = []
    original = ref.analyse_condition_number

    def recording(tab, MESSAGE="", VERBOSE=True):
        S, eig, con = original(tab, MESSAGE, VERBOSE)
        if MESSAGE != "Input":
            w = np.linalg.eigvalsh(S)
            seen.append((S.shape[0], float(con), int(np.sum(np.array(eig) < EIGVAL_TH)), float(w[w < EIGVAL_TH].max(initial=-np.inf)),
                         float(w[w >= EIGVAL_TH].min()), float(np.abs(w).max() / np.abs(w).min())))
        return S, eig, con

    ref.analyse_condition_number = recording
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            out = ref.process_table(df.copy(), NORM="no", MIN_VARIANCE=0.0, msg=name, COND_NUM=COND_NUM, eigval_th=EIGVAL_TH, VERBOSE=False)
    finally:
        ref.analyse_condition_number = original
    cols, con, below, gap_lo, gap_hi, con_h = (np.array(a) for a in zip(*seen))
    for r in range(len(seen)):
        print(f"  round {r}: {cols[r]} columns, con {con[r]:.6e} (eigvalsh {con_h[r]:.6e}), below {below[r]}, gap ({gap_lo[r]:.2e}, {gap_hi[r]:.2e})")
        assert gap_lo[r] < 1e-5 and gap_hi[r] > 1e-2, "an eigenvalue inside the margin around eigval_th"
        assert con[r] > 10 * COND_NUM or con[r] < COND_NUM / 10, "cond_num within 10 x of a round's condition number"
        print(f"    reference vs eigvalsh: {abs(con[r] - con_h[r]) / con_h[r]:.2e}")
        assert con[r] >= 1e12 or abs(con[r] - con_h[r]) <= 2.5e-7 * con_h[r], "the reference's own condition number is rounding noise here"
    assert len(seen) >= 2 and con[-1] < COND_NUM
    mine = host.process_table(df.copy(), NORM="no", COND_NUM=COND_NUM, eigval_th=EIGVAL_TH, VERBOSE=False)
    assert mine.equals(out), "the host restatement and the reference disagree"
    path = os.path.join(OUT, f"table_cond_{name}.npz")
    np.savez_compressed(path, table=table, cond_num=np.float64(COND_NUM), eigval_th=np.float64(EIGVAL_TH), kept=np.array(out.columns, dtype=np.int64),
                        round_cols=cols.astype(np.int64), round_con=con, round_below=below.astype(np.int64), round_gap_lo=gap_lo, round_gap_hi=gap_hi)
    print(f"{name}: N {N} D {D}: {len(seen) - 1} rounds, {out.shape[1]} columns kept; {os.path.getsize(path)} bytes", flush=True)
    assert os.path.getsize(path) < 1 << 20


make("n400_d96", collinear_table(400, 96, (3, 2, 2), 11))
make("n900_d288", collinear_table(900, 288, (4, 3, 3, 2), 12))
