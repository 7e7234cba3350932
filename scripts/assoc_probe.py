#!/usr/bin/env python3
"""Times the association matrix of a mixed table (uglad_association, csrc/assoc_wide.h) against the host routes to the same matrix.

    python scripts/assoc_probe.py [--out profiles/assoc_probe.txt] [--dims 288,1024,2048] [--loop-max-dim 288]

Tables: N x D, every other column categorical with 2 .. 12 levels, the rest real, all tied to a few latent factors; N = D / 2 and N = 2 D.
Columns (ms; medians of the timed runs after one warm-up, the pair loop one run):
  loop        a Python loop over the D (D + 1) / 2 pairs that calls the package's per-pair functions (cramers_v, correlation_ratio,
              np.corrcoef) -- the shape of the reference's pairwise_cov_matrix, whose own loop over pd.crosstab / scipy calls took 83.6 s on
              the 300 x 288 golden (tests/golden/assoc_deviation.json); only up to --loop-max-dim
  host        prepare_data.pairwise_cov_matrix: the vectorised fp64 formulation (one-hot Gram, reduction per pair), encoding included
  device      HIP events around HipLib.association without the repair, table on the device (the five small maps are uploaded inside)
  +repair     the same with the repair: 49 blocked Cholesky factorisations when the matrix fails the test at 1e-6 (these all do)
  e2e         wall clock of main.mixed_association: encode on the host, upload, kernels with repair, synchronise
max dev: the largest deviation of the device's fp64 matrix from `host`, entry by entry for r/r pairs and between the SQUARES of the entries
that involve a categorical (V and eta are square roots of quantities that may sit at the max(0, .) clamp: tests/test_association.py).
No time here is an acceptance criterion: the table is the record."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_table(N, D, seed):
    import pandas as pd

    rng = np.random.default_rng(seed)
    lat = rng.standard_normal((N, 8))
    cols, dtype = {}, {}
    for i in range(D):
        v = lat @ rng.standard_normal(8) * rng.uniform(0.2, 1.0) + rng.standard_normal(N)
        name = f"f{i}"
        if i % 2 == 0:
            card = int(rng.integers(2, 13))
            cols[name] = np.digitize(v, np.quantile(v, np.linspace(0, 1, card + 1)[1:-1]))
            dtype[name] = "c"
        else:
            cols[name] = v * rng.uniform(0.5, 20.0)
            dtype[name] = "r"
    return pd.DataFrame(cols), dtype


def pair_loop(df, dtype):
    from uglad_amd.utils import prepare_data as pd_

    names = list(df.columns)
    arrays = [np.asarray(df[n]) for n in names]
    D = len(names)
    A = np.zeros((D, D))
    for i in range(D):
        for j in range(i, D):
            ci, cj = dtype[names[i]] == "c", dtype[names[j]] == "c"
            if ci and cj:
                A[i, j] = pd_.cramers_v(arrays[i], arrays[j])
            elif ci or cj:
                A[i, j] = pd_.correlation_ratio(arrays[i], arrays[j]) if ci else pd_.correlation_ratio(arrays[j], arrays[i])
            else:
                A[i, j] = np.corrcoef(arrays[i], arrays[j])[0, 1]
            A[j, i] = A[i, j]
    return A


def median_ms(fn, reps):
    out = []
    for rep in range(reps + 1):
        ms = fn()
        if rep:
            out.append(ms)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_probe.txt"))
    ap.add_argument("--dims", default="288,1024,2048")
    ap.add_argument("--loop-max-dim", type=int, default=288)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from uglad_amd import _lib, main as um
    from uglad_amd.utils import prepare_data as pd_

    if not torch.cuda.is_available():
        raise SystemExit("assoc_probe.py measures on the GPU; none is visible")
    lib = _lib.get_lib()
    lines = [f"# scripts/assoc_probe.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; medians of {args.reps} after one warm-up",
             "# loop = Python loop over the pairs on the package's per-pair functions (one run); host = prepare_data.pairwise_cov_matrix; device = "
             "HIP events around HipLib.association; e2e = main.mixed_association (encode + upload + kernels + repair)",
             f"{'D':>5} {'N':>5} {'W':>6} {'loop ms':>10} {'host ms':>9} {'device ms':>10} {'+repair ms':>11} {'e2e ms':>9} {'min eig':>10} {'max dev':>9}"]
    print("\n".join(lines), flush=True)
    for D in [int(d) for d in args.dims.split(",")]:
        for N in (D // 2, 2 * D):
            df, dtype = make_table(N, D, seed=D + N)
            loop_ms = None
            if D <= args.loop_max_dim:
                t0 = time.perf_counter()
                pair_loop(df, dtype)
                loop_ms = (time.perf_counter() - t0) * 1e3

            def host():
                t0 = time.perf_counter()
                host.A = np.array(pd_.pairwise_cov_matrix(df, dtype))
                return (time.perf_counter() - t0) * 1e3

            table, maps = pd_.encode_mixed_table(df, dtype)
            Xd = torch.from_numpy(table[None]).cuda()

            def device(repair):
                def run():
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    run.out = lib.association(Xd, maps, eval_offset=0.1, repair=repair, want_f64=True)
                    stop.record()
                    torch.cuda.synchronize()
                    return start.elapsed_time(stop)
                return run

            def e2e():
                t0 = time.perf_counter()
                e2e.out = um.mixed_association(df, dtype, repair=True, eval_offset=0.1)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            plain, repaired = device(False), device(True)
            host_ms, dev_ms, rep_ms, e2e_ms = median_ms(host, args.reps), median_ms(plain, args.reps), median_ms(repaired, args.reps), median_ms(e2e, args.reps)
            assert torch.equal(e2e.out[0], repaired.out[0][0])
            A_dev = plain.out[2][0].cpu().numpy()
            cat = np.array([dtype[c] == "c" for c in df.columns])
            anycat = cat[:, None] | cat[None, :]
            dev = float(np.abs(np.where(anycat, A_dev ** 2, A_dev) - np.where(anycat, host.A ** 2, host.A)).max())
            loop = f"{loop_ms:>10.0f}" if loop_ms is not None else f"{'-':>10}"
            line = (f"{D:>5} {N:>5} {maps.W:>6} {loop} {host_ms:>9.1f} {dev_ms:>10.2f} {rep_ms:>11.2f} {e2e_ms:>9.2f} {e2e.out[1]:>10.3f} {dev:>9.1e}")
            print(line, flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
