#!/usr/bin/env python3
"""Times the spectrum of a table's covariance and process_table's conditioning loop on the device (uglad_eigvalsh_wide,
uglad_table_spectrum, uglad_correlated_features; csrc/eigvals_wide.h, csrc/corr_wide.h) against the host path of
uglad_amd.utils.prepare_data, on the same tables.

    python scripts/table_probe.py [--out profiles/table_probe.txt] [--dims 288,1024,2048]

Spectrum rows: K tables of N uniform rows and D columns, N = D / 2 (a singular covariance) and N = 2 D.  Columns:
  eigvals ms    wall clock of np.linalg.eigvals on the K covariances one after the other -- the general solver, which is what the reference and
                the host path call (eigen_val_condition_num)
  eigvalsh ms   the same with np.linalg.eigvalsh
  device ms     HIP events around the enqueue of HipLib.eigvalsh_wide on the K fp64 covariances already on the device
  e2e ms        wall clock of analyse_condition_number(table, device=True) for the K host tables one after the other: upload as fp64,
                uglad_table_spectrum, download of the covariance, the eigenvalues and the condition number
  err           max |lambda - lambda_eigvalsh| / ||S||_2 over the K matrices, for the eigenvalues of eigvalsh_wide
each time the median of the timed runs after one warm-up.
process_table rows: one table of N = 2 D rows whose columns are independent uniform but for D / 16 columns that are combinations of three
others plus noise of 1e-4; process_table(COND_NUM=1e4) on the host (one run) and with device=True (median of 3 after a warm-up), and the
rounds the loop took.  Both return the same DataFrame (asserted).
No threshold is assumed: the table reports, whichever side wins."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def median_ms(fn, reps):
    out = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def collinear_table(N, D, seed):
    rng = np.random.default_rng(seed)
    n_dep = max(D // 16, 1)
    base = rng.random((N, D - n_dep))
    dep = [base[:, rng.choice(D - n_dep, 3, replace=False)] @ (rng.uniform(0.6, 1.0, 3) * rng.choice([-1.0, 1.0], 3)) + 1e-4 * rng.standard_normal(N)
           for _ in range(n_dep)]
    return np.concatenate([base, np.stack(dep, axis=1)], axis=1)[:, rng.permutation(D)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_probe.txt"))
    ap.add_argument("--dims", default="288,1024,2048")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from uglad_amd import _lib
    from uglad_amd.utils import prepare_data

    if not torch.cuda.is_available():
        raise SystemExit("table_probe.py measures on the GPU; none is visible")
    lib = _lib.get_lib()
    dims = [int(d) for d in args.dims.split(",")]
    lines = [f"# scripts/table_probe.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; host threads {torch.get_num_threads()}; "
             f"median of {args.reps} after one warm-up",
             "# eigvals / eigvalsh = numpy on the K covariances in turn; device = HIP events around HipLib.eigvalsh_wide; e2e = "
             "analyse_condition_number(device=True) on the K host tables in turn; err = max |dlambda| / ||S||_2 against eigvalsh",
             f"{'D':>5} {'N':>5} {'K':>2} {'eigvals ms':>11} {'eigvalsh ms':>12} {'device ms':>10} {'e2e ms':>9} {'eigvalsh/e2e':>13} {'err':>9}"]
    print("\n".join(lines), flush=True)
    for D in dims:
        for N in (D // 2, 2 * D):
            for K in (1, 4):
                X = np.random.default_rng(D + N + K).random((K, N, D))
                S = np.stack([np.cov(x.T, bias=1) for x in X])
                t_eigvals = median_ms(lambda: [np.linalg.eigvals(s) for s in S], args.reps)
                t_eigvalsh = median_ms(lambda: [np.linalg.eigvalsh(s) for s in S], args.reps)
                ref = np.stack([np.linalg.eigvalsh(s) for s in S])
                Sd = torch.from_numpy(S).cuda()
                dev_ms = []
                for rep in range(args.reps + 1):
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    eig, _ = lib.eigvalsh_wide(Sd)
                    stop.record()
                    torch.cuda.synchronize()
                    if rep:
                        dev_ms.append(start.elapsed_time(stop))
                t_e2e = median_ms(lambda: [prepare_data.analyse_condition_number(x, VERBOSE=False, device=True) for x in X], args.reps)
                err = float((np.abs(eig.cpu().numpy() - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())
                d = statistics.median(dev_ms)
                line = f"{D:>5} {N:>5} {K:>2} {t_eigvals:>11.1f} {t_eigvalsh:>12.1f} {d:>10.2f} {t_e2e:>9.2f} {t_eigvalsh / t_e2e:>13.2f} {err:>9.1e}"
                print(line, flush=True)
                lines.append(line)
                del Sd
    head = ["# process_table(COND_NUM=1e4, eigval_th=1e-3) on a table of N = 2 D rows with D / 16 planted near-collinear columns: host (one run), "
            "device=True (median of 3 after a warm-up), rounds of the loop",
            f"{'D':>5} {'N':>5} {'host s':>9} {'device s':>9} {'host/device':>12} {'rounds':>7} {'kept':>5}"]
    print("\n".join(head), flush=True)
    lines += head
    for D in dims:
        table = collinear_table(2 * D, D, seed=D)
        t0 = time.perf_counter()
        host = prepare_data.process_table(table, COND_NUM=1e4, VERBOSE=False)
        t_host = time.perf_counter() - t0
        rounds = []
        dev = prepare_data.process_table(table, COND_NUM=1e4, VERBOSE=False, device=True, rounds=rounds)
        assert dev.equals(host)
        t_dev = median_ms(lambda: prepare_data.process_table(table, COND_NUM=1e4, VERBOSE=False, device=True), 3) / 1e3
        line = f"{D:>5} {2 * D:>5} {t_host:>9.2f} {t_dev:>9.2f} {t_host / t_dev:>12.1f} {len(rounds) - 1:>7} {dev.shape[1]:>5}"
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
