#!/usr/bin/env python3
"""Times the pairwise-complete covariance of tables with missing entries (uglad_pairwise_covariance, csrc/pairwise_wide.h) against pandas,
against the host formulation of the same matrix, and against uglad_covariance_wide on the mean-imputed table of the same shape.

    python scripts/pairwise_probe.py [--out profiles/pairwise_probe.txt] [--dims 288,1024,2048] [--batch 1,4] [--missing 0.25]

This process never opens the GPU.  Every (D, N) is a child process of its own, in a process group of its own and under its own time limit
(--step-timeout).  A step that runs out of time has its whole group killed; a step that times out, dies by a signal or ends with a non-zero
status ends the probe with a non-zero status and nothing further is started.

Tables: N x D, three latent factors plus noise plus 50, N = D / 2 and 2 D, --missing of the cells dropped independently.
Columns (ms; medians of --reps timed runs after one warm-up; a host run that takes more than two seconds is timed once):
  pandas      DataFrame.cov on ONE table
  host        prepare_data.pairwise_covariance_host on ONE table: vectorised fp64 numpy, three BLAS products
  device      HIP events around HipLib.pairwise_covariance without the repair, the K tables on the device
  +repair     the same with the repair (49 blocked Cholesky factorisations for a table that fails the test at 1e-6)
  e2e         wall clock of main.pairwise_covariance on host arrays: upload, kernels with repair, synchronise, the eigenvalues read back
  host/e2e    K x host over e2e
  min eig     of table 0, from the repair
  dev/bound   the largest deviation of the device's fp64 matrix (table 0) from `host`, as a fraction of the derived bound
              4 (N + 8) 2^-53 sqrt(q_i q_j) / n_ij (tests/test_pairwise_covariance.py)
  cov_wide    HIP events around HipLib.covariance_wide without the repair on the mean-imputed tables, in the same run
  ratio       device over cov_wide: four accumulator sets (16 MFMA per k-step of 4) against one (4) on the same loads
No time here is an acceptance criterion: the table is the record."""
import argparse
import json
import os
import signal
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RESULT = "RESULT "  # a child's line for the parent


def make_table(N, D, missing, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, 3)) @ rng.standard_normal((3, D)) + rng.standard_normal((N, D)) + 50.0
    X[rng.random((N, D)) < missing] = np.nan
    return X


def median_ms(fn, reps):
    out = []
    for rep in range(reps + 1):
        ms = fn()
        if rep:
            out.append(ms)
        if rep == 0 and ms > 2000.0:
            return ms  # (a long host run: once)
    return statistics.median(out)


# ============================================================================================ the child: the only GPU process
def child(args, D, N):
    """The timed runs of one (D, N): one RESULT line of JSON per K."""
    import numpy as np
    import pandas as pd
    import torch

    from uglad_amd import _lib, main as um
    from uglad_amd.utils import prepare_data as pd_

    if not torch.cuda.is_available():
        raise SystemExit("pairwise_probe.py measures on the GPU; none is visible")
    lib = _lib.get_lib()
    print(RESULT + json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__}), flush=True)
    host_ms = pandas_ms = None
    for K in [int(k) for k in args.batch.split(",")]:
        tables = np.stack([make_table(N, D, args.missing, seed=7 * D + N + k) for k in range(K)])
        if host_ms is None:
            frame = pd.DataFrame(tables[0])

            def pandas_cov():
                t0 = time.perf_counter()
                frame.cov()
                return (time.perf_counter() - t0) * 1e3

            def host():
                t0 = time.perf_counter()
                host.out = pd_.pairwise_covariance_host(tables[0])
                return (time.perf_counter() - t0) * 1e3

            pandas_ms, host_ms = median_ms(pandas_cov, args.reps), median_ms(host, args.reps)
            cov, counts = host.out
            z = np.where(np.isnan(tables[0]), 0.0, tables[0] - np.nanmean(tables[0], axis=0))
            q = (z * z).sum(axis=0)
            bound = 4.0 * (N + 8) * 2.0 ** -53 * np.sqrt(np.outer(q, q)) / counts
        Xd = torch.from_numpy(tables).cuda()
        imputed = torch.from_numpy(np.where(np.isnan(tables), np.nanmean(tables, axis=1, keepdims=True), tables)).cuda()

        def timed(call):
            def run():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                run.out = call()
                stop.record()
                torch.cuda.synchronize()
                return start.elapsed_time(stop)
            return run

        def e2e():
            t0 = time.perf_counter()
            e2e.out = um.pairwise_covariance(tables, repair=True, eval_offset=0.1)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        plain = timed(lambda: lib.pairwise_covariance(Xd, eval_offset=0.1, repair=False, want_f64=True))
        repaired = timed(lambda: lib.pairwise_covariance(Xd, eval_offset=0.1, repair=True))
        wide = timed(lambda: lib.covariance_wide(imputed, normalize=False, repair=False))
        dev_ms, rep_ms, wide_ms = median_ms(plain, args.reps), median_ms(repaired, args.reps), median_ms(wide, args.reps)
        e2e_ms = median_ms(e2e, args.reps)
        assert torch.equal(e2e.out[0], repaired.out.S) and not repaired.out.info.any()
        ratio = float((np.abs(plain.out.S64[0].cpu().numpy() - cov) / bound).max()) if K == int(args.batch.split(",")[0]) else None
        print(RESULT + json.dumps({"K": K, "pandas_ms": pandas_ms, "host_ms": host_ms, "dev_ms": dev_ms, "rep_ms": rep_ms, "e2e_ms": e2e_ms,
                                   "min_eig": float(repaired.out.min_eig[0]), "of_bound": ratio, "wide_ms": wide_ms}), flush=True)


# ============================================================================================ the parent: starts, limits and checks the steps
def run_step(cmd, limit, what):
    """One child step in a process group of its own, under `limit` seconds: its stdout, or the end of the probe (non-zero) if it ran out
    of time -- the whole group is killed -- or died by a signal or ended with a non-zero status."""
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, _ = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(proc.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        proc.communicate()
        raise SystemExit(f"pairwise_probe.py: {what} ran past its limit of {limit} s; its process group was killed and nothing further is started")
    if proc.returncode != 0:
        raise SystemExit(f"pairwise_probe.py: {what} ended with status {proc.returncode}; nothing further is started")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairwise_probe.txt"))
    ap.add_argument("--dims", default="288,1024,2048")
    ap.add_argument("--batch", default="1,4")
    ap.add_argument("--missing", type=float, default=0.25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds for every child step")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--D", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--N", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args, args.D, args.N)
    batch = [int(k) for k in args.batch.split(",")]
    lines = []
    for D in [int(d) for d in args.dims.split(",")]:
        for N in (D // 2, 2 * D):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batch", args.batch, "--missing", str(args.missing), "--reps",
                   str(args.reps), "--D", str(D), "--N", str(N)]
            out = run_step(cmd, args.step_timeout, f"the timed run of D = {D}, N = {N}")
            results = [json.loads(line[len(RESULT):]) for line in out.splitlines() if line.startswith(RESULT)]
            if len(results) != 1 + len(batch):
                raise SystemExit(f"pairwise_probe.py: the timed run of D = {D}, N = {N} reported {len(results)} lines, {1 + len(batch)} expected")
            if not lines:
                lines = [f"# scripts/pairwise_probe.py on {results[0]['device']}; torch {results[0]['torch']}; medians of {args.reps} after one "
                         f"warm-up; {100.0 * args.missing:.0f} % of the cells missing",
                         "# pandas = DataFrame.cov, host = prepare_data.pairwise_covariance_host, one table each (once when over 2 s); device = "
                         "HIP events around HipLib.pairwise_covariance; e2e = main.pairwise_covariance on host arrays; dev/bound = the largest "
                         "|device - host| as a fraction of 4 (N + 8) 2^-53 sqrt(q_i q_j) / n_ij; cov_wide = HipLib.covariance_wide without "
                         "repair on the mean-imputed tables; ratio = device / cov_wide",
                         f"{'D':>5} {'N':>5} {'K':>2} {'pandas ms':>10} {'host ms':>9} {'device ms':>10} {'+repair ms':>11} {'e2e ms':>9} "
                         f"{'host/e2e':>8} {'min eig':>9} {'dev/bound':>9} {'cov_wide':>9} {'ratio':>6}"]
                print("\n".join(lines), flush=True)
            for K, r in zip(batch, results[1:]):
                assert r["K"] == K
                of_bound = f"{r['of_bound']:>9.3f}" if r["of_bound"] is not None else f"{'':>9}"
                line = (f"{D:>5} {N:>5} {K:>2} {r['pandas_ms']:>10.1f} {r['host_ms']:>9.1f} {r['dev_ms']:>10.2f} {r['rep_ms']:>11.2f} "
                        f"{r['e2e_ms']:>9.2f} {K * r['host_ms'] / r['e2e_ms']:>8.2f} {r['min_eig']:>9.3f} {of_bound} {r['wide_ms']:>9.2f} "
                        f"{r['dev_ms'] / r['wide_ms']:>6.2f}")
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
