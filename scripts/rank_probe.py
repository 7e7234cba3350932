#!/usr/bin/env python3
"""Times the rank-based correlation matrices of the nonparanormal front-end (uglad_rank_correlation, csrc/rank_wide.h) against the host
formulation of the same matrices.

    python scripts/rank_probe.py [--out profiles/rank_probe.txt] [--dims 288,1024,2048] [--rows 512,2048] [--batch 1,4] [--no-split]

This process never opens the GPU.  Every GPU step is a child process of its own -- per (D, N) one traced run and one timed run of the
K x method configurations -- in a process group of its own and under its own time limit (--step-timeout).  A step that runs out of time
has its whole group killed; a step that times out, dies by a signal or ends with a non-zero status ends the probe with a non-zero status
and nothing further is started.  The probe goes on without the kernel split only where rocprofv3 is not installed or where its CSV cannot
be read after a clean exit.

Tables: N x D standard-normal columns driven by a few latent factors, every third column rounded to halves (ties).
Columns (ms; medians of --reps timed runs after one warm-up; a host run that takes more than two seconds is timed once):
  host        prepare_data.rank_correlation_host on ONE table: vectorised fp64 numpy, Kendall's Gram as float64 BLAS products of sign rows
  device      HIP events around HipLib.rank_correlation without the repair, the K tables on the device
  +repair     the same with the repair (49 blocked Cholesky factorisations for a table that fails the test at 1e-6)
  ranks, gram, finish, repair   the kernels of one repaired call by family, from a kernel trace taken in a run of its own (this script
              started once more under rocprofv3 --kernel-trace with --child trace; every call begins with one rank_kernel dispatch, which is
              how the dispatches are told apart): rank_kernel | the Gram product (Kendall: zero_kernel + rank_kendall_kernel; else
              covw_stats_kernel + covw_gram_kernel) | rank_finish_kernel | assoc_rowsum_kernel + the bisection.  '-' where no trace was taken
  e2e         wall clock of main.rank_correlation on host arrays: upload, kernels with repair, synchronise, the eigenvalues read back
  host/e2e    K x host over e2e
  max dev     the largest deviation of the device's fp64 matrix (table 0) from `host`
Kendall also gets the achieved integer rate: 2 P D (D + 1) / 2 operations per table (P = N (N - 1) / 2 pairs, a multiply and an add per pair
and entry of the upper triangle) over the traced Gram time (over device ms where no trace was taken: an underestimate), and that rate as a
share of the dense int8 MFMA peak, twice the BF16 peak of 2.5 PFLOP/s.  One Gram variant exists: signs made on the fly in the workgroup
and shared through LDS; the variant that materialises the sign rows in global memory was not built, so there is no second time.
No time here is an acceptance criterion: the table is the record."""
import argparse
import csv
import glob
import json
import os
import shutil
import signal
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METHODS = ("spearman", "kendall", "scores")
I8_PEAK = 5.0e15  # dense int8 MFMA operations per second: 2 x the BF16 peak
RESULT = "RESULT "  # a child's line for the parent


def make_table(N, D, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, 4)) @ rng.standard_normal((4, D)) + rng.standard_normal((N, D))
    X[:, ::3] = np.round(X[:, ::3] * 2.0) / 2.0
    return X


def tables_of(D, N, K):
    import numpy as np

    return np.stack([make_table(N, D, seed=7 * D + N + k) for k in range(K)])


def group_configs(args):
    """The configurations of one (D, N) step, in the order both children run them."""
    return [(K, method) for K in [int(k) for k in args.batch.split(",")] for method in METHODS]


def median_ms(fn, reps):
    out = []
    for rep in range(reps + 1):
        ms = fn()
        if rep:
            out.append(ms)
        if rep == 0 and ms > 2000.0:
            return ms  # (a long host run: once)
    return statistics.median(out)


# ============================================================================================ the children: the only GPU processes
def child_trace(args, D, N):
    """Under the kernel trace: per configuration one warm-up and one traced call."""
    import torch

    from uglad_amd import _lib

    lib = _lib.get_lib()
    for K, method in group_configs(args):
        Xd = torch.from_numpy(tables_of(D, N, K)).cuda()
        for _ in range(2):
            lib.rank_correlation(Xd, method, eval_offset=0.1, repair=True)
            torch.cuda.synchronize()


def child_time(args, D, N):
    """The timed runs of one (D, N): one RESULT line of JSON per configuration."""
    import numpy as np
    import torch

    from uglad_amd import _lib, main as um
    from uglad_amd.utils import prepare_data as pd_

    if not torch.cuda.is_available():
        raise SystemExit("rank_probe.py measures on the GPU; none is visible")
    lib = _lib.get_lib()
    print(RESULT + json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__}), flush=True)
    host_cache = {}
    for K, method in group_configs(args):
        tables = tables_of(D, N, K)
        if method not in host_cache:
            def host():
                t0 = time.perf_counter()
                host.A = pd_.rank_correlation_host(tables[0], method)
                return (time.perf_counter() - t0) * 1e3
            host_cache[method] = (median_ms(host, args.reps), host.A)
        host_ms, A_host = host_cache[method]
        Xd = torch.from_numpy(tables).cuda()

        def device(repair):
            def run():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                run.out = lib.rank_correlation(Xd, method, eval_offset=0.1, repair=repair, want_f64=True)
                stop.record()
                torch.cuda.synchronize()
                return start.elapsed_time(stop)
            return run

        def e2e():
            t0 = time.perf_counter()
            e2e.out = um.rank_correlation(tables, method=method, repair=True, eval_offset=0.1)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        plain, repaired = device(False), device(True)
        dev_ms, rep_ms, e2e_ms = median_ms(plain, args.reps), median_ms(repaired, args.reps), median_ms(e2e, args.reps)
        assert torch.equal(e2e.out[0], repaired.out.A)
        dev = float(np.abs(plain.out.A64[0].cpu().numpy() - A_host).max())
        chunks = lib.rank_pair_chunks(K, N, D) if method == "kendall" else None
        print(RESULT + json.dumps({"K": K, "method": method, "host_ms": host_ms, "dev_ms": dev_ms, "rep_ms": rep_ms, "e2e_ms": e2e_ms,
                                   "dev": dev, "chunks": chunks}), flush=True)


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
        raise SystemExit(f"rank_probe.py: {what} ran past its limit of {limit} s; its process group was killed and nothing further is started")
    if proc.returncode != 0:
        raise SystemExit(f"rank_probe.py: {what} ended with status {proc.returncode}; nothing further is started")
    return out


def family(name):
    if "rank_kernel" in name:
        return "ranks"
    if "rank_finish_kernel" in name:
        return "finish"
    if any(k in name for k in ("rank_kendall_kernel", "zero_kernel", "covw_stats_kernel", "covw_gram_kernel")):
        return "gram"
    if any(k in name for k in ("cholw_", "assoc_rowsum_kernel")):
        return "repair"
    return None


def read_split(where, n):
    """[{family: ms}] of the second call of each of the n configurations from the trace's CSV, or None when it cannot be read that way."""
    try:
        rows = []
        for path in glob.glob(os.path.join(where, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    low = {k.lower(): v for k, v in r.items()}
                    rows.append((int(low["start_timestamp"]), int(low["end_timestamp"]), low["kernel_name"]))
        rows.sort()
        calls = []
        for start, end, name in rows:
            fam = family(name)
            if fam == "ranks":
                calls.append({"ranks": 0.0, "gram": 0.0, "finish": 0.0, "repair": 0.0})
            if fam and calls:
                calls[-1][fam] += (end - start) * 1e-6
        if len(calls) != 2 * n:
            print(f"# kernel trace: {len(calls)} calls found, {2 * n} expected; no split for this step", flush=True)
            return None
        return [calls[2 * i + 1] for i in range(n)]
    except (OSError, KeyError, ValueError) as e:
        print(f"# kernel trace: the CSV cannot be read ({type(e).__name__}: {e}); no split for this step", flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_probe.txt"))
    ap.add_argument("--dims", default="288,1024,2048")
    ap.add_argument("--rows", default="512,2048")
    ap.add_argument("--batch", default="1,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds for every child step")
    ap.add_argument("--trace-dir", default=None, help="where the kernel traces are written (default: a temporary directory)")
    ap.add_argument("--child", choices=("trace", "time"), help=argparse.SUPPRESS)
    ap.add_argument("--D", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--N", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return (child_trace if args.child == "trace" else child_time)(args, args.D, args.N)
    profiler = None if args.no_split else shutil.which("rocprofv3")
    if not args.no_split and profiler is None:
        print("# rocprofv3 is not installed; no split", flush=True)
    trace_root = args.trace_dir or tempfile.mkdtemp(prefix="rank_probe_trace_")
    configs = group_configs(args)
    lines = []
    for D in [int(d) for d in args.dims.split(",")]:
        for N in [int(n) for n in args.rows.split(",")]:
            child = [sys.executable, os.path.abspath(__file__), "--batch", args.batch, "--reps", str(args.reps), "--D", str(D), "--N", str(N)]
            split = None
            if profiler:
                where = os.path.join(trace_root, f"d{D}_n{N}")
                run_step([profiler, "--kernel-trace", "--output-format", "csv", "-d", where, "--"] + child + ["--child", "trace"],
                         args.step_timeout, f"the traced run of D = {D}, N = {N}")
                split = read_split(where, len(configs))
            out = run_step(child + ["--child", "time"], args.step_timeout, f"the timed run of D = {D}, N = {N}")
            results = [json.loads(line[len(RESULT):]) for line in out.splitlines() if line.startswith(RESULT)]
            if len(results) != 1 + len(configs):
                raise SystemExit(f"rank_probe.py: the timed run of D = {D}, N = {N} reported {len(results)} lines, {1 + len(configs)} expected")
            if not lines:
                lines = [f"# scripts/rank_probe.py on {results[0]['device']}; torch {results[0]['torch']}; medians of {args.reps} after one warm-up",
                         "# host = prepare_data.rank_correlation_host, one table (once when over 2 s); device = HIP events around "
                         "HipLib.rank_correlation; ranks / gram / finish / repair = kernel families of one repaired call, from a kernel trace; "
                         "e2e = main.rank_correlation on host arrays",
                         "# Kendall: rate = K 2 P D (D + 1) / 2 integer operations over the Gram time; share of the dense int8 MFMA peak "
                         "(5 POP/s); one Gram variant (signs made in the workgroup, shared through LDS)",
                         f"{'method':>8} {'D':>5} {'N':>5} {'K':>2} {'chunks':>6} {'host ms':>10} {'device ms':>10} {'+repair ms':>11} {'ranks':>8} "
                         f"{'gram':>9} {'finish':>7} {'repair':>8} {'e2e ms':>9} {'host/e2e':>8} {'max dev':>8} {'TOP/s':>7} {'of peak':>7}"]
                print("\n".join(lines), flush=True)
            for index, r in enumerate(results[1:]):
                K, method = configs[index]
                assert (r["K"], r["method"]) == (K, method)
                fam = split[index] if split else None
                parts = (f"{fam['ranks']:>8.2f} {fam['gram']:>9.2f} {fam['finish']:>7.2f} {fam['repair']:>8.2f}" if fam
                         else f"{'-':>8} {'-':>9} {'-':>7} {'-':>8}")
                rate, chunks = f"{'':>7} {'':>7}", "-"
                if method == "kendall":
                    ops = K * 2.0 * (N * (N - 1) / 2.0) * (D * (D + 1) / 2.0)
                    per_s = ops / ((fam["gram"] if fam else r["dev_ms"]) * 1e-3)
                    rate, chunks = f"{per_s * 1e-12:>7.1f} {100.0 * per_s / I8_PEAK:>6.2f}%", str(r["chunks"])
                line = (f"{method:>8} {D:>5} {N:>5} {K:>2} {chunks:>6} {r['host_ms']:>10.1f} {r['dev_ms']:>10.2f} {r['rep_ms']:>11.2f} {parts} "
                        f"{r['e2e_ms']:>9.2f} {K * r['host_ms'] / r['e2e_ms']:>8.1f} {r['dev']:>8.1e} {rate}")
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
