#!/usr/bin/env python3
"""Times the wide fp64 utilities that the centred Gram product (csrc/cov_wide.h) and the symmetriser (csrc/chol_wide.h) feed, on two builds
of the library in ONE process, alternating: the in-tree build and another one (the parent's), on the tables and by the clocks of
table_probe.py, cov_wide_probe.py and score_probe.py, without their host baselines.

    python scripts/wide_feeders_probe.py --parent PARENT/libuglad_hip.so [--out profiles/wide_feeders_vs_parent.txt] [--dims 288,1024,2048]

Per row `--rounds` rounds of (parent, new), each `--reps` timed runs after one warm-up.  Columns: the parent's median, the spread of ALL
its timed runs of that row in this call (min .. max), the new build's median, and whether it lies inside that spread.
  spectrum device   HIP events around HipLib.eigvalsh_wide on K covariances on the device            (table_probe.py: device ms)
  spectrum e2e      wall clock of analyse_condition_number(table, device=True), K host tables in turn (table_probe.py: e2e ms)
  process_table     wall clock of process_table(COND_NUM=1e4, device=True) on the table with planted collinear columns
  cov device        HIP events around HipLib.covariance_wide with the repair                         (cov_wide_probe.py: device ms)
  scores device     HIP events around HipLib.sample_scores, one table for K models                   (score_probe.py: device ms)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def events_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_feeders_vs_parent.txt"))
    ap.add_argument("--dims", default="288,1024,2048")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    args = ap.parse_args()
    import cov_wide_probe
    import score_probe
    import table_probe
    from uglad_amd import _lib
    from uglad_amd.utils import prepare_data

    if not torch.cuda.is_available():
        raise SystemExit("wide_feeders_probe.py measures on the GPU; none is visible")
    builds = {"parent": _lib.HipLib(os.path.abspath(args.parent)), "new": _lib.get_lib()}
    lines = [f"# scripts/wide_feeders_probe.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; parent = the build of the commit before; per row "
             f"{args.rounds} rounds of (parent, new), {args.reps} timed runs each after one warm-up; ms",
             f"{'row':<18} {'D':>5} {'N':>6} {'K':>2} {'parent':>9} {'parent min .. max':>21} {'new':>9} {'new/parent':>10}  inside"]
    print("\n".join(lines), flush=True)
    outside = 0

    def row(name, D, N, K, clock, call):  # call(lib): one run on that build
        nonlocal outside
        t = {b: [] for b in builds}
        for _ in range(args.rounds):
            for b, lib in builds.items():
                _lib._instance = lib  # (what the e2e paths pick up)
                t[b] += [clock(lambda: call(lib)) for _ in range(args.reps + 1)][1:]
        _lib._instance = builds["new"]
        p, n, lo, hi = statistics.median(t["parent"]), statistics.median(t["new"]), min(t["parent"]), max(t["parent"])
        outside += not lo <= n <= hi
        line = f"{name:<18} {D:>5} {N:>6} {K:>2} {p:>9.2f} {lo:>9.2f} .. {hi:>9.2f} {n:>9.2f} {n / p:>10.3f}  {'yes' if lo <= n <= hi else 'NO'}"
        print(line, flush=True)
        lines.append(line)

    dims = [int(d) for d in args.dims.split(",")]
    for D in dims:
        for N in (D // 2, 2 * D):
            for K in (1, 4):
                X = np.random.default_rng(D + N + K).random((K, N, D))
                Sd = torch.from_numpy(np.stack([np.cov(x.T, bias=1) for x in X])).cuda()
                row("spectrum device", D, N, K, events_ms, lambda lib: lib.eigvalsh_wide(Sd))
                row("spectrum e2e", D, N, K, wall_ms, lambda lib: [prepare_data.analyse_condition_number(x, VERBOSE=False, device=True) for x in X])
                Xd = torch.from_numpy(cov_wide_probe.make_tables(K, N, D, seed=D + N + K)).cuda()
                row("cov device", D, N, K, events_ms, lambda lib: lib.covariance_wide(Xd, normalize=False, eval_offset=0.1, repair=True, return_min_eig=True))
                del Sd, Xd
        for N in (512, 65536):
            Xd = torch.from_numpy(np.random.default_rng(D + N).random((1, N, D))).cuda()
            for K in (1, 4):
                Pd, mud = (torch.from_numpy(a).cuda() for a in score_probe.make_models(K, D, seed=D + K))
                row("scores device", D, N, K, events_ms, lambda lib: lib.sample_scores(Xd, Pd, mud))
        table = table_probe.collinear_table(2 * D, D, seed=D)
        row("process_table", D, 2 * D, 1, wall_ms, lambda lib: prepare_data.process_table(table, COND_NUM=1e4, VERBOSE=False, device=True))
    lines.append(f"# rows whose new median lies outside the parent's spread: {outside} of {len(lines) - 2}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
