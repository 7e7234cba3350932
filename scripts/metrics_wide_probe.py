#!/usr/bin/env python3
"""Times the device support-recovery metrics beyond D = 256 (uglad_support_metrics_wide, csrc/metrics_wide.h) against the host formulation it
replaces in main.device_report_metrics (download of both matrices + utils.metrics.report_metrics_all per pair), on the same pairs.

    python scripts/metrics_wide_probe.py [--out profiles/metrics_wide_probe.txt] [--dims 288,1024,2048]

Pairs: K (true, predicted) fp32 matrices of order D on the device; the truth has the given density of non-zero edges, the prediction keeps
half of its entries, rounded to 3 decimals (tied scores, exact zeros).  Columns:
  host ms     wall clock of the download of both matrices and report_metrics_all for every pair
  device ms   HIP events around the enqueue of support_metrics_wide on tensors already on the device
  e2e ms      wall clock of main.device_report_metrics on those tensors: kernels, download of the (K, 11) result, the dicts
each the median of the timed runs after one warm-up.  In every run the device column's call follows the host's CPU-only section and the
e2e call follows that one directly, so the e2e figure can come out below the device figure: they are two calls, not parts of one.
same = the device's 3-decimal report equals the host's for every pair and key.
The device sorts the edges whatever their labels: at one (D, K) the 50 % rows must agree with the 2 % rows within timer noise (2x); a
kernel with a (true edges) x (edges) term would differ by 25x.  No threshold is assumed: the table reports, whichever side wins."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_pairs(K, D, density, seed):
    rng = np.random.default_rng(seed)
    T, G = np.zeros((K, D, D), dtype=np.float32), np.zeros((K, D, D), dtype=np.float32)
    for k in range(K):
        t = np.triu(rng.random((D, D)) < density, 1)
        T[k] = (t + t.T) * rng.standard_normal((D, D)) + np.eye(D)
        s = np.triu(np.round(rng.random((D, D)), 3) * (rng.random((D, D)) < 0.5), 1)
        G[k] = s + s.T + np.eye(D)
    return T, G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_wide_probe.txt"))
    ap.add_argument("--dims", default="288,1024,2048")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from uglad_amd import _lib, main as um

    if not torch.cuda.is_available():
        raise SystemExit("metrics_wide_probe.py measures on the GPU; none is visible")
    lib = _lib.get_lib()
    lines = [f"# scripts/metrics_wide_probe.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {args.reps} after one warm-up",
             "# host = download + utils.metrics.report_metrics_all per pair; device = HIP events around support_metrics_wide; e2e = "
             "main.device_report_metrics on device tensors",
             f"{'D':>5} {'K':>2} {'truth':>6} {'host ms':>10} {'device ms':>10} {'e2e ms':>9} {'host/e2e':>9} {'same':>5}"]
    print("\n".join(lines), flush=True)
    for D in [int(d) for d in args.dims.split(",")]:
        for K in (1, 4):
            for density in (0.02, 0.5):
                T, G = make_pairs(K, D, density, seed=D + K)
                Td, Gd = torch.from_numpy(T).cuda(), torch.from_numpy(G).cuda()
                host_ms, dev_ms, e2e_ms = [], [], []
                for rep in range(args.reps + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    Tn, Gn = Td.cpu().numpy(), Gd.cpu().numpy()
                    host = [um.report_metrics_all(Tn[k], Gn[k]) for k in range(K)]
                    t1 = time.perf_counter()
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    lib.support_metrics_wide(Td, Gd)
                    stop.record()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    got = um.device_report_metrics(Td, Gd)
                    t3 = time.perf_counter()
                    if rep:  # (the first run is the warm-up of all three)
                        host_ms.append((t1 - t0) * 1e3)
                        dev_ms.append(start.elapsed_time(stop))
                        e2e_ms.append((t3 - t2) * 1e3)
                same = all(np.array_equal(np.array(list(a.values())), np.array(list(b.values())), equal_nan=True) for a, b in zip(got, host))
                h, d, e = statistics.median(host_ms), statistics.median(dev_ms), statistics.median(e2e_ms)
                line = f"{D:>5} {K:>2} {density:>6.0%} {h:>10.1f} {d:>10.3f} {e:>9.2f} {h / e:>9.1f} {'yes' if same else 'NO':>5}"
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
