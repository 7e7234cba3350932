#!/usr/bin/env python3
"""Times the device covariance front-end beyond D = 256 (uglad_covariance_wide, csrc/cov_wide.h) against the host path it replaces
under device_covariance=True (prepare_data.get_covariance: fp64 numpy, one non-symmetric eigvals per table), on the same tables.

    python scripts/cov_wide_probe.py [--out profiles/cov_wide_probe.txt] [--dims 288,1024,2048]

Tables: K x N x D.  N = D / 2: mixed Gaussian factors, singular, so both sides repair them and the device bisects; N = 2 D: uniform columns,
well conditioned, so the device leaves after the one factorisation at the threshold while the host still runs its eigvals.  Columns:
  host ms     wall clock of get_covariance + the upload of S (what inputs._covariance does without device_covariance), one run
  device ms   HIP events around the enqueue of covariance_wide on tables already on the device: median of the timed runs after a warm-up
  e2e ms      wall clock of inputs._covariance under device_covariance(True): upload of the fp64 tables, kernels, synchronise (median)
No threshold: the table reports, whichever side wins."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_tables(K, N, D, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(K):
        if N < D:
            X = rng.standard_normal((N, D)) @ (rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D))
        else:
            X = rng.random((N, D))
        X = (X - X.min(0)) / (X.max(0) - X.min(0))  # fit() hands min-max normalised tables to the front-end
        out.append(X)
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cov_wide_probe.txt"))
    ap.add_argument("--dims", default="288,1024,2048")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from uglad_amd import _lib, inputs, main as um
    from uglad_amd.utils import prepare_data

    if not torch.cuda.is_available():
        raise SystemExit("cov_wide_probe.py measures on the GPU; none is visible")
    lib = _lib.get_lib()
    lines = [f"# scripts/cov_wide_probe.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; reps {args.reps} after one warm-up",
             "# host = prepare_data.get_covariance (fp64 numpy) + upload; device = HIP events around covariance_wide; e2e = inputs._covariance "
             "under device_covariance(True)",
             f"{'D':>5} {'N':>5} {'K':>2} {'repaired':>8} {'host ms':>10} {'device ms':>10} {'e2e ms':>9} {'host/e2e':>9} {'rel-Frobenius':>14}"]
    print("\n".join(lines), flush=True)
    for D in [int(d) for d in args.dims.split(",")]:
        for N in (D // 2, 2 * D):
            for K in (1, 4):
                X = make_tables(K, N, D, seed=D + N + K)
                t0 = time.perf_counter()
                S_host = inputs._to_dev(prepare_data.get_covariance(X, offset=0.1))
                torch.cuda.synchronize()
                host_ms = (time.perf_counter() - t0) * 1e3
                Xd = torch.from_numpy(X).cuda()
                dev_ms, e2e_ms = [], []
                for rep in range(args.reps + 1):
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    S_dev, mn, repaired = lib.covariance_wide(Xd, normalize=False, eval_offset=0.1, repair=True, return_min_eig=True)
                    stop.record()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with um.device_covariance(True):
                        S_e2e = inputs._covariance(list(X), 0.1)
                    torch.cuda.synchronize()
                    if rep:  # (the first run is the warm-up of both)
                        dev_ms.append(start.elapsed_time(stop))
                        e2e_ms.append((time.perf_counter() - t0) * 1e3)
                assert torch.equal(S_e2e, S_dev)
                err = float((S_dev.double() - S_host.double()).norm() / S_host.double().norm())
                d, e = statistics.median(dev_ms), statistics.median(e2e_ms)
                line = (f"{D:>5} {N:>5} {K:>2} {int(repaired.sum()):>6}/{K} {host_ms:>10.1f} {d:>10.2f} {e:>9.2f} {host_ms / e:>9.1f} {err:>14.2e}")
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
