#!/usr/bin/env python3
"""Times the device conditional Gaussian beyond D = 256 (uglad_conditional_mean_wide, csrc/after_wide.h) against the host formulation it
replaces (after._conditional_gaussian_host: np.linalg.inv and slogdet in fp64, one problem at a time), on the same problems.

    python scripts/after_wide_probe.py [--out profiles/after_wide_probe.txt] [--dims 288,1024,2048]

Problems: K dense, well conditioned precision matrices of order D, a third of the coordinates observed.  Columns:
  host ms     wall clock of _conditional_gaussian_host, download and upload included (it always forms the covariance)
  device ms   HIP events around the enqueue of conditional_mean_wide on fp64 inputs already on the device
  e2e ms      wall clock of main.conditional_gaussian_batch on host arrays: upload as fp64, kernels, synchronise
each the median of the timed runs after one warm-up; cov = whether cond_cov is asked for (compute_map_estimate asks for none).
mean / cov / logp: the device's outputs against the host's (max-abs over max |mean|; relative Frobenius; absolute), in the fp32 layout both return.
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


def make_problems(K, D, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((K, D, D))
    P = A @ A.transpose(0, 2, 1) / D + 0.5 * np.eye(D)
    P = 0.5 * (P + P.transpose(0, 2, 1))
    mask = np.zeros((K, D), dtype=np.float32)
    for k in range(K):
        mask[k, rng.choice(D, D // 3, replace=False)] = 1.0
    return P, rng.random((K, D)), mask, rng.random((K, D))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "after_wide_probe.txt"))
    ap.add_argument("--dims", default="288,1024,2048")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from uglad_amd import _lib, after, main as um

    if not torch.cuda.is_available():
        raise SystemExit("after_wide_probe.py measures on the GPU; none is visible")
    lib = _lib.get_lib()
    dev = _lib.device()
    lines = [f"# scripts/after_wide_probe.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {args.reps} after one warm-up",
             "# host = after._conditional_gaussian_host (fp64 numpy, per problem); device = HIP events around conditional_mean_wide; e2e = "
             "main.conditional_gaussian_batch on host arrays",
             f"{'D':>5} {'K':>2} {'cov':>4} {'host ms':>10} {'device ms':>10} {'e2e ms':>9} {'host/e2e':>9} {'mean':>9} {'cov':>9} {'logp':>9}"]
    print("\n".join(lines), flush=True)
    for D in [int(d) for d in args.dims.split(",")]:
        for K in (1, 4):
            P, mu, mask, vals = make_problems(K, D, seed=D + K)
            host_ms = []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                h_full, h_cov, h_logp = after._conditional_gaussian_host(P, mu, mask, vals, False, dev)
                torch.cuda.synchronize()
                if rep:
                    host_ms.append((time.perf_counter() - t0) * 1e3)
            h = statistics.median(host_ms)
            Pd, mud, md, vd = (torch.from_numpy(a).cuda() for a in (P, mu, mask, vals))
            for want_cov in (True, False):
                dev_ms, e2e_ms = [], []
                for rep in range(args.reps + 1):
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    d_full, d_cov, d_logp = lib.conditional_mean_wide(Pd, mud, md, vd, want_cov=want_cov)
                    stop.record()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e_full, e_cov, e_logp = um.conditional_gaussian_batch(P, mu, mask, vals, want_cov=want_cov)
                    torch.cuda.synchronize()
                    if rep:  # (the first run is the warm-up of both)
                        dev_ms.append(start.elapsed_time(stop))
                        e2e_ms.append((time.perf_counter() - t0) * 1e3)
                assert torch.equal(e_full, d_full.float()) and torch.equal(e_logp, d_logp.float())
                err_mean = float((e_full - h_full).abs().max() / h_full.abs().max())
                err_logp = float((e_logp - h_logp).abs().max())
                err_cov = float((e_cov.double() - h_cov.double()).norm() / h_cov.double().norm()) if want_cov else float("nan")
                d, e = statistics.median(dev_ms), statistics.median(e2e_ms)
                line = (f"{D:>5} {K:>2} {'yes' if want_cov else 'no':>4} {h:>10.1f} {d:>10.2f} {e:>9.2f} {h / e:>9.1f} {err_mean:>9.1e} "
                        f"{err_cov:>9.1e} {err_logp:>9.1e}")
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
