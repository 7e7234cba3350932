#!/usr/bin/env python3
"""Times the per-sample scores on the device (uglad_sample_scores, csrc/score_wide.h) against the fp64 numpy formulation of the same
numbers, on the same models and table.

    python scripts/score_probe.py [--out profiles/score_probe.txt] [--dims 288,1024,2048] [--rows 512,65536]

Problems: K well conditioned precision matrices of order D (asymmetric at 1e-5, as a fitted precision_ is), ONE table of N rows scored by
all of them.  Columns:
  host ms     wall clock of ((Xc @ P) * Xc).sum(1) and slogdet per model in fp64 numpy, P = (Theta + Theta^T) / 2, Xc = X - mu
  device ms   HIP events around the enqueue of HipLib.sample_scores on fp64 inputs already on the device
  e2e ms      wall clock of main.sample_scores on host arrays: upload as fp64, kernels, download of the (K, N) results
each the median of the timed runs after one warm-up.  q / dens: the device's outputs against the host's, the largest error over the rows
divided by the derived bound of tests/test_sample_scores.py (<= 1 means inside the bound).
No threshold is assumed: the table reports, whichever side wins; the route stays all-device."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

EPS = 2.0 ** -53


def make_models(K, D, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((K, D, D))
    P = A @ A.transpose(0, 2, 1) / D + 0.5 * np.eye(D)
    B = rng.standard_normal((K, D, D))
    return P + 1e-5 * (B - B.transpose(0, 2, 1)), 0.4 + 0.2 * rng.random((K, D))


def host_scores(theta, mu, X):
    K, D = mu.shape
    q, dens = np.empty((K, len(X))), np.empty((K, len(X)))
    for k in range(K):
        P = 0.5 * (theta[k] + theta[k].T)
        Xc = X - mu[k]
        q[k] = ((Xc @ P) * Xc).sum(1)
        dens[k] = 0.5 * (np.linalg.slogdet(P)[1] - D * np.log(2.0 * np.pi) - q[k])
    return q, dens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_probe.txt"))
    ap.add_argument("--dims", default="288,1024,2048")
    ap.add_argument("--rows", default="512,65536")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from uglad_amd import _lib, main as um

    if not torch.cuda.is_available():
        raise SystemExit("score_probe.py measures on the GPU; none is visible")
    lib = _lib.get_lib()
    lines = [f"# scripts/score_probe.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {args.reps} after one warm-up",
             "# host = ((Xc @ P) * Xc).sum(1) + slogdet per model (fp64 numpy); device = HIP events around HipLib.sample_scores; e2e = "
             "main.sample_scores on host arrays; one table for all K models",
             f"{'D':>5} {'N':>6} {'K':>2} {'host ms':>10} {'device ms':>10} {'e2e ms':>9} {'host/e2e':>9} {'q/bound':>8} {'dens/bound':>10}"]
    print("\n".join(lines), flush=True)
    for D in [int(d) for d in args.dims.split(",")]:
        for N in [int(n) for n in args.rows.split(",")]:
            X = np.random.default_rng(D + N).random((N, D))
            for K in (1, 4):
                theta, mu = make_models(K, D, seed=D + K)
                host_ms, dev_ms, e2e_ms = [], [], []
                for rep in range(args.reps + 1):
                    t0 = time.perf_counter()
                    h_q, h_dens = host_scores(theta, mu, X)
                    if rep:
                        host_ms.append((time.perf_counter() - t0) * 1e3)
                Xd, Pd, mud = (torch.from_numpy(a).cuda() for a in (X[None], theta, mu))
                for rep in range(args.reps + 1):
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    d_q, d_dens, _ = lib.sample_scores(Xd, Pd, mud)
                    stop.record()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e = um.sample_scores(theta, mu, X)
                    if rep:  # (the first run is the warm-up of both)
                        dev_ms.append(start.elapsed_time(stop))
                        e2e_ms.append((time.perf_counter() - t0) * 1e3)
                assert np.array_equal(e.mahalanobis, d_q.cpu().numpy()) and np.array_equal(e.log_density, d_dens.cpu().numpy())
                r_q = r_dens = 0.0
                for k in range(K):  # the derived bounds of the test suite
                    P = 0.5 * (theta[k] + theta[k].T)
                    Xc = np.abs(X - mu[k])
                    b_q = 4.0 * (D + 2) * EPS * ((Xc @ np.abs(P)) * Xc).sum(1)
                    b_dens = 0.5 * (b_q + D * D * np.linalg.cond(P) * EPS)
                    r_q = max(r_q, float((np.abs(e.mahalanobis[k] - h_q[k]) / b_q).max()))
                    r_dens = max(r_dens, float((np.abs(e.log_density[k] - h_dens[k]) / b_dens).max()))
                h, d, ee = statistics.median(host_ms), statistics.median(dev_ms), statistics.median(e2e_ms)
                line = f"{D:>5} {N:>6} {K:>2} {h:>10.1f} {d:>10.2f} {ee:>9.2f} {h / ee:>9.1f} {r_q:>8.2f} {r_dens:>10.2f}"
                print(line, flush=True)
                lines.append(line)
                del Xd, Pd, mud
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
