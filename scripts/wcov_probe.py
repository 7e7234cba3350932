#!/usr/bin/env python3
"""Times the covariances of ONE table under R weightings of its rows (uglad_weighted_covariance, csrc/wcov_wide.h) against the host
formulation, against the route a user had before it -- R resampled tables materialised on the host, uploaded, uglad_covariance_wide --
and against uglad_covariance_wide on the single table; then fit_stability against R separate fits on the same resamples.

    python scripts/wcov_probe.py [--out profiles/wcov_probe.txt] [--dims 288,1024,2048] [--resamples 1,4,16,64]

This process never opens the GPU.  Every (D, N), and the fit block, is a child process of its own, in a process group of its own and under
its own time limit (--step-timeout).  A step that runs out of time has its whole group killed; a step that times out, dies by a signal or
ends with a non-zero status ends the probe with a non-zero status and nothing further is started.

Tables: N x D, three latent factors plus noise plus 50, N = D / 2 and 2 D.  Weightings: half subsamples (even r) and bootstrap resamples
(odd r), seeded.  Columns (ms; medians of --reps timed runs after one warm-up; a host run that takes more than two seconds is timed once):
  host        prepare_data.weighted_covariance_host on the R weightings: fp64 numpy, one BLAS product per weighting
  material    the R resampled tables built on the host (np.repeat), uploaded, HipLib.covariance_wide without repair: wall clock, synchronised
  device      HIP events around HipLib.weighted_covariance without the repair, table and weights on the device
  +repair     the same with the repair (25 blocked Cholesky factorisations for a weighting that fails the test at 1e-6)
  e2e         wall clock of main.weighted_covariance on host arrays: upload, kernels with repair, synchronise, the eigenvalues read back
  dev/R       device over R: the cost of one weighting
  cov_wide    HIP events around HipLib.covariance_wide without repair on the single table, in the same run
  ratio       dev/R over cov_wide: below 1 where the staged chunk is shared to effect
  dev/bound   the largest deviation of the device's fp64 matrices from `host` over all R weightings (R <= 4 only), as a fraction of the
              derived bound 4 (N + 8) 2^-53 sqrt(q_i q_j) / s (tests/test_weighted_covariance.py)
The second block: uGLAD_GL.fit_stability (one table, one device call for the R + 1 covariances, one shared model) against R separate
uGLAD_GL.fit calls on the materialised subsamples, wall clock, once each after a warm-up of either; and the mean selection frequency on the
true and on the false edges of the generating graph.  At the end the resource table of the new kernels (scripts/kernel_meta.py: registers,
LDS, scratch), read from the built library.  No time here is an acceptance criterion: the table is the record."""
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


def make_table(N, D, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, 3)) @ rng.standard_normal((3, D)) + rng.standard_normal((N, D)) + 50.0


def make_weights(N, R, seed):
    import numpy as np

    from uglad_amd.utils import prepare_data as pd_

    rng = np.random.default_rng(seed)
    return np.stack([pd_.resample_weights(N, 1, "bootstrap" if r % 2 else "subsample", rng=rng)[0] for r in range(R)])


def median_ms(fn, reps):
    out = []
    for rep in range(reps + 1):
        ms = fn()
        if rep:
            out.append(ms)
        if rep == 0 and ms > 2000.0:
            return ms  # (a long host run: once)
    return statistics.median(out)


def wall(call, sync):
    def run():
        t0 = time.perf_counter()
        run.out = call()
        sync()
        return (time.perf_counter() - t0) * 1e3
    return run


# ============================================================================================ the children: the only GPU processes
def child(args, D, N):
    """The timed runs of one (D, N): one RESULT line of JSON per R."""
    import numpy as np
    import torch

    from uglad_amd import _lib, main as um
    from uglad_amd.utils import prepare_data as pd_

    if not torch.cuda.is_available():
        raise SystemExit("wcov_probe.py measures on the GPU; none is visible")
    lib = _lib.get_lib()
    print(RESULT + json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__}), flush=True)
    X = make_table(N, D, seed=7 * D + N)
    Xd = torch.from_numpy(X).cuda()
    Z = X - X.mean(axis=0)

    def timed(call):
        def run():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            run.out = call()
            stop.record()
            torch.cuda.synchronize()
            return start.elapsed_time(stop)
        return run

    wide_ms = median_ms(timed(lambda: lib.covariance_wide(Xd[None], normalize=False, repair=False)), args.reps)
    for R in [int(r) for r in args.resamples.split(",")]:
        W = make_weights(N, R, seed=D + N + R)
        Wd = torch.from_numpy(W).cuda()
        host = wall(lambda: pd_.weighted_covariance_host(X, W), lambda: None)
        host_ms = median_ms(host, args.reps)

        def materialised():
            tables = [np.repeat(X, w.astype(np.int64), axis=0) for w in W]
            groups = {}
            for r, t in enumerate(tables):  # (covariance_wide takes tables of one shape: one call per row count)
                groups.setdefault(t.shape[0], []).append(r)
            return [lib.covariance_wide(torch.from_numpy(np.stack([tables[r] for r in idx])).cuda(), normalize=False, repair=False)
                    for idx in groups.values()]

        mat_ms = median_ms(wall(materialised, torch.cuda.synchronize), args.reps)
        plain = timed(lambda: lib.weighted_covariance(Xd, Wd, repair=False, want_f64=R <= 4))
        repaired = timed(lambda: lib.weighted_covariance(Xd, Wd, eval_offset=0.1, repair=True))
        e2e = wall(lambda: um.weighted_covariance(X, W, repair=True, eval_offset=0.1), torch.cuda.synchronize)
        dev_ms, rep_ms, e2e_ms = median_ms(plain, args.reps), median_ms(repaired, args.reps), median_ms(e2e, args.reps)
        assert torch.equal(e2e.out[0], repaired.out.S) and not repaired.out.info.any()
        ratio = None
        if R <= 4:
            q = W @ (Z * Z)
            bound = 4.0 * (N + 8) * 2.0 ** -53 * np.sqrt(q[:, :, None] * q[:, None, :]) / W.sum(axis=1)[:, None, None]
            ratio = float((np.abs(plain.out.S64.cpu().numpy() - host.out[0]) / bound).max())
        print(RESULT + json.dumps({"R": R, "host_ms": host_ms, "mat_ms": mat_ms, "dev_ms": dev_ms, "rep_ms": rep_ms, "e2e_ms": e2e_ms,
                                   "wide_ms": wide_ms, "of_bound": ratio}), flush=True)
        del plain, repaired, e2e, host
        torch.cuda.empty_cache()


def fit_child(args):
    """fit_stability against R separate fits on the same subsamples: D = 64, N = 512, R = 16, few epochs."""
    import numpy as np
    import torch

    import uglad_amd
    from uglad_amd.utils import prepare_data as pd_

    D, N, R, epochs = 64, 512, 16, 20
    Xb, theta = pd_.get_data(D, [0.05, 0.1], N, rng=64)
    X = Xb[0]
    kw = dict(epochs=epochs, L=15, verbose=False)

    def stability():
        torch.manual_seed(0)
        est = uglad_amd.uGLAD_GL()
        est.fit_stability(X, n_resamples=R, seed=1, **kw)
        return est

    def separate():
        out = []
        for w in pd_.resample_weights(N, R, rng=1):
            torch.manual_seed(0)
            est = uglad_amd.uGLAD_GL()
            est.fit(X[w > 0], **kw)
            out.append(est.precision_)
        return np.stack(out)

    one, many = wall(stability, torch.cuda.synchronize), wall(separate, torch.cuda.synchronize)
    one(), many()  # warm-up
    one_ms, many_ms = one(), many()
    est = one.out
    freq_separate, _, instability_separate = uglad_amd.edge_frequency(many.out, sparsity=0.1)
    true = (np.abs(theta[0]) > 0) & ~np.eye(D, dtype=bool)
    false = ~true & ~np.eye(D, dtype=bool)
    print(RESULT + json.dumps({"D": D, "N": N, "R": R, "epochs": epochs, "stability_ms": one_ms, "separate_ms": many_ms,
                               "true_edges": int(true.sum() // 2), "freq_true": float(est.edge_frequency_[true].mean()),
                               "freq_false": float(est.edge_frequency_[false].mean()), "instability": float(est.instability_),
                               "freq_true_separate": float(freq_separate[true].mean()), "freq_false_separate": float(freq_separate[false].mean()),
                               "instability_separate": float(instability_separate), "stable_08": len(est.stable_edges(0.8))}), flush=True)


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
        raise SystemExit(f"wcov_probe.py: {what} ran past its limit of {limit} s; its process group was killed and nothing further is started")
    if proc.returncode != 0:
        raise SystemExit(f"wcov_probe.py: {what} ended with status {proc.returncode}; nothing further is started")
    return [json.loads(line[len(RESULT):]) for line in out.splitlines() if line.startswith(RESULT)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wcov_probe.txt"))
    ap.add_argument("--dims", default="288,1024,2048")
    ap.add_argument("--resamples", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds for every child step")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--fit-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--D", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--N", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args, args.D, args.N)
    if args.fit_child:
        return fit_child(args)
    resamples = [int(r) for r in args.resamples.split(",")]
    lines = []
    for D in [int(d) for d in args.dims.split(",")]:
        for N in (D // 2, 2 * D):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--resamples", args.resamples, "--reps", str(args.reps), "--D", str(D),
                   "--N", str(N)]
            results = run_step(cmd, args.step_timeout, f"the timed run of D = {D}, N = {N}")
            if len(results) != 1 + len(resamples):
                raise SystemExit(f"wcov_probe.py: the timed run of D = {D}, N = {N} reported {len(results)} lines, {1 + len(resamples)} expected")
            if not lines:
                lines = [f"# scripts/wcov_probe.py on {results[0]['device']}; torch {results[0]['torch']}; medians of {args.reps} after one warm-up "
                         "(a host run over 2 s: once); weightings: half subsamples (even r) and bootstrap resamples (odd r)",
                         "# host = prepare_data.weighted_covariance_host; material = R resampled tables built on the host, uploaded, "
                         "HipLib.covariance_wide without repair (wall clock); device = HIP events around HipLib.weighted_covariance; e2e = "
                         "main.weighted_covariance on host arrays; cov_wide = HipLib.covariance_wide without repair on the single table; ratio = "
                         "(device / R) / cov_wide; dev/bound = the largest |device - host| as a fraction of 4 (N + 8) 2^-53 sqrt(q_i q_j) / s",
                         f"{'D':>5} {'N':>5} {'R':>3} {'host ms':>10} {'material ms':>12} {'device ms':>10} {'+repair ms':>11} {'e2e ms':>10} "
                         f"{'dev/R ms':>9} {'cov_wide':>9} {'ratio':>6} {'dev/bound':>9}"]
                print("\n".join(lines), flush=True)
            for R, r in zip(resamples, results[1:]):
                assert r["R"] == R
                of_bound = f"{r['of_bound']:>9.3f}" if r["of_bound"] is not None else f"{'':>9}"
                line = (f"{D:>5} {N:>5} {R:>3} {r['host_ms']:>10.1f} {r['mat_ms']:>12.1f} {r['dev_ms']:>10.2f} {r['rep_ms']:>11.2f} "
                        f"{r['e2e_ms']:>10.2f} {r['dev_ms'] / R:>9.3f} {r['wide_ms']:>9.3f} {r['dev_ms'] / R / r['wide_ms']:>6.2f} {of_bound}")
                print(line, flush=True)
                lines.append(line)
    (f,) = run_step([sys.executable, os.path.abspath(__file__), "--fit-child"], args.step_timeout, "the fit block")
    block = ["#", f"# fit_stability against {f['R']} separate fit calls on the same half subsamples: D = {f['D']}, N = {f['N']}, {f['epochs']} epochs, "
             "L = 15; wall clock, once each after a warm-up of either",
             f"fit_stability ms {f['stability_ms']:.0f}   separate fits ms {f['separate_ms']:.0f}   separate / fit_stability "
             f"{f['separate_ms'] / f['stability_ms']:.2f}",
             f"selection frequency at sparsity 0.1 over the {f['true_edges']} true edges / over the false ones: fit_stability "
             f"{f['freq_true']:.3f} / {f['freq_false']:.3f} (instability {f['instability']:.4f}, {f['stable_08']} edges at >= 0.8); separate fits "
             f"{f['freq_true_separate']:.3f} / {f['freq_false_separate']:.3f} (instability {f['instability_separate']:.4f})"]
    print("\n".join(block), flush=True)
    lines += block
    # the compile-time record of the new kernels (scripts/kernel_meta.py reads the built library; nothing is run)
    for flt in ("wcov_", "gw_frequency"):
        meta = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_meta.py"), "--filter", flt, "--loops"],
                              capture_output=True, text=True)
        if meta.returncode != 0:
            raise SystemExit(f"wcov_probe.py: scripts/kernel_meta.py --filter {flt} ended with status {meta.returncode}")
        lines += ["#"] + meta.stdout.splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
