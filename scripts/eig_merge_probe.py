#!/usr/bin/env python3
"""Times the kernels that stand on the divide & conquer of csrc/eig_lean.h on two builds of the library in ONE process, alternating (the
method of wide_feeders_probe.py): the in-tree build and another one (the parent's).

    python scripts/eig_merge_probe.py --parent PARENT/libuglad_hip.so [--out profiles/eig_merge_phases_vs_parent.txt]

Per row `--rounds` rounds of (parent, new), each `--reps` timed runs after one warm-up; a timed run is HIP events around `--calls` calls.
Columns: the parent's median, the spread of ALL its timed runs of that row in this call (min .. max), the new build's median, and whether
it lies inside that spread.
  symeig      uglad_symeig on M seeded random symmetric matrices
  cell        uglad_cell_fwd (NS10, training outputs) on M matrices
  cell wide   the same with the eigensolver route forced and many workgroups per matrix (the handed-over last merge)"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eig_merge_phases_vs_parent.txt"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    from uglad_amd import _lib

    if not torch.cuda.is_available():
        raise SystemExit("eig_merge_probe.py measures on the GPU; none is visible")
    builds = {"parent": _lib.HipLib(os.path.abspath(args.parent)), "new": _lib.get_lib()}
    pz = np.load(os.path.join(ROOT, "tests", "golden", "params_trained.npz"))
    params = torch.tensor(np.concatenate([pz[k].ravel() for k in pz.files]), dtype=torch.float32, device="cuda")
    lines = [f"# scripts/eig_merge_probe.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; parent = the build of the commit before; per row "
             f"{args.rounds} rounds of (parent, new), {args.reps} timed runs of {args.calls} calls each after one warm-up; ms per call",
             f"{'row':<10} {'D':>4} {'M':>5} {'parent':>9} {'parent min .. max':>21} {'new':>9} {'new/parent':>10}  inside"]
    print("\n".join(lines), flush=True)
    outside = 0

    def events_ms(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.calls):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.calls

    def row(name, D, M, call):  # call(lib): one call on that build
        nonlocal outside
        t = {b: [] for b in builds}
        for _ in range(args.rounds):
            for b, lib in builds.items():
                t[b] += [events_ms(lambda: call(lib)) for _ in range(args.reps + 1)][1:]
        p, n, lo, hi = statistics.median(t["parent"]), statistics.median(t["new"]), min(t["parent"]), max(t["parent"])
        outside += not lo <= n <= hi
        line = f"{name:<10} {D:>4} {M:>5} {p:>9.4f} {lo:>9.4f} .. {hi:>9.4f} {n:>9.4f} {n / p:>10.3f}  {'yes' if lo <= n <= hi else 'NO'}"
        print(line, flush=True)
        lines.append(line)

    def symmetric(M, D, seed):
        a = torch.from_numpy(np.random.default_rng(seed).standard_normal((M, D, D)).astype(np.float32)).cuda()
        return ((a + a.transpose(1, 2)) / 2).contiguous()

    for D, M in ((25, 1024), (64, 1024), (96, 1024), (128, 1024), (256, 64)):
        A = symmetric(M, D, D)
        U, beta = torch.empty_like(A), torch.empty(M, D, dtype=torch.float32, device="cuda")
        wsp = {b: lib.workspace(M, D, A) for b, lib in builds.items()}
        row("symeig", D, M, lambda lib: lib._call("uglad_symeig", lib._p(A), lib._p(U), lib._p(beta), lib._p(wsp["parent" if lib is builds["parent"] else "new"]), M, D))
    for name, D, M, wide in (("cell", 128, 1024, -1), ("cell wide", 256, 2, 1)):
        i = torch.arange(D, device="cuda")
        S = (0.5 ** (i[:, None] - i[None, :]).abs().float() + 0.05 * symmetric(M, D, 1000 + D)).contiguous()
        Z = (0.5 * torch.eye(D, device="cuda") + 0.02 * symmetric(M, D, 2000 + D)).contiguous()
        lam = torch.ones(1, dtype=torch.float32, device="cuda")
        Zo, half, U = (torch.empty_like(S) for _ in range(3))
        beta, nfp = torch.empty(M, D, dtype=torch.float32, device="cuda"), torch.empty(M, dtype=torch.float32, device="cuda")
        for lib in builds.values():
            lib.set_matrix_iteration(0 if wide == 1 else -1)
            lib.set_wide_mode(wide)
        try:
            wsp = {b: lib.workspace(M, D, S) for b, lib in builds.items()}
            row(name, D, M, lambda lib: lib.cell_fwd(S, Z, lam, params, Zo, half, U, beta, nfp, wsp["parent" if lib is builds["parent"] else "new"], 1))
        finally:
            for lib in builds.values():
                lib.set_wide_mode(-1)
                lib.set_matrix_iteration(-1)
    lines.append(f"# rows whose new median lies outside the parent's spread: {outside} of {len(lines) - 2}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
