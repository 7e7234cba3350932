#!/usr/bin/env python3
"""Times the recovered graph on the device (uglad_graph_wide, csrc/graph_wide.h) against the package's own host formulation of the same
definitions (after._recovered_graph_host: float64, vectorised -- sort, compare, (A A) o A through BLAS), on the same partial correlations.

    python scripts/graph_probe.py [--out profiles/graph_probe.txt] [--dims 288,1024,2048]

Problems: K matrices of partial correlations of order D on the device, float32 (so both sides decide on identical values), from precision
matrices with exact zeros under a dominant diagonal.  Two patterns: `random` -- non-zeros of density 0.3 anywhere; `blocks` -- four
communities of D / 4 nodes, density 0.6 inside a community and 0.02, at a tenth of the magnitude, between communities (sparsity 0.1 then keeps
edges inside the communities only).  Columns:
  host ms     wall clock of the download of the matrices and the host formulation for every problem
  nx ms       networkx average_clustering + transitivity on problem 0's graph (what the reference's compute_graph_statistics calls), ONE run,
              the graph already built; not part of `host ms`
  device ms   HIP events around the enqueue of graph_wide on tensors already on the device
  e2e ms      wall clock of after._recovered_graphs on those tensors: kernels, download of thresholds, counts, edge lists, degrees, triangles
              and statistics, the result objects
  tri %       share of the device time that the triangle product, its row sums and the six statistics take: 1 - (device ms without
              statistics) / (device ms)
  skipped     fraction of the 64 x 64 tiles of the triangle product that leave at once (their own adjacency tile is empty), problem 0
each but nx the median of the timed runs after one warm-up.  same = edges, degrees, triangle counts and the six statistics of the device equal
the host formulation's for every problem, the statistics as bits.  No threshold is assumed: the table reports, whichever side wins."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

STATS = ("num_nodes", "num_edges", "avg_degree", "density", "avg_clustering", "transitivity")


def make_rho(K, D, pattern, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((K, D, D), dtype=np.float32)
    block = np.arange(D) * 4 // D
    inside = block[:, None] == block[None, :]
    for k in range(K):
        if pattern == "random":
            mask, scale = rng.random((D, D)) < 0.3, 1.0
        else:
            mask, scale = rng.random((D, D)) < np.where(inside, 0.6, 0.02), np.where(inside, 1.0, 0.1)
        u = np.triu(mask, 1) * rng.uniform(0.1, 1.0, size=(D, D)) * scale * np.where(rng.random((D, D)) < 0.5, 1.0, -1.0)
        P = u + u.T
        d = np.abs(P).sum(axis=1) + rng.uniform(0.5, 1.5, size=D)
        P = P.astype(np.float32)
        d = d.astype(np.float32)
        rho = -P / np.sqrt(d[:, None] * d[None, :])
        rho[np.arange(D), np.arange(D)] = 1.0
        out[k] = rho
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_probe.txt"))
    ap.add_argument("--dims", default="288,1024,2048")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import networkx as nx

    from uglad_amd import _lib, after, main as um

    if not torch.cuda.is_available():
        raise SystemExit("graph_probe.py measures on the GPU; none is visible")
    lib = _lib.get_lib()
    lines = [f"# scripts/graph_probe.py on {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {args.reps} after one warm-up (nx: one run)",
             "# host = download + after._recovered_graph_host per problem; nx = networkx average_clustering + transitivity, problem 0; device = HIP "
             "events around graph_wide; e2e = after._recovered_graphs on device tensors; tri % = share of the statistics kernels",
             f"{'pattern':>7} {'D':>5} {'K':>2} {'spars':>5} {'edges':>8} {'host ms':>9} {'nx ms':>9} {'device ms':>10} {'e2e ms':>8} {'host/e2e':>9} "
             f"{'tri %':>6} {'skipped':>8} {'same':>5}"]
    print("\n".join(lines), flush=True)

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop)

    for pattern in ("random", "blocks"):
        for D in [int(d) for d in args.dims.split(",")]:
            E = D * (D - 1) // 2
            nx_ms = {}
            for K in (1, 4):
                rho = make_rho(K, D, pattern, seed=D + K)
                Rd = torch.from_numpy(rho).cuda()
                for sparsity in (0.1, 1.0):
                    n_keep = int(sparsity * E)
                    host_ms, dev_ms, lean_ms, e2e_ms = [], [], [], []
                    for rep in range(args.reps + 1):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        Rn = Rd.cpu().numpy()
                        host = [after._recovered_graph_host(Rn[k], False, n_keep, None, True) for k in range(K)]
                        t1 = time.perf_counter()
                        full = timed(lambda: lib.graph_wide(Rd, n_keep=n_keep, from_precision=False, want_stats=True))
                        lean = timed(lambda: lib.graph_wide(Rd, n_keep=n_keep, from_precision=False, want_stats=False))
                        t2 = time.perf_counter()
                        got = after._recovered_graphs(Rd, False, n_keep, None, True)
                        t3 = time.perf_counter()
                        if rep:  # (the first run is the warm-up of all)
                            host_ms.append((t1 - t0) * 1e3)
                            dev_ms.append(full)
                            lean_ms.append(lean)
                            e2e_ms.append((t3 - t2) * 1e3)
                    same = all(np.array_equal(a.edges, b.edges) and np.array_equal(a.degree, b.degree) and np.array_equal(a.triangles, b.triangles)
                               and np.array_equal(a.weights.astype(np.float64), b.weights)
                               and np.array([a.stats[s] for s in STATS]).tobytes() == np.array([b.stats[s] for s in STATS], dtype=np.float64).tobytes()
                               for a, b in zip(got, host))
                    e0 = got[0].edges
                    if sparsity not in nx_ms:
                        G = nx.Graph()
                        G.add_nodes_from(range(D))
                        G.add_edges_from(e0.tolist())
                        t0 = time.perf_counter()
                        nx.average_clustering(G), nx.transitivity(G)
                        nx_ms[sparsity] = (time.perf_counter() - t0) * 1e3
                    nt = -(-D // 64)
                    used = np.zeros((nt, nt), dtype=bool)
                    used[e0[:, 0] // 64, e0[:, 1] // 64] = used[e0[:, 1] // 64, e0[:, 0] // 64] = True
                    h, d, lean, e = (statistics.median(x) for x in (host_ms, dev_ms, lean_ms, e2e_ms))
                    line = (f"{pattern:>7} {D:>5} {K:>2} {sparsity:>5.1f} {len(e0):>8} {h:>9.1f} {nx_ms[sparsity]:>9.1f} {d:>10.3f} {e:>8.2f} {h / e:>9.1f} "
                            f"{100.0 * (1.0 - lean / d):>6.1f} {1.0 - used.mean():>8.1%} {'yes' if same else 'NO':>5}")
                    print(line, flush=True)
                    lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
