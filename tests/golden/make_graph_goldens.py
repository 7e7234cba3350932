#!/usr/bin/env python3
"""Golden vectors for the recovered graph (uglad_graph_wide), made by the REAL reference on CPU (build container only): its
get_partial_correlations (uglad/main.py:796-821), graph_from_partial_correlations (:825-946) and compute_graph_statistics (:1263-1300, networkx
behind it), imported the way make_goldens.py imports the reference (a stub for the absent `pyvis`).  The first argument is the checkout of
the reference (Harshs27/uGLAD):

    python tests/golden/make_graph_goldens.py <reference checkout>

graph_k2_d70.npz, graph_k2_d288.npz: `precision` (2, D, D) float32 with exact zeros -- a sparse symmetric pattern of density about 0.3 under a
dominant diagonal; the second matrix has its values rounded to one decimal under a constant diagonal, so that |rho| has tie groups -- `names`,
`rho` (2, D, D), the reference's float64 partial correlations stored as the float32 they are exactly (asserted), `sparsity` (4,) = 0, 0.05, 0.1, 1, and per matrix k and sparsity index s
    strings_k_s   the reference's edge-string list (unicode array)
    edges_k_s     (m, 2) int32 node indices of G.edges in the reference's insertion order
    weights_k_s   (m,) float64, the rounded `weight` attribute;  positive_k_s (m,) bool: color == "green" and label == "+"
    stats_k_s     (8,) float64, the columns of compute_graph_statistics, NaN for None
Asserted here: the reference's float64 rho holds float32 values exactly (its loop computes in the float32 of `precision_`), every case of
the second matrix has a tie group at its threshold, and the threshold of sparsity 0 equals that of sparsity 1 (rho_upper[-0]).  Data only, no
reference source."""
import os
import sys
import types

sys.dont_write_bytecode = True
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "uglad")):
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.abspath(sys.argv[1]))
os.environ.setdefault("MPLBACKEND", "Agg")
pv = types.ModuleType("pyvis")
pv.network = types.ModuleType("pyvis.network")
pv.network.Network = object
sys.modules["pyvis"] = pv
sys.modules["pyvis.network"] = pv.network

import numpy as np  # noqa: E402

from uglad import main as uG  # noqa: E402  (the reference)

OUT = os.path.dirname(os.path.abspath(__file__))
SPARSITY = (0.0, 0.05, 0.1, 1.0)
STAT_KEYS = ("num_nodes", "num_edges", "avg_degree", "density", "avg_clustering", "transitivity", "diameter", "avg_shortest_path")


def precision(D, seed, tied):
    rng = np.random.default_rng(seed)
    mask = np.triu(rng.random((D, D)) < 0.3, 1)
    vals = rng.uniform(0.1, 1.0, size=(D, D)) * np.where(rng.random((D, D)) < 0.5, 1.0, -1.0)
    if tied:
        vals = np.round(vals, 1)
    U = mask * vals
    P = U + U.T
    rows = np.abs(P).sum(axis=1)
    P[np.arange(D), np.arange(D)] = np.ceil(rows.max()) + 1.0 if tied else rows + rng.uniform(0.5, 1.5, size=D)
    return P.astype(np.float32)


for D in (70, 288):
    names = [f"n{i}" for i in range(D)]
    index = {n: i for i, n in enumerate(names)}
    P = np.array([precision(D, 7000 + D, False), precision(D, 7001 + D, True)])
    out = {"precision": P, "names": np.array(names), "sparsity": np.array(SPARSITY)}
    rhos = []
    for k in range(2):
        rho = uG.get_partial_correlations(P[k])
        assert rho.dtype == np.float64 and np.array_equal(rho.astype(np.float32).astype(np.float64), rho)
        rhos.append(rho)
        s_abs = np.sort(np.abs(rho[np.triu_indices(D, 1)]))
        E = len(s_abs)
        for s, sparsity in enumerate(SPARSITY):
            G, image, strings = uG.graph_from_partial_correlations(rho, names, sparsity=sparsity, PLOT=False)
            assert image is None and len(strings) == G.number_of_edges() and list(G.nodes) == names
            th = s_abs[-int(sparsity * E)]
            if k == 1:
                assert np.count_nonzero(s_abs == th) > 1, (D, sparsity)  # a tie group at the threshold
            edges = np.array([(index[a], index[b]) for a, b in G.edges], dtype=np.int32).reshape(-1, 2)
            data = [G.edges[e] for e in G.edges]
            assert all((d["color"] == "green") == (d["label"] == "+") for d in data)
            row = uG.compute_graph_statistics(G).iloc[0]
            out[f"strings_{k}_{s}"] = np.array(strings, dtype=np.str_)
            out[f"edges_{k}_{s}"] = edges
            out[f"weights_{k}_{s}"] = np.array([d["weight"] for d in data], dtype=np.float64)
            out[f"positive_{k}_{s}"] = np.array([d["color"] == "green" for d in data], dtype=bool)
            out[f"stats_{k}_{s}"] = np.array([np.nan if row[key] is None else float(row[key]) for key in STAT_KEYS], dtype=np.float64)
            print(f"D {D} matrix {k} sparsity {sparsity}: threshold {th!r}, {len(strings)} edges, stats {out[f'stats_{k}_{s}']}")
        assert np.array_equal(out[f"edges_{k}_0"], out[f"edges_{k}_3"])  # rho_upper[-0] is rho_upper[0]
    out["rho"] = np.array(rhos).astype(np.float32)  # (lossless: asserted above; the test widens it again)
    path = os.path.join(OUT, f"graph_k2_d{D}.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20
