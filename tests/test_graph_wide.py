"""The recovered graph on the device (uglad_graph_wide, csrc/graph_wide.h): threshold, edge list, degrees, triangle counts and the six graph
statistics.  CPU: the unmodified kernel sources on the SIMT emulator against a vectorised numpy checker (rho in float32, sort, compare,
(A A) o A in float64) and against goldens made by the real reference and networkx (tests/golden/make_graph_goldens.py).  GPU: both goldens,
the checker at D = 2048, batch independence and fit().

The sort works on tiles of 2048 keys (256 threads x 8 keys), the adjacency plane and the triangle product on tiles of 64 x 64.

Equality: there is no tolerance anywhere.  Edges, counts, degrees and triangle counts are integers; threshold and weights come from the same
correctly rounded float32 operations on both sides (compared as bits); the six statistics are one float64 division of exact integers each, the
c_i summed in node order, on both sides."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SORT_TILE = 2048
STAT_KEYS = ("num_nodes", "num_edges", "avg_degree", "density", "avg_clustering", "transitivity", "diameter", "avg_shortest_path")


# ============================================================================================ the checker
def edge_values(V, from_precision):
    """float32 values of the strict upper triangle in row-major order."""
    V = np.asarray(V, dtype=np.float32)
    i, j = np.triu_indices(V.shape[-1], 1)
    if not from_precision:
        return i, j, V[i, j]
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = -V[i, j] / np.sqrt(V[i, i] * V[j, j])
    assert rho.dtype == np.float32
    return i, j, rho


def checker(V, from_precision=True, n_keep=None, threshold=None):
    D = V.shape[-1]
    i, j, rho = edge_values(V, from_precision)
    E = rho.size
    if n_keep is None:
        th = np.float32(threshold)
    else:
        s = np.sort(np.abs(rho))  # (NaN last)
        th = s[E - n_keep] if n_keep > 0 else s[0]
    with np.errstate(invalid="ignore"):
        keep = (rho > th) | (rho < -th)
    A = np.zeros((D, D))
    A[i[keep], j[keep]] = 1.0
    A = A + A.T
    degree = A.sum(axis=1).astype(np.int64)
    t2 = ((A @ A) * A).sum(axis=1).astype(np.int64)
    d, t, m = [int(x) for x in degree], [int(x) for x in t2], int(keep.sum())
    c = [0 if ti == 0 else ti / (di * (di - 1)) for di, ti in zip(d, t)]
    pairs = sum(di * (di - 1) for di in d)
    stats = np.array([D, m, sum(d) / D, m / (D * (D - 1)) * 2, sum(c) / D, 0 if sum(t) == 0 else sum(t) / pairs], dtype=np.float64)
    return dict(threshold=np.float32(th), edges=np.stack([i[keep], j[keep]], axis=1).astype(np.int32), weights=rho[keep], degree=degree, t2=t2,
                stats=stats, A=A)


def run(lib, V, n_keep=None, threshold=None, from_precision=True, want_stats=True, device="cpu"):
    g = lib.graph_wide(torch.from_numpy(np.array(V, dtype=np.float32)).to(device), n_keep=n_keep, threshold=threshold,
                       from_precision=from_precision, want_stats=want_stats)
    if device != "cpu":
        torch.cuda.synchronize()
    K, D = V.shape[0], V.shape[-1]
    assert g.edge_ij.dtype == torch.int32 and tuple(g.edge_ij.shape) == (K, D * (D - 1) // 2, 2) and g.edge_w.dtype == torch.float32
    assert g.degree.dtype == torch.int32 and g.threshold.dtype == torch.float32 and g.edge_count.dtype == torch.int32
    out = []
    for k in range(K):
        m = int(g.edge_count[k])
        out.append(dict(threshold=g.threshold[k].cpu().numpy(), edges=g.edge_ij[k, :m].cpu().numpy(), weights=g.edge_w[k, :m].cpu().numpy(),
                        degree=g.degree[k].cpu().numpy(), t2=g.triangles2[k].cpu().numpy() if want_stats else None,
                        stats=g.stats[k].cpu().numpy() if want_stats else None))
    return out


def assert_same(got, ref, label="", stats=True):
    print(f"{label}: threshold {got['threshold']!r} (checker {ref['threshold']!r}), {len(got['edges'])} edges (checker {len(ref['edges'])}), "
          f"stats {got['stats']} (checker {ref['stats']})")
    np.testing.assert_array_equal(got["threshold"], ref["threshold"], err_msg=label)  # (NaN equals NaN)
    if not np.isnan(ref["threshold"]):
        assert got["threshold"].view(np.uint32) == ref["threshold"].view(np.uint32), label
    np.testing.assert_array_equal(got["edges"], ref["edges"], err_msg=label)
    np.testing.assert_array_equal(got["weights"].view(np.uint32), ref["weights"].view(np.uint32), err_msg=label)
    np.testing.assert_array_equal(got["degree"], ref["degree"], err_msg=label)
    if stats:
        np.testing.assert_array_equal(got["t2"], ref["t2"], err_msg=label)
        np.testing.assert_array_equal(got["stats"].view(np.uint64), ref["stats"].view(np.uint64), err_msg=label)


def check(lib, V, n_keep=None, threshold=None, from_precision=True, device="cpu", label=""):
    """n_keep / threshold: one per problem.  Returns the checker's results."""
    K = len(V)
    got = run(lib, V, n_keep=n_keep, threshold=threshold, from_precision=from_precision, device=device)
    refs = []
    for k in range(K):
        ref = checker(V[k], from_precision, None if n_keep is None else n_keep[k], None if threshold is None else threshold[k])
        assert_same(got[k], ref, f"{label}[{k}]")
        refs.append(ref)
    return refs


def precisions(K, D, seed, density=0.3, decimals=None):
    """K float32 precision matrices with exact zeros: a sparse symmetric pattern under a dominant diagonal; with `decimals` the values are
    rounded and the diagonal is constant, so that |rho| has tie groups (the zeros are one in any case)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((K, D, D), dtype=np.float32)
    for k in range(K):
        u = np.triu(rng.random((D, D)) < density, 1) * rng.uniform(0.1, 1.0, size=(D, D)) * np.where(rng.random((D, D)) < 0.5, 1.0, -1.0)
        if decimals is not None:
            u = np.round(u, decimals)
        P = u + u.T
        rows = np.abs(P).sum(axis=1)
        P[np.arange(D), np.arange(D)] = np.ceil(rows.max()) + 1.0 if decimals is not None else rows + rng.uniform(0.5, 1.5, size=D)
        out[k] = P
    return out


def n_edges(D):
    return D * (D - 1) // 2


# ============================================================================================ CPU: the kernels on the emulator
@pytest.mark.parametrize("D", [2, 3])
def test_emulated_smallest_sizes_every_n_keep(emul, D):
    """One and three edges; every n_keep from 0 to E (0 reads s[0], like E)."""
    E = n_edges(D)
    P = precisions(E + 1, D, seed=100 + D, density=1.0)
    refs = check(emul, P, n_keep=list(range(E + 1)), label=f"d{D}")
    assert [len(r["edges"]) for r in refs] == [E - 1] + list(range(E))  # distinct values: n_keep keeps n_keep - 1 (strict), 0 keeps E - 1


def test_emulated_below_one_sort_tile(emul):
    D = 37
    assert n_edges(D) < SORT_TILE
    P = precisions(2, D, seed=137, decimals=1)
    refs = check(emul, P, n_keep=[int(0.1 * n_edges(D)), int(0.5 * n_edges(D))], label="d37")
    assert all(r["stats"][5] > 0 for r in refs[1:])  # triangles exist


def test_emulated_two_sort_tiles_ragged_planes_and_both_ends_of_n_keep(emul):
    """(K = 2, D = 70): E = 2415 = one sort tile and a ragged one; the adjacency plane is 2 x 2 tiles of 64 whose last is 6 wide.  Problem 0
    gets n_keep = 0 and problem 1 n_keep = E: both read s[0] = 0 and keep every non-zero rho."""
    D = 70
    E = n_edges(D)
    assert SORT_TILE < E < 2 * SORT_TILE and D % 64 == 6
    P = precisions(2, D, seed=170)
    refs = check(emul, P, n_keep=[0, E], label="d70")
    assert refs[0]["threshold"] == 0 and len(refs[0]["edges"]) == np.count_nonzero(np.triu(P[0], 1))
    check(emul, P, n_keep=[int(0.1 * E), int(0.05 * E)], label="d70 sparse")


def test_emulated_zero_tie_group_across_a_sort_tile_boundary(emul):
    """(D = 92): three sort tiles; about 70 % of the 4186 values are exact zeros (both signs of zero), so the group of zeros spans two tile
    boundaries, and n_keep beyond the non-zeros puts the threshold inside it: th = 0, every non-zero rho is an edge."""
    D = 92
    E = n_edges(D)
    assert -(-E // SORT_TILE) == 3
    P = precisions(2, D, seed=192, decimals=1)
    nz = [np.count_nonzero(np.triu(P[k], 1)) for k in range(2)]
    assert all(E - n > SORT_TILE for n in nz)
    refs = check(emul, P, n_keep=[nz[0] + 5, nz[1]], label="d92")
    assert refs[0]["threshold"] == 0 and len(refs[0]["edges"]) == nz[0]
    assert refs[1]["threshold"] > 0 and len(refs[1]["edges"]) < nz[1]  # the smallest non-zero |rho| is a tie group: strict comparison drops it


def test_emulated_empty_and_full_adjacency_tiles_and_the_complete_graph(emul):
    """(D = 130): 3 x 3 tiles whose last is 2 wide.  Case 1, given as partial correlations: the off-diagonal tile (0, 1) is full, (0, 2) is
    empty (the triangle kernel leaves it at once), the others are sparse.  Case 2: the complete graph (a threshold below every |rho|): the
    largest counts, t_i = (D - 1)(D - 2)."""
    D = 130
    rng = np.random.default_rng(1130)
    u = np.triu(rng.random((D, D)) < 0.2, 1) * rng.uniform(0.1, 0.9, size=(D, D)) * np.where(rng.random((D, D)) < 0.5, 1.0, -1.0)
    u[:64, 64:128] = rng.uniform(0.1, 0.9, size=(64, 64)) * np.where(rng.random((64, 64)) < 0.5, 1.0, -1.0)
    u[:64, 128:] = 0.0
    rho = (u + u.T + np.eye(D)).astype(np.float32)[None]
    nz = np.count_nonzero(np.triu(rho[0], 1))
    ref = check(emul, rho, n_keep=[nz + 1], from_precision=False, label="d130 tiles")[0]
    assert ref["A"][:64, 64:128].all() and not ref["A"][:64, 128:].any() and ref["A"][64:128, 128:].any() and len(ref["edges"]) == nz
    dense = rng.uniform(0.1, 0.9, size=(D, D)) * np.where(rng.random((D, D)) < 0.5, 1.0, -1.0)
    dense = (np.triu(dense, 1) + np.triu(dense, 1).T + np.eye(D)).astype(np.float32)[None]
    ref = check(emul, dense, threshold=[0.05], from_precision=False, label="d130 complete")[0]
    assert len(ref["edges"]) == n_edges(D) and (ref["t2"] == (D - 1) * (D - 2)).all() and ref["stats"][4] == 1.0 and ref["stats"][5] == 1.0


def test_emulated_special_values(emul):
    """A NaN diagonal entry (NaN rho in one row and one column: never edges, sorted last), a negative diagonal entry (sqrt of a negative
    product: NaN again), all-zero off-diagonals (th = 0, no edge, every quotient guarded)."""
    D = 37
    P = precisions(4, D, seed=237)
    P[0, 5, 5] = np.float32("nan")
    P[1, 7, 7] = -P[1, 7, 7]
    P[2] = np.diag(np.diag(P[2]))
    P[3, 5, 5] = np.float32("nan")
    E = n_edges(D)
    refs = check(emul, P, n_keep=[E // 2, E // 2, E // 2, 3], label="special")
    assert not (refs[0]["edges"] == 5).any() and not (refs[1]["edges"] == 7).any()
    assert refs[2]["threshold"] == 0 and len(refs[2]["edges"]) == 0 and (refs[2]["stats"][1:] == 0).all()
    assert np.isnan(refs[3]["threshold"]) and len(refs[3]["edges"]) == 0  # the threshold itself is one of the 36 NaN: it keeps nothing


def test_emulated_given_threshold_equals_rank_mode(emul):
    D = 70
    P = precisions(2, D, seed=270, decimals=1)
    E = n_edges(D)
    ranked = run(emul, P, n_keep=[E // 10, E // 3])
    th = [float(r["threshold"]) for r in ranked]
    given = run(emul, P, threshold=th)
    mixed = run(emul, P, n_keep=[-1, E // 3], threshold=th)
    for k in range(2):
        assert_same(given[k], checker(P[k], True, threshold=th[k]), f"given[{k}]")
        for other in (given, mixed):
            for key in ("threshold", "edges", "weights", "degree", "t2", "stats"):
                assert ranked[k][key].tobytes() == other[k][key].tobytes(), (k, key)
    no_stats = run(emul, P, n_keep=[E // 10, E // 3], want_stats=False)
    assert all(no_stats[k]["edges"].tobytes() == ranked[k]["edges"].tobytes() and no_stats[k]["stats"] is None for k in range(2))


def test_emulated_problem_does_not_depend_on_its_batch(emul):
    D = 70
    P = precisions(3, D, seed=370, decimals=1)
    P[1, 3, 3] = np.float32("nan")  # a neighbour with NaN
    keep = [100, 200, 300]
    batch, solo = run(emul, P, n_keep=keep), run(emul, P[:1], n_keep=keep[:1])
    for key in ("threshold", "edges", "weights", "degree", "t2", "stats"):
        assert batch[0][key].tobytes() == solo[0][key].tobytes(), key
    assert_same(batch[0], checker(P[0], True, keep[0]), "problem 0")


def test_emulated_argument_errors_launch_nothing(emul, monkeypatch, tmp_path):
    from uglad_amd._lib import UgladError

    log = tmp_path / "launches.txt"
    monkeypatch.setenv("UGLAD_EMUL_LAUNCH_LOG", str(log))
    size = emul._dll.uglad_graph_wide_workspace_floats
    assert size(0, 8) < 0 and size(1, 1) < 0 and size(1, emul.max_dim + 1) < 0 and size(65536, 8) < 0
    assert size(1, 2) > 0 and size(2, 70) == 2 * size(1, 70) and size(1, 70) % 2 == 0
    K, D = 1, 8
    E = n_edges(D)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    t = dict(values=torch.eye(D)[None].contiguous(), th_in=torch.zeros(K), threshold=torch.zeros(K), count=torch.zeros(K, dtype=torch.int32),
             ij=torch.zeros(K, E, 2, dtype=torch.int32), w=torch.zeros(K, E), degree=torch.zeros(K, D, dtype=torch.int32),
             t2=torch.zeros(K, D, dtype=torch.int32), stats=torch.zeros(K, 6, dtype=torch.float64), wsp=torch.empty(size(K, D) + 2))
    order = ("values", "th_in", "threshold", "count", "ij", "w", "degree", "t2", "stats")

    def call(n_keep=(3,), want_stats=1, from_precision=1, K=K, D=D, wsp="wsp", **null):
        p = {key: None if key in null else vp(t[key]) for key in order}
        keep = None if n_keep is None else (ctypes.c_int * len(n_keep))(*n_keep)
        w = None if wsp is None else (vp(t["wsp"]) if wsp == "wsp" else wsp)
        emul._call("uglad_graph_wide", p["values"], from_precision, keep, p["th_in"], p["threshold"], p["count"], p["ij"], p["w"], p["degree"],
                   p["t2"], p["stats"], want_stats, K, D, w)

    for key in ("values", "n_keep", "threshold", "count", "ij", "w", "degree", "t2", "stats"):
        with pytest.raises(UgladError, match="NULL"):
            call(**{key: None})
    odd = ctypes.c_void_p(t["wsp"].data_ptr() + (4 if t["wsp"].data_ptr() % 8 == 0 else 8))
    for bad in (None, odd):  # missing / misaligned workspace
        with pytest.raises(UgladError, match="NULL"):
            call(wsp=bad)
    with pytest.raises(UgladError, match="NULL"):  # n_keep = -1 without a threshold
        call(n_keep=(-1,), th_in=None)
    for kw in (dict(D=1), dict(D=emul.max_dim + 1), dict(K=0), dict(n_keep=(E + 1,)), dict(n_keep=(-2,))):
        with pytest.raises(UgladError, match="dimension"):
            call(**kw)
    with pytest.raises(UgladError, match="mode"):
        call(want_stats=2)
    assert not log.exists()  # no kernel was launched
    call(want_stats=0, t2=None, stats=None, th_in=None)  # both may be NULL without statistics, threshold_in when no n_keep is -1
    launched = log.read_text()
    assert "gw_edges_kernel" in launched and "gw_triangles_kernel" not in launched and "gw_finish_kernel" not in launched
    with pytest.raises(UgladError):  # the wrapper: fp64 input, shapes, neither n_keep nor threshold
        emul.graph_wide(torch.zeros(1, 8, 8, dtype=torch.float64), n_keep=1)
    with pytest.raises(UgladError):
        emul.graph_wide(torch.zeros(1, 8, 7), n_keep=1)
    with pytest.raises(UgladError):
        emul.graph_wide(torch.zeros(1, 8, 8))


# ============================================================================================ the goldens of the real reference
@functools.lru_cache(maxsize=None)
def load_golden(D):
    path = os.path.join(GOLDEN, f"graph_k2_d{D}.npz")
    assert os.path.getsize(path) < 1 << 20
    g = np.load(path, allow_pickle=False)
    return {key: g[key] for key in g.files}


def no_host(*a, **k):
    raise AssertionError("the host formulation ran for values float32 holds")


def _check_golden(D):
    """graph_from_partial_correlations, compute_graph_statistics, recovered_graph and the estimator's method against the reference's output."""
    import uglad_amd
    from uglad_amd import main

    g = load_golden(D)
    names = [str(n) for n in g["names"]]
    rho64 = g["rho"].astype(np.float64)  # (what the reference's get_partial_correlations returned: float64 holding float32 values)
    assert g["precision"].dtype == np.float32 and g["precision"].shape == (2, D, D)
    for k in range(2):
        for s, sparsity in enumerate(g["sparsity"].tolist()):
            tag = f"{k}_{s}"
            G, image, strings = main.graph_from_partial_correlations(rho64[k], names, sparsity=sparsity, PLOT=False)
            assert image is None and list(G.nodes) == names
            assert strings == [str(x) for x in g["strings_" + tag]], tag
            np.testing.assert_array_equal(np.array([(names.index(a), names.index(b)) for a, b in G.edges]).reshape(-1, 2), g["edges_" + tag])
            data = [G.edges[e] for e in G.edges]
            np.testing.assert_array_equal(np.array([d["weight"] for d in data], dtype=np.float64), g["weights_" + tag])
            assert [d["color"] for d in data] == ["green" if p else "red" for p in g["positive_" + tag]]
            assert [d["label"] for d in data] == ["+" if p else "-" for p in g["positive_" + tag]]
            frame = main.compute_graph_statistics(G)
            assert list(frame.columns) == list(STAT_KEYS) and len(frame) == 1
            row = np.array([np.nan if frame.iloc[0][key] is None else float(frame.iloc[0][key]) for key in STAT_KEYS])
            print(f"golden d{D} {tag}: {row} (reference {g['stats_' + tag]})")
            np.testing.assert_array_equal(row.view(np.uint64), g["stats_" + tag].view(np.uint64), err_msg=tag)
            r = uglad_amd.recovered_graph(g["precision"][k], sparsity=sparsity)
            np.testing.assert_array_equal(r.edges, g["edges_" + tag])
            assert r.edges.dtype == np.int32 and r.weights.dtype == np.float32 and list(r.stats) == list(STAT_KEYS)
            np.testing.assert_array_equal(np.array([round(np.float64(w), 5) for w in r.weights]), g["weights_" + tag])
            np.testing.assert_array_equal(r.positive, g["positive_" + tag])
            np.testing.assert_array_equal(np.array([r.stats[key] for key in STAT_KEYS[:6]], dtype=np.float64).view(np.uint64),
                                          g["stats_" + tag][:6].view(np.uint64))
            assert r.stats["diameter"] is None and r.stats["avg_shortest_path"] is None
            np.testing.assert_array_equal(np.bincount(g["edges_" + tag].reshape(-1), minlength=D), r.degree)
            assert r.triangles.sum() * 2 == round(r.stats["transitivity"] * float((r.degree * (r.degree - 1)).sum()))
    both = uglad_amd.recovered_graph(g["precision"], sparsity=0.1)  # a batch; the estimators
    assert len(both) == 2 and all(np.array_equal(both[k].edges, g[f"edges_{k}_2"]) for k in range(2))
    est, multi = uglad_amd.uGLAD_GL(), uglad_amd.uGLAD_multitask()
    for m in (est, multi):
        with pytest.raises(ValueError, match="call fit"):
            m.recovered_graph()
    est.precision_, multi.precision_ = g["precision"][1], g["precision"]
    np.testing.assert_array_equal(est.recovered_graph(sparsity=0.05).edges, g["edges_1_1"])
    assert [len(r.edges) for r in multi.recovered_graph()] == [len(g["edges_0_2"]), len(g["edges_1_2"])]


def test_emulated_matches_the_reference_golden(emul, monkeypatch):
    from uglad_amd import main

    monkeypatch.setattr("uglad_amd.after._recovered_graph_host", no_host)
    _check_golden(70)


def test_emulated_routing_and_argument_errors_of_the_python_surface(emul, monkeypatch):
    """A float64 rho with two values that float32 merges, one of them the threshold: the host formulation, equal to float64 numpy (on the
    device both would fall on the threshold and neither would be an edge).  A float32-exact rho never takes the host formulation."""
    from uglad_amd import main

    D = 12
    rng = np.random.default_rng(12)
    u = np.triu(rng.uniform(0.1, 0.9, size=(D, D)).astype(np.float32).astype(np.float64), 1)
    E = n_edges(D)
    order = np.sort(u[np.triu_indices(D, 1)])
    a = order[E - 10]  # th for n_keep = 10
    i, j = [int(x[0]) for x in np.where(u == order[E - 9])]
    u[i, j] = a * (1.0 + 2.0 ** -40)  # above the threshold in float64, on it in float32
    assert np.float32(u[i, j]) == np.float32(a) and u[i, j] > a
    rho = u + u.T + np.eye(D)
    names = [f"v{q}" for q in range(D)]
    G, _, strings = main.graph_from_partial_correlations(rho, names, sparsity=10 / E + 1e-9, PLOT=False)
    iu = np.triu_indices(D, 1)
    keep = rho[iu] > a
    assert keep.sum() == 9 and len(strings) == 9 and G.has_edge(names[i], names[j])
    assert strings == [f"({names[p]}, {names[q]}, {round(rho[p, q], 5)}, green)" for p, q in zip(iu[0][keep], iu[1][keep])]
    monkeypatch.setattr("uglad_amd.after._recovered_graph_host", no_host)
    with pytest.raises(AssertionError, match="host formulation"):
        main.graph_from_partial_correlations(rho, names, sparsity=10 / E + 1e-9, PLOT=False)
    exact = rho.astype(np.float32).astype(np.float64)
    G32, _, strings32 = main.graph_from_partial_correlations(exact, names, sparsity=10 / E + 1e-9, PLOT=False)
    assert len(strings32) == 8 and not G32.has_edge(names[i], names[j])  # merged with the threshold
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            main.graph_from_partial_correlations(exact, names, sparsity=bad, PLOT=False)
        with pytest.raises(ValueError):
            main.recovered_graph(exact, sparsity=bad)


def test_emulated_drawing_and_disconnected_statistics(emul, tmp_path):
    import matplotlib

    matplotlib.use("Agg")
    import networkx as nx

    from uglad_amd import main

    rho = np.eye(6)
    rho[0, 1] = rho[1, 0] = 0.5
    rho[1, 2] = rho[2, 1] = -0.25
    rho[0, 2] = rho[2, 0] = 0.75
    rho[3, 4] = rho[4, 3] = -0.125
    G, png, strings = main.graph_from_partial_correlations(rho, list("abcdef"), title="t", fig_size=3, save_file=str(tmp_path / "g.png"))
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and (tmp_path / "g.png").stat().st_size > 0
    assert strings == ["(a, b, 0.5, green)", "(a, c, 0.75, green)", "(b, c, -0.25, red)", "(d, e, -0.125, red)"]
    row = main.compute_graph_statistics(G).iloc[0]
    assert row["diameter"] is None and row["avg_shortest_path"] is None and row["num_edges"] == 4 and row["num_nodes"] == 6
    assert row["avg_clustering"] == nx.average_clustering(G) == 0.5 and row["transitivity"] == nx.transitivity(G) == 1.0
    assert row["density"] == nx.density(G) and row["avg_degree"] == 8 / 6


# ============================================================================================ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("D", [70, 288])
def test_gpu_matches_the_reference_golden(monkeypatch, D):
    from uglad_amd import main

    monkeypatch.setattr("uglad_amd.after._recovered_graph_host", no_host)
    _check_golden(D)


@functools.lru_cache(maxsize=None)
def largest_case():
    """(K = 1, D = 2048): a dense precision matrix without zeros, values rounded to two decimals under a constant diagonal (tie groups)."""
    D = 2048
    rng = np.random.default_rng(2048)
    u = np.round(rng.uniform(0.01, 1.0, size=(D, D)), 2) * np.where(rng.random((D, D)) < 0.5, 1.0, -1.0)
    P = np.triu(u, 1) + np.triu(u, 1).T + 1100.0 * np.eye(D)
    P = P.astype(np.float32)[None]
    P.setflags(write=False)
    return P


@pytest.mark.gpu
@pytest.mark.parametrize("sparsity", [1.0, 0.1])
def test_gpu_largest_size(sparsity):
    """E = 2 096 128.  Sparsity 1.0: every edge above the smallest |rho| -- a dense adjacency matrix, no tile of the triangle product is
    skipped, the largest counts.  Sparsity 0.1: the default."""
    from uglad_amd import _lib

    P = largest_case()
    E = n_edges(2048)
    ref = check(_lib.get_lib(), P, n_keep=[int(sparsity * E)], device="cuda", label=f"d2048 sparsity {sparsity}")[0]
    assert (len(ref["edges"]) > 0.98 * E) if sparsity == 1.0 else (0.09 * E < len(ref["edges"]) <= 0.1 * E)


@pytest.mark.gpu
def test_gpu_problem_does_not_depend_on_its_batch():
    from uglad_amd import _lib

    lib = _lib.get_lib()
    P = precisions(3, 288, seed=388, decimals=1)
    keep = [4000, 400, 40000]
    batch, solo = run(lib, P, n_keep=keep, device="cuda"), run(lib, P[:1], n_keep=keep[:1], device="cuda")
    for key in ("threshold", "edges", "weights", "degree", "t2", "stats"):
        assert batch[0][key].tobytes() == solo[0][key].tobytes(), key
    for k in range(3):
        assert_same(batch[k], checker(P[k], True, keep[k]), f"d288[{k}]")


@pytest.mark.gpu
def test_gpu_fit_at_288_recovers_the_graph_on_the_device(monkeypatch):
    """fit() as in test_metrics_wide.test_gpu_fit_at_288_reports_from_the_device, then the estimator's recovered_graph() with the host
    formulation taken away.  (Two epochs leave this precision_ without off-diagonal non-zeros: th = 0 inside the group of zeros and an
    empty graph, which is what the checker says too; the goldens and the D = 2048 cases carry the non-trivial graphs.)"""
    import uglad_amd
    from uglad_amd import main
    from uglad_amd.utils.prepare_data import get_data

    monkeypatch.setattr("uglad_amd.after._recovered_graph_host", no_host)
    X, _ = get_data(288, (0.02, 0.04), 600, 1, eig_offset=1.0, rng=11)
    est = uglad_amd.uGLAD_GL()
    with pytest.raises(ValueError, match="call fit"):
        est.recovered_graph()
    est.fit(X[0], epochs=2, lr=0.01, L=3, verbose=False)
    r = est.recovered_graph()
    ref = checker(est.precision_, True, int(0.1 * n_edges(288)))
    got = dict(threshold=r.threshold, edges=r.edges, weights=r.weights, degree=r.degree, t2=None,
               stats=np.array([r.stats[key] for key in STAT_KEYS[:6]], dtype=np.float64))
    assert_same(got, ref, "fit d288", stats=False)
    np.testing.assert_array_equal(r.triangles, ref["t2"] // 2)
    np.testing.assert_array_equal(got["stats"].view(np.uint64), ref["stats"].view(np.uint64))
