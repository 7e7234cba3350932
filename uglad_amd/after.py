"""Everything after the path, on fitted precision matrices: row scores (uglad_sample_scores), support-recovery metrics
(uglad_support_metrics*), partial correlations, the recovered graph with its drawing and statistics (uglad_graph_wide), the edge
frequencies over the graphs of many resamples (uglad_edge_frequency), the conditional Gaussian and the MAP estimate
(uglad_conditional_mean*).  Mirrors the reference's main.py:796-1300; `uglad_amd.main` re-exports the
public names."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .inputs import _to_dev
from .utils.metrics import report_metrics_all


# ============================================================================================ scoring rows against fitted models
class SampleScores(NamedTuple):
    """What sample_scores returns, float64 numpy arrays."""
    mahalanobis: np.ndarray   # (K, N) squared distances xc^T P xc ((N,) for a single (D, D) model)
    log_density: np.ndarray   # (K, N) (logdet P - D log 2 pi - q) / 2
    logdet: np.ndarray        # (K,)   (a float64 scalar for a single model); NaN where P is not positive definite


SCORE_ROW_CHUNK = 65536  # rows per call of uglad_sample_scores unless row_chunk says otherwise (halved while the workspace is refused)


def _to_model_coordinates(X, min_range, D: int) -> np.ndarray:
    """(N, D) float64: X as given (min_range None) or mapped by (X - min) / range, the normalisation fit() applied to its own table."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != D:
        raise ValueError(f"X must be (N, {D}): the columns fit() kept, in node_names_ order; got {X.shape}")
    if min_range is None:
        return X
    mn, rg = min_range
    if mn is None or rg is None:
        raise ValueError("this model carries no data_min_ / data_range_ (fitted before they were kept?): pass normalized=True")
    return (X - mn) / rg


def sample_scores(precision, location, X, row_chunk=None) -> SampleScores:
    """Squared Mahalanobis distance and Gaussian log-density of every row of X under every model, on the device in fp64
    (uglad_sample_scores, csrc/score_wide.h): precision (D, D) or (K, D, D) -- its symmetric part is used --, location (D,) or (K, D), X
    (N, D) (one table for every model) or (K, N, D); numpy arrays or device tensors.  Rows go through in chunks of `row_chunk` (default
    SCORE_ROW_CHUNK, less where the workspace demands it), so any N fits; a row's numbers do not depend on the chunking, bit for bit.  A
    model that is not positive definite gets NaN in logdet and log_density and keeps its distances; a NaN in a row stays in that row."""
    lib = _lib.get_lib()
    to = lambda a: _to_dev(a, torch.float64)  # noqa: E731
    single = np.ndim(precision) == 2
    if np.ndim(precision) not in (2, 3) or np.shape(precision)[-1] > lib.max_dim:
        raise ValueError(f"precision must be (D, D) or (K, D, D) with D <= max_dim = {lib.max_dim}; got {tuple(np.shape(precision))}")
    P, mu = to(precision), to(location)
    P = P[None] if P.dim() == 2 else P
    mu = mu[None] if mu.dim() == 1 else mu
    if P.dim() != 3 or P.shape[1] != P.shape[2] or tuple(mu.shape) != tuple(P.shape[:2]):
        raise ValueError(f"precision (K, D, D) and location (K, D); got {tuple(P.shape)} and {tuple(mu.shape)}")
    K, D = mu.shape
    if not torch.is_tensor(X):
        X = np.asarray(X, dtype=np.float64)
    X = X[None] if X.ndim == 2 else X
    if X.ndim != 3 or X.shape[2] != D or X.shape[0] not in (1, K) or X.shape[1] < 1:
        raise ValueError(f"X must be (N, {D}) or ({K}, N, {D}) with N >= 1; got {tuple(X.shape)}")
    N = X.shape[1]
    chunk = min(N, int(row_chunk) if row_chunk else SCORE_ROW_CHUNK)
    if chunk < 1:
        raise ValueError("row_chunk must be positive")
    while chunk > 1 and int(lib._dll.uglad_sample_scores_workspace_floats(K, chunk, D)) < 0:
        chunk = (chunk + 1) // 2
    maha, dens, logdet = np.empty((K, N)), np.empty((K, N)), None
    for a in range(0, N, chunk):
        q, ld, det = lib.sample_scores(to(X[:, a:a + chunk]), P, mu)
        maha[:, a:a + chunk], dens[:, a:a + chunk] = q.cpu().numpy(), ld.cpu().numpy()
        logdet = det.cpu().numpy() if logdet is None else logdet  # (the same bits in every chunk)
    if single:
        return SampleScores(maha[0], dens[0], logdet[0])
    return SampleScores(maha, dens, logdet)


# ============================================================================================ after the path
METRIC_KEYS = ("FDR", "TPR", "FPR", "SHD", "nnzTrue", "nnzPred", "precision", "recall", "Fbeta", "aupr", "auc")


def device_report_metrics(true_theta, pred_theta, beta: int = 1):
    """`report_metrics_all` (ref utils/metrics.py:25-108) for K (true, predicted) precision matrices at once, counted on the
    device: list of K dicts with the reference's keys, rounded to 3 decimals as the reference does.  D <= max_eig_dim:
    uglad_support_metrics (one workgroup per pair); beyond, up to max_dim: uglad_support_metrics_wide (the edges sorted by score, many
    workgroups per pair)."""
    lib = _lib.get_lib()
    T, G = (_to_dev(a.real if torch.is_tensor(a) else np.asarray(a).real) for a in (true_theta, pred_theta))
    if T.dim() == 2:
        T, G = T[None], G[None]
    D = T.shape[-1]
    if D > lib.max_dim:
        # beyond what the device covers: the report is evaluated where the reference evaluates it -- on the host, from the same definitions
        # (utils/metrics.py = ref utils/metrics.py:25-108).  After the path, once per fit; round 3 raised UgladError here AFTER all epochs
        # of a fit(X, true_theta=...) at D > 256 had run.
        Tn, Gn = T.cpu().numpy(), G.cpu().numpy()
        return [report_metrics_all(Tn[k], Gn[k], beta=beta) for k in range(Tn.shape[0])]
    metrics = lib.support_metrics if D <= lib.max_eig_dim else lib.support_metrics_wide
    out = metrics(T, G, beta=beta).cpu().numpy()
    return [{k: round(float(v), 3) for k, v in zip(METRIC_KEYS, row)} for row in out]


def get_partial_correlations(precision):
    """rho_ij = -p_ij / sqrt(p_ii p_jj), ones on the diagonal (ref main.py:796-821: its double loop fills the upper triangle
    with that formula and mirrors it).  (D,D) or (K,D,D).
    A host array (what the reference takes: `precision_` is numpy) is evaluated on the host in float64 like the reference -- an O(D^2)
    formula needs no GPU and loses nothing to fp32; a tensor already on the device goes through uglad_partial_correlations (fp32, K
    matrices per launch) and comes back as a device tensor."""
    if torch.is_tensor(precision) and precision.is_cuda:
        P = precision.detach().to(dtype=torch.float32)
        single = P.dim() == 2
        rho = _lib.get_lib().partial_correlations((P[None] if single else P).contiguous())
        return rho[0] if single else rho
    P = np.asarray(precision.detach().cpu() if torch.is_tensor(precision) else precision, dtype=np.float64)
    d = np.sqrt(np.diagonal(P, axis1=-2, axis2=-1))
    up = np.triu(-P / (d[..., :, None] * d[..., None, :]), k=1)  # the reference reads the upper triangle and mirrors it
    rho = up + np.swapaxes(up, -1, -2)
    idx = np.arange(P.shape[-1])
    rho[..., idx, idx] = 1.0
    return rho


# -------------------------------------------------------------------------------------------- the recovered graph
GRAPH_STAT_KEYS = ("num_nodes", "num_edges", "avg_degree", "density", "avg_clustering", "transitivity", "diameter", "avg_shortest_path")


class RecoveredGraph(object):
    """One recovered graph: `edges` (m, 2) int32 with i < j in row-major order, `weights` (m,) -- the partial correlation of every edge
    (float32 from the device, float64 from the host formulation) -- `threshold`, `degree` (D,), `triangles` (D,) (None without stats) and
    `stats`, a dict with the keys of the reference's compute_graph_statistics (diameter and avg_shortest_path None: networkx's to give)."""

    __slots__ = ("edges", "weights", "threshold", "degree", "triangles", "stats")

    def __init__(self, edges, weights, threshold, degree, triangles, stats):
        self.edges, self.weights, self.threshold, self.degree, self.triangles, self.stats = edges, weights, threshold, degree, triangles, stats

    @property
    def positive(self) -> np.ndarray:
        """(m,) bool: the edge's sign ("+", the reference's green: rho > th)."""
        return self.weights > self.threshold


def _stats_dict(six) -> dict:
    d = {"num_nodes": int(six[0]), "num_edges": int(six[1])}
    d.update({key: float(x) for key, x in zip(GRAPH_STAT_KEYS[2:6], six[2:6])})
    d["diameter"] = d["avg_shortest_path"] = None
    return d


def _n_keep(sparsity, D: int) -> int:
    E = D * (D - 1) // 2
    n = int(sparsity * E)  # (ref main.py:865)
    if not 0 <= n <= E:
        raise ValueError(f"sparsity {sparsity} keeps {n} of {E} edges")
    return n


def _recovered_graph_host(values, from_precision: bool, n_keep, threshold, stats: bool) -> RecoveredGraph:
    """uglad_graph_wide's definitions for ONE (D, D) matrix on the host in float64, vectorised (sort, compare, (A A) o A): for a host array
    whose values float32 cannot hold -- rounding could merge a value with the threshold -- and for sizes the device does not cover."""
    V = np.asarray(values, dtype=np.float64)
    D = V.shape[-1]
    i, j = np.triu_indices(D, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = -V[i, j] / np.sqrt(V[i, i] * V[j, j]) if from_precision else V[i, j]
    if n_keep is None:
        th = np.float64(threshold)
    else:
        s = np.sort(np.abs(rho))
        th = s[len(s) - n_keep] if n_keep > 0 else s[0]  # (the reference's rho_upper[-0])
    keep = (rho > th) | (rho < -th)
    ei, ej = i[keep], j[keep]
    A = np.zeros((D, D))
    A[ei, ej] = A[ej, ei] = 1.0
    degree = A.sum(axis=1).astype(np.int64)
    triangles = st = None
    if stats:
        t2 = ((A @ A) * A).sum(axis=1).astype(np.int64)  # (exact: integers below 2^53)
        triangles = t2 // 2
        st = _stats_dict(_six_statistics(D, int(keep.sum()), degree, t2))
    return RecoveredGraph(np.stack([ei, ej], axis=1).astype(np.int32), rho[keep], th, degree, triangles, st)


def _six_statistics(D: int, m: int, degree, t2):
    """The operations networkx performs (density, average_clustering, transitivity), in its order, on Python integers."""
    d = [int(x) for x in degree]
    t = [int(x) for x in t2]
    c = [0 if ti == 0 else ti / (di * (di - 1)) for di, ti in zip(d, t)]
    return (D, m, sum(d) / D, m / (D * (D - 1)) * 2, sum(c) / D, 0 if sum(t) == 0 else sum(t) / sum(di * (di - 1) for di in d))


def _fits_float32(a: np.ndarray) -> bool:
    if a.dtype == np.float32:
        return True
    with np.errstate(over="ignore", invalid="ignore"):
        back = a.astype(np.float32).astype(a.dtype)
    return bool(np.all((back == a) | (a != a)))


def _recovered_graphs(values, from_precision: bool, n_keep, threshold, stats: bool):
    """K graphs of a (K, D, D) device tensor or host array: on the device wherever float32 holds the values (uglad_graph_wide), else by
    the host formulation."""
    lib = _lib.get_lib()
    on_device = torch.is_tensor(values) and values.device.type != "cpu"
    host = None if on_device else np.asarray(values.detach() if torch.is_tensor(values) else values)
    K, D = int(values.shape[0]), int(values.shape[-1])
    if D < 2 or D > lib.max_dim or not (on_device or _fits_float32(host)):
        host = values.detach().cpu().numpy() if on_device else host
        return [_recovered_graph_host(host[k], from_precision, n_keep, threshold, stats) for k in range(K)]
    g = lib.graph_wide(_to_dev(values if on_device else host), n_keep=n_keep, threshold=None if n_keep is not None else threshold,
                       from_precision=from_precision, want_stats=stats)
    count = g.edge_count.cpu().numpy()
    th, degree = g.threshold.cpu().numpy(), g.degree.cpu().numpy()
    t2, six = (g.triangles2.cpu().numpy(), g.stats.cpu().numpy()) if stats else (None, None)
    out = []
    for k in range(K):
        m = int(count[k])
        out.append(RecoveredGraph(g.edge_ij[k, :m].cpu().numpy(), g.edge_w[k, :m].cpu().numpy(), th[k], degree[k],
                                  t2[k] // 2 if stats else None, _stats_dict(six[k]) if stats else None))
    return out


def recovered_graph(precision, sparsity: float = 0.1, threshold=None, stats: bool = True):
    """The graph a precision matrix stands for (ref main.py:985-1005: partial correlations, then the `sparsity` fraction of the edges
    with the largest |rho|; or every edge beyond a given `threshold`), with degrees, triangle counts and the statistics of the reference's
    compute_graph_statistics, all computed on the device (uglad_graph_wide).  (D, D) or (K, D, D), a numpy array or a device tensor ->
    a RecoveredGraph or a list of K.  No networkx: graph_from_partial_correlations builds its nx.Graph from the same edge list."""
    single = len(precision.shape) == 2
    P = precision[None] if single else precision
    n_keep = None if threshold is not None else _n_keep(sparsity, int(P.shape[-1]))
    out = _recovered_graphs(P, True, n_keep, threshold, stats)
    return out[0] if single else out


def edge_frequency(precisions, sparsity: float = 0.1):
    """How often every edge comes back over R precision matrices -- the fits on R resamples of one table -- on the device (additive: the
    selection frequencies of stability selection and the instability of StARS; uglad_graph_wide for the R graphs at `sparsity`, then
    uglad_edge_frequency).  (R, D, D), a numpy array or a device tensor -> (frequency, sign_frequency, instability): frequency (D, D)
    float64 = the number of graphs that hold edge {i, j}, over R (symmetric, zero diagonal); sign_frequency the same over the graphs that
    hold it with a positive partial correlation; instability = 2 sum_{i<j} c_ij (R - c_ij) / (R^2 E) from exact integer totals, the
    mean over the E = D (D - 1) / 2 edges of 2 f (1 - f)."""
    lib = _lib.get_lib()
    if len(precisions.shape) != 3 or precisions.shape[1] != precisions.shape[2]:
        raise ValueError("edge_frequency takes (R, D, D) precision matrices")
    R, D = int(precisions.shape[0]), int(precisions.shape[-1])
    if D < 2 or D > lib.max_dim:
        raise ValueError(f"edge_frequency: D = {D} is outside 2 .. {lib.max_dim}")
    g = lib.graph_wide(_to_dev(precisions), n_keep=_n_keep(sparsity, D), from_precision=True, want_stats=False)
    out = lib.edge_frequency(g, D)
    count, positive = out.count.cpu().numpy().astype(np.int64), out.positive.cpu().numpy().astype(np.int64)
    totals = [int(t) for t in out.totals.cpu().numpy()]
    return count / R, positive / R, 2 * totals[1] / (R * R * (D * (D - 1) // 2))


def graph_from_partial_correlations(rho, names, sparsity=1, title="", fig_size=12, PLOT=True, save_file=None, roundOFF=5):
    """The reference's graph_from_partial_correlations (main.py:825-946), same arguments and return values: (nx.Graph with every node
    of `names` and the kept edges -- attributes color, weight rounded to `roundOFF` decimals, label -- , the PNG bytes of its drawing or
    None without PLOT, the edge list as strings).  The threshold, the membership test and the edge order come from uglad_graph_wide instead
    of a Python loop over D^2 entries: a device tensor stays on the device, a host array goes there when float32 holds its values
    exactly, and is otherwise evaluated on the host in float64 (rounding could merge values with the threshold)."""
    import networkx as nx

    names = list(names)
    D = int(rho.shape[-1])
    g = _recovered_graphs(rho[None], False, _n_keep(sparsity, D), None, False)[0]
    G = nx.Graph()
    G.add_nodes_from(names)
    edge_strings = []
    for (i, j), w, plus in zip(g.edges.tolist(), g.weights, g.positive):
        colour, w = ("green", "+") if plus else ("red", "-"), round(np.float64(w), roundOFF)
        G.add_edge(names[i], names[j], color=colour[0], weight=w, label=colour[1])
        edge_strings.append(f"({names[i]}, {names[j]}, {w}, {colour[0]})")
    return G, _draw_graph(G, title, fig_size, save_file) if PLOT else None, edge_strings


def _draw_graph(G, title, fig_size, save_file):
    """PNG bytes of a spring layout of G: grey nodes with their names just above them, edges in their colour, as wide as |weight| relative
    to the largest."""
    import io

    import matplotlib.pyplot as plt
    import networkx as nx

    colours = [c for _, _, c in G.edges(data="color")]
    widths = np.abs(np.array([w for _, _, w in G.edges(data="weight")], dtype=np.float64))
    if widths.size:
        widths = widths / widths.max()
    fig = plt.figure(figsize=(fig_size, fig_size))
    try:
        ax = fig.gca()
        where = nx.spring_layout(G, scale=0.2, k=1.0 / np.sqrt(G.number_of_edges() + 10))
        nx.draw_networkx_nodes(G, where, node_color="grey", node_size=100, ax=ax)
        nx.draw_networkx_edges(G, where, edge_color=colours, width=widths, ax=ax)
        nx.draw_networkx_labels(G, {node: (x, y + 0.008) for node, (x, y) in where.items()}, ax=ax)
        ax.set_title(str(title), fontsize=20)
        ax.margins(0.15)
        fig.tight_layout()
        if save_file:
            fig.savefig(save_file, bbox_inches="tight")
        png = io.BytesIO()
        fig.savefig(png)
        return png.getvalue()
    finally:
        plt.close(fig)


def compute_graph_statistics(G):
    """The reference's compute_graph_statistics (main.py:1263-1300): a one-row DataFrame with num_nodes, num_edges, avg_degree, density,
    avg_clustering, transitivity, diameter, avg_shortest_path.  The first six are counted on the device from G's adjacency matrix
    (uglad_graph_wide with the threshold 0.5: degrees, the triangle product); the last two are all-pairs searches and stay networkx's,
    for a connected graph only.  A graph the device does not cover (fewer than 2 or more than max_dim nodes, self-loops, directed or
    parallel edges) is networkx's as a whole."""
    import networkx as nx
    import pandas as pd

    D = G.number_of_nodes()
    if D < 2 or D > _lib.get_lib().max_dim or G.is_directed() or G.is_multigraph() or nx.number_of_selfloops(G):
        row = {"num_nodes": D, "num_edges": G.number_of_edges(), "avg_degree": sum(dict(G.degree()).values()) / D if D > 0 else 0,
               "density": nx.density(G), "avg_clustering": nx.average_clustering(G), "transitivity": nx.transitivity(G)}
    else:
        A = nx.to_numpy_array(G, dtype=np.float32, weight=None)
        row = _recovered_graphs(A[None], False, None, 0.5, True)[0].stats
    connected = nx.is_connected(G)
    row["diameter"] = nx.diameter(G) if connected else None
    row["avg_shortest_path"] = nx.average_shortest_path_length(G) if connected else None
    return pd.DataFrame([{key: row[key] for key in GRAPH_STAT_KEYS}])


def conditional_gaussian_batch(precision, mean, observed_mask, observed_values, clip01: bool = False, want_cov: bool = True):
    """K conditional-Gaussian problems on the device: precision (K,D,D), mean (K,D), observed_mask (K,D) bool, observed_values (K,D)
    (read where observed) -> full_mean (K,D), cond_cov (K,D,D) (L_uu^-1 on the unobserved block, identity elsewhere), log_pdf (K) --
    fp32 torch tensors on the device.  D <= max_eig_dim: uglad_conditional_mean (the path's eigensolver, fp32); beyond, up to max_dim:
    uglad_conditional_mean_wide (fp64 Cholesky, many workgroups per problem; `want_cov=False` skips the inverse and returns None for it)."""
    full, cov, logp = _conditional_gaussian_device(precision, mean, observed_mask, observed_values, clip01, want_cov)
    return full.to(torch.float32), cov, logp.to(torch.float32)


def _conditional_gaussian_device(precision, mean, observed_mask, observed_values, clip01, want_cov):
    """conditional_gaussian_batch in the precision the entry point computes in: full_mean and log_pdf are fp64 beyond max_eig_dim."""
    lib = _lib.get_lib()
    D = np.shape(precision)[-1]
    if D <= lib.max_eig_dim:
        return lib.conditional_mean(_to_dev(precision), _to_dev(mean), _to_dev(observed_mask), _to_dev(observed_values), clip01=clip01)
    if D > lib.max_dim:
        return _conditional_gaussian_host(precision, mean, observed_mask, observed_values, clip01, _lib.device())
    f = lambda a: _to_dev(a, torch.float64)  # noqa: E731
    return lib.conditional_mean_wide(f(precision), f(mean), _to_dev(observed_mask), f(observed_values), clip01=clip01, want_cov=want_cov)


def _conditional_gaussian_host(precision, mean, observed_mask, observed_values, clip01, dev):
    """D beyond what the device covers (uglad_conditional_mean_wide, D <= max_dim = 2048): the reference's own formulation on the host in
    float64 (ref main.py:1176-1227: mean_u - L_uu^-1 L_uo (x_o - mean_o), conditional covariance L_uu^-1, the density at the MAP point), returned
    in the layout of the device entry point (full mean; L_uu^-1 on the unobserved block, identity elsewhere; log density)."""
    to64 = lambda a: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)  # noqa: E731
    P, mu, mask, vals = to64(precision), to64(mean), to64(observed_mask) != 0, to64(observed_values)
    K, D = mu.shape
    full, cov, logp = np.empty((K, D)), np.empty((K, D, D)), np.empty(K)
    for k in range(K):
        o, u = np.where(mask[k])[0], np.where(~mask[k])[0]
        Luu_inv = np.linalg.inv(P[k][np.ix_(u, u)]) if u.size else np.zeros((0, 0))
        m = mu[k].copy()
        m[o] = vals[k][o]
        if u.size:
            m[u] = mu[k][u] - Luu_inv @ (P[k][np.ix_(u, o)] @ (vals[k][o] - mu[k][o]))
        if clip01:
            m = np.clip(m, 0.0, 1.0)
        full[k] = m
        cov[k] = np.eye(D)
        cov[k][np.ix_(u, u)] = Luu_inv
        # density of the conditional Gaussian at its own mean: (2 pi)^(-n_u / 2) det(L_uu)^(1/2)
        sign, ld = np.linalg.slogdet(P[k][np.ix_(u, u)]) if u.size else (1.0, 0.0)
        logp[k] = -0.5 * u.size * np.log(2.0 * np.pi) + 0.5 * ld if sign > 0 else np.nan
    t = lambda a: torch.as_tensor(a, dtype=torch.float32).to(dev)  # noqa: E731
    return t(full), t(cov), t(logp)


def conditional_gaussian_with_probabilities(precision, mean, observed_idx, observed_values):
    """Conditional mean, conditional covariance and density at the MAP point of a Gaussian given observed coordinates
    (ref main.py:1176-1227, same arguments and return values): (full_mean (n,), conditional_cov (n_u, n_u), pdf).
    The reference solves with scipy on the host; here the path's eigensolver does it on the device (fp32), and beyond its size the fp64
    Cholesky of uglad_conditional_mean_wide: the density is the exponential of its fp64 logarithm."""
    precision = np.asarray(precision)
    mean = np.asarray(mean, dtype=np.float64)
    n = len(mean)
    observed_idx = [int(i) for i in observed_idx]
    mask = np.zeros(n, dtype=np.float32)
    mask[observed_idx] = 1.0
    vals = np.zeros(n, dtype=np.float64)
    vals[observed_idx] = np.asarray(observed_values, dtype=np.float64)
    full, cov, logp = _conditional_gaussian_device(precision[None], mean[None], mask[None], vals[None], False, True)
    unobs = [i for i in range(n) if mask[i] == 0.0]
    cov = cov[0].cpu().numpy().astype(np.float64)
    return full[0].cpu().numpy().astype(np.float64), cov[np.ix_(unobs, unobs)], float(np.exp(np.float64(logp[0].item())))


def compute_map_estimate(observed_nodes: dict, model_uGLAD) -> np.ndarray:
    """MAP estimate of all nodes given some observed ones, clamped to [0, 1] (ref main.py:1229-1260): uses the estimator's
    precision_, location_ and node_names_."""
    names = list(model_uGLAD.node_names_)
    idx = [names.index(k) for k in observed_nodes.keys()]
    n = len(names)
    mask = np.zeros(n, dtype=np.float32)
    mask[idx] = 1.0
    vals = np.zeros(n, dtype=np.float64)
    vals[idx] = list(observed_nodes.values())
    full, _, _ = conditional_gaussian_batch(np.asarray(model_uGLAD.precision_)[None], np.asarray(model_uGLAD.location_)[None],
                                            mask[None], vals[None], clip01=True, want_cov=False)
    return full[0].cpu().numpy().astype(np.float64)
