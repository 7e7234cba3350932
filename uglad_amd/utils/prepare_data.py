"""Host-side table preparation and synthetic Gaussian-graph data for the GLAD path.

This is the one-off O(M*D^2) numpy/pandas work that runs once per ``fit`` before the
unrolled GLAD cell takes over on the device.  Semantics follow the reference
(``uglad/utils/prepare_data.py``): ``process_table`` :361-516, ``normalize_table``
:597-613, ``get_covariance`` :328-356, ``convert_to_torch`` :288-307, ``get_data``
:93-140, ``add_noise_dropout`` :143-169, ``cramers_v`` / ``correlation_ratio`` /
``pairwise_cov_matrix`` :177-285 (vectorised, no scipy).  Differences, all additive:

* every random draw takes an explicit ``rng`` (``numpy.random.Generator``); the reference
  consumes numpy's and Python's *global* RNG streams, which is why its notebook numbers
  are not reproducible;
* the Erdos-Renyi adjacency is drawn with numpy instead of networkx;
* nothing prints unless ``VERBOSE`` is true.
"""
from __future__ import annotations

from time import time
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from .. import _lib

__all__ = [
    "generate_random_graph",
    "simulate_gaussian_samples",
    "get_data",
    "add_noise_dropout",
    "convert_to_torch",
    "eigen_val_condition_num",
    "empirical_covariance",
    "get_covariance",
    "normalize_table",
    "process_table",
    "analyse_condition_number",
    "get_highly_correlated_features",
    "eigvalsh_device",
    "synthetic_covariance_batch",
    "cramers_v",
    "correlation_ratio",
    "pairwise_cov_matrix",
    "encode_mixed_table",
    "association_from_codes",
    "MixedMaps",
]


def _rng(rng) -> np.random.Generator:
    if isinstance(rng, np.random.Generator):
        return rng
    return np.random.default_rng(rng)


# --------------------------------------------------------------------------- synthetic
def generate_random_graph(num_nodes: int, sparsity, rng=None) -> np.ndarray:
    """Symmetric 0/1 adjacency of a G(n, p) graph, p ~ U[sparsity] (ref :13-35)."""
    rng = _rng(rng)
    lo, hi = sparsity
    p = rng.uniform(lo, hi)
    upper = np.triu(rng.random((num_nodes, num_nodes)) < p, 1)
    adj = (upper | upper.T).astype(np.float64)
    return adj


def simulate_gaussian_samples(
    num_nodes: int,
    edge_connections: np.ndarray,
    num_samples: int,
    rng=None,
    u: float = 0.1,
    w_min: float = 0.5,
    w_max: float = 1.0,
):
    """Precision = sym(adj * U[w_min,w_max]) + I, shifted so lambda_min == u; samples ~ N(0, P^-1)
    (ref :38-90).  Returns (X (num_samples, D), precision (D, D))."""
    rng = _rng(rng)
    W = rng.random((num_nodes, num_nodes)) * (w_max - w_min) + w_min
    theta = np.asarray(edge_connections, dtype=np.float64) * W
    theta = (theta + theta.T) / 2.0 + np.eye(num_nodes)
    smallest = np.linalg.eigvalsh(theta).min()
    precision = theta + np.eye(num_nodes) * (u - smallest)
    cov = np.linalg.inv(precision)
    cov = (cov + cov.T) / 2.0
    X = rng.multivariate_normal(np.zeros(num_nodes), cov, size=num_samples, method="cholesky")
    return X, precision


def get_data(
    num_nodes: int,
    sparsity,
    num_samples: int,
    batch_size: int = 1,
    w_min: float = 0.5,
    w_max: float = 1.0,
    eig_offset: float = 0.1,
    rng=None,
):
    """Batch of (samples, true precision) pairs (ref :93-140)."""
    rng = _rng(rng)
    Xb, thetas = [], []
    for _ in range(batch_size):
        adj = generate_random_graph(num_nodes, sparsity, rng)
        X, P = simulate_gaussian_samples(
            num_nodes, adj, num_samples, rng, u=eig_offset, w_min=w_min, w_max=w_max
        )
        Xb.append(X)
        thetas.append(P)
    return np.array(Xb), np.array(thetas)


def add_noise_dropout(Xb: np.ndarray, dropout: float = 0.25, rng=None) -> np.ndarray:
    """Replace a fraction of the entries of each table by NaN (ref :143-169)."""
    rng = _rng(rng)
    out = []
    for X in Xb:
        flat = np.array(X, dtype=np.float64).reshape(-1)
        idx = rng.choice(flat.size, size=int(flat.size * dropout), replace=False)
        flat[idx] = np.nan
        out.append(flat.reshape(X.shape))
    return np.array(out)


# --------------------------------------------------------------------------- conversion
def convert_to_torch(data, req_grad: bool = False, device=None) -> torch.Tensor:
    """numpy -> fp32 torch tensor (ref :288-307).  ``device`` replaces the reference's
    ``use_cuda`` flag; default stays host memory like the reference."""
    if not torch.is_tensor(data):
        data = torch.from_numpy(np.asarray(data).astype(np.float64, copy=False)).to(torch.float32)
    if device is not None:
        data = data.to(device)
    data.requires_grad = req_grad
    return data


# --------------------------------------------------------------------------- covariance
def empirical_covariance(X, assume_centered: bool = False) -> np.ndarray:
    """Maximum-likelihood covariance X^T X / n, as sklearn.covariance.empirical_covariance
    (the routine the reference calls at :342 and main.py:139)."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(1, -1)
    if assume_centered:
        return X.T @ X / X.shape[0]
    return np.cov(X.T, bias=1).reshape(X.shape[1], X.shape[1])


def eigen_val_condition_num(A: np.ndarray):
    """Real parts of the eigenvalues and max|eig|/min|eig| (ref :310-325)."""
    eig = [float(v.real) for v in np.linalg.eigvals(A)]
    a = np.abs(eig)
    return eig, float(a.max() / a.min())


def get_covariance(Xb, offset: float = 0.1, VERBOSE: bool = False) -> np.ndarray:
    """Batch covariance with the reference's eigenvalue repair (ref :328-356): when the
    smallest eigenvalue is <= 1e-6 the matrix is shifted so that it becomes ``offset``."""
    Sb = []
    for X in Xb:
        S = empirical_covariance(X, assume_centered=False)
        eig, con = eigen_val_condition_num(S)
        if min(eig) <= 1e-6:
            if VERBOSE:
                print(f"Adjust the eval: min {min(eig)}, con {con}")
            S = S + np.eye(S.shape[-1]) * (offset - min(eig))
        Sb.append(S)
    return np.array(Sb)


# --------------------------------------------------------------------------- table checks
def normalize_table(df, typeN: str):
    """'min_max' | 'mean' | anything else = untouched (ref :597-613)."""
    if typeN == "min_max":
        return (df - df.min()) / (df.max() - df.min())
    if typeN == "mean":
        return (df - df.mean()) / df.std()
    return df


# The device path of the three functions below (device=True): the covariance, ALL its eigenvalues and the ranking of correlated features
# come from the library (csrc/eigvals_wide.h, csrc/corr_wide.h; every D <= max_dim = 2048), the table is uploaded once as float64 and only
# a handful of numbers come back per round.  Nothing falls back to the host silently: a table the device cannot take raises UgladError.
def _device_lib(D: int, what: str):
    from .. import _lib

    lib = _lib.get_lib()
    if D < 1 or D > lib.max_dim:
        raise _lib.UgladError(f"{what}(device=True): {D} columns; the device path covers 1 <= D <= max_dim = {lib.max_dim}")
    return lib, _lib.device()


def _to_device_f64(a, dev) -> torch.Tensor:
    if torch.is_tensor(a):
        return a.to(device=dev, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def eigvalsh_device(A, th: float = 0.0, return_summary: bool = False):
    """All eigenvalues of the symmetric part of A, (D, D) or (K, D, D), D <= max_dim, in float64 on the device (uglad_eigvalsh_wide),
    ASCENDING.  A numpy array comes back as a numpy array, a tensor as a tensor on the device.  With `return_summary` also the (.., 6)
    array min, max, min |.|, max |.|, con = max |.| / min |.|, number of eigenvalues < th."""
    if np.ndim(A) not in (2, 3) or np.shape(A)[-1] != np.shape(A)[-2]:
        raise ValueError(f"eigvalsh_device takes (D, D) or (K, D, D); got {tuple(np.shape(A))}")
    lib, dev = _device_lib(int(np.shape(A)[-1]), "eigvalsh_device")
    Ad = _to_device_f64(A, dev)
    single = Ad.dim() == 2
    eig, summary = lib.eigvalsh_wide(Ad[None] if single else Ad, th=th)
    if single:
        eig, summary = eig[0], summary[0]
    if not torch.is_tensor(A):
        eig, summary = eig.cpu().numpy(), summary.cpu().numpy()
    return (eig, summary) if return_summary else eig


def _table_spectrum_device(Xd, eigval_th: float, want_cov: bool):
    """One uglad_table_spectrum call on the (N, D) device table: (eig tensor (D,), con, number of eigenvalues < eigval_th, cov (D, D))."""
    lib, _ = _device_lib(int(Xd.shape[1]), "analyse_condition_number")
    eig, summary, cov = lib.table_spectrum(Xd[None], th=eigval_th, want_cov=want_cov)
    back = summary[0, 4:6].cpu().numpy()  # the readback: con and the count
    return eig[0], float(back[0]), int(back[1]), (None if cov is None else cov[0])


def analyse_condition_number(table, MESSAGE: str = "", VERBOSE: bool = True, device: bool = False):
    """Covariance, eigenvalues and condition number of a table (ref :569-594).  With ``device=True`` all three come from the device
    (uglad_table_spectrum, fp64): the eigenvalues are then ASCENDING, where LAPACK's general solver on the host returns them in no
    particular order -- nothing in the package depends on the order."""
    if device:
        X = np.ascontiguousarray(np.asarray(table, dtype=np.float64))
        _, dev = _device_lib(int(X.shape[1]) if X.ndim == 2 else 0, "analyse_condition_number")
        eig_d, con, _, cov = _table_spectrum_device(_to_device_f64(X, dev), 0.0, True)
        S, eig = cov.cpu().numpy(), [float(x) for x in eig_d.cpu().numpy()]
    else:
        S = empirical_covariance(np.asarray(table, dtype=np.float64), assume_centered=False)
        eig, con = eigen_val_condition_num(S)
    if VERBOSE:
        print(f"{MESSAGE} covariance matrix: condition number {con}, min eig {min(eig)} max eig {max(eig)}")
    return S, eig, con


def get_highly_correlated_features(input_cov: np.ndarray, device: bool = False) -> np.ndarray:
    """Rank features by how many top-10% |cov-of-cov| partners they have (ref :519-550).  ``device=True``: the same list from
    uglad_correlated_features (the threshold by an exact radix select on the fp64 magnitudes; ties by index ascending, which is what the
    reference's dict insertion order under its stable sort amounts to)."""
    if device:
        lib, dev = _device_lib(int(np.shape(input_cov)[-1]), "get_highly_correlated_features")
        order, _, n_listed = lib.correlated_features(_to_device_f64(input_cov, dev)[None])
        return order[0, : int(n_listed[0])].cpu().numpy().astype(np.int64)
    cov2 = empirical_covariance(input_cov)
    np.fill_diagonal(cov2, 0.0)
    a = np.abs(cov2)
    r, c = np.triu_indices(a.shape[0], 1)
    upper = np.sort(a[r, c])[::-1]
    th = upper[int(0.1 * len(upper))]
    rows, _ = np.nonzero(a >= th)
    feats, counts = np.unique(rows, return_counts=True)
    order = np.argsort(-counts, kind="stable")
    return feats[order]


def process_table(
    table,
    NORM: str = "no",
    MIN_VARIANCE: float = 0.0,
    msg: str = "",
    COND_NUM: float = np.inf,
    eigval_th: float = 1e-3,
    VERBOSE: bool = True,
    device: bool = False,
    rounds: Optional[list] = None,
):
    """Make a real-valued table fit for sparse graph recovery (ref :361-516), in the
    reference's order: drop all-zero rows, fill NaN with the column mean, drop
    single-valued columns, normalise, drop duplicate columns, drop low-variance columns,
    then (only when ``COND_NUM`` is finite) drop highly correlated columns until the
    covariance condition number is acceptable.  Returns a pandas DataFrame.

    ``device=True`` runs the conditioning loop with the table resident on the device: the pandas steps stay on the host, the cleaned
    table is uploaded once as float64, and every round costs one uglad_table_spectrum call, one uglad_correlated_features call and the
    readback of con, the number of eigenvalues below ``eigval_th`` and the indices to drop; columns leave by index_select.  The returned
    DataFrame is cut from the host table: its values never pass through the device.  More than max_dim = 2048 columns raise UgladError.
    ``rounds``: a list that receives one ``(columns, con, eigenvalues below eigval_th)`` per covariance analysed from "Processed" on."""
    import pandas as pd

    start = time()
    table = pd.DataFrame(table).astype(float)
    n0 = table.shape[0]
    table = table.loc[~(table == 0).all(axis=1)]
    if VERBOSE:
        print(f"{msg}: input {n0} samples x {table.shape[1]} features; zero rows dropped {n0 - table.shape[0]}")
    table = table.fillna(table.mean())
    single = [c for c in table.columns if table[c].nunique(dropna=False) == 1]
    table = table.drop(columns=single)
    table = normalize_table(table, NORM)
    if VERBOSE:
        print(f"{msg}: single-valued columns dropped {len(single)}")
        analyse_condition_number(table, "Input", VERBOSE, device=device)
    cols = table.columns
    table = table.T.drop_duplicates().T
    if VERBOSE:
        print(f"{msg}: duplicate columns dropped {len(cols) - len(table.columns)}")
    var = table.var()
    low = list(var[var < MIN_VARIANCE].index)
    table = table.drop(columns=low)
    if device:
        table = _condition_on_device(table, msg, COND_NUM, eigval_th, VERBOSE, rounds)
    else:
        cov_table, eig, con = analyse_condition_number(table, "Processed", VERBOSE)
        if rounds is not None:
            rounds.append((table.shape[1], con, int(np.sum(np.array(eig) < eigval_th))))
        itr = 1
        while con > COND_NUM:
            lb = int(np.sum(np.array(eig) < eigval_th))
            if lb == 0:
                lb = 1
            feats = get_highly_correlated_features(cov_table)
            feats = feats[: min(lb, len(feats))]
            table = table.drop(columns=table.columns[feats])
            cov_table, eig, con = analyse_condition_number(table, f"{msg} {itr}: corr dropped", VERBOSE)
            if rounds is not None:
                rounds.append((table.shape[1], con, int(np.sum(np.array(eig) < eigval_th))))
            itr += 1
    if VERBOSE:
        print(f"{msg}: processed table {table.shape[0]} x {table.shape[1]} in {np.round(time() - start, 3)} s")
    return table


def _condition_on_device(table, msg, COND_NUM, eigval_th, VERBOSE, rounds):
    """process_table's loop over the covariance's condition number with the table on the device; returns the host table's kept columns."""
    lib, dev = _device_lib(int(table.shape[1]), "process_table")
    X = _to_device_f64(table.to_numpy(dtype=np.float64), dev)  # the one upload
    finite = bool(np.isfinite(COND_NUM))

    def analyse(X, message):
        eig, con, below, cov = _table_spectrum_device(X, eigval_th, finite)
        if VERBOSE:
            ends = eig[[0, -1]].cpu().numpy()
            print(f"{message} covariance matrix: condition number {con}, min eig {float(ends[0])} max eig {float(ends[1])}")
        if rounds is not None:
            rounds.append((int(X.shape[1]), con, below))
        return con, below, cov

    con, below, cov = analyse(X, "Processed")
    itr = 1
    while con > COND_NUM:
        lb = below if below > 0 else 1
        order, _, n_listed = lib.correlated_features(cov[None])
        feats = order[0, : min(lb, int(n_listed[0]))].cpu().numpy()
        keep = np.setdiff1d(np.arange(table.shape[1]), feats)
        table = table.drop(columns=table.columns[feats])
        X = X.index_select(1, torch.from_numpy(keep).to(dev)).contiguous()
        con, below, cov = analyse(X, f"{msg} {itr}: corr dropped")
        itr += 1
    return table


def kept_min_range(raw_table, processed):
    """Column minima and ranges, (D,) float64 each, of what ``process_table(raw_table, NORM="min_max")`` normalised, over the rows and
    columns it kept (``processed`` is its return value): ``(raw[kept rows][:, kept columns] - min) / range`` reproduces ``processed`` bit
    for bit.  The reference throws both away inside its fit; a new row can be placed in the model's coordinates only with them.  (The
    NaN that process_table fills with the column mean cannot move a minimum or a maximum.)"""
    import pandas as pd

    raw = pd.DataFrame(raw_table).astype(float)
    sub = raw.loc[processed.index, processed.columns]
    mn, mx = sub.min(), sub.max()
    return mn.to_numpy(dtype=np.float64), (mx - mn).to_numpy(dtype=np.float64)


# --------------------------------------------------------------------------- mixed tables
# The association matrix of a table that mixes categorical ('c') and real ('r') columns (ref :177-285): bias-corrected Cramer's V for
# c/c pairs, the correlation ratio eta for c/r pairs, Pearson's r for r/r pairs.  The reference loops over the D^2 pairs with
# pd.crosstab / scipy's chi2_contingency / pearsonr; here the table is expanded once -- a 0/1 column per level of every categorical,
# every real column centred and scaled to unit norm -- and ONE Gram product of the expanded table holds every contingency table, every
# per-level sum and every Pearson coefficient; a reduction per pair of features finishes it.  The device (csrc/assoc_wide.h) does the
# same on the expanded layout that encode_mixed_table describes.
ASSOC_TILE = 64           # a feature's expanded columns never straddle a multiple of this (csrc/chol_wide.h: kT64)
ASSOC_MAX_DIM = 2048      # uglad_max_dim()
ASSOC_MAX_WIDTH = 16384   # UGLAD_ASSOC_MAX_WIDTH (include/uglad_hip.h)
ASSOC_REAL = -1           # the level of a real feature's single expanded column
ASSOC_PAD = -2            # the level of a padding column (its feature is -1)


class MixedMaps(NamedTuple):
    """The expanded layout of an encoded mixed table (encode_mixed_table): W = len(col_feature) expanded columns, a multiple of 64."""
    names: list               # the D column names
    kinds: np.ndarray         # (D,) 'c' | 'r'
    cards: np.ndarray         # (D,) int32: levels of a categorical, 0 for a real column
    col_feature: np.ndarray   # (W,) int32: the feature of every expanded column, -1 for padding
    col_level: np.ndarray     # (W,) int32: its level, ASSOC_REAL for a real column, ASSOC_PAD for padding
    feat_offset: np.ndarray   # (D,) int32: a feature's first expanded column
    feat_width: np.ndarray    # (D,) int32: its number of expanded columns (levels, or 1)
    tile_first: np.ndarray    # (W / 64 + 1,) int32: the first feature of every tile of 64 expanded columns; the last entry is D

    @property
    def W(self) -> int:
        return int(self.col_feature.shape[0])


def _expanded_layout(names, kinds, cards) -> MixedMaps:
    D = len(names)
    width = np.where(kinds == "c", cards, 1).astype(np.int32)
    offset = np.zeros(D, dtype=np.int32)
    at = 0
    for i in range(D):
        if at % ASSOC_TILE + int(width[i]) > ASSOC_TILE:  # would straddle: start at the next multiple
            at = (at // ASSOC_TILE + 1) * ASSOC_TILE
        offset[i] = at
        at += int(width[i])
    W = -(-at // ASSOC_TILE) * ASSOC_TILE
    if W > ASSOC_MAX_WIDTH:
        raise ValueError(f"the expanded table is {W} columns wide; the limit is {ASSOC_MAX_WIDTH}")
    col_feature = np.full(W, -1, dtype=np.int32)
    col_level = np.full(W, ASSOC_PAD, dtype=np.int32)
    for i in range(D):
        o, w = int(offset[i]), int(width[i])
        col_feature[o:o + w] = i
        col_level[o:o + w] = np.arange(w) if kinds[i] == "c" else ASSOC_REAL
    tile_first = np.searchsorted(offset, np.arange(0, W + 1, ASSOC_TILE)).astype(np.int32)
    return MixedMaps(list(names), kinds, cards.astype(np.int32), col_feature, col_level, offset, width, tile_first)


def encode_mixed_table(df, dtype):
    """A table of categorical and real columns -> (table, maps): the float64 (N, D) table whose 'c' columns hold the level codes
    0 .. card - 1 (pd.factorize order) and whose 'r' columns hold the values, and the MixedMaps of its expanded layout.  `dtype` maps
    column name -> 'c' | 'r' (ref :253-267).  ValueError, naming the column, for a categorical with more than 64 levels or with missing
    values, a column with a single value, an unknown type letter; also for more than ASSOC_MAX_DIM columns or an expanded width
    beyond ASSOC_MAX_WIDTH."""
    import pandas as pd

    df = pd.DataFrame(df)
    names = list(df.columns)
    N, D = df.shape
    if D > ASSOC_MAX_DIM:
        raise ValueError(f"{D} columns; the limit is {ASSOC_MAX_DIM}")
    table = np.empty((N, D), dtype=np.float64)
    kinds = np.empty(D, dtype="<U1")
    cards = np.zeros(D, dtype=np.int32)
    for i, name in enumerate(names):
        kind = dtype.get(name) if hasattr(dtype, "get") else dtype[name]
        col = df.iloc[:, i]
        if kind == "c":
            if col.isna().any():
                raise ValueError(f"categorical column {name!r} has missing values")
            codes, levels = pd.factorize(col)
            if len(levels) > ASSOC_TILE:
                raise ValueError(f"categorical column {name!r} has {len(levels)} levels; the limit is {ASSOC_TILE}")
            if len(levels) < 2:
                raise ValueError(f"categorical column {name!r} has a single value")
            table[:, i] = codes
            cards[i] = len(levels)
        elif kind == "r":
            vals = np.asarray(col, dtype=np.float64)
            seen = vals[~np.isnan(vals)]
            if seen.size == 0 or seen.min() == seen.max():
                raise ValueError(f"real column {name!r} has a single value")
            table[:, i] = vals
        else:
            raise ValueError(f"column {name!r} has type {kind!r}; expected 'c' or 'r'")
        kinds[i] = kind
    return table, _expanded_layout(names, kinds, cards)


def association_from_codes(table, kinds, cards) -> np.ndarray:
    """The (D, D) float64 association matrix of an encoded table (encode_mixed_table): one-hot Gram, then a reduction per pair.
    A level without a row in this table is ignored, as pd.crosstab ignores it."""
    table = np.asarray(table, dtype=np.float64)
    N, D = table.shape
    kinds = np.asarray(kinds)
    cat, real = np.nonzero(kinds == "c")[0], np.nonzero(kinds == "r")[0]
    A = np.zeros((D, D))
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = table[:, real]
        Zc = Z - Z.mean(axis=0)
        Zn = Zc * (1.0 / np.sqrt((Zc * Zc).sum(axis=0)))  # unit norm: Zn^T Zn is Pearson's r (scipy: dot(xm / |xm|, ym / |ym|))
        A[np.ix_(real, real)] = Zn.T @ Zn
        if cat.size == 0:
            return A
        width = np.asarray(cards)[cat].astype(np.int64)
        start = np.concatenate([[0], np.cumsum(width)[:-1]])
        owner = np.repeat(np.arange(cat.size), width)             # the categorical (its index in `cat`) of every level column
        level = np.arange(int(width.sum())) - start[owner]
        H = (table[:, cat[owner]] == level).astype(np.float64)     # (N, levels of all categoricals)
        cnt = H.sum(axis=0)
        live = cnt > 0
        # c/r: eta^2 = sum_a s_a^2 / n_a, s_a the per-level sum of the unit-norm column (= sum_a n_a (mean_a - mean)^2 / sum (y - mean)^2)
        if real.size:
            q = np.where(live[:, None], (H.T @ Zn) ** 2 / cnt[:, None], 0.0)
            eta2 = np.add.reduceat(q, start, axis=0)
            eta = np.where(eta2 == 0, 0.0, np.sqrt(eta2))
            A[np.ix_(cat, real)] = eta
            A[np.ix_(real, cat)] = eta.T
        # c/c: chi^2 of every contingency table (the Gram blocks), Yates' correction at one degree of freedom, bias-corrected V
        G = H.T @ H
        nlive = np.add.reduceat(live.astype(np.int64), start)      # r, k: the levels that occur
        n = float(N)
        for a, i in enumerate(cat):
            rows = slice(start[a], start[a] + width[a])
            O = G[rows]
            E = np.outer(cnt[rows], cnt) / n
            both = live[rows][:, None] & live[None, :]
            yates = ((nlive[a] - 1) * (nlive - 1) == 1)[owner]
            diff = E - O
            O = np.where(yates[None, :], O + np.sign(diff) * np.minimum(0.5, np.abs(diff)), O)
            chi2 = np.add.reduceat(np.where(both, (O - E) ** 2 / E, 0.0).sum(axis=0), start)
            r, k = float(nlive[a]), nlive.astype(np.float64)
            phi2corr = np.maximum(0.0, chi2 / n - (k - 1) * (r - 1) / (n - 1))
            denom = np.minimum(k - (k - 1) ** 2 / (n - 1) - 1, r - (r - 1) ** 2 / (n - 1) - 1)
            A[i, cat] = np.where(denom == 0, 0.0, np.sqrt(phi2corr / denom))
    return A


def _encode_pair(x, kx, y, ky):
    import pandas as pd

    cols, cards = [], []
    for v, kind in ((x, kx), (y, ky)):
        if kind == "c":
            codes, levels = pd.factorize(np.asarray(v))
            cols.append(codes.astype(np.float64))
            cards.append(len(levels))
        else:
            cols.append(np.asarray(v, dtype=np.float64))
            cards.append(0)
    return np.stack(cols, axis=1), np.array([kx, ky]), np.array(cards)


def cramers_v(x, y) -> float:
    """Bias-corrected Cramer's V of two categorical variables, with Yates' correction on a 2 x 2 table as scipy's chi2_contingency
    applies it (ref :177-209)."""
    return float(association_from_codes(*_encode_pair(x, "c", y, "c"))[0, 1])


def correlation_ratio(categories, measurements) -> float:
    """The correlation ratio eta of a categorical and a real variable (ref :212-250)."""
    return float(association_from_codes(*_encode_pair(categories, "c", measurements, "r"))[0, 1])


def pairwise_cov_matrix(df, dtype):
    """The association matrix of a mixed table as a DataFrame indexed by the features (ref :253-285), without the reference's
    per-row progress lines."""
    import pandas as pd

    table, maps = encode_mixed_table(df, dtype)
    return pd.DataFrame(association_from_codes(table, maps.kinds, maps.cards), index=maps.names, columns=maps.names)


# --------------------------------------------------------------------------- rank correlations (the nonparanormal front-end)
# The host formulation of uglad_rank_correlation (csrc/rank_wide.h; additive, the reference has no such option): vectorised fp64 numpy.  The
# tests' oracle beyond the goldens, and the probe's baseline.
RANK_METHODS = tuple(_lib.RANK_METHODS)  # "spearman", "kendall", "scores": the names of UGLAD_RANK_* in their order, stated in _lib
RANK_MAX_ROWS = 65536  # include/uglad_hip.h: where a diagonal entry of Kendall's Gram matrix reaches 2^31


def doubled_midranks(X) -> np.ndarray:
    """r2[a, i] = 2 #{b : x_bi < x_ai} + #{b : x_bi = x_ai} + 1 per column of an (N, D) table, int64: twice
    scipy.stats.rankdata(method="average").  A NaN is below and equal to nothing, and nothing is below or equal to it."""
    X = np.asarray(X, dtype=np.float64)
    r2 = np.empty(X.shape, dtype=np.int64)
    for i in range(X.shape[1]):
        x = X[:, i]
        s = np.sort(x[~np.isnan(x)])
        r2[:, i] = np.where(np.isnan(x), 1, np.searchsorted(s, x, "left") + np.searchsorted(s, x, "right") + 1)
    return r2


def rank_gram_host(X, method: str, chunk_pairs: int = 8192) -> np.ndarray:
    """The (D, D) float64 Gram matrix the coefficient of `method` is a ratio of (include/uglad_hip.h): for "spearman" sum_a c_ai c_aj with
    c = r2 - (N + 1); for "kendall" G = s^T s over the N (N - 1) / 2 row pairs a < b, s = sign(x_a - x_b), as float64 BLAS products of
    the sign rows in chunks -- both exact integers below 2^53; for "scores" the centred sums of products of Phi^-1(r2 / (2 (N + 1)))."""
    if method not in RANK_METHODS:
        raise ValueError(f"method {method!r} is none of {RANK_METHODS}")
    r2 = doubled_midranks(X)
    N, D = r2.shape
    if method == "spearman":
        c = (r2 - (N + 1)).astype(np.float64)
        return c.T @ c
    if method == "scores":
        z = torch.special.ndtri(torch.from_numpy(r2.astype(np.float64) / (2.0 * (N + 1)))).numpy()
        z = z - z.mean(axis=0)
        return z.T @ z
    G = np.zeros((D, D))
    rows, held = [], 0
    for a in range(N - 1):
        rows.append(np.sign(r2[a] - r2[a + 1:]).astype(np.float64))
        held += N - 1 - a
        if held >= chunk_pairs or a == N - 2:
            S = np.concatenate(rows)
            G += S.T @ S
            rows, held = [], 0
    return G


def rank_correlation_host(X, method: str, transform: bool = True) -> np.ndarray:
    """The rank-based correlation matrix of an (N, D) table as uglad_rank_correlation defines it, float64, unrepaired: Spearman's rho
    (`transform`: 2 sin(pi rho / 6)), Kendall's tau-b (`transform`: sin(pi tau / 2)) or the correlation of the normal scores; exactly 1
    on the diagonal, NaN in the row and column of a feature that holds a NaN or is constant."""
    X = np.asarray(X, dtype=np.float64)
    g = rank_gram_host(X, method)
    root = np.sqrt(np.diag(g))
    with np.errstate(invalid="ignore", divide="ignore"):
        A = g / (root[:, None] * root[None, :])
    if transform and method == "spearman":
        A = 2.0 * np.sin(np.pi * A / 6.0)
    if transform and method == "kendall":
        A = np.sin(np.pi * A / 2.0)
    A[np.diag_indices_from(A)] = 1.0
    bad = np.isnan(X).any(axis=0) | (X == X[:1]).all(axis=0)
    A[bad, :] = np.nan
    A[:, bad] = np.nan
    return A


# --------------------------------------------------------------------------- tables with missing entries
def observed_min_scale(X):
    """(min, 1 / (max - min)) over the observed (not NaN) entries of every column of an (N, D) table, float64: the min-max map of
    uglad_pairwise_covariance under normalize = 1, y = (x - min) * scale.  NaN for a column without an observed entry."""
    X = np.asarray(X, dtype=np.float64)
    seen = ~np.isnan(X)
    mn = np.where(seen, X, np.inf).min(axis=0)
    mx = np.where(seen, X, -np.inf).max(axis=0)
    empty = ~seen.any(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(empty, np.nan, mn), np.where(empty, np.nan, 1.0 / (mx - mn))


def pairwise_covariance_host(X, normalize: bool = False, min_pairs: int = 2):
    """The available-case (pairwise-complete) covariance of an (N, D) table whose NaN are missing entries, as uglad_pairwise_covariance
    defines it (include/uglad_hip.h, csrc/pairwise_wide.h; additive: the reference imputes column means), vectorised fp64 numpy: the
    tests' oracle and the probe's baseline.  With m = 1 where observed, y = x or (`normalize`) the column min-max normalised over its
    observed entries, z = m (y - the observed mean): cov_ij = p_ij / n_ij - (a_ij / n_ij) (a_ji / n_ij) with n = m^T m, a = z^T m,
    p = z^T z -- pandas' DataFrame.cov times (n_ij - 1) / n_ij.  Returns (cov (D, D) float64, exactly symmetric, NaN where n_ij <
    min_pairs and wherever the arithmetic gives it: a column that is all NaN, constant under `normalize`, or holds an infinity; counts
    (D, D) int64, n_ij)."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("pairwise_covariance_host takes one (N, D) table")
    if min_pairs < 1:
        raise ValueError(f"min_pairs must be at least 1, got {min_pairs}")
    seen = ~np.isnan(X)
    m = seen.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        y = X
        if normalize:
            mn, scale = observed_min_scale(X)
            y = (X - mn) * scale
        count = m.sum(axis=0)
        mu = np.where(seen, y, 0.0).sum(axis=0) / count
        z = np.where(seen, y - mu, 0.0)
        n, a, p = m.T @ m, z.T @ m, z.T @ z
        cov = p / n - (a / n) * (a.T / n)
    cov[n < min_pairs] = np.nan
    cov = np.triu(cov) + np.triu(cov, 1).T  # (the mirror is a copy, as on the device)
    return cov, np.rint(n).astype(np.int64)


# --------------------------------------------------------------------------- resamples of one table
def weighted_covariance_host(X, W):
    """The covariances of ONE (N, D) table under the (R, N) row weightings W, as uglad_weighted_covariance defines them
    (include/uglad_hip.h, csrc/wcov_wide.h; additive), fp64 numpy: per weighting, with s = sum_n w_n and mu = sum_n w_n x_n / s,
    S = sum_n w_n (x_n - mu)(x_n - mu)^T / s -- centred DIRECTLY at each mu, deliberately not the device's shifted form: the tests'
    oracle and the probe's baseline.  Integer weights give empirical_covariance of the table with row n repeated w_n times.  Returns
    (S (R, D, D) float64, exactly symmetric, mu (R, D)); a weighting that sums to zero or holds a NaN comes out NaN by the arithmetic."""
    X = np.asarray(X, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    if X.ndim != 2 or W.ndim != 2 or W.shape[1] != X.shape[0]:
        raise ValueError("weighted_covariance_host takes one (N, D) table and (R, N) weights")
    R, D = W.shape[0], X.shape[1]
    S, mean = np.empty((R, D, D)), np.empty((R, D))
    with np.errstate(invalid="ignore", divide="ignore"):
        for r, w in enumerate(W):
            s = w.sum()
            mean[r] = (w[:, None] * X).sum(axis=0) / s
            Z = X - mean[r]
            cov = (Z * w[:, None]).T @ Z / s
            S[r] = np.triu(cov) + np.triu(cov, 1).T  # (the mirror is a copy, as on the device)
    return S, mean


def resample_weights(N: int, n_resamples: int, scheme: str = "subsample", fraction: float = 0.5, rng=None) -> np.ndarray:
    """(n_resamples, N) float64 row weights of `n_resamples` resamples of a table of N rows, integer-valued: "bootstrap" the
    multiplicities of N draws with replacement (every row sums to N); "subsample" 0 / 1 with floor(fraction N) ones, drawn without
    replacement (the subsampling of stability selection and StARS).  Seeded through `rng` (a seed or a Generator)."""
    rng = _rng(rng)
    if N < 1 or n_resamples < 1:
        raise ValueError(f"resample_weights: N = {N} rows, {n_resamples} resamples")
    W = np.zeros((n_resamples, N), dtype=np.float64)
    if scheme == "bootstrap":
        for r in range(n_resamples):
            W[r] = np.bincount(rng.integers(0, N, size=N), minlength=N)
    elif scheme == "subsample":
        m = int(np.floor(fraction * N))
        if not 1 <= m <= N:
            raise ValueError(f"resample_weights: fraction {fraction} keeps {m} of {N} rows")
        for r in range(n_resamples):
            W[r, rng.choice(N, size=m, replace=False)] = 1.0
    else:
        raise ValueError(f"resample_weights: scheme {scheme!r} is neither 'bootstrap' nor 'subsample'")
    return W


# --------------------------------------------------------------------------- bench inputs
def synthetic_covariance_batch(
    num_tasks: int,
    num_nodes: int,
    num_samples: Optional[int] = None,
    seed: int = 1234,
    sparsity: Sequence[float] = (0.1, 0.2),
    eig_offset: float = 1.0,
    task_offset: int = 0,
) -> np.ndarray:
    """The benchmark/parity input of SURVEY.md section 8(d): per task draw a Gaussian graph,
    sample it, min-max normalise the columns (what ``fit`` always does, ref main.py:85) and take
    the repaired empirical covariance.  Task ``i`` uses ``default_rng(seed + task_offset + i)``
    so a sharded rank generates exactly its slice of the global batch.  Returns fp32 (K, D, D)."""
    if num_samples is None:
        num_samples = 1024 if num_nodes >= 256 else 500
    out = np.empty((num_tasks, num_nodes, num_nodes), dtype=np.float32)
    for i in range(num_tasks):
        rng = np.random.default_rng(seed + task_offset + i)
        Xb, _ = get_data(num_nodes, sparsity, num_samples, 1, eig_offset=eig_offset, rng=rng)
        X = Xb[0]
        X = (X - X.min(0)) / (X.max(0) - X.min(0))
        out[i] = get_covariance([X], offset=0.1)[0].astype(np.float32)
    return out
