"""How a table becomes the matrix the path runs on: the covariance (host fp64 like the reference's prepare_data.get_covariance, or under
`device_covariance` the device front-ends uglad_covariance / uglad_covariance_wide), the association matrix of a mixed table
(uglad_association), the rank correlations of the nonparanormal model (uglad_rank_correlation), the pairwise-complete covariance of a
table with missing entries (uglad_pairwise_covariance) and the covariances of one table under many weightings of its rows -- its
resamples -- (uglad_weighted_covariance).  `uglad_amd.main` re-exports the public names."""
from __future__ import annotations

import contextlib
import warnings

import numpy as np
import torch

from . import _lib
from .utils import prepare_data


_NUMPY_DTYPE = {torch.float32: np.float32, torch.float64: np.float64}


def _to_dev(a, dtype=torch.float32) -> torch.Tensor:
    """`a` (array or tensor) as a contiguous, detached tensor of `dtype` on the library's device.  A device tensor is converted on the
    device; a host array is converted on the host and uploaded once (a read-only one is copied first: torch.from_numpy wants to write)."""
    if torch.is_tensor(a):
        return a.detach().to(device=_lib.device(), dtype=dtype).contiguous()
    a = np.ascontiguousarray(a, dtype=_NUMPY_DTYPE[dtype])
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(_lib.device())


_DEVICE_COVARIANCE = False  # set for the duration of a fit()/predict() by uGLAD_GL / uGLAD_multitask(device_covariance=True)


@contextlib.contextmanager
def device_covariance(enabled: bool = True):
    """Within this context the drivers form the covariances (and the reference's eigenvalue repair) on the GPU
    (`uglad_covariance`, beyond the eigensolver's size `uglad_covariance_wide`) instead of in fp64 numpy on the host
    (prepare_data.py:328-356)."""
    global _DEVICE_COVARIANCE
    saved, _DEVICE_COVARIANCE = _DEVICE_COVARIANCE, bool(enabled)
    try:
        yield
    finally:
        _DEVICE_COVARIANCE = saved


REPAIR_THRESHOLD = 1e-6  # prepare_data.py:347: "min eig <= 1e-6 -> S += (offset - min eig) I"
REPAIR_BAND = 1e-4       # fp32 eigenvalues within this (relative to ||S||_2-ish scale) of the threshold are re-decided in fp64


def _device_covariance_group(X: np.ndarray, eval_offset: float) -> torch.Tensor:
    """(K, N, D) equally-shaped tables -> (K, D, D) repaired covariances on the device.

    The reference decides its repair from fp64 eigenvalues (prepare_data.py:343-352); the device sees fp32 eigenvalues of an
    fp32 covariance, whose absolute error is ~1e-7 ||S||.  Where the device's smallest eigenvalue lies within REPAIR_BAND of
    the threshold the decision could flip -- an O(offset) discontinuity -- so exactly those matrices (rare: nearly singular
    with a minimum eigenvalue of ~1e-6) are re-decided from an fp64 eigvalsh on the host and corrected in place.
    Tables wider than the eigensolver's size go to the fp64 front-end, which needs no such band."""
    lib = _lib.get_lib()
    if X.shape[-1] > lib.max_eig_dim:
        # beyond the eigensolver's size: the fp64 front-end (csrc/cov_wide.h) takes the reference's decision itself, in fp64
        return lib.covariance_wide(_to_dev(X, torch.float64), normalize=False, eval_offset=eval_offset, repair=True)
    S, mn = lib.covariance(_to_dev(X), normalize=False, eval_offset=eval_offset, repair=True, return_min_eig=True)
    mn = mn.cpu().numpy().astype(np.float64)
    scale = np.maximum(1.0, S.diagonal(dim1=1, dim2=2).abs().sum(1).cpu().numpy())  # trace >= ||S||_2 for a PSD matrix
    for k in np.nonzero(np.abs(mn - REPAIR_THRESHOLD) <= REPAIR_BAND * scale)[0]:
        applied = mn[k] <= REPAIR_THRESHOLD
        Sk = S[k].double().cpu().numpy()
        if applied:
            Sk = Sk - (eval_offset - mn[k]) * np.eye(Sk.shape[0])  # undo the device's shift, decide again
        mn64 = float(np.linalg.eigvalsh(0.5 * (Sk + Sk.T)).min())
        if mn64 <= REPAIR_THRESHOLD:
            Sk = Sk + (eval_offset - mn64) * np.eye(Sk.shape[0])
        S[k] = torch.from_numpy(Sk.astype(np.float32)).to(S.device)
    return S


def _covariance(Xb, eval_offset):
    """Tables (K,N,D) -> (K,D,D) fp32 covariances on the device, repaired as prepare_data.get_covariance does.
    Under device_covariance the tables are grouped by shape (missing mode's row-subsampled folds and multitask tables may
    differ in length) and every group of equal shape is one launch of the device front-end."""
    if _DEVICE_COVARIANCE:
        tables = [np.asarray(x) for x in Xb]
        max_dim = _lib.get_lib().max_dim  # (what the cell covers; wider tables take the host path below, and fail at the cell)
        if tables and all(t.ndim == 2 and t.shape[1] <= max_dim and t.dtype != object for t in tables):
            groups = {}
            for i, t in enumerate(tables):
                groups.setdefault(t.shape, []).append(i)
            D = tables[0].shape[1]
            if all(shape[1] == D for shape in groups):
                out = torch.empty(len(tables), D, D, dtype=torch.float32, device=_lib.device())
                for idx in groups.values():
                    out[idx] = _device_covariance_group(np.stack([tables[i] for i in idx]), eval_offset)
                return out
    return _to_dev(prepare_data.get_covariance(Xb, offset=eval_offset))


def mixed_association(df, dtype, repair: bool = True, eval_offset: float = 0.1):
    """The association matrix of a table that mixes categorical ('c') and real ('r') columns, on the device (uglad_association,
    csrc/assoc_wide.h; the reference's pairwise_cov_matrix, prepare_data.py:253-285): `dtype` maps column name -> 'c' | 'r'.  Returns
    (A, min_eig): A the (D, D) fp32 matrix on the device, with `repair` shifted like a covariance (min eig <= 1e-6: A += (eval_offset -
    min eig) I, prepare_data.py:347-352), and min_eig the smallest eigenvalue before the repair as a float (+inf where none was needed;
    None without `repair`)."""
    table, maps = prepare_data.encode_mixed_table(df, dtype)
    A, mn, _ = _lib.get_lib().association(torch.from_numpy(table[None]).to(_lib.device()), maps, eval_offset=eval_offset, repair=repair)
    return A[0], (None if mn is None else float(mn[0]))


def _stacked_tables(X, what: str):
    """(tables (K, N, D) float64 contiguous, single, names): an (N, D) array or DataFrame, or a list / (K, N, D) array of tables."""
    names = [str(c) for c in X.columns] if hasattr(X, "columns") else None
    single = hasattr(X, "columns") or (not isinstance(X, (list, tuple)) and np.ndim(X) == 2)
    tables = np.array(X, dtype=np.float64, order="C")  # (a copy of its own: the caller's array may be read-only)
    tables = tables[None] if single else tables
    if tables.ndim != 3:
        raise ValueError(f"{what} takes an (N, D) table, or a list / (K, N, D) array of tables of one shape")
    return tables, single, names


def _rank_tables(X):
    """_stacked_tables for the rank correlations, which have no meaning for a NaN."""
    tables, single, names = _stacked_tables(X, "rank_correlation")
    if np.isnan(tables).any():
        raise ValueError("rank_correlation: the table holds NaN; impute or drop those rows first")
    return tables, single, names


def rank_correlation(X, method: str = "kendall", transform: bool = True, repair: bool = True, eval_offset: float = 0.1):
    """The rank-based correlation matrix of the nonparanormal (Gaussian copula) model, on the device (uglad_rank_correlation,
    csrc/rank_wide.h; additive, what R's huge.npn offers): `method` "spearman" (with `transform` 2 sin(pi rho / 6)), "kendall" (tau-b,
    sin(pi tau / 2): the SKEPTIC estimator) or "scores" (the correlation of Phi^-1(rank / (N + 1))).  X is an (N, D) array or DataFrame,
    or a list / (K, N, D) array of tables of one shape.  Returns (A, min_eig) like mixed_association: A the (D, D) -- or (K, D, D) -- fp32
    matrix on the device, with `repair` shifted like a covariance (min eig <= 1e-6: A += (eval_offset - min eig) I), and min_eig the
    smallest eigenvalue before the repair as a float -- or a (K,) float64 array -- (+inf where none was needed; None without `repair`).
    A constant column gives NaN in its row and column; a NaN raises ValueError."""
    tables, single, _ = _rank_tables(X)
    out = _lib.get_lib().rank_correlation(torch.from_numpy(tables).to(_lib.device()), method, transform=transform,
                                          eval_offset=eval_offset, repair=repair)
    mn = None if out.min_eig is None else out.min_eig.cpu().numpy()
    if single:
        return out.A[0], (None if mn is None else float(mn[0]))
    return out.A, mn


def pairwise_flag_message(info, names=None) -> str:
    """What the flag words of one table (uglad_pairwise_covariance's info_out, (D,) int32) say, column by column; "" when none is set."""
    info = np.asarray(info)
    names = names if names is not None else [f"node_{i}" for i in range(len(info))]
    parts = [f"{[names[i] for i in np.nonzero(info & bit)[0]]}: {why}" for bit, why in _lib.PAIRWISE_FLAGS.items() if (info & bit).any()]
    return "; ".join(parts)


def pairwise_covariance(X, normalize: bool = False, repair: bool = True, eval_offset: float = 0.1, min_pairs: int = 2):
    """The available-case (pairwise-complete) covariance of a table with missing entries (NaN), on the device (uglad_pairwise_covariance,
    csrc/pairwise_wide.h; additive -- the reference imputes column means, which shrinks every covariance --, what pandas' DataFrame.cov
    and R's cov(use = "pairwise.complete.obs") offer, divided by n_ij like the reference's covariance by N): entry (i, j) over the rows
    where columns i and j are both observed; with `normalize` of the columns min-max normalised over their observed entries.  X is an
    (N, D) array or DataFrame, or a list / (K, N, D) array of tables of one shape.  Returns (S, min_eig, counts): S the (D, D) -- or
    (K, D, D) -- fp32 matrix on the device, with `repair` shifted like a covariance (min eig <= 1e-6: S += (eval_offset - min eig) I; the
    matrix is in general indefinite); min_eig the smallest eigenvalue before the repair as a float -- or a (K,) float64 array -- (+inf
    where none was needed; None without `repair`); counts the int32 device tensor of the n_ij.  An entry with n_ij < min_pairs is NaN, as
    are the row and column of a column that is never observed, constant under `normalize`, or holds an infinity; such a table is not
    repaired and its min_eig is NaN; a RuntimeWarning names its columns and says why (HipLib.pairwise_covariance returns the flag words)."""
    tables, single, names = _stacked_tables(X, "pairwise_covariance")
    out = _lib.get_lib().pairwise_covariance(torch.from_numpy(tables).to(_lib.device()), normalize=normalize, min_pairs=min_pairs,
                                             eval_offset=eval_offset, repair=repair, want_counts=True)
    for k, info in enumerate(out.info.cpu().numpy()):
        if info.any():
            warnings.warn(f"pairwise_covariance: table {k} holds NaN and is not repaired: {pairwise_flag_message(info, names)}",
                          RuntimeWarning, stacklevel=2)
    mn = None if out.min_eig is None else out.min_eig.cpu().numpy()
    if single:
        return out.S[0], (None if mn is None else float(mn[0])), out.counts[0]
    return out.S, mn, out.counts


def weight_flag_message(flag: int) -> str:
    """What one weighting's flag word (uglad_weighted_covariance's info_out) says; "" when none is set."""
    return "; ".join(why for bit, why in _lib.WEIGHT_FLAGS.items() if int(flag) & bit)


def weighted_covariance(X, W, repair: bool = True, eval_offset: float = 0.1):
    """The covariances of ONE table under R weightings of its rows, on the device (uglad_weighted_covariance, csrc/wcov_wide.h; additive:
    what resampling needs -- prepare_data.resample_weights draws bootstrap multiplicities and 0 / 1 subsamples): per weighting
    sum_n w_n (x_n - mu)(x_n - mu)^T / sum_n w_n about its own weighted mean mu, the table uploaded and staged once for all of them.  X
    is an (N, D) array or DataFrame, taken as it is (normalise it first where the model wants that); W is (R, N).  Returns (S, min_eig,
    mean): S the (R, D, D) fp32 matrices on the device, with `repair` each shifted like a covariance (min eig <= 1e-6: S += (eval_offset -
    min eig) I); min_eig the (R,) float64 array of the smallest eigenvalues before the repair (+inf where none was needed; None without
    `repair`); mean the (R, D) float64 device tensor of the weighted means.  A NaN or an infinity in X raises ValueError.  A weighting
    with a negative, NaN or infinite weight, or whose weights sum to zero, is NaN throughout and not repaired; a RuntimeWarning names it."""
    tables, single, _ = _stacked_tables(X, "weighted_covariance")
    if not single:
        raise ValueError("weighted_covariance takes one (N, D) table")
    table = tables[0]
    if not np.isfinite(table).all():
        raise ValueError("weighted_covariance: the table holds NaN or infinity; impute or drop those rows first")
    W = np.ascontiguousarray(W, dtype=np.float64)
    if W.ndim != 2 or W.shape[1] != table.shape[0]:
        raise ValueError(f"weighted_covariance: weights of shape {W.shape} for a table of {table.shape[0]} rows; (R, N) expected")
    out = _lib.get_lib().weighted_covariance(torch.from_numpy(table).to(_lib.device()), _to_dev(W, torch.float64), eval_offset=eval_offset,
                                             repair=repair, want_mean=True)
    for r, flag in enumerate(out.info.cpu().numpy()):
        if flag:
            warnings.warn(f"weighted_covariance: weighting {r} holds NaN and is not repaired: {weight_flag_message(flag)}",
                          RuntimeWarning, stacklevel=2)
    return out.S, (None if out.min_eig is None else out.min_eig.cpu().numpy()), out.mean
