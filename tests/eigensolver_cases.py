"""Classic eigensolver test matrices and the checks a symmetric eigen-decomposition has to pass on them, shared by the emulator and the GPU
tests of tests/test_eigensolver_spectra.py (a helper like eigen_path_checks.py, not a conftest).  numpy only; everything is judged in fp64
against the fp32 input cast up.

Three groups, by the bound their eigenvalues and residual have to meet:
  general     G = 5e-6, the bound test_symeig applies to dense random matrices at every size;
  clustered   C = 5e-6 + 4 * 2^-24 * D.  eig_lean.h does not deflate: poles that coincide are pushed 4 eps max|d| past their neighbour, and in a
              merge of D coinciding poles the pushes add up to 4 * 2^-24 * D ||A|| (2.0e-5 / 3.6e-5 / 6.6e-5 at D = 64 / 128 / 256) -- the term is
              derived from that gap rule and has to be re-derived from the rule, not from what the kernel returns, should the rule change;
  tiny block  G.  Matrices whose tridiagonal form has blocks many orders of magnitude below ||A|| (the constant matrix: d = 1, D - 1, 8e-7,
              -9e-14, 5e-21, ...), where a divide & conquer that judges every merge by the merge's own scale solves a 1e-26 eigenproblem in
              full and leaves the fp32 range.
Orthogonality max |U^T U - I| <= 5e-6 holds for every group."""
from collections import OrderedDict

import numpy as np

G_BOUND = 5e-6
ORTH_BOUND = 5e-6

GENERAL = ["wilkinson", "glued wilkinson", "toeplitz 1-2-1", "identity + rank one", "geometric 1e-6", "weak coupling", "tridiag random", "arrowhead",
           "kms", "near-diagonal 1e-6", "graded"]
CLUSTERED = ["cluster 1e-5", "cluster 1e-7", "two clusters", "repeated pairs"]
TINY_BLOCK = ["ones", "0.37 ones", "ones block + zero block", "two ones blocks", "decaying tridiagonal"]
# the subset the emulator runs at D >= 129, where one matrix costs more than a second: one family per group plus every tiny-block family
REDUCED = ["wilkinson", "cluster 1e-5"] + TINY_BLOCK


def group_of(name):
    return "general" if name in GENERAL else "clustered" if name in CLUSTERED else "tiny block"


def bound_kind(name):
    return "C" if name in CLUSTERED else "G"


def bound(kind, D):
    return G_BOUND + (4.0 * 2.0 ** -24 * D if kind == "C" else 0.0)


def tridiag(d, e):
    return np.diag(np.asarray(d, dtype=np.float64)) + np.diag(np.asarray(e, dtype=np.float64), 1) + np.diag(np.asarray(e, dtype=np.float64), -1)


def families(D, rng=None):
    """name -> fp64 symmetric D x D matrix, in a fixed order.  A family whose construction needs more rows than D has is left out."""
    rng = np.random.default_rng(D) if rng is None else rng
    i = np.arange(D)
    Q, Rq = np.linalg.qr(rng.standard_normal((D, D)))
    Q = Q * np.sign(np.diag(Rq))[None, :]
    R = rng.standard_normal((D, D))
    R = R + R.T
    spectrum = lambda lam: (Q * np.asarray(lam, dtype=np.float64)[None, :]) @ Q.T
    out = OrderedDict()
    # ---- general
    if D >= 2:
        out["wilkinson"] = tridiag(np.abs(i - (D - 1) / 2.0), np.ones(D - 1))
        out["glued wilkinson"] = tridiag(np.abs((i % 21) - 10.0), np.where((i[:-1] + 1) % 21 == 0, 1e-4, 1.0))
        out["toeplitz 1-2-1"] = tridiag(np.full(D, 2.0), np.ones(D - 1))
    v = rng.standard_normal(D)
    out["identity + rank one"] = np.eye(D) + np.outer(v, v)
    out["geometric 1e-6"] = spectrum(10.0 ** np.linspace(0.0, -6.0, D))
    if D >= 2:
        out["weak coupling"] = tridiag(np.linspace(-1.0, 1.0, D), np.where(i[:-1] % 2 == 0, 3e-7, 1e-7))
        out["tridiag random"] = tridiag(rng.standard_normal(D), np.abs(rng.standard_normal(D - 1)) * np.where(i[:-1] % 2 == 0, 1.0, -1.0))
        arrow = np.diag(np.linspace(1.0, 2.0, D))
        arrow[0, 1:] = arrow[1:, 0] = 0.1 * rng.standard_normal(D - 1)
        out["arrowhead"] = arrow
    out["kms"] = 0.5 ** np.abs(i[:, None] - i[None, :])
    out["near-diagonal 1e-6"] = 1e-6 * R + np.diag(np.linspace(-2.0, 2.0, D))
    s = 10.0 ** np.linspace(-3.0, 0.0, D)
    out["graded"] = s[:, None] * (np.eye(D) + 1e-2 * R) * s[None, :]
    # ---- clustered
    if D >= 2:
        out["cluster 1e-5"] = spectrum(1.0 + 1e-5 * i / (D - 1))
        out["cluster 1e-7"] = spectrum(1.0 + 1e-7 * i / (D - 1))
        out["two clusters"] = spectrum(np.where(i < D / 2.0, -1.0, 1.0))
        out["repeated pairs"] = spectrum(np.repeat(np.linspace(-1.0, 1.0, (D + 1) // 2), 2)[:D])
    # ---- tiny blocks
    out["ones"] = np.ones((D, D))
    out["0.37 ones"] = 0.37 * np.ones((D, D))
    k = D // 2 + 1
    if k < D:
        blk = np.zeros((D, D))
        blk[:k, :k] = 1.0
        out["ones block + zero block"] = blk.copy()
        blk[k:, k:] = 1.0
        out["two ones blocks"] = blk
    if D >= 3:
        g = np.maximum(10.0 ** (-6.5 * np.maximum(i - 1, 0)), 1e-26)
        d = g.copy()
        d[0], d[1] = 1.0, D - 1.0
        e = g[1:].copy()
        e[0] = np.sqrt(D - 1.0)
        out["decaying tridiagonal"] = tridiag(d, e)
    for name in out:  # (Q diag Q^T and the graded scaling are symmetric only to rounding)
        out[name] = 0.5 * (out[name] + out[name].T)
        assert out[name].shape == (D, D), name
    assert set(out) <= set(GENERAL + CLUSTERED + TINY_BLOCK)
    return out


def measure(A32, beta, U):
    """(finite, sorted, eigenvalue error / ||A||_2, ||A U - U diag beta||_F / ||A||_F, max |U^T U - I|) in fp64; A32 is the fp32 input."""
    A = np.asarray(A32, dtype=np.float64)
    beta = np.asarray(beta, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    finite = bool(np.isfinite(beta).all() and np.isfinite(U).all())
    if not finite:
        return False, False, np.inf, np.inf, np.inf
    w = np.linalg.eigvalsh(A)
    norm2 = max(np.abs(w).max(), 1e-300)
    eig = np.abs(beta - w).max() / norm2
    res = np.linalg.norm(A @ U - U * beta[None, :]) / max(np.linalg.norm(A), 1e-300)
    orth = np.abs(U.T @ U - np.eye(A.shape[0])).max()
    return True, bool((np.diff(beta) >= 0).all()), float(eig), float(res), float(orth)


def check(A32, beta, U, kind, family="?"):
    """The five checks of this module's header on one decomposition; returns (eigenvalue error, residual, orthogonality)."""
    D = np.asarray(A32).shape[0]
    b = bound(kind, D)
    finite, ordered, eig, res, orth = measure(A32, beta, U)
    assert finite, (D, family, "beta and U finite", "non-finite entries", "all finite")
    assert ordered, (D, family, "beta non-decreasing", float(np.diff(np.asarray(beta, dtype=np.float64)).min()), 0.0)
    assert eig <= b, (D, family, "max |beta - eigvalsh(A)| / ||A||_2", eig, b)
    assert res <= b, (D, family, "||A U - U diag(beta)||_F / ||A||_F", res, b)
    assert orth <= ORTH_BOUND, (D, family, "max |U^T U - I|", orth, ORTH_BOUND)
    return eig, res, orth
