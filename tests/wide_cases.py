"""The nine many-workgroup fp64 utilities (csrc/host_wide.h) on the smallest shapes at which each piece they share can go wrong -- the shift
bisection, the reductions and the symmetriser of chol_wide.h, the radix sort of sort_wide.h, the centred Gram product of cov_wide.h: shapes, inputs and the comparison shared by the GPU test
(test_wide_parent_bits.py) and the generator of its golden (golden/make_wide_parent_goldens.py).  `lib` is the HipLib under test, `dev` where its
tensors live.  Inputs come from seeded numpy alone, outputs through the HipLib wrappers.

A CASE is (entry, name, parameters); run(lib, dev, case) returns {output: [one array per problem]}:
  "cov"      covariance_wide, normalize on, of K tables of 200 rows.  Table 0 is 30 rows repeated -- rank < D, singular: bisected and repaired --,
             the others 200 independent rows: positive definite, they leave at step 0.  Both exits of the controller in one batch (a batch
             shares N, so the rank-deficient table repeats its rows instead of having fewer).  K = 1: the singular table alone.
             -> S, min_eig, repaired
  "assoc"    association with the repair: "mixed" a c/r table with cardinalities 2 .. 12 (indefinite: bisected on the bracket of the row
             sums), "real" an all-real table of 200 rows (positive definite).  -> A, A64, min_eig
  "after"    conditional_mean_wide, clip01 off and on.  K = 3: an ordinary problem, one with every coordinate observed, one whose unobserved
             block is not positive definite (flagged: NaN).  K = 1: the ordinary one.  -> full_mean, cond_cov, log_pdf, each also as *_clip
  "scores"   sample_scores with one table for every model and with one per model; with K = 2 model 1 is indefinite (NaN densities, finite
             distances).  -> mahalanobis, log_density, logdet, each also as *_shared (x_batch = 1)
  "metrics"  support_metrics_wide on scores with ties, exact zeros (of both signs) and, from D = 70, one NaN.  -> out
  "graph"    graph_wide on the same kind of matrix read as a precision matrix: ranked with n_keep = 0, 1 and E, a given threshold, and ranked
             with the statistics.  -> per run threshold, edge_count, edge_ij, edge_w (the m defined rows), degree, and triangles2, stats
  "eigvals"  eigvalsh_wide with th = 0.25, inside the spectrum of an indefinite matrix that is asymmetric at 1e-5 (the symmetriser of
             chol_wide.h).  D = 1: one element; D = 40: one ragged tile; D = 70: column 64 starts a second panel (eigw_update_kernel runs), and
             matrix 1 holds one NaN -- its slab comes back all NaN, slab 0 untouched; D = 129: two trailing updates, the second ragged.
             -> eig, summary
  "spectrum" table_spectrum with the covariance: N = 30 < D = 70, singular, zeros in the spectrum; N = 200, D = 129.  The centred Gram product of
             cov_wide.h through the eigensolver's sink.  -> eig, summary, cov
  "corr"     correlated_features.  D = 2: n = 1, rank 0.  D = 40: two pairs of duplicated columns whose entries are the largest, so that the
             magnitude at the threshold's rank and those around it tie to the bit.  -> order, counts, n_listed
D = 2: E = 1, one ragged tile of everything; D = 40, 70, 129: one ragged tile of 64, two tiles (E = 2415: two key tiles of 2048, the second
ragged), three."""
import zlib

import numpy as np
import torch

# (entry, name, parameters) -- the first case of an entry is kept in full in the golden, the others as a CRC32 per problem and output
CASES = [
    ("cov", "K2_D40", dict(K=2, D=40)), ("cov", "K2_D70", dict(K=2, D=70)), ("cov", "K1_D129", dict(K=1, D=129)),
    ("assoc", "mixed_D12", dict(D=12, N=97, mixed=True)), ("assoc", "mixed_D40", dict(D=40, N=150, mixed=True)),
    ("assoc", "real_D20", dict(D=20, N=200, mixed=False)),
    ("after", "K3_D70", dict(K=3, D=70)), ("after", "K1_D129", dict(K=1, D=129)),
    ("scores", "K2_N100_D70", dict(K=2, N=100, D=70)), ("scores", "K1_N257_D129", dict(K=1, N=257, D=129)),
    ("metrics", "K2_D2", dict(K=2, D=2)), ("metrics", "K2_D70", dict(K=2, D=70)), ("metrics", "K1_D129", dict(K=1, D=129)),
    ("graph", "K2_D2", dict(K=2, D=2)), ("graph", "K2_D70", dict(K=2, D=70)), ("graph", "K1_D129", dict(K=1, D=129)),
    ("eigvals", "K1_D1", dict(K=1, D=1)), ("eigvals", "K2_D40", dict(K=2, D=40)), ("eigvals", "K2_D70", dict(K=2, D=70)),
    ("eigvals", "K1_D129", dict(K=1, D=129)),
    ("spectrum", "K2_N30_D70", dict(K=2, N=30, D=70)), ("spectrum", "K1_N200_D129", dict(K=1, N=200, D=129)),
    ("corr", "K2_D2", dict(K=2, D=2)), ("corr", "K2_D40", dict(K=2, D=40)), ("corr", "K1_D129", dict(K=1, D=129)),
]
# golden file -> the entries it holds: the second one was recorded later, from the parent of the change that gave its three entry points'
# feeders (the centred Gram product, the symmetriser) one owner each
GOLDENS = {"wide_parent_bits.npz": ("cov", "assoc", "after", "scores", "metrics", "graph"),
           "wide_parent_bits_eigw.npz": ("eigvals", "spectrum", "corr")}
FULL = {entry: next(n for e, n, _ in CASES if e == entry) for entries in GOLDENS.values() for entry in entries}


def case_id(case):
    return f"{case[0]}_{case[1]}"


def kept_in_full(case):
    return FULL[case[0]] == case[1]


def _rng(case):
    return np.random.default_rng(zlib.crc32(case_id(case).encode()))


def _spd(rng, D):
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    P = (Q * np.linspace(0.5, 4.0, D)) @ Q.T
    return 0.5 * (P + P.T)


def _scored(rng, K, D):
    """(K, D, D) float32, symmetric to the bit, positive diagonal: off-diagonal magnitudes from 12 values (ties), a third exact zeros of
    either sign, from D = 70 one NaN pair."""
    vals = np.concatenate([[0.0, -0.0], np.linspace(0.05, 0.9, 10)]).astype(np.float32)
    out = np.empty((K, D, D), dtype=np.float32)
    for k in range(K):
        U = np.triu(rng.choice(vals, size=(D, D)) * rng.choice(np.float32([1, -1]), size=(D, D)), 1)
        U[rng.random((D, D)) < 1 / 3] = 0.0
        if D >= 70:
            U[3, 17] = np.nan
        out[k] = U + U.T + np.diag(rng.uniform(1.0, 2.0, D).astype(np.float32))
    return out


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return None if t is None else t.cpu().numpy().copy()


def _per_problem(a):
    return [a[k] for k in range(a.shape[0])]


def run(lib, dev, case):
    entry, _, p = case
    rng = _rng(case)
    out = {}
    if entry == "cov":
        K, D, N = p["K"], p["D"], 200
        X = rng.standard_normal((K, N, D)) * rng.uniform(0.5, 5.0, D) + rng.uniform(-2, 2, D)
        X[0] = X[0, np.arange(N) % 30]
        S, mn, repaired = lib.covariance_wide(_t(X, dev), normalize=True, eval_offset=0.1, return_min_eig=True)
        out = {"S": _np(S), "min_eig": _np(mn), "repaired": _np(repaired)}
    elif entry == "assoc":
        from uglad_amd.utils import prepare_data as pd_

        D, N = p["D"], p["N"]
        cards = np.where(np.arange(D) % 3 == 2, 0, 2 + (np.arange(D) * 5) % 11).astype(np.int32) if p["mixed"] else np.zeros(D, dtype=np.int32)
        lat = rng.standard_normal((N, 4))
        table = np.empty((1, N, D))
        for i in range(D):
            v = lat @ rng.standard_normal(4) * rng.uniform(0.2, 1.0) + rng.standard_normal(N)
            if cards[i]:  # cut at its own quantiles: every level occurs
                table[0, :, i] = np.digitize(v, np.quantile(v, np.linspace(0, 1, cards[i] + 1)[1:-1]))
            else:
                table[0, :, i] = v * rng.uniform(0.5, 20.0) + rng.uniform(-5, 5)
        maps = pd_._expanded_layout([f"f{i}" for i in range(D)], np.where(cards > 0, "c", "r"), cards)
        A, mn, A64 = lib.association(_t(table, dev), maps, eval_offset=0.1, repair=True, want_f64=True)
        out = {"A": _np(A), "A64": _np(A64), "min_eig": _np(mn)}
    elif entry == "after":
        K, D = p["K"], p["D"]
        P = np.stack([_spd(rng, D) for _ in range(K)])
        mean, values = rng.uniform(0.2, 0.8, (K, D)), rng.uniform(-0.5, 1.5, (K, D))
        observed = (rng.random((K, D)) < 0.5).astype(np.float32)
        if K == 3:
            observed[1] = 1.0
            P[2] = -P[2]
        for clip, tag in ((False, ""), (True, "_clip")):
            fm, cov, lp = lib.conditional_mean_wide(_t(P, dev), _t(mean, dev), _t(observed, dev), _t(values, dev), clip01=clip, want_cov=True)
            out.update({"full_mean" + tag: _np(fm), "cond_cov" + tag: _np(cov), "log_pdf" + tag: _np(lp)})
    elif entry == "scores":
        K, N, D = p["K"], p["N"], p["D"]
        P = np.stack([_spd(rng, D) + 1e-5 * rng.standard_normal((D, D)) for _ in range(K)])  # (asymmetric at 1e-5, as a fitted precision_)
        if K == 2:
            P[1] -= 2.0 * np.eye(D)  # eigenvalues from -1.5: indefinite
        mean, X = rng.standard_normal((K, D)), rng.standard_normal((K, N, D)) * 2.0
        for Xin, tag in ((X, ""), (X[:1], "_shared")):
            q, dens, logdet = lib.sample_scores(_t(Xin, dev), _t(P, dev), _t(mean, dev), want_density=True)
            out.update({"mahalanobis" + tag: _np(q), "log_density" + tag: _np(dens), "logdet" + tag: _np(logdet)})
    elif entry == "metrics":
        K, D = p["K"], p["D"]
        pred, true = _scored(rng, K, D), _scored(rng, K, D)
        out = {"out": _np(lib.support_metrics_wide(_t(true, dev), _t(pred, dev), beta=1))}
    elif entry == "graph":
        K, D = p["K"], p["D"]
        E = D * (D - 1) // 2
        V = _t(_scored(rng, K, D), dev)
        runs = [("keep0", dict(n_keep=0, want_stats=False)), ("keep1", dict(n_keep=1, want_stats=False)), ("keepE", dict(n_keep=E, want_stats=False)),
                ("given", dict(threshold=0.25, want_stats=False)), ("stats", dict(n_keep=[max(1, E // (4 + k)) for k in range(K)], want_stats=True))]
        for tag, kw in runs:
            g = lib.graph_wide(V, from_precision=True, **kw)
            m = _np(g.edge_count)
            out.update({f"{tag}/threshold": _np(g.threshold), f"{tag}/edge_count": m, f"{tag}/degree": _np(g.degree)})
            out[f"{tag}/edge_ij"] = [_np(g.edge_ij[k, :m[k]]) for k in range(K)]
            out[f"{tag}/edge_w"] = [_np(g.edge_w[k, :m[k]]) for k in range(K)]
            if kw["want_stats"]:
                out.update({f"{tag}/triangles2": _np(g.triangles2), f"{tag}/stats": _np(g.stats)})
    elif entry == "eigvals":
        K, D = p["K"], p["D"]
        G = rng.standard_normal((K, D, D))
        A = 0.5 * (G + G.transpose(0, 2, 1)) + 1e-5 * rng.standard_normal((K, D, D))  # (asymmetric at 1e-5; indefinite: 0.25 is interior)
        if D == 70:
            A[1, 5, 33] = np.nan
        eig, summary = lib.eigvalsh_wide(_t(A, dev), th=0.25)
        out = {"eig": _np(eig), "summary": _np(summary)}
    elif entry == "spectrum":
        K, N, D = p["K"], p["N"], p["D"]
        X = rng.standard_normal((K, N, D)) * rng.uniform(0.5, 5.0, D) + rng.uniform(-2, 2, D)
        eig, summary, cov = lib.table_spectrum(_t(X, dev), th=1.0, want_cov=True)
        out = {"eig": _np(eig), "summary": _np(summary), "cov": _np(cov)}
    elif entry == "corr":
        K, D = p["K"], p["D"]
        G = rng.standard_normal((K, D, D))
        S = 0.5 * (G + G.transpose(0, 2, 1))
        if D == 40:
            # columns 5 = 3 and 20 = 11, the four of them ten times the others: every entry of cov2 in one of these columns equals its twin
            # in the duplicate to the bit, and these 150 of the 780 magnitudes are the largest -- the one at rank 78 has an exact tie
            S[:, :, [3, 11]] *= 10.0
            S[:, [3, 11], :] *= 10.0
            for a, b in ((3, 5), (11, 20)):
                S[:, :, b] = S[:, :, a]
                S[:, b, :] = S[:, a, :]
        order, counts, n_listed = lib.correlated_features(_t(S, dev))
        out = {"order": _np(order), "counts": _np(counts), "n_listed": _np(n_listed)}
    if dev != "cpu":
        torch.cuda.synchronize()
    return {name: v if isinstance(v, list) else _per_problem(v) for name, v in out.items()}


def canonical(a):
    """`a` with every NaN replaced by the one quiet NaN, so that bytes (and a CRC32 of them) compare bits where finite and NaN-ness elsewhere."""
    a = np.ascontiguousarray(a).copy()
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return a


def crc(a):
    return np.uint32(zlib.crc32(canonical(a).tobytes()))


def same_bits(a, b):
    """Equal shape, type and bits where finite, NaN in the same places (NaN payloads are not compared)."""
    a, b = canonical(a), canonical(b)  # (a scalar per problem is kept as an array of one)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def nan_counts(outputs):
    """{output: NaNs per problem}: what a case exercised of the flagged paths."""
    return {name: [int(np.isnan(x).sum()) if x.dtype.kind == "f" else 0 for x in per] for name, per in outputs.items()}
