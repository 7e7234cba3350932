"""The Python surface pinned to the parent's bits: the cases of tests/test_surface_parent_bits.py and of
tests/golden/make_surface_parent_goldens.py.  A helper module like wide_cases.py: no conftest, no pytest setting.

`run(case)` -> {output name: numpy array}.  It reaches the package through public names only (`uglad_amd.X`, `uglad_amd.glad.glad.glad_grouped`,
`uglad_amd._lib.device() / get_lib()`), so that the same file records the golden on the commit before the surface was consolidated
and checks every commit after it.  Every case seeds torch (the draw of the 42 parameters) and takes its data from a numpy generator
seeded by its own name; nothing is printed.  Shapes are the smallest that reach every line of glad/glad.py, main.py, inputs.py and
after.py: D = 3 and 33 (one and two tiles), a grouped pass of two groups, a table of 48 x 6, and for everything after the path D = 6
and D = max_eig_dim + 4 -- the first size of the wide entry points.
"""
import os
import tempfile
import zlib

import numpy as np
import torch

FULL_UP_TO = 4096  # the golden keeps an output of up to this many elements itself, a CRC32 of it beyond

PASSES = [("glad", dict(M=2, D=3, L=3)), ("glad", dict(M=3, D=33, L=3)), ("grouped", dict(G=2, M=4, D=33, L=3))]
HOWS = ("nograd", "train", "train_S")
DRIVERS = ("direct", "direct_truth", "cv", "cv_batched", "cv_parallel", "missing", "multitask", "mixed", "copula", "device_cov")
AFTER = ("small", "wide")


def cases():
    out = [f"pass/{kind}_{'_'.join(f'{k}{v}' for k, v in shape.items())}/{how}/mon{mon}"
           for kind, shape in PASSES for how in HOWS for mon in (0, 1)]
    return out + [f"driver/{d}" for d in DRIVERS] + [f"after/{a}" for a in AFTER]


def _rng(case):
    return np.random.default_rng(zlib.crc32(case.encode()))


def _seed(case):
    torch.manual_seed(zlib.crc32(case.encode()) % (2 ** 31))


def _device():
    from uglad_amd import _lib

    return _lib.device()


def _covariances(rng, M, D):
    X = rng.standard_normal((M, 4 * D + 5, D)) @ (np.eye(D) + 0.3 * rng.standard_normal((D, D)) / np.sqrt(D))
    X = (X - X.min(axis=1, keepdims=True)) / (X.max(axis=1, keepdims=True) - X.min(axis=1, keepdims=True))
    return np.stack([np.cov(x, rowvar=False, bias=True) for x in X]).astype(np.float32)


def _table(rng, N, D):
    """N rows of D correlated columns on different scales: nothing for process_table to drop."""
    mix = np.eye(D) + 0.4 * np.triu(rng.standard_normal((D, D)), 1)
    return (rng.standard_normal((N, D)) @ mix) * np.linspace(1.0, 3.0, D) + np.arange(D)


def _sparse_precision(rng, K, D):
    P = np.zeros((K, D, D))
    for k in range(K):
        A = np.triu(rng.standard_normal((D, D)) * (rng.random((D, D)) < min(0.4, 3.0 / D)), 1)
        P[k] = A + A.T + np.eye(D) * (np.abs(A + A.T).sum(axis=1).max() + 1.0)
    return P


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _dict_values(d):
    return np.array([np.nan if d[k] is None else float(d[k]) for k in sorted(d)], dtype=np.float64)


def _graph(prefix, g):
    out = {f"{prefix}.edges": g.edges, f"{prefix}.weights": g.weights, f"{prefix}.threshold": np.asarray(g.threshold),
           f"{prefix}.degree": np.asarray(g.degree)}
    if g.triangles is not None:
        out[f"{prefix}.triangles"] = np.asarray(g.triangles)
        out[f"{prefix}.stats"] = _dict_values(g.stats)
    return out


# ---------------------------------------------------------------------------------------------------------------- passes
def _models(G):
    import uglad_amd

    return [uglad_amd.init_uGLAD(lr=0.002)[0] for _ in range(G)]


def _pass_inputs(case, shape):
    _seed(case.rsplit("/", 2)[0])  # (the same parameters and matrices for the three ways and with or without a monitor)
    rng = _rng(case.rsplit("/", 2)[0])
    models = _models(shape.get("G", 1))
    S = torch.from_numpy(_covariances(rng, shape["M"], shape["D"])).to(_device())
    W = torch.from_numpy(rng.standard_normal((shape["M"], shape["D"], shape["D"])).astype(np.float32)).to(_device())
    return models, S, W


def _one_pass(kind, models, S, W, L, how):
    import uglad_amd
    from uglad_amd.glad.glad import glad_grouped

    out = {}
    S = S.clone().requires_grad_(how == "train_S")
    with torch.no_grad() if how == "nograd" else torch.enable_grad():
        if kind == "glad":
            theta, lam = uglad_amd.glad(S, models[0], L=L, return_lambdas=True)
            assert tuple(lam.shape) == (L + 1,) and not lam.requires_grad
            out["lam"] = _np(lam)
            params = list(models[0].parameters())
        else:
            params = [torch.stack([m.packed().detach() for m in models]).requires_grad_(True)]
            theta = glad_grouped(S, params[0], L=L)
        out["theta"] = _np(theta)
        if how != "nograd":
            for p in params:
                p.grad = None
            (theta * W).sum().backward()
            out["grad"] = np.concatenate([_np(p.grad).reshape(-1) for p in params])
            assert out["grad"].shape == (42 * len(models),)
            if how == "train_S":
                out["S.grad"] = _np(S.grad)
    return out


def _run_pass(case):
    import uglad_amd

    _, name, how, mon = case.split("/")
    kind, shape = next((k, s) for k, s in PASSES if name == f"{k}_{'_'.join(f'{a}{b}' for a, b in s.items())}")
    models, S, W = _pass_inputs(case, shape)
    if mon == "mon1":
        with uglad_amd.regime_monitor() as monitor:
            out = _one_pass(kind, models, S, W, shape["L"], how)
        out["cond_max"] = np.float64(monitor.result())
    else:
        out = _one_pass(kind, models, S, W, shape["L"], how)
    return out


def grouped_of_one_equals_glad():
    """glad_grouped with G = 1 against glad on the same inputs, the three ways: [(what, glad's array, glad_grouped's array)]."""
    case = "pass/glad_M3_D33_L3/x/x"
    pairs = []
    for how in HOWS:
        models, S, W = _pass_inputs(case, dict(M=3, D=33, L=3))
        a = _one_pass("glad", models, S, W, 3, how)
        b = _one_pass("grouped", models, S, W, 3, how)
        pairs += [(f"{how}:{key}", a[key], b[key]) for key in b]
    return pairs


# ---------------------------------------------------------------------------------------------------------------- drivers
FIT = dict(epochs=12, L=4, verbose=False)


def _fitted(prefix, est, compare=None):
    out = {f"{prefix}precision_": est.precision_, f"{prefix}params": _np(est.model_glad.packed()),
           f"{prefix}covariance_": np.asarray(est.covariance_), f"{prefix}location_": est.location_,
           f"{prefix}cond_max_": np.float64(est.cond_max_)}
    if isinstance(compare, dict):
        out[f"{prefix}metrics"] = _dict_values(compare)
    return out


def _run_driver(case):
    import pandas as pd

    import uglad_amd

    what = case.split("/")[1]
    _seed(case)
    rng = _rng(case)
    X = _table(rng, 48, 6)
    if what in ("direct", "direct_truth", "device_cov"):
        truth = _sparse_precision(rng, 1, 6)[0] if what == "direct_truth" else None
        est = uglad_amd.uGLAD_GL(device_covariance=what == "device_cov")
        compare = est.fit(X, true_theta=truth, mode="direct", **FIT)
        out = _fitted("", est, compare)
        if what == "direct":  # the estimator's own view of everything after the path
            new = _table(rng, 9, 6)
            out.update({"predict_X": est.predict(X=new), "predict_S": est.predict(S=est.covariance_),
                        "predict_cond_max_": np.float64(est.predict_cond_max_), "mahalanobis": est.mahalanobis(new),
                        "score_samples": est.score_samples(new), "score": np.float64(est.score(new)),
                        "data_min_": est.data_min_, "data_range_": est.data_range_})
            out.update(_graph("graph", est.recovered_graph(sparsity=0.5)))
        return out
    if what.startswith("cv"):
        est = uglad_amd.uGLAD_GL()
        est.fit(X, mode="cv", k_fold=3, batched_folds=what == "cv_batched", parallel_folds=what == "cv_parallel", **FIT)
        return _fitted("", est)
    if what == "missing":
        X[rng.integers(0, 48, 7), rng.integers(0, 6, 7)] = np.nan
        est = uglad_amd.uGLAD_GL()
        compare = est.fit(X, true_theta=_sparse_precision(rng, 1, 6)[0], mode="missing", k_fold=3, **FIT)
        return _fitted("", est, compare)
    if what == "multitask":
        tables = [_table(rng, n, 6) for n in (48, 40, 31)]
        est = uglad_amd.uGLAD_multitask()
        compare = est.fit(tables, true_theta_b=_sparse_precision(rng, 3, 6), **FIT)
        out = _fitted("", est)
        out["metrics"] = np.stack([_dict_values(c) for c in compare])
        new = [_table(rng, n, 6) for n in (5, 5, 8)]
        out.update({"predict_X": est.predict(Xb=new), "mahalanobis_one": est.mahalanobis(new[0]), "score": est.score(new[0]),
                    "score_samples_ragged": np.concatenate(est.score_samples(new))})
        for k, g in enumerate(est.recovered_graph(sparsity=0.5)):
            out.update(_graph(f"graph{k}", g))
        return out
    if what == "mixed":
        frame = pd.DataFrame(X, columns=[f"c{i}" for i in range(6)])
        frame["c1"] = rng.integers(0, 3, 48).astype(str)
        frame["c4"] = np.where(X[:, 4] > np.median(X[:, 4]), "hi", "lo")
        kinds = {c: "c" if c in ("c1", "c4") else "r" for c in frame.columns}
        est = uglad_amd.uGLAD_GL()
        est.fit_mixed(frame, kinds, **FIT)
        out = _fitted("", est)
        out["association_min_eig_"] = np.float64(est.association_min_eig_)
        A, mn = uglad_amd.mixed_association(frame, kinds)
        out.update({"mixed_association": _np(A), "mixed_association.min_eig": np.float64(mn)})
        return out
    if what == "copula":
        est = uglad_amd.uGLAD_GL()
        est.fit_copula(np.exp(X / 3.0), method="kendall", **FIT)
        out = _fitted("", est)
        out["copula_min_eig_"] = np.float64(est.copula_min_eig_)
        A, mn = uglad_amd.rank_correlation(np.exp(X / 3.0), method="kendall")
        out.update({"rank_correlation": _np(A), "rank_correlation.min_eig": np.float64(mn)})
        return out
    raise ValueError(case)


# ---------------------------------------------------------------------------------------------------------------- after the path
class _Fitted:
    """What compute_map_estimate reads of an estimator."""

    def __init__(self, precision, location):
        self.precision_, self.location_ = precision, location
        self.node_names_ = [f"n{i}" for i in range(len(location))]


def _run_after(case):
    import uglad_amd
    from uglad_amd import _lib

    K = 2
    D = 6 if case.endswith("small") else _lib.get_lib().max_eig_dim + 4
    _seed(case)
    rng = _rng(case)
    dev = _device()
    tables = [_table(rng, 40, D) for _ in range(K)]
    est = uglad_amd.uGLAD_multitask()
    est.fit(tables, epochs=2, L=2, verbose=False)
    out = _fitted("fit.", est)
    new = [_table(rng, 11, D) for _ in range(K)]
    out.update({"predict_X": est.predict(Xb=new), "predict_S": est.predict(S=est.covariance_ + 0.1 * np.eye(D)),
                "predict_cond_max_": np.float64(est.predict_cond_max_), "mahalanobis": est.mahalanobis(new),
                "score_samples": est.score_samples(new[0]), "score": est.score(new)})
    for k, g in enumerate(est.recovered_graph(sparsity=0.05)):
        out.update(_graph(f"graph{k}", g))
    # the free functions, on well-conditioned models of their own (a fit of two epochs is far from a usable precision matrix)
    P = _sparse_precision(rng, K, D)
    mu = rng.random((K, D))
    truth = _sparse_precision(rng, K, D)
    P32 = torch.from_numpy(P.astype(np.float32)).to(dev)
    out["metrics_numpy"] = np.stack([_dict_values(m) for m in uglad_amd.device_report_metrics(truth, P)])
    out["metrics_device"] = np.stack([_dict_values(m) for m in uglad_amd.device_report_metrics(torch.from_numpy(truth).to(dev), P32)])
    out["partial_correlations_host"] = uglad_amd.get_partial_correlations(P)
    out["partial_correlations_device"] = _np(uglad_amd.get_partial_correlations(P32))
    out.update(_graph("threshold_graph", uglad_amd.recovered_graph(P32[0], threshold=0.05, stats=False)))
    mask = rng.random((K, D)) < 0.4
    mask[:, 0], mask[:, 1] = True, False
    vals = rng.random((K, D))
    full, cov, logp = uglad_amd.conditional_gaussian_batch(P, mu, mask, vals)
    out.update({"conditional.full": _np(full), "conditional.cov": _np(cov), "conditional.logp": _np(logp)})
    full, cov, logp = uglad_amd.conditional_gaussian_batch(P32, torch.from_numpy(mu).to(dev), torch.from_numpy(mask).to(dev),
                                                           torch.from_numpy(vals).to(dev), clip01=True, want_cov=False)
    out.update({"conditional_device.full": _np(full), "conditional_device.logp": _np(logp)})
    obs = np.nonzero(mask[0])[0]
    full, cov, pdf = uglad_amd.conditional_gaussian_with_probabilities(P[0], mu[0], obs, vals[0][obs])
    out.update({"with_probabilities.full": full, "with_probabilities.cov": cov, "with_probabilities.pdf": np.float64(pdf)})
    out["map_estimate"] = uglad_amd.compute_map_estimate({f"n{i}": float(vals[0][i]) for i in obs}, _Fitted(P[0], mu[0]))
    rows = rng.random((13, D))
    rows.flags.writeable = False
    scores = uglad_amd.sample_scores(P, mu, rows, row_chunk=5)
    out.update({"sample_scores.mahalanobis": scores.mahalanobis, "sample_scores.log_density": scores.log_density,
                "sample_scores.logdet": scores.logdet})
    with tempfile.TemporaryDirectory() as tmp:
        uglad_amd.save_uGLAD_model(est, os.path.join(tmp, "model"))
        back = uglad_amd.load_uGLAD_model(os.path.join(tmp, "model"))
    assert type(back) is type(est) and sorted(back.__dict__) == sorted(est.__dict__)
    out["reloaded.predict_X"] = back.predict(Xb=new)
    return out


def run(case):
    """{output: numpy array} of one case."""
    kind = case.split("/")[0]
    out = {"pass": _run_pass, "driver": _run_driver, "after": _run_after}[kind](case)
    return {f"{case}:{name}": np.asarray(a) for name, a in out.items()}


# ---------------------------------------------------------------------------------------------------------------- comparing
def canonical(a):
    """`a` contiguous with every NaN replaced by the one quiet NaN: its bytes compare bits where finite and NaN-ness elsewhere."""
    a = np.array(a, order="C")
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return a


def crc(a):
    a = canonical(a)
    return np.uint32(zlib.crc32(f"{a.dtype}{a.shape}".encode() + a.tobytes()))


def stored(a):
    """What the golden keeps of an output: the array itself up to FULL_UP_TO elements, its CRC32 beyond."""
    a = canonical(a)
    return a if a.size <= FULL_UP_TO else crc(a)


def same_bits(a, kept):
    """`a` against what `stored` kept of the parent's: equal shape, type and bits where finite, NaN in the same places."""
    a, kept = stored(a), np.asarray(kept)
    return a.shape == kept.shape and a.dtype == kept.dtype and a.tobytes() == kept.tobytes()
