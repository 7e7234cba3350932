"""The case table of test_buffer_contract.py and scripts/buffer_contract_probe.py: every workspace-taking entry point through HipLib -- whole
passes through forward_uGLAD + loss.backward(), so that glad.py's and main.py's state tensors are guarded too -- at the smallest shapes
that reach a distinct route or layout of make_route / eig_layout / ns_layout (csrc/host_route.h) and at the tile edges of the wide
utilities (the shapes of test_launch_routes_wide.py).  Inputs are seeded; trained parameters from golden/params_trained.npz;
covariances S = X^T X / N + 0.1 I.  A case resets every process-wide switch it sets in a `finally`.

cases(dev) -> the GPU table; cases(dev, emulated=True) -> the smallest shape of every entry point (D <= 40, K <= 2; the cell with L = 1)."""
import os
import zlib

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Case:
    def __init__(self, entry, shape, make_inputs, call, switches="", exempt=None, device="cuda"):
        self.entry, self.shape, self.switches = entry, shape, switches
        self.id = "-".join(s for s in (entry, shape, switches.replace(" ", "_").replace("=", "")) if s)
        self.device = device
        self._make, self._call = make_inputs, call
        self.exempt = exempt or {}

    def inputs(self):
        return self._make(np.random.default_rng(zlib.crc32(f"{self.entry} {self.shape}".encode())), self.device)

    def call(self, inputs):
        return self._call(inputs)


def _lib():
    from uglad_amd import _lib

    return _lib.get_lib()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cov(rng, M, D):
    """S = X^T X / N + 0.1 I with N = 2 D rows: well conditioned."""
    X = rng.standard_normal((M, 2 * D, D))
    return (X.transpose(0, 2, 1) @ X / (2 * D) + 0.1 * np.eye(D)).astype(np.float32)


def _spd64(rng, K, D):
    out = np.empty((K, D, D))
    for k in range(K):
        Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
        P = (Q * np.linspace(0.5, 4.0, D)) @ Q.T
        out[k] = 0.5 * (P + P.T)
    return out


def _trained_model(dev):
    import uglad_amd

    pz = np.load(os.path.join(GOLDEN, "params_trained.npz"))
    model = uglad_amd.GladParams(1.0, device=dev)
    model.load_state_dict({k: torch.from_numpy(np.array(pz[k])) for k in pz.files})
    return model


class _switches:
    """wide mode, matrix-iteration mode and environment switches for the duration of one call."""

    def __init__(self, wide=None, ns=None, env=None):
        self.wide, self.ns, self.env = wide, ns, env or {}

    def __enter__(self):
        lib = _lib()
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        if self.wide is not None:
            lib.set_wide_mode(self.wide)
        if self.ns is not None:
            lib.set_matrix_iteration(self.ns)

    def __exit__(self, *exc):
        lib = _lib()
        lib.set_wide_mode(-1)
        lib.set_matrix_iteration(-1)
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def _tag(wide, ns, env, extra=""):
    parts = ([] if wide is None else [f"wide={wide}"]) + ([] if ns is None else [f"ns={ns}"]) + [f"{k}={v}" for k, v in (env or {}).items()]
    return " ".join(parts + ([extra] if extra else []))


# ---------------------------------------------------------------------------------------------------------------- the cell
def cell(M, D, L=2, init_diag=0, wide=None, ns=None, env=None, s_grad=False, forward_only=False, indefinite=None, struct=False, one_s=False,
         beta_unused=False, device="cuda"):
    """forward_uGLAD + loss.backward(): uglad_glad_forward, uglad_loss_fwd, uglad_loss_bwd*, uglad_glad_backward* (and Theta_0 inside)."""
    extra = " ".join(w for w, on in (("S.grad", s_grad), ("forward-only", forward_only), ("indefinite", indefinite is not None), ("struct", struct),
                                     ("s_batch=1", one_s)) if on)

    def make(rng, dev):
        S = _cov(rng, M, D)
        if indefinite is not None:
            S[indefinite] -= 3.0 * np.eye(D, dtype=np.float32)  # S + t I (t ~ 1) is not positive definite: the Cholesky kernel flags it
        inp = {"S": _t(S, dev)}
        if struct:
            A = (rng.random((M, D, D)) < 0.3).astype(np.float32)
            inp["struct"] = _t(np.maximum(A, A.transpose(0, 2, 1)), dev)
        if one_s:
            inp["S_loss"] = _t(_cov(rng, 1, D), dev)
            if struct:
                inp["struct"] = inp["struct"][:1].contiguous()
        model = _trained_model(dev)
        inp.update({"param." + k: p.detach() for k, p in model.named_parameters()})
        inp["_model"] = model
        return inp

    def call(inp):
        import uglad_amd

        model = inp["_model"]
        for p in model.parameters():
            p.grad = None
        S = inp["S"].detach().requires_grad_() if s_grad else inp["S"]
        out = {}
        with _switches(wide, ns, env):
            if forward_only:
                with torch.no_grad():
                    theta, loss = uglad_amd.forward_uGLAD(S, model, L=L, INIT_DIAG=init_diag)
            else:
                theta, loss = uglad_amd.forward_uGLAD(S, model, L=L, INIT_DIAG=init_diag, loss_Sb=inp.get("S_loss"), struct_theta=inp.get("struct"))
                loss.backward()
                out.update({"grad." + k: p.grad for k, p in model.named_parameters()})
                if s_grad:
                    out["S.grad"] = S.grad
        out.update(theta=theta.detach(), loss=loss.detach())
        return out

    return Case("cell", f"M{M}_D{D}_L{L}_diag{init_diag}", make, call, _tag(wide, ns, env, extra),
                exempt={"beta": "matrix_iteration.beta"} if beta_unused else None, device=device)


def cell_grouped(M, D, groups, L=2, device="cuda"):
    """uglad_glad_forward_grouped / uglad_glad_backward_grouped as the batched CV folds drive them (main.py, _cv_folds_batched)."""

    def make(rng, dev):
        model = _trained_model(dev)
        P = model.packed().detach()
        P = torch.stack([P * (1.0 + 0.01 * g) for g in range(groups)]).contiguous()
        return {"S": _t(_cov(rng, M, D), dev), "P": P}

    def call(inp):
        from uglad_amd.glad.glad import glad_grouped
        from uglad_amd.main import loss_uGLAD

        P = inp["P"].detach().requires_grad_()
        theta = glad_grouped(inp["S"], P, L=L, INIT_DIAG=0)
        loss = loss_uGLAD(theta, inp["S"], batch_divisor=1)
        loss.backward()
        return {"theta": theta.detach(), "loss": loss.detach(), "P.grad": P.grad}

    return Case("cell_grouped", f"M{M}_D{D}_G{groups}_L{L}", make, call, device=device)


# ---------------------------------------------------------------------------------------------------------------- the spectral path, D <= 256
def symeig(M, D, device="cuda"):
    def make(rng, dev):
        A = rng.standard_normal((M, D, D)).astype(np.float32)
        return {"A": _t(A + A.transpose(0, 2, 1), dev)}

    def call(inp):
        A = inp["A"]
        U, beta = torch.empty_like(A), torch.empty(M, D, dtype=torch.float32, device=A.device)
        _lib().symeig(A, U, beta)
        return {"U": U, "beta": beta}

    return Case("symeig", f"M{M}_D{D}", make, call, device=device)


def tridiagonalize(M, D, device="cuda"):
    def make(rng, dev):
        S, Z = _cov(rng, M, D), _cov(rng, M, D)
        return {"A0": _t(S, dev), "A1": _t(Z, dev), "lam": torch.tensor([0.7], dtype=torch.float32, device=dev)}

    def call(inp):
        lib = _lib()
        R = torch.empty_like(inp["A0"])
        wsp = lib.workspace(M, D, R)
        lib.tridiagonalize(inp["A0"], inp["A1"], inp["lam"], R, wsp)
        DP = 32 * ((D + 31) // 32)
        return {"R": R, "d_e_tau": wsp[:M * 3 * DP].clone()}  # (the header: "workspace receives d, e, tau")

    return Case("tridiagonalize", f"M{M}_D{D}", make, call, device=device)


def covariance(K, N, D, device="cuda"):
    def make(rng, dev):
        return {"X": _t((rng.standard_normal((K, N, D)) * rng.uniform(0.5, 5.0, D) + rng.uniform(-2, 2, D)).astype(np.float32), dev)}

    def call(inp):
        S, mn = _lib().covariance(inp["X"], normalize=True, eval_offset=0.1, repair=True, return_min_eig=True)
        return {"S": S, "min_eig": mn}

    return Case("covariance", f"K{K}_N{N}_D{D}", make, call, "repair", device=device)


def conditional_mean(K, D, device="cuda"):
    def make(rng, dev):
        return {"P": _t(_spd64(rng, K, D).astype(np.float32), dev), "mean": _t(rng.uniform(0.2, 0.8, (K, D)).astype(np.float32), dev),
                "observed": _t((rng.random((K, D)) < 0.5).astype(np.float32), dev), "values": _t(rng.uniform(-0.5, 1.5, (K, D)).astype(np.float32), dev)}

    def call(inp):
        fm, cov, lp = _lib().conditional_mean(inp["P"], inp["mean"], inp["observed"], inp["values"])
        return {"full_mean": fm, "cond_cov": cov, "log_pdf": lp}

    return Case("conditional_mean", f"K{K}_D{D}", make, call, device=device)


def _scored(rng, K, D, nan=False):
    """(K, D, D) float32, symmetric, positive diagonal: magnitudes from 12 values (ties), a third exact zeros of either sign."""
    vals = np.concatenate([[0.0, -0.0], np.linspace(0.05, 0.9, 10)]).astype(np.float32)
    out = np.empty((K, D, D), dtype=np.float32)
    for k in range(K):
        U = np.triu(rng.choice(vals, size=(D, D)) * rng.choice(np.float32([1, -1]), size=(D, D)), 1)
        U[rng.random((D, D)) < 1 / 3] = 0.0
        if nan and D >= 70:
            U[3, 17] = np.nan
        out[k] = U + U.T + np.diag(rng.uniform(1.0, 2.0, D).astype(np.float32))
    return out


def support_metrics(K, D, wide=False, device="cuda"):
    def make(rng, dev):
        return {"true": _t(_scored(rng, K, D), dev), "pred": _t(_scored(rng, K, D, nan=wide), dev)}

    def call(inp):
        lib = _lib()
        return {"out": (lib.support_metrics_wide if wide else lib.support_metrics)(inp["true"], inp["pred"], beta=1)}

    return Case("support_metrics_wide" if wide else "support_metrics", f"K{K}_D{D}", make, call, device=device)


def partial_correlations(K, D, device="cuda"):
    def make(rng, dev):
        return {"P": _t(_spd64(rng, K, D).astype(np.float32), dev)}

    return Case("partial_correlations", f"K{K}_D{D}", make, lambda inp: {"rho": _lib().partial_correlations(inp["P"])}, device=device)


# ---------------------------------------------------------------------------------------------------------------- the wide utilities
def covariance_wide(K, N, D, repair, device="cuda"):
    def make(rng, dev):
        return {"X": _t(rng.standard_normal((K, N, D)) * rng.uniform(0.5, 5.0, D) + rng.uniform(-2, 2, D), dev)}

    def call(inp):
        if repair:
            S, mn, _ = _lib().covariance_wide(inp["X"], normalize=True, eval_offset=0.1, repair=True, return_min_eig=True)
            return {"S": S, "min_eig": mn}
        return {"S": _lib().covariance_wide(inp["X"], normalize=True, repair=False)}

    return Case("covariance_wide", f"K{K}_N{N}_D{D}", make, call, "repair" if repair else "plain", device=device)


def association(K, D, W, N, want_f64, repair, device="cuda"):
    from uglad_amd.utils import prepare_data as pd_

    # every third feature real; the categorical ones with 2 .. 12 levels (D = 12) or 2 .. 5 (D = 40): W = 64 and 128 expanded columns
    cards = np.where(np.arange(D) % 3 == 2, 0, 2 + (np.arange(D) * 5) % (11 if D <= 12 else 4)).astype(np.int32)
    maps = pd_._expanded_layout([f"f{i}" for i in range(D)], np.where(cards > 0, "c", "r"), cards)
    assert int(maps.W) == W, (D, int(maps.W), W)

    def make(rng, dev):
        table = np.empty((K, N, D))
        for k in range(K):
            lat = rng.standard_normal((N, 4))
            for i in range(D):
                v = lat @ rng.standard_normal(4) * rng.uniform(0.2, 1.0) + rng.standard_normal(N)
                table[k, :, i] = np.digitize(v, np.quantile(v, np.linspace(0, 1, cards[i] + 1)[1:-1])) if cards[i] else \
                    v * rng.uniform(0.5, 20.0) + rng.uniform(-5, 5)
        return {"table": _t(table, dev)}

    def call(inp):
        A, mn, A64 = _lib().association(inp["table"], maps, eval_offset=0.1, repair=repair, want_f64=want_f64)
        return {"A": A, "min_eig": mn, "A64": A64}

    return Case("association", f"K{K}_D{D}_W{W}", make, call, _tag(None, None, None, " ".join(w for w, on in (("f64", want_f64), ("repair", repair)) if on) or "plain"),
                device=device)


def rank_correlation(method, K, N, D, full, special="", device="cuda"):
    def make(rng, dev):
        X = rng.standard_normal((K, N, D)) + 0.5 * rng.standard_normal((K, N, 1))
        X = np.round(X, 1)  # ties
        if special == "constant":
            X[:, :, D // 2] = 1.25
        if special == "nan":
            X[0, N // 3, D // 3] = np.nan
        return {"X": _t(X, dev)}

    def call(inp):
        r = _lib().rank_correlation(inp["X"], method, transform=True, eval_offset=0.1, repair=full, want_f64=full, want_gram=full)
        return {"A": r.A, "min_eig": r.min_eig, "A64": r.A64, "gram": r.gram, "info": r.info}

    return Case("rank_correlation", f"{method}_K{K}_N{N}_D{D}", make, call, " ".join(s for s in ("all" if full else "plain", special) if s), device=device)


def conditional_mean_wide(K, D, want_cov, not_pd=False, device="cuda"):
    def make(rng, dev):
        P = _spd64(rng, K, D)
        if not_pd:
            P[K - 1] = -P[K - 1]
        return {"P": _t(P, dev), "mean": _t(rng.uniform(0.2, 0.8, (K, D)), dev), "observed": _t((rng.random((K, D)) < 0.5).astype(np.float32), dev),
                "values": _t(rng.uniform(-0.5, 1.5, (K, D)), dev)}

    def call(inp):
        fm, cov, lp = _lib().conditional_mean_wide(inp["P"], inp["mean"], inp["observed"], inp["values"], clip01=False, want_cov=want_cov)
        return {"full_mean": fm, "cond_cov": cov, "log_pdf": lp}

    return Case("conditional_mean_wide", f"K{K}_D{D}", make, call, " ".join(s for s, on in (("cov", want_cov), ("not-pd", not_pd)) if on) or "plain", device=device)


def sample_scores(K, N, D, x_batch, want_density, device="cuda"):
    def make(rng, dev):
        P = _spd64(rng, K, D) + 1e-5 * rng.standard_normal((K, D, D))
        return {"X": _t(rng.standard_normal((x_batch, N, D)) * 2.0, dev), "P": _t(P, dev), "mean": _t(rng.standard_normal((K, D)), dev)}

    def call(inp):
        q, dens, logdet = _lib().sample_scores(inp["X"], inp["P"], inp["mean"], want_density=want_density)
        return {"mahalanobis": q, "log_density": dens, "logdet": logdet}

    return Case("sample_scores", f"K{K}_N{N}_D{D}", make, call, f"x_batch={x_batch}" + (" density" if want_density else ""), device=device)


def graph_wide(K, D, want_stats, keep, device="cuda"):
    E = D * (D - 1) // 2
    n_keep = {"0": 0, "E/10": E // 10, "E": E}[keep]

    def make(rng, dev):
        return {"V": _t(_scored(rng, K, D, nan=True), dev)}

    def call(inp):
        return _lib().graph_wide(inp["V"], n_keep=n_keep, from_precision=True, want_stats=want_stats)._asdict()

    return Case("graph_wide", f"K{K}_D{D}", make, call, f"n_keep={keep.replace('/', 'over')}" + (" stats" if want_stats else ""),
                exempt={"edge_ij": "graph_wide.edges", "edge_w": "graph_wide.edges"}, device=device)


def eigvalsh_wide(K, D, nan=False, device="cuda"):
    def make(rng, dev):
        G = rng.standard_normal((K, D, D))
        A = 0.5 * (G + G.transpose(0, 2, 1)) + 1e-5 * rng.standard_normal((K, D, D))
        if nan:
            A[1, min(5, D - 1), D // 2] = np.nan
        return {"A": _t(A, dev)}

    def call(inp):
        eig, summary = _lib().eigvalsh_wide(inp["A"], th=0.25)
        return {"eig": eig, "summary": summary}

    return Case("eigvalsh_wide", f"K{K}_D{D}", make, call, "nan" if nan else "", device=device)


def table_spectrum(K, N, D, want_cov, device="cuda"):
    def make(rng, dev):
        return {"X": _t(rng.standard_normal((K, N, D)) * rng.uniform(0.5, 5.0, D) + rng.uniform(-2, 2, D), dev)}

    def call(inp):
        eig, summary, cov = _lib().table_spectrum(inp["X"], th=1.0, want_cov=want_cov)
        return {"eig": eig, "summary": summary, "cov": cov}

    return Case("table_spectrum", f"K{K}_N{N}_D{D}", make, call, "cov" if want_cov else "", device=device)


def correlated_features(K, D, device="cuda"):
    def make(rng, dev):
        G = rng.standard_normal((K, D, D))
        return {"S": _t(0.5 * (G + G.transpose(0, 2, 1)), dev)}

    def call(inp):
        order, counts, n_listed = _lib().correlated_features(inp["S"])
        return {"order": order, "counts": counts, "n_listed": n_listed}

    return Case("correlated_features", f"K{K}_D{D}", make, call, device=device)


# (K, N, D) of the Kendall case whose row pairs are dealt over more than one chunk (uglad_rank_correlation_pair_chunks > 1: few tiles, many rows)
KENDALL_CHUNKED = (1, 300, 12)


def cases(dev="cuda", emulated=False):
    d = dict(device=dev)
    if emulated:
        return [
            cell(3, 7, L=1, **d), cell(3, 33, L=1, **d), cell(3, 33, L=1, s_grad=True, **d), cell_grouped(6, 20, 3, L=1, **d),
            cell(2, 20, L=1, ns=1, beta_unused=True, **d),
            symeig(2, 31, **d), tridiagonalize(2, 33, **d), covariance(2, 30, 40, **d), conditional_mean(2, 25, **d), support_metrics(2, 20, **d),
            partial_correlations(2, 37, **d),
            covariance_wide(2, 20, 40, True, **d), association(2, 12, 64, 40, True, True, **d), rank_correlation("spearman", 2, 30, 20, True, **d),
            rank_correlation("kendall", 1, 30, 20, True, **d), rank_correlation("scores", 1, 30, 20, False, **d),
            conditional_mean_wide(2, 40, True, **d), sample_scores(2, 1, 1, 2, True, **d), sample_scores(2, 20, 30, 1, True, **d),
            support_metrics(2, 2, wide=True, **d), graph_wide(2, 2, True, "E", **d), graph_wide(1, 30, True, "E/10", **d), eigvalsh_wide(2, 40, **d),
            table_spectrum(2, 80, 40, True, **d), correlated_features(2, 40, **d),
        ]
    out = []
    # -- the cell, one workgroup per matrix: one case per tridiagonalisation and LDS class, both initialisations
    for M, D in ((3, 7), (3, 32), (3, 33), (2, 96), (2, 100), (2, 128)):
        out += [cell(M, D, init_diag=0, **d), cell(M, D, init_diag=1, **d)]
    out.append(cell(3, 32, env={"UGLAD_TRIDIAG_WAVE": "0"}, **d))
    out.append(cell(3, 40, indefinite=1, **d))
    out.append(cell_grouped(6, 20, 3, **d))
    # (one matrix of D = 129 goes to the matrix iteration by itself; with both modes off it stays with one workgroup, its slabs in the workspace)
    out += [cell(3, 33, s_grad=True, **d), cell(1, 129, s_grad=True, beta_unused=True, **d), cell(1, 129, s_grad=True, wide=0, ns=0, **d)]
    out += [cell(2, 20, struct=True, **d), cell(2, 20, struct=True, one_s=True, **d)]
    # -- 128 < D <= 256 on the spectral path
    out += [cell(2, 129, wide=0, ns=0, **d), cell(1, 200, wide=0, ns=0, **d)]
    out += [cell(2, 129, wide=1, ns=0, **d), cell(1, 200, wide=1, ns=0, **d), cell(1, 256, wide=1, ns=0, **d)]
    out.append(cell(257, 129, L=1, ns=0, forward_only=True, **d))
    # -- the matrix iteration
    out += [cell(2, 20, ns=1, beta_unused=True, **d), cell(1, 70, ns=1, beta_unused=True, **d), cell(1, 129, ns=1, beta_unused=True, **d)]
    out.append(cell(1, 200, beta_unused=True, **d))
    out += [cell(1, 258, beta_unused=True, **d), cell(1, 450, beta_unused=True, **d)]
    out.append(cell(11, 258, forward_only=True, **d))
    out.append(cell(1, 1030, beta_unused=True, **d))
    out.append(cell(1, 1930, L=1, beta_unused=True, **d))
    # -- single entry points of the spectral path
    out += [symeig(3, 31, **d), symeig(2, 129, **d), tridiagonalize(2, 33, **d), covariance(2, 30, 40, **d), covariance(1, 100, 129, **d),
            conditional_mean(2, 25, **d), conditional_mean(1, 129, **d), support_metrics(3, 20, **d), partial_correlations(2, 37, **d)]
    # -- the wide utilities
    for K, D in ((2, 40), (1, 65), (3, 129)):
        out += [covariance_wide(K, D // 2, D, True, **d), covariance_wide(K, 2 * D, D, True, **d), covariance_wide(K, 2 * D, D, False, **d)]
    for K, D, W, N in ((2, 12, 64, 97), (1, 40, 128, 150)):
        out += [association(K, D, W, N, f64, rep, **d) for f64 in (True, False) for rep in (True, False)]
    for method in ("spearman", "kendall", "scores"):
        for K, N, D in ((2, 71, 70), (1, 41, 140)):
            out += [rank_correlation(method, K, N, D, True, **d), rank_correlation(method, K, N, D, False, **d)]
    out.append(rank_correlation("kendall", *KENDALL_CHUNKED, True, **d))
    out += [rank_correlation("spearman", 2, 71, 70, True, "constant", **d), rank_correlation("kendall", 2, 71, 70, True, "nan", **d)]
    for K, D in ((2, 40), (1, 129)):
        out += [conditional_mean_wide(K, D, True, **d), conditional_mean_wide(K, D, False, **d)]
    out.append(conditional_mean_wide(2, 40, True, not_pd=True, **d))
    for K, N, D in ((2, 1, 1), (2, 100, 70), (1, 257, 129)):
        for xb in sorted({1, K}):
            out += [sample_scores(K, N, D, xb, True, **d), sample_scores(K, N, D, xb, False, **d)]
    out += [support_metrics(K, D, wide=True, **d) for K, D in ((2, 2), (1, 70), (1, 129))]
    for K, D in ((2, 2), (1, 70), (1, 129)):
        out += [graph_wide(K, D, stats, keep, **d) for stats in (True, False) for keep in ("0", "E/10", "E")]
    out += [eigvalsh_wide(1, 1, **d), eigvalsh_wide(2, 40, **d), eigvalsh_wide(1, 65, **d), eigvalsh_wide(3, 129, **d), eigvalsh_wide(3, 40, nan=True, **d)]
    for K, D in ((1, 1), (2, 40), (1, 65), (3, 129)):
        out += [table_spectrum(K, 2 * D, D, True, **d), table_spectrum(K, 2 * D, D, False, **d)]
    out += [correlated_features(1, 2, **d), correlated_features(2, 40, **d), correlated_features(1, 129, **d)]
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out
