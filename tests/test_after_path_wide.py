"""The conditional Gaussian / MAP estimate for every D the cell covers (uglad_conditional_mean_wide, csrc/after_wide.h): fp64 throughout,
a blocked Cholesky factorisation of the masked precision matrix instead of the eigensolver.  CPU: the unmodified kernel sources on the SIMT
emulator (small D: the entry point takes every 1 <= D <= max_dim) against oracle.after_path.conditional_gaussian.  GPU: the widemap_*
goldens made by the real reference (tests/golden/make_widemap_goldens.py), the oracle at larger sizes, main's routing and a graph capture.

Tolerances, derived from the arithmetic (c = cond(L_uu), computed here by numpy; the inputs keep c <= 100):
  full_mean (max-abs over max |mean|)   <= D c 2^-53        a Cholesky solve with one step of refinement, fp64
  log_pdf (absolute)                    <= D^2 c 2^-53      a sum of D logarithms of pivots, each at the pivot's relative accuracy
  cond_cov (relative Frobenius)         <= 2^-23            twice the one fp32 rounding of the store
Through conditional_gaussian_batch, whose return layout is fp32, the mean is held to 2^-23 as well."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import after_path as oap

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
EPS = 2.0 ** -53
TOL32 = 2.0 ** -23


def problems(K, D, seed, frac=1.0 / 3.0):
    """K dense, well conditioned precision matrices (the generator of tests/test_after_path.py), means, ragged masks and values."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((K, D, D))
    P = A @ A.transpose(0, 2, 1) / D + 0.5 * np.eye(D)
    P = 0.5 * (P + P.transpose(0, 2, 1))
    mask = rng.random((K, D)) < (frac * (1.0 + 0.5 * np.arange(K)[:, None] / max(K, 1)))  # another observation count per problem
    return P, rng.random((K, D)), mask, rng.random((K, D))


def run_wide(lib, P, mu, mask, vals, device, **kw):
    f = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)  # noqa: E731
    full, cov, logp = lib.conditional_mean_wide(f(P, np.float64), f(mu, np.float64), f(mask, np.float32), f(vals, np.float64), **kw)
    if device != "cpu":
        torch.cuda.synchronize()
    assert full.dtype == torch.float64 and logp.dtype == torch.float64 and (cov is None or cov.dtype == torch.float32)
    return full.cpu().numpy(), None if cov is None else cov.cpu().numpy(), logp.cpu().numpy()


def oracle(P, mu, mask, vals):
    """(full_mean, cond_cov in the device's layout: identity on the observed coordinates, log_pdf, cond(L_uu))"""
    D = len(mu)
    obs, un = np.nonzero(mask)[0], np.nonzero(~mask)[0]
    if un.size == 0:
        return vals.copy(), np.eye(D), 0.0, 1.0
    full, cc, logp = oap.conditional_gaussian(P, mu, obs, vals[obs])
    cov = np.eye(D)
    cov[np.ix_(un, un)] = cc
    return full, cov, logp, float(np.linalg.cond(P[np.ix_(un, un)]))


def check_against_oracle(got, P, mu, mask, vals, label=""):
    full, cov, logp = got
    K, D = mu.shape
    for k in range(K):
        rf, rc, rl, c = oracle(P[k], mu[k], mask[k], vals[k])
        assert c <= 100.0
        e_mean = np.abs(full[k] - rf).max() / np.abs(rf).max()
        e_logp = abs(logp[k] - rl)
        line = f"{label}[{k}] D {D} observed {int(mask[k].sum())} cond {c:.1f}: mean {e_mean:.2e} (bound {D * c * EPS:.2e}), " \
               f"log pdf {e_logp:.2e} (bound {D * D * c * EPS:.2e})"
        if cov is not None:
            e_cov = np.linalg.norm(cov[k] - rc) / np.linalg.norm(rc)
            line += f", cond_cov {e_cov:.2e} (bound {TOL32:.2e})"
        print(line)
        assert e_mean <= D * c * EPS, (k, e_mean)
        assert e_logp <= D * D * c * EPS, (k, e_logp)
        assert np.array_equal(full[k][mask[k]], vals[k][mask[k]])  # observed values pass through, bit for bit
        if cov is not None:
            assert e_cov <= TOL32, (k, e_cov)
            assert np.array_equal(cov[k], cov[k].T)  # exactly symmetric
            obs = np.nonzero(mask[k])[0]
            assert np.array_equal(cov[k][obs], np.eye(D, dtype=np.float32)[obs])  # observed rows (and columns): exactly the identity


# ============================================================================================ CPU: the kernels on the emulator
def test_emulated_two_block_columns_one_padded_and_the_batch_stride(emul):
    """(K = 2, D = 70): two block columns, the second padded; the first size with an off-diagonal tile of W = L^-1."""
    P, mu, mask, vals = problems(2, 70, seed=51)
    check_against_oracle(run_wide(emul, P, mu, mask, vals, "cpu"), P, mu, mask, vals, "d70")


def test_emulated_three_block_columns(emul):
    """(K = 1, D = 130): W(2, 0) = -L(2,2)^-1 (L(2,0) W(0,0) + L(2,1) W(1,0)) is the first tile with a two-term sum, and X(0, 0) sums
    three block rows."""
    P, mu, mask, vals = problems(1, 130, seed=52)
    check_against_oracle(run_wide(emul, P, mu, mask, vals, "cpu"), P, mu, mask, vals, "d130")


def test_emulated_edges_at_two_block_columns(emul):
    P, mu, mask, vals = problems(3, 70, seed=53)
    mask[0] = False  # nothing observed: cond_cov = P^-1 and the mean is unchanged
    mask[1] = True   # everything observed: the values pass through, cond_cov is exactly the identity, log_pdf = 0
    mu[2] += 0.7     # so that clip01 has something to clamp on either side
    mu[2, ::2] -= 1.4
    full, cov, logp = got = run_wide(emul, P, mu, mask, vals, "cpu")
    check_against_oracle(got, P, mu, mask, vals, "edges")
    assert np.array_equal(full[0], mu[0])
    assert np.linalg.norm(cov[0] - np.linalg.inv(P[0])) / np.linalg.norm(np.linalg.inv(P[0])) <= TOL32
    assert np.array_equal(full[1], vals[1]) and np.array_equal(cov[1], np.eye(70, dtype=np.float32)) and logp[1] == 0.0
    # clip01 clamps the same solution to [0, 1]
    clipped, _, logp_c = run_wide(emul, P, mu, mask, vals, "cpu", clip01=True)
    assert (full[2] < 0).any() and (full[2] > 1).any()
    assert np.array_equal(clipped, np.clip(full, 0.0, 1.0)) and np.array_equal(logp_c, logp)
    # without the covariance: the same bits
    full_n, cov_n, logp_n = run_wide(emul, P, mu, mask, vals, "cpu", want_cov=False)
    assert cov_n is None and np.array_equal(full_n, full) and np.array_equal(logp_n, logp)


@pytest.mark.parametrize("where", ["first", "last"])
def test_emulated_not_positive_definite_next_to_a_healthy_problem(emul, where):
    """A negative pivot in the first and in the last of the three block columns of D = 130, batched with a healthy problem."""
    P, mu, mask, vals = problems(2, 130, seed=54)
    mask[:, [3, 129]] = False
    bad = 3 if where == "first" else 129
    P[0, bad, bad] = -P[0, bad, bad]
    for clip01 in (False, True):
        full, cov, logp = run_wide(emul, P, mu, mask, vals, "cpu", clip01=clip01)
        obs, un = np.nonzero(mask[0])[0], np.nonzero(~mask[0])[0]
        assert np.isnan(logp[0]) and np.isnan(full[0][un]).all() and np.isnan(cov[0][np.ix_(un, un)]).all()
        assert np.array_equal(full[0][obs], np.clip(vals[0][obs], 0.0, 1.0) if clip01 else vals[0][obs])
        assert np.array_equal(cov[0][obs], np.eye(130, dtype=np.float32)[obs]) and np.array_equal(cov[0][:, obs], np.eye(130, dtype=np.float32)[:, obs])
        solo = run_wide(emul, P[1:], mu[1:], mask[1:], vals[1:], "cpu", clip01=clip01)
        assert np.array_equal(full[1], solo[0][0]) and np.array_equal(cov[1], solo[1][0]) and np.array_equal(logp[1], solo[2][0])
        if not clip01:
            check_against_oracle((full[1:], cov[1:], logp[1:]), P[1:], mu[1:], mask[1:], vals[1:], "healthy")


def test_emulated_argument_errors(emul):
    from uglad_amd._lib import UgladError

    z64 = lambda *s: torch.zeros(*s, dtype=torch.float64)  # noqa: E731
    with pytest.raises(UgladError):  # fp32 input belongs to lib.conditional_mean
        emul.conditional_mean_wide(torch.zeros(1, 8, 8), z64(1, 8), torch.zeros(1, 8), z64(1, 8))
    with pytest.raises(UgladError):
        emul.conditional_mean_wide(z64(1, 8, 8), torch.zeros(1, 8), torch.zeros(1, 8), z64(1, 8))
    D = emul.max_dim + 1
    with pytest.raises(UgladError, match="dimension"):
        emul.conditional_mean_wide(torch.empty(1, D, D, dtype=torch.float64), z64(1, D), torch.zeros(1, D), z64(1, D))
    size = emul._dll.uglad_conditional_mean_wide_workspace_floats
    assert size(0, 8) < 0 and size(1, 0) < 0 and size(1, emul.max_dim + 1) < 0 and size(65536, 8) < 0 and size(-1, -1) < 0
    assert size(1, 8) > 0 and size(2, 70) == 2 * size(1, 70)
    P, m, ob, x = z64(1, 8, 8), z64(1, 8), torch.zeros(1, 8), z64(1, 8)
    full, logp = z64(1, 8), z64(1)
    wsp = torch.empty(size(1, 8) + 2, dtype=torch.float32)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    odd = ctypes.c_void_p(wsp.data_ptr() + (4 if wsp.data_ptr() % 8 == 0 else 8))  # 4 mod 8: a float's alignment, not a double's
    assert odd.value % 8 == 4
    for bad_wsp in (None, odd):  # missing / misaligned workspace
        with pytest.raises(UgladError, match="NULL"):
            emul._call("uglad_conditional_mean_wide", vp(P), vp(m), vp(ob), vp(x), vp(full), None, vp(logp), bad_wsp, 1, 8, 0)
    with pytest.raises(UgladError, match="NULL"):  # no full_mean
        emul._call("uglad_conditional_mean_wide", vp(P), vp(m), vp(ob), vp(x), None, None, vp(logp), emul._p(wsp), 1, 8, 0)
    with pytest.raises(UgladError, match="dimension"):
        emul._call("uglad_conditional_mean_wide", vp(P), vp(m), vp(ob), vp(x), vp(full), None, vp(logp), emul._p(wsp), 0, 8, 0)


def test_emulated_routing_needs_no_host(emul, monkeypatch):
    """main's routing on the emulator (the library's eigensolver limit lowered so that D = 70 counts as wide): conditional_gaussian_batch,
    conditional_gaussian_with_probabilities and compute_map_estimate stay on the device, in the layout they return today."""
    from uglad_amd import main

    def no_host(*a, **k):
        raise AssertionError("the host formulation ran for a D the device covers")

    monkeypatch.setattr("uglad_amd.after._conditional_gaussian_host", no_host)
    monkeypatch.setattr(emul, "max_eig_dim", 32)
    P, mu, mask, vals = problems(2, 70, seed=55)
    full, cov, logp = main.conditional_gaussian_batch(P, mu, mask.astype(np.float32), vals)
    assert full.dtype == cov.dtype == logp.dtype == torch.float32 and cov.shape == (2, 70, 70)
    obs = np.nonzero(mask[0])[0]
    rf, rc, rl, c = oracle(P[0], mu[0], mask[0], vals[0])
    assert np.abs(full[0].numpy() - rf).max() / np.abs(rf).max() <= TOL32
    f1, c1, pdf = main.conditional_gaussian_with_probabilities(P[0], mu[0], obs, vals[0][obs])
    un = np.nonzero(~mask[0])[0]
    assert np.abs(f1 - rf).max() / np.abs(rf).max() <= 70 * c * EPS  # fp64 here
    assert c1.shape == (un.size, un.size) and np.array_equal(c1, c1.T) and np.linalg.norm(c1 - rc[np.ix_(un, un)]) <= TOL32 * np.linalg.norm(rc[np.ix_(un, un)])
    assert abs(np.log(pdf) - rl) <= 70 * 70 * c * EPS + 2 * EPS * abs(rl)  # (exp and log of the fp64 log density: one rounding each)

    class Fitted:
        precision_, location_ = P[0].astype(np.float32), mu[0]
        node_names_ = [f"n{i}" for i in range(70)]

    got = main.compute_map_estimate({f"n{i}": float(vals[0][i]) for i in obs}, Fitted)
    ref = oap.map_estimate(Fitted.precision_, mu[0], obs, vals[0][obs])
    assert np.abs(got - ref).max() <= TOL32 and got.min() >= 0.0 and got.max() <= 1.0


# ============================================================================================ goldens
WIDE = ["widemap_d288", "widemap_d320_sparse"]


@functools.lru_cache(maxsize=None)
def load_golden(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    D = len(g["mean"])
    obs = g["observed_idx"]
    nu = D - len(obs)
    P, C = np.zeros((D, D)), np.zeros((nu, nu))
    iu, ju = np.triu_indices(D), np.triu_indices(nu)
    P[iu] = g["precision_triu"]
    P.T[iu] = g["precision_triu"]  # (symmetric to the bit: make_widemap_goldens.py asserts it)
    C[ju] = g["cond_cov_triu"]
    C.T[ju] = g["cond_cov_triu"]   # (the reference's inverse is symmetric to 1e-13 of its norm or better: cond_cov_asym)
    return dict(precision=P, cond_cov=C, mean=g["mean"], observed_idx=obs, observed_values=g["observed_values"], full_mean=g["full_mean"],
                map_clipped=g["map_clipped"], log_pdf=float(g["log_pdf"]), asym=float(g["cond_cov_asym"]))


def test_wide_goldens_hold_what_the_generator_says():
    for name, (D, n_obs) in zip(WIDE, [(288, 96), (320, 40)]):
        g = load_golden(name)
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1 << 20
        assert g["precision"].shape == (D, D) and len(g["observed_idx"]) == n_obs and g["asym"] < 1e-13
        mask = np.zeros(D, dtype=bool)
        mask[g["observed_idx"]] = True
        vals = np.zeros(D)
        vals[g["observed_idx"]] = g["observed_values"]
        rf, rc, rl, c = oracle(g["precision"], g["mean"], mask, vals)  # (the restatement agrees with the real reference here too)
        un = np.nonzero(~mask)[0]
        assert c <= 100.0 and np.abs(rf - g["full_mean"]).max() <= D * c * EPS * np.abs(rf).max()
        assert np.linalg.norm(rc[np.ix_(un, un)] - g["cond_cov"]) <= 1e-12 * np.linalg.norm(g["cond_cov"]) and abs(rl - g["log_pdf"]) <= D * D * c * EPS
        assert np.array_equal(g["map_clipped"], np.clip(g["full_mean"], 0.0, 1.0))
    assert np.count_nonzero(load_golden("widemap_d320_sparse")["precision"]) < 0.1 * 320 * 320


# ============================================================================================ GPU
def _check_golden(name):
    import uglad_amd

    g = load_golden(name)
    D = len(g["mean"])
    obs = g["observed_idx"]
    mask = np.zeros(D, dtype=bool)
    mask[obs] = True
    c = float(np.linalg.cond(g["precision"][np.ix_(~mask, ~mask)]))
    full, cov, pdf = uglad_amd.conditional_gaussian_with_probabilities(g["precision"], g["mean"], obs, g["observed_values"])
    e_mean = np.abs(full - g["full_mean"]).max() / np.abs(g["full_mean"]).max()
    e_cov = np.linalg.norm(cov - g["cond_cov"]) / np.linalg.norm(g["cond_cov"])
    e_logp = abs(np.log(pdf) - g["log_pdf"])
    print(f"{name}: cond {c:.1f}; mean {e_mean:.2e} (bound {D * c * EPS:.2e}), cond_cov {e_cov:.2e} (bound {TOL32:.2e}), "
          f"log pdf {e_logp:.2e} (bound {D * D * c * EPS:.2e})")
    assert c <= 100.0 and e_mean <= D * c * EPS and e_cov <= TOL32 and e_logp <= D * D * c * EPS
    assert cov.shape == g["cond_cov"].shape and np.array_equal(cov, cov.T)
    assert np.array_equal(full[obs], g["observed_values"])  # observed values pass through

    class Fitted:
        precision_, location_ = g["precision"], g["mean"]
        node_names_ = [f"n{i}" for i in range(D)]

    got = uglad_amd.compute_map_estimate({f"n{i}": float(v) for i, v in zip(obs, g["observed_values"])}, Fitted)
    e_map = np.abs(got - g["map_clipped"]).max()
    print(f"{name}: MAP estimate {e_map:.2e} (bound {TOL32:.2e}: the fp32 return layout of conditional_gaussian_batch)")
    assert e_map <= TOL32 * np.abs(g["map_clipped"]).max() and got.min() >= 0.0 and got.max() <= 1.0


@pytest.mark.parametrize("name", WIDE)
def test_emulated_matches_reference_goldens(emul, monkeypatch, name):
    """The goldens through main's routing on the emulator (its build's eigensolver stops at D = 160, so both are wide there too)."""
    from uglad_amd import main

    def no_host(*a, **k):
        raise AssertionError("the host formulation ran for a D the device covers")

    monkeypatch.setattr("uglad_amd.after._conditional_gaussian_host", no_host)
    _check_golden(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", WIDE)
def test_gpu_matches_reference_goldens(name):
    _check_golden(name)


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,seed", [(3, 300, 61), (1, 520, 62)])
def test_gpu_against_the_oracle_with_and_without_the_covariance(K, D, seed):
    """D = 300 (not a multiple of 4), three problems with ragged observation counts; D = 520: DP = 576, nine block columns."""
    from uglad_amd import _lib

    lib = _lib.get_lib()
    P, mu, mask, vals = problems(K, D, seed)
    assert len({int(m.sum()) for m in mask}) == K
    got = run_wide(lib, P, mu, mask, vals, "cuda")
    check_against_oracle(got, P, mu, mask, vals, f"d{D}")
    full_n, cov_n, logp_n = run_wide(lib, P, mu, mask, vals, "cuda", want_cov=False)
    assert cov_n is None and np.array_equal(full_n, got[0]) and np.array_equal(logp_n, got[2])


@pytest.mark.gpu
def test_gpu_main_routes_beyond_256_to_the_device(monkeypatch):
    import uglad_amd
    from uglad_amd import main

    def no_host(*a, **k):
        raise AssertionError("the host formulation ran for a D the device covers")

    monkeypatch.setattr("uglad_amd.after._conditional_gaussian_host", no_host)
    P, mu, mask, vals = problems(2, 300, seed=63)
    full, cov, logp = uglad_amd.conditional_gaussian_batch(P, mu, mask.astype(np.float32), vals)
    assert full.is_cuda and full.dtype == cov.dtype == logp.dtype == torch.float32 and cov.shape == (2, 300, 300)
    # a device fp32 tensor is converted on the device: the same problem up to the rounding of its input
    P32 = torch.from_numpy(P.astype(np.float32)).cuda()
    full32, _, _ = uglad_amd.conditional_gaussian_batch(P32, mu, mask.astype(np.float32), vals, want_cov=False)
    full, full32 = full.cpu().numpy(), full32.cpu().numpy()
    for k in range(2):
        rf, _, rl, c = oracle(P[k], mu[k], mask[k], vals[k])
        assert np.abs(full[k] - rf).max() / np.abs(rf).max() <= TOL32
        assert abs(float(logp[k]) - rl) <= TOL32 * abs(rl)
        assert np.abs(full32[k] - rf).max() / np.abs(rf).max() <= 300 * c * TOL32  # (the input's own fp32 rounding, amplified by cond)

    class Fitted:
        precision_, location_ = P[0], mu[0]
        node_names_ = [f"n{i}" for i in range(300)]

    obs = np.nonzero(mask[0])[0]
    got = uglad_amd.compute_map_estimate({f"n{i}": float(vals[0][i]) for i in obs}, Fitted)
    assert np.abs(got - oap.map_estimate(P[0], mu[0], obs, vals[0][obs])).max() <= TOL32 and got.min() >= 0.0 and got.max() <= 1.0


@pytest.mark.gpu
def test_gpu_wide_conditional_mean_can_be_captured_into_the_callers_graph():
    """Nothing in the 23 launches at D = 288 allocates, synchronises or reads back: captured on a side stream and replayed on NEW inputs,
    the call gives the bits of the eager call on those inputs."""
    from uglad_amd import _lib

    lib = _lib.get_lib()
    K, D = 2, 288
    first, second = problems(K, D, seed=64), problems(K, D, seed=65)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()  # noqa: E731
    P, mu, ob, x = dev(first[0], np.float64), dev(first[1], np.float64), dev(first[2], np.float32), dev(first[3], np.float64)
    full = torch.empty(K, D, dtype=torch.float64, device="cuda")
    cov = torch.empty(K, D, D, dtype=torch.float32, device="cuda")
    logp = torch.empty(K, dtype=torch.float64, device="cuda")
    wsp = torch.empty(int(lib._dll.uglad_conditional_mean_wide_workspace_floats(K, D)), dtype=torch.float32, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call():
        lib._call("uglad_conditional_mean_wide", vp(P), vp(mu), vp(ob), vp(x), vp(full), vp(cov), vp(logp), lib._p(wsp), K, D, 0)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        call()  # warm-up on the capture stream
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            call()
    for dst, src, dt in zip((P, mu, ob, x), second, (np.float64, np.float64, np.float32, np.float64)):
        dst.copy_(dev(src, dt))
    call()
    torch.cuda.synchronize()
    plain = (full.clone(), cov.clone(), logp.clone())
    assert torch.isfinite(plain[0]).all() and torch.isfinite(plain[2]).all()
    full.zero_(), cov.zero_(), logp.zero_(), wsp.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(full, plain[0]) and torch.equal(cov, plain[1]) and torch.equal(logp, plain[2])
