"""CPU suite: the real kernel sources (uglad_amd/csrc) executed on the SIMT emulator (tests/simt_emul) through the same
C ABI and the same host code as on the GPU, checked against the reference-captured goldens and the fp64 oracle.
Sizes are small because every work-item is a fiber; the GPU suite (test_gpu_parity.py) covers the real sizes."""
import os

import numpy as np
import pytest
import torch

import eigen_path_checks
from oracle import glad_exact as ex

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def relF(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def load_model(g, prefix="param."):
    import uglad_amd

    m = uglad_amd.GladParams(1.0)
    m.load_state_dict({k: torch.from_numpy(np.array(g[prefix + k])) for k in ex.PARAM_KEYS})
    return m


@pytest.mark.parametrize("D", [2, 7, 25, 32, 33, 64, (25, "wg")])
def test_symeig(emul, D, monkeypatch):
    import uglad_amd

    if isinstance(D, tuple):  # D <= 32 goes through the one-wave tridiagonalisation (tridiag_wave.h); the workgroup kernel stays covered
        D = D[0]
        monkeypatch.setenv("UGLAD_TRIDIAG_WAVE", "0")
    torch.manual_seed(D)
    A = torch.randn(2, D, D)
    A = (A + A.transpose(1, 2)).contiguous()
    A[1] = torch.diag(torch.arange(D, dtype=torch.float32) % 3)  # degenerate diagonal spectrum
    beta, U = uglad_amd.batch_symeig(A)
    rec = (U * beta[:, None, :]) @ U.transpose(1, 2)
    assert relF(rec[0], A[0]) < 3e-6
    assert relF(rec[1], A[1]) < 1e-6
    assert (U.transpose(1, 2) @ U - torch.eye(D)).abs().max() < 3e-6
    w = np.linalg.eigvalsh(A[0].double().numpy())
    assert np.abs(np.sort(beta[0].numpy()) - w).max() < 3e-6 * np.abs(w).max()


def test_symeig_of_a_merge_whose_model_is_exact(emul):
    """Round 4: a nearly diagonal 3 x 3 matrix.  Its one merge has a third pole of negligible weight, so the starting point's test evaluation sits on
    the last root to rounding; the first step then lands on the end of a bracket a few 1e-5 wide, and the midpoint that replaced it was accepted
    unseen by the small-step rule: lambda_max off by 2.3e-5 (found by test_symeig_every_size_up_to_64 on the GPU)."""
    import uglad_amd

    g = torch.Generator(device="cpu").manual_seed(1003)
    A = torch.randn(3, 3, 3, generator=g)
    A = A + A.transpose(1, 2)
    A = (A[2:3] * 1e-3 + torch.diag(torch.linspace(-2.0, 2.0, 3))).contiguous()
    beta, U = uglad_amd.batch_symeig(A)
    w = np.linalg.eigvalsh(A[0].double().numpy())
    assert np.abs(np.sort(beta[0].numpy()) - w).max() < 1e-6
    assert relF((U * beta[:, None, :]) @ U.transpose(1, 2), A) < 1e-6


def test_one_structural_prior_for_the_whole_batch(emul):
    """loss_uGLAD's structure penalty with ONE prior for M matrices -- the reference's (1 - struct_theta) - eye broadcasts it (main.py:325-334) --
    equals the penalty with the prior repeated M times, value and gradient; (D, D) and (1, D, D) are both accepted."""
    import uglad_amd
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    S = torch.from_numpy(synthetic_covariance_batch(3, 8, seed=4))
    rng = np.random.default_rng(0)
    st = (rng.random((8, 8)) < 0.4).astype(np.float32)
    st = np.maximum(st, st.T)
    out = []
    for prior in (torch.from_numpy(st), torch.from_numpy(st)[None], torch.from_numpy(st)[None].repeat(3, 1, 1)):
        th = torch.linalg.inv(S + torch.eye(8)).contiguous().requires_grad_(True)
        ls = uglad_amd.loss_uGLAD(th, S, struct_theta=prior)
        ls.backward()
        out.append((ls.item(), th.grad.clone()))
    assert out[0][0] == out[2][0] and out[1][0] == out[2][0]
    assert torch.equal(out[0][1], out[2][1]) and torch.equal(out[1][1], out[2][1])
    with pytest.raises(ValueError):
        uglad_amd.loss_uGLAD(th, S, struct_theta=torch.zeros(2, 8, 8))


@pytest.mark.parametrize("D", [1, 2, 3, 33, 128, (129, "one workgroup")])
def test_theta0_and_loss_on_the_eigen_path_for_every_matrix(emul, D, monkeypatch):
    """CPU twin of the GPU test of this name (tests/eigen_path_checks.py) at the sizes this build has, NT = 1, 2, 4, 5: init_inverse_kernel and
    loss_fwd_kernel on csrc/eig_lean.h for every matrix.  (D = 129 on the one-workgroup route only: the route three such matrices take by
    default, L D L^T, does not touch these kernels.)"""
    monkeypatch.setenv("UGLAD_CHOLESKY", "0")
    M = 3
    if isinstance(D, tuple):
        D, M = D[0], 1  # (every work-item is a fiber: one matrix at this size)
        monkeypatch.setenv("UGLAD_WIDE_BWD", "0")
        monkeypatch.setenv("UGLAD_MATRIX_ITERATION", "0")
    eigen_path_checks.every_matrix_on_the_eigen_path(emul, "cpu", D, M=M)


def test_flagged_matrices_in_a_batch_larger_than_the_t_region_of_one_matrix(emul, monkeypatch):
    """CPU twin of the GPU test of this name: D = 7, M = 520 > NT * 512 with matrices 0, 1 and 519 flagged by the Cholesky kernels."""
    monkeypatch.setenv("UGLAD_CHOLESKY", "1")
    eigen_path_checks.flagged_matrices_in_a_large_batch(emul, "cpu")


SMALL_CELLS = ["cell_d16_b3_L6_diag0_fresh", "cell_d16_b3_L6_diag1_fresh", "cell_d16_b3_L6_diag0_trained",
               "cell_d25_b1_L15_fresh", "cell_d25_b1_L15_trained", "cell_d20_b5_L15_trained",
               "cell_missing_d20_k3_L15_fresh", "cell_struct_d16_b1_L6_fresh"]


@pytest.mark.parametrize("name", SMALL_CELLS)
def test_forward_backward_vs_reference_goldens(emul, name):
    import uglad_amd

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    model = load_model(g)
    S = torch.from_numpy(g["S"])
    kw = {}
    if "loss_S" in g:
        kw["loss_Sb"] = torch.from_numpy(g["loss_S"])
    if "struct" in g:
        kw["struct_theta"] = torch.from_numpy(g["struct"])
    theta, loss = uglad_amd.forward_uGLAD(S, model, L=int(g["L"]), INIT_DIAG=int(g["INIT_DIAG"]), **kw)
    loss.backward()
    err = max(relF(theta[i].detach().numpy(), g["theta_L"][i]) for i in range(S.shape[0]))
    assert err < 1e-4, err  # the north-star tolerance; measured ~1e-6
    assert err < 2e-5, err
    assert abs(loss.item() - float(g["loss"])) < 5e-5 * max(1.0, abs(float(g["loss"])))
    sd = dict(model.named_parameters())
    for key in ex.PARAM_KEYS:
        ref, got = g["grad." + key], sd[key].grad.numpy()
        # the gradient contract; the fp64 oracle itself is within 1.1e-5 of the reference on these goldens
        assert relF(got, ref) < 1e-4 or np.abs(got - ref).max() < 1e-6, (key, got, ref)


@pytest.mark.parametrize("name", ["regime_rawcov_d32_eo0.1_trained", "regime_rawcov_d32_eo0.03_trained", "regime_scaled_d32_c4_trained",
                                  "regime_lam_small_d32_fresh"])
def test_regime_goldens_cond_diagnostic_and_warning(emul, name):
    """Outside the comfortable regime (tests/golden/make_goldens_r3.py): the kernels' cond_max diagnostic equals the oracle's number, Theta stays
    within 2e-5 of the fp64 evaluation of the reference's function, and predict(S=...) warns exactly beyond the validated bound."""
    import json
    import warnings

    import uglad_amd
    from uglad_amd.glad import glad as gmod

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    row = {r["case"]: r for r in json.load(open(os.path.join(GOLDEN, "regime_sweep.json")))}[name]
    model = load_model(g)
    L = int(g["L"])
    with gmod.regime_monitor() as mon, torch.no_grad():
        theta = gmod.glad(torch.from_numpy(g["S"]), model, L=L)
    cond = mon.result()
    assert abs(cond - row["cond_max"]) < 2e-2 * row["cond_max"], (cond, row["cond_max"])
    ref64, _ = ex.glad_forward(g["S"], ex.params64(g, "param."), L, 0, mode="ns10")
    assert max(relF(theta[i].numpy(), ref64[i]) for i in range(theta.shape[0])) < 2e-5
    est = uglad_amd.uGLAD_GL()
    est.model_glad, est._fit_cfg = model, dict(L=L, INIT_DIAG=0, eval_offset=0.1, sqrt_mode=None)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        est.predict(S=g["S"])
    warned = [w for w in caught if issubclass(w.category, uglad_amd.UgladRegimeWarning)]
    assert (len(warned) > 0) == (cond > emul.validated_cond)


def test_lambdas_and_intermediates(emul):
    from uglad_amd.glad import glad as gmod

    g = np.load(os.path.join(GOLDEN, "cell_d16_b3_L6_diag0_trained.npz"))
    model = load_model(g)
    with torch.no_grad():
        theta, lam = gmod.glad(torch.from_numpy(g["S"]), model, L=6, return_lambdas=True)
    np.testing.assert_allclose(lam.numpy(), g["lambdas"], rtol=2e-5)
    # exact mode differs from the reference where its Newton-Schulz has not converged, agrees with the fp64 oracle
    with torch.no_grad():
        th_exact = gmod.glad(torch.from_numpy(g["S"]), model, L=6, sqrt_mode="exact")
    ref, _ = ex.glad_forward(g["S"], ex.params64(g, "param."), 6, 0, mode="exact")
    assert max(relF(th_exact[i].numpy(), ref[i]) for i in range(3)) < 2e-5


def test_single_cell_d64_vs_oracle(emul):
    """One cell at D=64 (two 32-wide MFMA tiles per side) forward and backward against the fp64 oracle, both modes."""
    from uglad_amd import _lib

    g = np.load(os.path.join(GOLDEN, "cell_d64_b4_L30_trained.npz"))
    p = ex.params64(g, "param.")
    pk = torch.tensor(np.concatenate([p[k].ravel() for k in ex.PARAM_KEYS]), dtype=torch.float32)
    S = torch.from_numpy(g["S"][:1].copy())
    Z = torch.from_numpy(g["theta_init"][:1].copy())
    lam = torch.tensor([float(g["lambdas"][0])])
    rng = np.random.default_rng(0)
    Gn = rng.standard_normal((1, 64, 64)).astype(np.float32)
    Gn = torch.from_numpy(Gn + Gn.transpose(0, 2, 1))
    for mode in ("ns10", "exact"):
        Zo, half, U = (torch.empty(1, 64, 64) for _ in range(3))
        beta, nf = torch.empty(1, 64), torch.empty(1)
        wsp = emul.workspace(1, 64, S)
        emul.cell_fwd(S, Z, lam, pk, Zo, half, U, beta, nf, wsp, _lib.SQRT_MODES[mode])
        Zr, hr, _, _, nr = ex.cell_fwd(S.double().numpy(), Z.double().numpy(), float(lam), p, mode)
        assert relF(half.numpy(), hr) < 3e-6 and relF(Zo.numpy(), Zr) < 3e-6
        assert abs(nf.item() - nr[0]) < 1e-4 * nr[0]
        Go, grho, glam = torch.empty(1, 64, 64), torch.zeros(1, 28), torch.empty(1)
        emul.cell_bwd(Gn, S, Z, half, U, beta, lam, pk, Go, grho, glam, _lib.SQRT_MODES[mode])
        grads = {k: np.zeros_like(p[k]) for k in ex.PARAM_KEYS}
        Gr, glr = ex.cell_bwd(Gn.double().numpy(), S.double().numpy(), Z.double().numpy(), float(lam), p, grads, mode)
        assert relF(Go.numpy(), Gr) < 2e-5, mode
        assert abs(glam.item() - glr) < 1e-3 * abs(glr), mode  # two cancelling sums under a random (non-gradient) G
        ref_rho = np.concatenate([grads[k].ravel() for k in ex.PARAM_KEYS[1:7]])
        assert relF(grho.numpy()[0], ref_rho) < 1e-4, mode


@pytest.mark.parametrize("wide", [0, 1])
def test_workspace_resident_path_d129_vs_oracle(emul, wide):
    """D = 129: one past the LDS-resident size -- the NT = 5 instantiation with its big matrices in the caller's workspace (odd D,
    padded to 160), as one workgroup per matrix (wide = 0) and as many workgroups per matrix (wide = 1: csrc/wide_bwd.h, the
    3 x 3 grid of 64 x 64 tiles with ragged edges).  Two unrolled steps forward + backward against the fp64 oracle, and the
    solver alone."""
    import uglad_amd

    g = np.load(os.path.join(GOLDEN, "cell_d129_b2_L30_trained.npz"))
    model = load_model(g)
    S = torch.from_numpy(g["S"][:1].copy())
    emul.set_wide_mode(wide)
    emul.set_matrix_iteration(0)  # (left alone, one 129 x 129 matrix goes to the matrix-iteration path: tested further down)
    try:
        theta, loss = uglad_amd.forward_uGLAD(S, model, L=2)
        loss.backward()
    finally:
        emul.set_wide_mode(-1)
        emul.set_matrix_iteration(-1)
    assert torch.equal(theta, theta.transpose(1, 2))
    p = ex.params64(g, "param.")
    ref, tr = ex.glad_forward(g["S"][:1], p, 2, 0, mode="ns10")
    assert relF(theta[0].detach().numpy(), ref[0]) < 1e-5
    grads = ex.glad_backward(g["S"][:1], p, 2, tr, 0, mode="ns10")
    sd = dict(model.named_parameters())
    for key in ex.PARAM_KEYS:
        assert relF(sd[key].grad.numpy(), grads[key]) < 1e-4, key
    if wide:
        return
    torch.manual_seed(150)
    A = torch.randn(1, 150, 150)
    A = (A + A.transpose(1, 2)).contiguous()
    beta, U = uglad_amd.batch_symeig(A)
    assert relF((U * beta[:, None, :]) @ U.transpose(1, 2), A) < 3e-6
    assert (U.transpose(1, 2) @ U - torch.eye(150)).abs().max() < 3e-6


def test_matrix_iteration_path_forced_equals_spectral_path(emul, monkeypatch):
    """csrc/wide_ns.h -- the cell as the reference's own Newton-Schulz / Lyapunov matrix iteration on fp64 tile products, what D beyond
    the eigensolver runs on -- forced at sizes the spectral path serves: same Theta and gradients, the cond diagnostic an upper bound of
    the spectral path's.  Both output tilings of the products: 32 x 32 (few matrices; 4 x 4 ragged tiles at D = 100) and 64 x 64 (2 x 2)."""
    import uglad_amd
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    for D, B, L, tile in ((12, 3, 4, "32"), (100, 1, 1, "32"), (100, 1, 1, "64")):
        monkeypatch.setenv("UGLAD_NS_TILE", tile)
        S = torch.from_numpy(synthetic_covariance_batch(B, D, seed=5))
        W = torch.from_numpy(np.random.default_rng(3).standard_normal((B, D, D)).astype(np.float32))
        out = []
        for forced in (0, 1):  # 0: the spectral path wherever it exists
            emul.set_matrix_iteration(forced)
            try:
                torch.manual_seed(1)
                model = uglad_amd.GladParams(1.0)
                with uglad_amd.regime_monitor() as mon:
                    th = uglad_amd.glad(S, model, L=L)
                (th * W).sum().backward()
            finally:
                emul.set_matrix_iteration(-1)
            out.append((th.detach(), torch.cat([p.grad.reshape(-1) for p in model.parameters()]), mon.result()))
        (t0, g0, c0), (t1, g1, c1) = out
        assert relF(t1.numpy(), t0.numpy()) < 2e-6
        assert ((g1 - g0).abs().max() / g0.abs().max()).item() < 1e-5
        assert torch.equal(t1, t1.transpose(1, 2))
        assert c0 * 0.999 <= c1 < 16 * c0, (c0, c1)


@pytest.mark.parametrize("ldl_launches", ["0", "1"])
def test_beyond_the_eigensolver_vs_oracle(emul, monkeypatch, ldl_launches):
    """(UGLAD_LDL_LAUNCHES: the factorisation as one workgroup per matrix / as the sequence of launches of round 4, ns_ldl_phase_kernel.)
    D = 161, one past this build's eigensolver (UGLAD_MAX_NT = 5; 256 in the product build): Theta_0 and the loss through the padded
    L D L^T + Newton steps, one step of the matrix iteration forward and backward, the shift's gradient through the tile inner product --
    against the fp64 oracle."""
    import uglad_amd
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    assert emul.max_eig_dim == 160 and emul.max_dim == 2048
    monkeypatch.setenv("UGLAD_LDL_LAUNCHES", ldl_launches)
    D, L = 161, 1
    g = np.load(os.path.join(GOLDEN, "cell_d129_b2_L30_trained.npz"))
    model = load_model(g)
    Snp = synthetic_covariance_batch(1, D, seed=7)
    theta, loss = uglad_amd.forward_uGLAD(torch.from_numpy(Snp), model, L=L)
    loss.backward()
    p = ex.params64(g, "param.")
    ref, tr = ex.glad_forward(Snp, p, L, 0, mode="ns10")
    assert relF(theta[0].detach().numpy(), ref[0]) < 5e-6
    assert abs(loss.item() - tr["loss"]) < 1e-5 * abs(tr["loss"])
    grads = ex.glad_backward(Snp, p, L, tr, 0, mode="ns10")
    sd = dict(model.named_parameters())
    for key in ex.PARAM_KEYS:
        assert relF(sd[key].grad.numpy(), grads[key]) < 2e-5, key
    with pytest.raises(Exception):
        uglad_amd.glad(torch.from_numpy(Snp), model, L=1, sqrt_mode="exact")


@pytest.mark.parametrize("ldl_launches", ["0", "1"])
def test_logdet_and_inverse_of_indefinite_matrices_beyond_the_eigensolver(emul, monkeypatch, ldl_launches):
    """torch.logdet's rules without an eigensolver (main.py:307): finite for an even number of negative eigenvalues, NaN for an odd one;
    the inverse (the loss's gradient S - Theta^-1) also for an indefinite matrix -- L D L^T carries the signs (ldl_wide.h)."""
    import uglad_amd

    monkeypatch.setenv("UGLAD_LDL_LAUNCHES", ldl_launches)
    rng = np.random.default_rng(1)
    D = 200
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    for negatives in (0, 2, 3):
        w = np.linspace(0.5, 5.0, D)
        w[:negatives] = [-1.0, -3.0, -0.7][:negatives]
        A = (Q * w) @ Q.T
        th = torch.from_numpy(A.astype(np.float32))[None].contiguous().requires_grad_(True)
        loss = uglad_amd.loss_uGLAD(th, torch.eye(D)[None].contiguous())
        if negatives % 2:
            assert torch.isnan(loss)
            continue
        ref = -np.linalg.slogdet(A)[1] + np.trace(A)
        assert abs(loss.item() - ref) < 1e-5 * abs(ref)
        loss.backward()
        assert relF(th.grad[0].numpy(), np.eye(D) - np.linalg.inv(A)) < 5e-6


def test_consensus_and_predict_surface(emul):
    import uglad_amd

    g = np.load(os.path.join(GOLDEN, "consensus.npz"))
    out = uglad_amd.get_final_precision_from_batch(torch.from_numpy(g["theta_K"]), type="min")
    np.testing.assert_array_equal(out.numpy(), g["out_min"])
    with pytest.raises(ValueError):
        uglad_amd.get_final_precision_from_batch(torch.from_numpy(g["theta_K"]), type="median")


def test_fit_direct_first_epochs_track_reference(emul, monkeypatch):
    """uGLAD_GL.fit(mode='direct') from the reference's own initial parameters: the per-epoch losses must track the
    reference's trajectory (3 epochs here; the GPU suite runs all 120)."""
    import uglad_amd
    from uglad_amd import main

    g = np.load(os.path.join(GOLDEN, "fit_direct_d25.npz"))
    losses = []
    real_init, real_fwd = main.init_uGLAD, main.forward_uGLAD

    def init(*a, **k):
        m, _ = real_init(*a, **k)
        m.load_state_dict({key: torch.from_numpy(np.array(g["init0." + key])) for key in ex.PARAM_KEYS})
        return m, main.glad.get_optimizers(m, lr_glad=k.get("lr", a[0] if a else 0.002))

    def fwd(*a, **k):
        th, ls = real_fwd(*a, **k)
        losses.append(float(ls.item()))
        return th, ls

    monkeypatch.setattr(main, "init_uGLAD", init)
    monkeypatch.setattr(main, "forward_uGLAD", fwd)
    est = uglad_amd.uGLAD_GL()
    res = est.fit(g["X"].copy(), epochs=3, lr=float(g["lr"]), L=int(g["L"]), verbose=False, mode="direct")
    assert res is None
    np.testing.assert_allclose(losses, g["losses"][:3], rtol=2e-5)
    assert est.precision_.shape == (25, 25) and est.precision_.dtype == np.float32
    np.testing.assert_allclose(est.covariance_, g["covariance_"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(est.location_, g["location_"], rtol=1e-9)
    assert est.node_names_[3] == "node_3"
    pred = est.predict(S=est.covariance_)
    assert pred.shape == (25, 25)


def test_partial_correlations_and_save_load_roundtrip(emul, tmp_path):
    """get_partial_correlations (ref main.py:794-819) and a save/load that really restores the model."""
    import uglad_amd

    rng = np.random.default_rng(3)
    A = rng.standard_normal((6, 6))
    P = A @ A.T + 6 * np.eye(6)
    rho = uglad_amd.get_partial_correlations(P)
    ref = np.zeros((6, 6))  # the reference's double loop, restated
    for i in range(6):
        for j in range(6):
            ref[i, j] = 1.0 if i == j else -P[min(i, j), max(i, j)] / np.sqrt(P[i, i] * P[j, j])
    assert np.allclose(rho, ref, rtol=0, atol=1e-15)  # host array in: float64 on the host, like the reference
    rho32 = emul.partial_correlations(torch.tensor(P[None], dtype=torch.float32))[0].numpy()  # the device kernel (fp32)
    assert np.allclose(rho32, ref, rtol=0, atol=2e-7)

    X = rng.standard_normal((60, 7))
    m = uglad_amd.uGLAD_GL()
    m.fit(X, centered=False, epochs=10, lr=0.002, INIT_DIAG=0, L=5, verbose=False)
    path = str(tmp_path / "model.pkl")
    uglad_amd.save_uGLAD_model(m, path)
    m2 = uglad_amd.load_uGLAD_model(path)
    assert isinstance(m2, uglad_amd.uGLAD_GL) and m2.model_glad is not None
    assert np.array_equal(m2.precision_, m.precision_) and np.array_equal(m2.covariance_, m.covariance_)
    for (k1, v1), (k2, v2) in zip(m.model_glad.state_dict().items(), m2.model_glad.state_dict().items()):
        assert k1 == k2 and torch.equal(v1.cpu(), v2.cpu())
    assert np.array_equal(m2.predict(X), m.predict(X))


def test_grouped_pass_equals_independent_passes(emul):
    """G problems with their own parameters and lambda sequences in one batch == G separate glad() calls
    (forward Theta, per-group parameter gradients), for one and for two matrices per group."""
    import uglad_amd
    from uglad_amd.glad.glad import glad_grouped
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    D, L = 12, 5
    for G, gs in ((3, 1), (2, 2)):
        S = torch.from_numpy(synthetic_covariance_batch(G * gs, D, seed=21))
        models = []
        for g in range(G):
            torch.manual_seed(100 + g)
            models.append(uglad_amd.GladParams(1.0 + 0.1 * g))
        P = torch.stack([m.packed().detach() for m in models]).requires_grad_(True)
        W = torch.from_numpy(np.random.default_rng(2).standard_normal((G * gs, D, D)).astype(np.float32))
        th = glad_grouped(S, P, L=L)
        (th * W).sum().backward()
        for g in range(G):
            sl = slice(g * gs, (g + 1) * gs)
            t1 = uglad_amd.glad(S[sl], models[g], L=L)
            (t1 * W[sl]).sum().backward()
            assert torch.equal(t1.detach(), th[sl].detach())
            g1 = torch.cat([p.grad.reshape(-1) for p in models[g].parameters()])
            assert torch.allclose(g1, P.grad[g], rtol=0, atol=0), (g, (g1 - P.grad[g]).abs().max())


def test_backward_pass_in_one_launch_equals_one_launch_per_step(emul, monkeypatch):
    """D <= 128: the backward pass keeps dL/dZ in LDS over all L steps of ONE launch (rhoNN gradient sums in registers until the end);
    UGLAD_PERSISTENT_BWD=0 launches one kernel per step as rounds 1-2 did.  Same dL/dZ chain bit for bit, so the gradients may differ
    only by the order in which the 28 per-matrix sums are added up."""
    import uglad_amd
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    for D, B, L in ((9, 3, 4), (40, 2, 3), (64, 1, 1)):
        S = torch.from_numpy(synthetic_covariance_batch(B, D, seed=5))
        W = torch.from_numpy(np.random.default_rng(3).standard_normal((B, D, D)).astype(np.float32))
        grads = []
        for flag in ("1", "0"):
            monkeypatch.setenv("UGLAD_PERSISTENT_BWD", flag)
            torch.manual_seed(1)
            model = uglad_amd.GladParams(1.0)
            (uglad_amd.glad(S, model, L=L) * W).sum().backward()
            grads.append(torch.cat([p.grad.reshape(-1) for p in model.parameters()]))
        scale = grads[1].abs().max()
        assert torch.allclose(grads[0], grads[1], rtol=0, atol=2e-6 * float(scale)), ((grads[0] - grads[1]).abs().max(), scale)
        if L == 1:
            assert torch.equal(grads[0], grads[1])


def test_cv_batched_folds_match_sequential(emul):
    """The folds of CV mode as one grouped batch give the estimator of the sequential driver."""
    import uglad_amd

    X = np.random.default_rng(11).standard_normal((60, 6))
    out = []
    for batched in (False, True):
        torch.manual_seed(5)
        est = uglad_amd.uGLAD_GL()
        est.fit(X.copy(), epochs=5, lr=0.002, L=4, verbose=False, k_fold=3, mode="cv", batched_folds=batched)
        out.append((est.precision_.copy(), torch.cat([v.detach().reshape(-1) for v in est.model_glad.state_dict().values()])))
    assert np.allclose(out[0][0], out[1][0], rtol=0, atol=1e-6), np.abs(out[0][0] - out[1][0]).max()
    assert torch.allclose(out[0][1], out[1][1], rtol=0, atol=1e-6)


def test_sharded_whole_pass_entry_with_an_injected_exchange(emul):
    """uglad_glad_forward_sharded on the emulator: with an exchange that adds nothing (a world of one rank) the pass equals
    uglad_glad_forward bit for bit; with one that adds a constant, lambda_k moves exactly as LambdaNN says (the exchange sits between
    the local sum and LambdaNN, the divisor is the global batch).  RCCL itself is not available to the host build (UGLAD_E_RCCL)."""
    from uglad_amd import _lib

    g = np.load(os.path.join(GOLDEN, "cell_d16_b3_L6_diag0_trained.npz"))
    p = ex.params64(g, "param.")
    pk = torch.tensor(np.concatenate([p[k].ravel() for k in ex.PARAM_KEYS]), dtype=torch.float32)
    S = torch.from_numpy(g["S"])
    M, D, L, mode = 3, 16, 6, _lib.SQRT_MODES["ns10"]

    def run(exchange=None, m_global=M):
        Z, lam, lam_in = torch.empty(2, M, D, D), torch.empty(L + 1), torch.empty(L + 1, 2)
        nfp, nfs, wsp = torch.empty(M), torch.empty(1), emul.workspace(M, D, S)
        args = (S, pk, 1.0, 0, L, Z, None, None, None, lam, lam_in, nfp, nfs, wsp, mode)
        if exchange is None:
            emul.glad_forward(*args)
        else:
            emul.glad_forward_sharded(*args, m_global, exchange)
        return Z[L & 1].clone(), lam.clone(), lam_in.clone(), nfs

    th0, lam0, lin0, _ = run()
    calls = []
    ident = _lib.HipLib.ALLREDUCE_FN(lambda buf, n, ctx, stream: calls.append(n) or 0)
    th1, lam1, lin1, _ = run((ident, None))
    assert calls == [1] * L and torch.equal(th1, th0) and torch.equal(lam1, lam0)
    # the exchange doubles the sum and the global batch is twice the local one: the batch MEAN, hence lambda_k, is unchanged
    holder = {}

    def doubling(buf, n, ctx, stream):
        holder["nfs"].mul_(2.0)
        return 0

    Z, lam, lam_in = torch.empty(2, M, D, D), torch.empty(L + 1), torch.empty(L + 1, 2)
    nfp, nfs, wsp = torch.empty(M), torch.empty(1), emul.workspace(M, D, S)
    holder["nfs"] = nfs
    emul.glad_forward_sharded(S, pk, 1.0, 0, L, Z, None, None, None, lam, lam_in, nfp, nfs, wsp, mode, 2 * M,
                              (_lib.HipLib.ALLREDUCE_FN(doubling), None))
    assert torch.equal(lam, lam0) and torch.equal(Z[L & 1], th0)
    with pytest.raises(_lib.UgladError, match="RCCL"):
        emul.rccl_unique_id()


@pytest.mark.parametrize("policy", ["ahead", "behind"])
def test_results_do_not_depend_on_how_far_one_wave_runs_ahead(policy):
    """The emulator's skewed schedules (tests/simt_emul: UGLAD_EMUL_SCHED=ahead / behind -- the lowest / highest wave always gets the next
    turn, so it runs ahead of the others up to the next workgroup barrier) must give the bits of the fair schedule: a missing barrier
    between two phases that reuse one LDS region would not.  A forward + backward pass at D = 25 and D = 64 (one and two MFMA tiles per side,
    Cholesky and eigen paths) in a subprocess, because the policy is read once per process."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import hashlib, os, sys
import numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import conftest
assert conftest.install_emulated_lib() is not None
import uglad_amd
from oracle import glad_exact as ex
h = hashlib.sha256()
for name, L in (("cell_d25_b1_L15_trained", 15), ("cell_d64_b4_L30_trained", 3)):
    g = np.load(os.path.join(%r, "tests", "golden", name + ".npz"))
    m = uglad_amd.GladParams(1.0)
    m.load_state_dict({k: torch.from_numpy(np.array(g["param." + k])) for k in ex.PARAM_KEYS})
    th, loss = uglad_amd.forward_uGLAD(torch.from_numpy(g["S"][:1].copy()), m, L=L)
    loss.backward()
    h.update(th.detach().numpy().tobytes())
    for p in m.parameters():
        h.update(p.grad.numpy().tobytes())
print("DIGEST", h.hexdigest())
""" % (root, root, root)
    digests = []
    for pol in ("fair", policy):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, UGLAD_EMUL_SCHED=pol), capture_output=True, text=True,
                             timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        digests.append([ln for ln in out.stdout.splitlines() if ln.startswith("DIGEST")][0])
    assert digests[0] == digests[1]
