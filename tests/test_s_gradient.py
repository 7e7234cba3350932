"""The gradient with respect to the input covariance S (include/uglad_hip.h: uglad_glad_backward_wrt_s, uglad_loss_bwd_wrt_s).

glad(), glad_grouped() and loss_uGLAD() keep S in the autograd graph when it requires grad, as the reference does (glad.py:109-144,
main.py:309).  S.grad is the SYMMETRIC part (G + G^T) / 2 of the gradient G that autograd forms for the reference -- which treats the D^2
entries of S as independent -- and is checked here against that part of the fp64 oracle's autograd gradient (oracle/glad_ns.py), and
convention-free through S = cov(X) with X learnable.

CPU tests run the real kernels on the SIMT emulator (NT = 1, 2, 4, 5); the GPU tests run the same checks on the MI355X at the sizes the
emulator cannot afford.  Bounds: 2e-5 relative Frobenius against the fp64 oracle on the spectral path (the floor of the package's
gradient bound), 1e-4 on the matrix-iteration path.
"""
import os

import numpy as np
import pytest
import torch

from oracle import glad_ns as ns

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL = 2e-5  # spectral path: relative Frobenius, fp32 kernels against the fp64 oracle
TOL_NS = 1e-4  # matrix-iteration path


def relF(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def sym(a):
    return 0.5 * (a + np.swapaxes(a, -1, -2))


def _model(g, device="cpu"):
    import uglad_amd

    m = uglad_amd.GladParams(1.0, device=device)
    m.load_state_dict({k: torch.from_numpy(np.array(g["param." + k])) for k in ns.PARAM_KEYS})
    return m


def _p64(g):
    return {k: torch.tensor(np.array(g["param." + k]), dtype=torch.float64) for k in ns.PARAM_KEYS}


def oracle_sgrad(S, p64, L, init_diag, glad_only=False, W=None):
    """sym(dL/dS) of the fp64 oracle: L = the glasso loss of forward_uGLAD (glad_only: the loss against a detached copy of S, so only
    the glad part is differentiated), or <W, Theta_L> when W is given."""
    S64 = torch.tensor(np.asarray(S, dtype=np.float64), requires_grad=True)
    theta = ns.glad(S64, p64, L=L, INIT_DIAG=init_diag)
    if W is not None:
        loss = (theta * torch.as_tensor(W, dtype=torch.float64)).sum()
    else:
        loss = ns.loss_uGLAD(theta, S64.detach().clone() if glad_only else S64)
    loss.backward()
    return sym(S64.grad.numpy())


def kernel_sgrad(S, model, L, init_diag, glad_only=False, device="cpu"):
    import uglad_amd

    St = torch.tensor(np.asarray(S, dtype=np.float32), device=device, requires_grad=True)
    _, loss = uglad_amd.forward_uGLAD(St, model, L=L, INIT_DIAG=init_diag, loss_Sb=St.detach().clone() if glad_only else None)
    loss.backward()
    assert St.grad is not None, "S.grad is None: S was cut out of the graph"
    return St.grad


CASES = [  # (golden, matrices, L, init_diag)
    ("cell_d25_b1_L15_trained", 1, 6, 0),
    ("cell_d16_b3_L6_diag1_fresh", 3, 6, 1),
    ("cell_d16_b3_L6_diag0_trained", 3, 6, 0),
    ("cell_d33_b3_L15_fresh", 1, 3, 0),
    ("cell_d64_b4_L30_trained", 1, 2, 0),
    ("cell_d64_b4_L30_trained", 1, 6, 1),
]


@pytest.mark.parametrize("glad_only", [False, True])
@pytest.mark.parametrize("name,B,L,init_diag", CASES)
def test_s_grad_against_fp64_oracle(emul, name, B, L, init_diag, glad_only):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    S = g["S"][:B]
    got = kernel_sgrad(S, _model(g), L, init_diag, glad_only)
    assert got.dtype == torch.float32 and torch.equal(got, got.transpose(1, 2))  # exactly symmetric
    ref = oracle_sgrad(S, _p64(g), L, init_diag, glad_only)
    assert relF(got.numpy(), ref) < TOL, relF(got.numpy(), ref)


def test_s_grad_both_init_modes_on_one_input(emul):
    """init_diag 0 and 1 on the same S and parameters: the Theta_0 terms differ (-Theta0 G0 Theta0 vs -G0_ii Theta0_ii^2)."""
    g = np.load(os.path.join(GOLDEN, "cell_d25_b1_L15_trained.npz"))
    for init_diag in (0, 1):
        got = kernel_sgrad(g["S"], _model(g), 3, init_diag)
        ref = oracle_sgrad(g["S"], _p64(g), 3, init_diag)
        assert relF(got.numpy(), ref) < TOL, (init_diag, relF(got.numpy(), ref))


def test_s_grad_workspace_resident_d129(emul):
    """D = 129: the NT = 5 instantiation with its big matrices in the caller's workspace, one launch per step (wide mode off)."""
    g = np.load(os.path.join(GOLDEN, "cell_d129_b2_L30_trained.npz"))
    emul.set_wide_mode(0)
    emul.set_matrix_iteration(0)
    try:
        got = kernel_sgrad(g["S"][:1], _model(g), 2, 0)
    finally:
        emul.set_wide_mode(-1)
        emul.set_matrix_iteration(-1)
    ref = oracle_sgrad(g["S"][:1], _p64(g), 2, 0)
    assert torch.equal(got, got.transpose(1, 2))
    assert relF(got.numpy(), ref) < TOL, relF(got.numpy(), ref)


def test_s_grad_in_one_launch_equals_one_launch_per_step(emul, monkeypatch):
    """UGLAD_PERSISTENT_BWD=0 (one launch per step) and the default (all steps in one launch) accumulate the same gS."""
    import uglad_amd
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    S = torch.from_numpy(synthetic_covariance_batch(2, 20, seed=7))
    W = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 20, 20)).astype(np.float32))
    out = []
    for flag in ("1", "0"):
        monkeypatch.setenv("UGLAD_PERSISTENT_BWD", flag)
        torch.manual_seed(1)
        model = uglad_amd.GladParams(1.0)
        St = S.clone().requires_grad_(True)
        (uglad_amd.glad(St, model, L=4) * W).sum().backward()
        out.append(St.grad)
    assert torch.equal(out[0], out[1])


def test_theta_and_parameter_gradients_are_bitwise_unchanged_by_requesting_s_grad(emul):
    import uglad_amd

    g = np.load(os.path.join(GOLDEN, "cell_d16_b3_L6_diag0_trained.npz"))
    res = []
    for want in (False, True):
        model = _model(g)
        St = torch.from_numpy(g["S"].copy()).requires_grad_(want)
        theta, loss = uglad_amd.forward_uGLAD(St, model, L=6)
        loss.backward()
        res.append((theta.detach(), [p.grad.clone() for p in model.parameters()], St.grad))
    assert res[0][2] is None and res[1][2] is not None
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))


def test_no_grad_and_detached_inputs_behave_as_before(emul):
    import uglad_amd

    g = np.load(os.path.join(GOLDEN, "cell_d16_b3_L6_diag0_trained.npz"))
    model = _model(g)
    St = torch.from_numpy(g["S"].copy()).requires_grad_(True)
    with torch.no_grad():
        theta = uglad_amd.glad(St, model, L=2)
    assert not theta.requires_grad
    for p in model.parameters():
        p.requires_grad_(False)
    theta = uglad_amd.glad(St, model, L=2)  # S alone asks for the gradient: the forward keeps the state for the backward
    theta.sum().backward()
    assert St.grad is not None and torch.equal(St.grad, St.grad.transpose(1, 2))


def test_x_grad_through_the_sample_covariance(emul):
    """S = Xc^T Xc / N with X learnable: X.grad is free of any convention (the antisymmetric part of dL/dS has no effect on it)."""
    import uglad_amd

    g = np.load(os.path.join(GOLDEN, "cell_d25_b1_L15_trained.npz"))
    X0 = np.random.default_rng(3).standard_normal((40, 12))

    def cov(X):
        Xc = X - X.mean(0, keepdim=True)
        return (Xc.T @ Xc / X.shape[0] + 0.1 * torch.eye(X.shape[1], dtype=X.dtype))[None]

    X = torch.tensor(X0, dtype=torch.float32, requires_grad=True)
    _, loss = uglad_amd.forward_uGLAD(cov(X), _model(g), L=4)
    loss.backward()
    X64 = torch.tensor(X0, dtype=torch.float64, requires_grad=True)
    S64 = cov(X64)
    _, loss64 = ns.forward_uGLAD(S64, _p64(g), L=4)
    loss64.backward()
    assert relF(X.grad.numpy(), X64.grad.numpy()) < TOL, relF(X.grad.numpy(), X64.grad.numpy())


def test_grouped_pass_equals_per_group_passes(emul):
    import uglad_amd
    from uglad_amd.glad.glad import glad_grouped
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    S = torch.from_numpy(synthetic_covariance_batch(4, 12, seed=2))
    models = []
    for k in range(2):
        torch.manual_seed(10 + k)
        models.append(uglad_amd.GladParams(1.0 + 0.1 * k))
    P = torch.stack([m.packed().detach() for m in models]).requires_grad_(True)
    Sg = S.clone().requires_grad_(True)
    th = glad_grouped(Sg, P, L=3)
    uglad_amd.loss_uGLAD(th, Sg, batch_divisor=1).backward()
    for k in range(2):
        Sk = S[2 * k:2 * k + 2].clone().requires_grad_(True)
        tk = uglad_amd.glad(Sk, models[k], L=3)
        uglad_amd.loss_uGLAD(tk, Sk, batch_divisor=1).backward()
        assert torch.equal(Sg.grad[2 * k:2 * k + 2], Sk.grad), k


def test_loss_with_one_s_broadcast_against_the_batch(emul):
    """The missing-data call: one S (1, D, D) against K precision matrices, divisor 1 and an explicit batch_divisor."""
    import uglad_amd
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    S = torch.from_numpy(synthetic_covariance_batch(1, 10, seed=4))
    theta = torch.linalg.inv(torch.from_numpy(synthetic_covariance_batch(3, 10, seed=5)) + torch.eye(10))
    theta = theta + 0.01 * torch.randn(3, 10, 10, generator=torch.Generator().manual_seed(0))  # not symmetric on purpose
    for divisor in (None, 5):
        St = S.clone().requires_grad_(True)
        uglad_amd.loss_uGLAD(theta.contiguous(), St, batch_divisor=divisor).backward()
        ref = theta.double().sum(0, keepdim=True)
        ref = 0.5 * (ref + ref.transpose(1, 2)) / (divisor or 1)
        assert torch.equal(St.grad, St.grad.transpose(1, 2))
        assert relF(St.grad.numpy(), ref.numpy()) < 1e-6


@pytest.mark.parametrize("D,B,L", [(7, 3, 6), (100, 1, 2)])
def test_s_grad_synthetic_sizes(emul, D, B, L):
    """NT = 1 with a batch, and NT = 4 (D = 100: the largest LDS-resident size the emulator builds)."""
    g = np.load(os.path.join(GOLDEN, "cell_d25_b1_L15_trained.npz"))
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    S = synthetic_covariance_batch(B, D, seed=D)
    for init_diag in (0, 1):
        got = kernel_sgrad(S, _model(g), L, init_diag)
        ref = oracle_sgrad(S, _p64(g), L, init_diag)
        assert relF(got.numpy(), ref) < TOL, (D, init_diag, relF(got.numpy(), ref))


def test_wide_backward_equals_one_workgroup_backward_d150(emul):
    """D = 150 with wide mode on (many workgroups per matrix, csrc/wide_bwd.h; dL/dS formed behind each step) and off (cell_bwd_gs_kernel)."""
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    g = np.load(os.path.join(GOLDEN, "cell_d25_b1_L15_trained.npz"))
    S = synthetic_covariance_batch(1, 150, seed=3)
    out = []
    emul.set_matrix_iteration(0)
    try:
        for wide in (0, 1):
            emul.set_wide_mode(wide)
            out.append(kernel_sgrad(S, _model(g), 2, 0))
    finally:
        emul.set_wide_mode(-1)
        emul.set_matrix_iteration(-1)
    assert torch.equal(out[1], out[1].transpose(1, 2))
    assert relF(out[1].numpy(), out[0].numpy()) < 1e-5, relF(out[1].numpy(), out[0].numpy())


def test_matrix_iteration_forced_equals_spectral_path(emul):
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    g = np.load(os.path.join(GOLDEN, "cell_d25_b1_L15_trained.npz"))
    S = synthetic_covariance_batch(3, 12, seed=5)
    out = []
    for forced in (0, 1):
        emul.set_matrix_iteration(forced)
        try:
            out.append(kernel_sgrad(S, _model(g), 4, 0))
        finally:
            emul.set_matrix_iteration(-1)
    assert torch.equal(out[1], out[1].transpose(1, 2))
    assert relF(out[1].numpy(), out[0].numpy()) < 1e-5, relF(out[1].numpy(), out[0].numpy())


def test_beyond_the_eigensolver_d161_vs_oracle(emul):
    """D = 161: the emulator build's first matrix-iteration size (Theta_0 by the tiled products, every step on csrc/wide_ns.h)."""
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    g = np.load(os.path.join(GOLDEN, "cell_d25_b1_L15_trained.npz"))
    S = synthetic_covariance_batch(1, 161, seed=9)
    got = kernel_sgrad(S, _model(g), 2, 0)
    ref = oracle_sgrad(S, _p64(g), 2, 0)
    assert torch.equal(got, got.transpose(1, 2))
    assert relF(got.numpy(), ref) < TOL_NS, relF(got.numpy(), ref)


def test_exact_square_root_against_central_differences(emul):
    """sqrt_mode="exact": <S.grad, E> against central differences in fp64 of oracle/glad_exact.py along random symmetric directions E, with
    the lambda sequence held at the base run's (the reference detaches LambdaNN's inputs).  A direction whose +/- runs change the active
    set of the threshold at any step is skipped."""
    import uglad_amd
    from oracle import glad_exact as ex

    g = np.load(os.path.join(GOLDEN, "cell_d16_b3_L6_diag0_trained.npz"))
    S = g["S"][:1].astype(np.float64)
    L = 4
    p = ex.params64(g, "param.")
    _, tr = ex.glad_forward(S, p, L, 0, mode="exact")
    lams = tr["lambdas"]

    def run(Sx):
        Z = ex.init_theta(Sx, float(p["theta_init_offset"][0]), 0)
        pattern = []
        for k in range(L):
            Z = ex.cell_fwd(Sx, Z, lams[k], p, "exact")[0]
            pattern.append(Z == 0)
        return ex.loss_fwd(Z, Sx), np.stack(pattern)

    St = torch.tensor(S, dtype=torch.float32, requires_grad=True)
    _, loss = uglad_amd.forward_uGLAD(St, _model(g), L=L, sqrt_mode="exact")
    loss.backward()
    gS = St.grad.double().numpy()
    rng = np.random.default_rng(0)
    checked = 0
    for _ in range(6):
        E = rng.standard_normal(S.shape)
        E = 0.5 * (E + E.transpose(0, 2, 1))
        h = 1e-7  # (1e-5 moves entries of the trained parameters' thresholds across it)
        (lp, pp), (lm, pm) = run(S + h * E), run(S - h * E)
        if not np.array_equal(pp, pm):
            continue
        fd = (lp - lm) / (2 * h)
        assert abs(float(np.sum(gS * E)) - fd) < 1e-4 * max(1.0, abs(fd)), (float(np.sum(gS * E)), fd)
        checked += 1
    assert checked >= 3


# ------------------------------------------------------------------------------------------------------------------------------- GPU
def _synthetic(B, D, seed):
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    return synthetic_covariance_batch(B, D, seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("D,B,L,wide", [(25, 2, 6, -1), (64, 2, 4, -1), (80, 2, 3, -1), (128, 1, 3, -1), (200, 1, 2, -1), (200, 2, 2, 0),
                                        (256, 2, 2, 1), (257, 1, 2, -1), (300, 1, 2, -1), (511, 1, 1, -1)])
def test_gpu_s_grad_against_fp64_oracle(D, B, L, wide):
    """Every path glad() takes: the spectral one-workgroup backward (D <= 128, and D = 200 with wide mode off), the many-workgroups backward
    (K = 2 matrices of D = 256 with wide mode on) and the matrix iteration (one matrix of D = 200, and D > 256) -- default settings otherwise."""
    from uglad_amd import _lib

    g = np.load(os.path.join(GOLDEN, "cell_d25_b1_L15_trained.npz"))  # trained parameters
    S = _synthetic(B, D, seed=D)
    lib = _lib.get_lib()
    if wide >= 0:
        lib.set_wide_mode(wide)
        lib.set_matrix_iteration(0)
    ns_path = lib.cond_is_upper_bound(B, D, True, _lib.SQRT_MODES["ns10"])
    try:
        for init_diag in (0, 1):
            got = kernel_sgrad(S, _model(g, "cuda"), L, init_diag, device="cuda").cpu()
            assert torch.equal(got, got.transpose(1, 2))
            ref = oracle_sgrad(S, _p64(g), L, init_diag)
            assert relF(got.numpy(), ref) < (TOL_NS if ns_path else TOL), (D, init_diag, relF(got.numpy(), ref))
    finally:
        lib.set_wide_mode(-1)
        lib.set_matrix_iteration(-1)


@pytest.mark.gpu
def test_gpu_config3_shape_with_an_oracle_subbatch():
    """Config 3's shape (M = 1024, D = 128, L = 30): the whole batch for finiteness and symmetry; lambda_k depends on the batch mean of the
    norm, so the oracle comparison runs a 4-matrix sub-batch alone on both sides (as test_full_size_properties_and_subsample_parity does)."""
    import uglad_amd

    g = np.load(os.path.join(GOLDEN, "cell_d25_b1_L15_trained.npz"))
    S = _synthetic(1024, 128, seed=3)
    St = torch.tensor(S, device="cuda", requires_grad=True)
    _, loss = uglad_amd.forward_uGLAD(St, _model(g, "cuda"), L=30)
    loss.backward()
    full = St.grad
    assert torch.isfinite(full).all() and torch.equal(full, full.transpose(1, 2))
    got = kernel_sgrad(S[:4], _model(g, "cuda"), 30, 0, device="cuda").cpu().numpy()
    ref = oracle_sgrad(S[:4], _p64(g), 30, 0)
    assert relF(got, ref) < TOL, relF(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [25, 128])
def test_gpu_theta_and_parameter_gradients_bitwise_unchanged(D):
    import uglad_amd

    g = np.load(os.path.join(GOLDEN, "cell_d25_b1_L15_trained.npz"))
    S = _synthetic(3, D, seed=11)
    res = []
    for want in (False, True):
        model = _model(g, "cuda")
        St = torch.tensor(S, device="cuda", requires_grad=want)
        theta, loss = uglad_amd.forward_uGLAD(St, model, L=15)
        loss.backward()
        res.append((theta.detach().cpu(), [p.grad.cpu() for p in model.parameters()], St.grad))
    assert res[0][2] is None and res[1][2] is not None
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
