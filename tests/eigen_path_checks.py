"""Theta_0 and the loss on the eigen path (init_inverse_kernel, loss_fwd_kernel on csrc/eig_lean.h), shared by the GPU suite
(test_gpu_parity.py) and its CPU twins on the emulator (test_kernels_emulated.py): `lib` is the HipLib under test, `dev` where its
tensors live.  Reference: numpy fp64.  Bounds: those of test_cholesky_inverse_logdet_and_the_eigen_fallback."""
import numpy as np
import torch


def relF(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def spd_batch(M, D, seed):
    A = np.random.default_rng(seed).standard_normal((M, D, 2 * D))
    return (A @ A.transpose(0, 2, 1) / (2 * D)).astype(np.float32)  # SPD, cond ~ 30


def loss_bound(want):
    return 2e-6 * max(1.0, abs(want)) + 1e-4


def loss_want(S0, Th):
    Th = Th.astype(np.float64)
    return -np.linalg.slogdet(Th)[1] + float(np.sum(S0.astype(np.float64) * Th.T))


def flags_of(wsp, M, D):
    return wsp[M * 3 * (32 * ((D + 31) // 32)):][:M].view(torch.int32).cpu().numpy()


def every_matrix_on_the_eigen_path(lib, dev, D, M=3, t=0.05):
    """With UGLAD_CHOLESKY=0 set by the caller: (S + tI)^-1 of init_theta, and loss / Theta^-1 of loss_fwd, for M SPD matrices."""
    S = spd_batch(M, D, seed=D)
    St = torch.from_numpy(S).to(dev)
    pk = torch.zeros(42, device=dev)
    pk[0] = t
    th0 = torch.empty_like(St)
    wsp = lib.workspace(M, D, St)
    lib.init_theta(St, pk, 0, th0, wsp)
    ref = np.linalg.inv(S.astype(np.float64) + t * np.eye(D))
    got = th0.cpu().numpy()
    err_inv = max(relF(got[m], ref[m]) for m in range(M))
    lp, tinv = torch.empty(M, device=dev), torch.empty_like(St)
    lib.loss_fwd(St, St[:1].contiguous(), None, lp, tinv, wsp)
    lp = lp.cpu().numpy()
    want = [loss_want(S[0], S[m]) for m in range(M)]
    err_tinv = max(relF(tinv[m].cpu().numpy(), np.linalg.inv(S[m].astype(np.float64))) for m in range(M))
    print(f"eigen path D={D}: Theta_0 relF {err_inv:.2e}, Theta^-1 relF {err_tinv:.2e}, "
          f"loss |delta| {max(abs(lp[m] - want[m]) for m in range(M)):.2e} (bound {min(loss_bound(w) for w in want):.2e})")
    assert err_inv < 1e-6, err_inv
    assert err_tinv < 1e-6, err_tinv
    for m in range(M):
        assert abs(lp[m] - want[m]) < loss_bound(want[m]), (m, lp[m], want[m])
    assert torch.equal(th0, th0.transpose(1, 2)) and torch.equal(tinv, tinv.transpose(1, 2))


def flagged_matrices_in_a_large_batch(lib, dev, D=7, M=520, t=0.05):
    """With the Cholesky kernels on: a batch larger than the T region of one matrix (M > NT * 512 floats) whose matrices 0, 1 and M - 1
    go to the eigen path.  Their T factors must not land on the flag words that workgroups scheduled later still have to read."""
    bad = [0, 1, M - 1]
    good = [m for m in range(M) if m not in bad]
    spd = spd_batch(M, D, seed=M)
    S = spd.copy()
    for m in bad:
        S[m] -= 1.5 * np.eye(D, dtype=np.float32)  # indefinite (eigenvalues of both signs)
    St = torch.from_numpy(S).to(dev)
    pk = torch.zeros(42, device=dev)
    pk[0] = t
    th0 = torch.empty_like(St)
    wsp = lib.workspace(M, D, St)
    lib.init_theta(St, pk, 0, th0, wsp)
    assert np.flatnonzero(flags_of(wsp, M, D)).tolist() == bad
    ref = np.linalg.inv(S.astype(np.float64) + t * np.eye(D))
    got = th0.cpu().numpy()
    err_good, err_bad = max(relF(got[m], ref[m]) for m in good), max(relF(got[m], ref[m]) for m in bad)
    print(f"flagged batch M={M} D={D}: Theta_0 relF SPD {err_good:.2e}, indefinite {err_bad:.2e}")
    assert err_good < 1e-6, err_good
    assert err_bad < 1e-3, err_bad  # (eigenvalues on both sides of zero: ill-conditioned)
    assert torch.equal(th0, th0.transpose(1, 2))
    # the loss: Theta = the SPD batch; matrix 0 with one negative eigenvalue (det < 0: NaN), matrices 1 and M - 1 with two (det > 0: finite,
    # and flagged like matrix 0)
    Th = spd.copy()
    Th[0][0, 0] -= 100.0
    for m in bad[1:]:
        Th[m][0, 0] -= 100.0
        Th[m][1, 1] -= 100.0
    Tt = torch.from_numpy(Th).to(dev)
    lp, tinv = torch.empty(M, device=dev), torch.empty_like(Tt)
    lib.loss_fwd(Tt, St[2:3].contiguous(), None, lp, tinv, wsp)
    assert np.flatnonzero(flags_of(wsp, M, D)).tolist() == bad
    lp = lp.cpu().numpy()
    assert np.flatnonzero(np.isnan(lp)).tolist() == [0]
    want = {m: loss_want(S[2], Th[m]) for m in range(1, M)}
    tinv = tinv.cpu().numpy()
    inv = np.linalg.inv(Th.astype(np.float64))
    # Theta^-1 of the SPD matrices (no shift here): the 1e-6 of the existing test belongs to cond ~ 30, and the error of an fp32 inverse grows
    # in proportion to the condition number, which reaches 105 among 517 matrices of 14 samples -- per matrix 1e-6 * max(1, cond / 30)
    cond = np.linalg.cond(Th.astype(np.float64))
    err_good = max(relF(tinv[m], inv[m]) / max(1.0, cond[m] / 30.0) for m in good)
    err_bad = max(relF(tinv[m], inv[m]) for m in bad)
    print(f"flagged batch M={M} D={D}: Theta^-1 relF SPD (over max(1, cond / 30)) {err_good:.2e}, indefinite {err_bad:.2e}, loss |delta| SPD "
          f"{max(abs(lp[m] - want[m]) for m in good):.2e}, indefinite {max(abs(lp[m] - want[m]) for m in bad[1:]):.2e}")
    for m in good:
        assert abs(lp[m] - want[m]) < loss_bound(want[m]), (m, lp[m], want[m])
    assert err_good < 1e-6, err_good
    assert err_bad < 1e-3, err_bad
