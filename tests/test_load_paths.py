"""The load phases of the tridiagonalisation (tridiag.h, tridiag_wave.h) and of the backward cell (cell_bwd.h) request their data in batches.
tridiag.h and cell_bwd.h take 16-byte loads where the matrix is contiguous and 16-byte aligned (D a multiple of 4 -- for the backward cell D a
multiple of 32 -- and aligned tensors) and 4-byte loads everywhere else; tridiag_wave.h has 4-byte loads only.  Both paths do the same arithmetic
on the same values, so the same numbers handed over once in freshly allocated tensors and once as views that start one float into a larger
buffer (data pointer 4 mod 16) must give the same BITS; M = 3 puts the matrices of an odd D at odd offsets as well.  On the SIMT emulator,
and with -m gpu on the device, where the sizes of the flagship workload (127, 128) and of the NT = 3 instantiations (90, 96: one column slot
per 4-byte batch, not built for the emulator) join in."""
import os

import numpy as np
import pytest
import torch

from oracle import glad_exact as ex

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
M = 3
SIZES_CPU = [30, 32, 33, 64]


def fresh(t, dev):
    """The values of `t` in a tensor of its own on `dev`: 16-byte aligned."""
    out = torch.empty(t.shape, dtype=torch.float32, device=dev)
    out.copy_(t)
    assert out.data_ptr() % 16 == 0
    return out


def shifted(t, dev):
    """The same values viewed one float into a larger buffer: data pointer 4 mod 16."""
    n = t.numel()
    buf = torch.empty(n + 8, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + n].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def sym_batch(D, seed):
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    S = torch.from_numpy(synthetic_covariance_batch(M, D, seed=seed))
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(M, D, D, generator=g)
    return S.contiguous(), (0.5 * (Z + Z.transpose(1, 2))).contiguous()


def check_eigenvalues(got, A64):
    w = np.linalg.eigvalsh(A64)
    assert np.abs(np.sort(np.asarray(got, dtype=np.float64)) - w).max() < 3e-6 * np.abs(w).max()  # (test_symeig's bound)


# ------------------------------------------------------------------------------------------------------------ tridiagonalisation
def run_tridiag(lib, dev, D):
    DP = 32 * ((D + 31) // 32)
    S, Z = sym_batch(D, 11 + D)
    lam = torch.tensor([0.7], device=dev)
    outs = []
    for place in (fresh, shifted):
        A0, A1 = place(S, dev), place(Z, dev)
        R = torch.zeros(M, D, D, device=dev)  # (rows n-2, n-1 of R and the columns up to the diagonal are not written)
        wsp = lib.workspace(M, D, A0).zero_()
        lib.tridiagonalize(A0, A1, lam, R, wsp)
        outs.append((R.cpu(), wsp[:M * 3 * DP].cpu().clone()))
    assert torch.equal(outs[0][0], outs[1][0]), "reflectors differ between the aligned and the offset call"
    assert torch.equal(outs[0][1], outs[1][1]), "d, e, tau differ between the aligned and the offset call"
    tri = outs[0][1].view(M, 3, DP).double().numpy()
    A = S.double().numpy() / 0.7 - Z.double().numpy()
    for m in range(M):
        d, e = tri[m, 0, :D], tri[m, 1, :D - 1]
        T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
        check_eigenvalues(np.linalg.eigvalsh(T), A[m])


def run_symeig(lib, dev, D):
    S, Z = sym_batch(D, 23 + D)
    A = (S - Z).contiguous()
    outs = []
    for place in (fresh, shifted):
        Ad = place(A, dev)
        U = torch.empty(M, D, D, device=dev)
        beta = torch.empty(M, D, device=dev)
        lib.symeig(Ad, U, beta)
        outs.append((U.cpu(), beta.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for m in range(M):
        check_eigenvalues(outs[0][1][m].numpy(), A[m].double().numpy())


def tridiag_switches(monkeypatch, kernel):
    if kernel == "wg":  # D <= 32 goes to the one-wave kernel, D <= 96 to 128 NT threads: the 512-thread workgroup kernel stays covered
        monkeypatch.setenv("UGLAD_TRIDIAG_WAVE", "0")
        monkeypatch.setenv("UGLAD_TRIDIAG_SMALL", "0")
    elif kernel == "small":
        monkeypatch.setenv("UGLAD_TRIDIAG_WAVE", "0")


TRIDIAG_CASES = [(30, "wave"), (32, "wave"), (30, "small"), (32, "small"), (33, "small"), (64, "small"), (30, "wg"), (32, "wg"), (33, "wg"),
                 (64, "wg")]


@pytest.mark.parametrize("D,kernel", TRIDIAG_CASES)
def test_tridiagonalize_aligned_and_offset_inputs(emul, monkeypatch, D, kernel):
    tridiag_switches(monkeypatch, kernel)
    run_tridiag(emul, torch.device("cpu"), D)


@pytest.mark.parametrize("D,kernel", TRIDIAG_CASES)
def test_symeig_aligned_and_offset_inputs(emul, monkeypatch, D, kernel):
    tridiag_switches(monkeypatch, kernel)
    run_symeig(emul, torch.device("cpu"), D)


def gpu_lib():
    from uglad_amd import _lib

    return _lib.get_lib(), torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("D,kernel", TRIDIAG_CASES + [(90, "small"), (96, "small"), (90, "wg"), (96, "wg"), (127, "wg"), (128, "wg")])
def test_tridiagonalize_aligned_and_offset_inputs_gpu(monkeypatch, D, kernel):
    tridiag_switches(monkeypatch, kernel)
    run_tridiag(*gpu_lib(), D)


@pytest.mark.gpu
@pytest.mark.parametrize("D,kernel", TRIDIAG_CASES + [(90, "small"), (96, "small"), (90, "wg"), (96, "wg"), (127, "wg"), (128, "wg")])
def test_symeig_aligned_and_offset_inputs_gpu(monkeypatch, D, kernel):
    tridiag_switches(monkeypatch, kernel)
    run_symeig(*gpu_lib(), D)


# ------------------------------------------------------------------------------------------------------------------ backward pass
L = 2
_state = {}  # (device type, D) -> the forward pass's saved state and G_L, computed once and left unchanged


def trained():
    g = np.load(os.path.join(GOLDEN, "params_trained.npz"))
    p = ex.params64(g)
    return p, torch.tensor(np.concatenate([p[k].ravel() for k in ex.PARAM_KEYS]), dtype=torch.float32)


def forward_state(lib, dev, D):
    from uglad_amd import _lib
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    key = (dev.type, D)
    if key not in _state:
        p, packed = trained()
        S64 = synthetic_covariance_batch(M, D, seed=40 + D).astype(np.float64)
        f32 = dict(dtype=torch.float32, device=dev)
        S, params = torch.from_numpy(S64.astype(np.float32)).to(dev), packed.to(dev)
        Z, half, U = torch.empty(L + 1, M, D, D, **f32), torch.empty(L, M, D, D, **f32), torch.empty(L, M, D, D, **f32)
        beta, lam, lam_in = torch.empty(L, M, D, **f32), torch.empty(L + 1, **f32), torch.empty(L + 1, 2, **f32)
        nfp, nfs = torch.empty(M, **f32), torch.empty(1, **f32)
        mode = _lib.SQRT_MODES["ns10"]
        lib.glad_forward(S, params, 1.0, 0, L, Z, half, U, beta, lam, lam_in, nfp, nfs, lib.workspace(M, D, S), mode)
        # the oracle's own pass in fp64, and its loss gradient at ITS Theta_L as the G_L both are given
        _, tr = ex.glad_forward(S64, p, L, 0, mode="ns10")
        ref = ex.glad_backward(S64, p, L, tr, 0, mode="ns10")
        G_L = torch.from_numpy(ex.loss_bwd(tr["theta_L"], S64).astype(np.float32)).to(dev)
        _state[key] = dict(S=S, params=params, Z=Z, half=half, U=U, beta=beta, lam=lam, lam_in=lam_in, G_L=G_L, mode=mode, ref=ref)
    return _state[key]


def backward(lib, dev, D, st, place, with_gs=False):
    from uglad_amd import _lib

    f32 = dict(dtype=torch.float32, device=dev)
    Z, half, U, beta, G_L = (place(st[k], dev) for k in ("Z", "half", "U", "beta", "G_L"))
    bufs = (torch.zeros(M, D, D, **f32), torch.zeros(M, D, D, **f32))
    grp, glp, gtp = torch.empty(M, _lib.NRHO, **f32), torch.empty(L, M, **f32), torch.empty(M, **f32)
    grad = torch.empty(_lib.NPARAM, **f32)
    gS = torch.empty(M, D, D, **f32) if with_gs else None
    lib.glad_backward(G_L, st["S"], st["params"], 0, L, Z, half, U, beta, st["lam"], st["lam_in"], bufs[0], bufs[1], grp, glp, gtp, grad,
                      lib.workspace(M, D, st["S"]), st["mode"], gS=gS)
    out = dict(G_out=bufs[0].cpu(), grad=grad.cpu(), glam=glp.cpu())  # (dL/dZ_0 ends up in the first buffer on either route)
    if with_gs:
        out["gS"] = gS.cpu()
    return out


def run_backward(lib, dev, D, monkeypatch, with_gs=False):
    st = forward_state(lib, dev, D)
    a = backward(lib, dev, D, st, fresh, with_gs)
    b = backward(lib, dev, D, st, shifted, with_gs)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k} differs between the aligned and the offset call"
    # one launch for the pass == one launch per step (test_backward_pass_in_one_launch_equals_one_launch_per_step: the same dL/dZ chain bit
    # for bit, the sums over the steps in another order)
    monkeypatch.setenv("UGLAD_PERSISTENT_BWD", "0")
    c = backward(lib, dev, D, st, fresh, with_gs)
    monkeypatch.delenv("UGLAD_PERSISTENT_BWD")
    assert torch.equal(a["G_out"], c["G_out"])
    assert torch.equal(a["glam"], c["glam"])
    scale = float(c["grad"].abs().max())
    assert torch.allclose(a["grad"], c["grad"], rtol=0, atol=2e-6 * scale), ((a["grad"] - c["grad"]).abs().max(), scale)
    if with_gs:
        assert torch.allclose(a["gS"], c["gS"], rtol=0, atol=2e-6 * float(c["gS"].abs().max()))
        assert torch.equal(a["gS"], a["gS"].transpose(1, 2))
    # the gradient contract against the fp64 oracle (as test_forward_backward_vs_reference_goldens states it)
    got, at = a["grad"].double().numpy(), 0
    for key in ex.PARAM_KEYS:
        ref = st["ref"][key]
        g = got[at:at + ref.size].reshape(ref.shape)
        at += ref.size
        err = float(np.linalg.norm(g - ref) / max(np.linalg.norm(ref), 1e-30))
        assert err < 1e-4 or np.abs(g - ref).max() < 1e-6, (key, err, g, ref)
    assert at == got.size


@pytest.mark.parametrize("D", SIZES_CPU)
def test_backward_pass_aligned_and_offset_state(emul, monkeypatch, D):
    run_backward(emul, torch.device("cpu"), D, monkeypatch)


def test_backward_pass_wrt_s_aligned_and_offset_state(emul, monkeypatch):
    run_backward(emul, torch.device("cpu"), 32, monkeypatch, with_gs=True)


@pytest.mark.gpu
@pytest.mark.parametrize("D", SIZES_CPU + [96, 128])
def test_backward_pass_aligned_and_offset_state_gpu(monkeypatch, D):
    run_backward(*gpu_lib(), D, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [32, 128])
def test_backward_pass_wrt_s_aligned_and_offset_state_gpu(monkeypatch, D):
    run_backward(*gpu_lib(), D, monkeypatch, with_gs=True)
