"""K_ij of the NS10 backward (glad_device.h: ns_divided_difference): the ten-factor product

    K_ij = prod_{t<10} 1/2 (3 - (a_i^t)^2 - (a_j^t)^2 + a_i^t a_j^t) / (2 ||R||),     a^{t+1} = 1/2 a^t (3 - (a^t)^2),   a^0 = r / ||R||

telescopes, because factor t equals (a_i^{t+1} + a_j^{t+1}) / (a_i^t + a_j^t), to (a_i^10 + a_j^10) / ((a_i^0 + a_j^0) 2 ||R||).  Here both are
restated in numpy fp32, operation by operation as the kernels evaluate them (the product as it stood in cell_bwd.h / wide_bwd.h, the quotient with
div_acc's reciprocal and one Newton step), and compared with the product in fp64: the quotient must be no further from it than the product was.
Then the backward cell itself on the SIMT emulator at two small sizes against the fp64 oracle, both square-root modes."""
import os

import numpy as np
import pytest
import torch

from oracle import glad_exact as ex

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
F = np.float32
NS = ex.NS_ITERS


def iterates32(r):
    """a^0 and a^10 of the spectrum r (fp32), with the kernel's rounding: ||R|| and every step in fp32.  Also every iterate, for the product."""
    r = r.astype(F)
    nrm = np.sqrt(np.sum(r * r, dtype=F), dtype=F)
    a = (r / nrm).astype(F)
    its = []
    for _ in range(NS):
        its.append(a)
        a = (F(0.5) * a * (F(3.0) - a * a)).astype(F)
    return its, a, nrm


def k_product32(r):
    its, _, nrm = iterates32(r)
    P = np.ones((r.size, r.size), dtype=F)
    for a in its:
        q = a * a
        P = P * (F(0.5) * (F(3.0) - q[:, None] - q[None, :] + a[:, None] * a[None, :]))
    return (P * (F(1.0) / (F(2.0) * nrm))).astype(F)


def div_acc32(a, b):
    """glad_device.h div_acc: reciprocal, one Newton step (two fused multiply-adds: each evaluated in fp64 and rounded once), a * q."""
    q = (F(1.0) / b).astype(F)
    e = (1.0 - b.astype(np.float64) * q.astype(np.float64)).astype(F)
    q = (q.astype(np.float64) * e.astype(np.float64) + q.astype(np.float64)).astype(F)
    return (a * q).astype(F)


def k_telescoped32(r):
    its, aN, nrm = iterates32(r)
    a0 = its[0]
    return (div_acc32(aN[:, None] + aN[None, :], a0[:, None] + a0[None, :]) * (F(1.0) / (F(2.0) * nrm))).astype(F)


def k_product64(r):
    return ex.inv_pair_sum(r.astype(F).astype(np.float64), "ns10")


def spectra():
    rng = np.random.default_rng(20261019)
    out = []
    for D in (1, 2, 3, 128):
        for _ in range(6):
            out.append(rng.uniform(20.0, 300.0, D))
            out.append(np.exp(rng.uniform(np.log(0.05), np.log(300.0), D)))
            out.append(np.concatenate([1.0 + 1e-3 * rng.standard_normal(D - 1), [1e3]]))  # the small ones: a^0 ~ 1e-3, not converged after ten steps
            out.append(rng.uniform(0.5, 3.0, D))
        out.append(np.full(D, 7.25))
        out.append(np.full(D, 0.3))
    return out


def worst_errors():
    wp = wt = wd = 0.0
    for r in spectra():
        ref = k_product64(r)
        kp, kt = k_product32(r).astype(np.float64), k_telescoped32(r).astype(np.float64)
        wp = max(wp, float(np.max(np.abs(kp - ref) / ref)))
        wt = max(wt, float(np.max(np.abs(kt - ref) / ref)))
        wd = max(wd, float(np.max(np.abs(kt - kp) / ref)))
    return wp, wt, wd


def test_factor_identity_in_fp64():
    """Every factor of the product is the quotient of consecutive pair sums -- the identity the telescoping rests on."""
    rng = np.random.default_rng(3)
    a = rng.uniform(1e-4, 1.0, 64)
    for _ in range(NS):
        an = 0.5 * a * (3.0 - a * a)
        f = 0.5 * (3.0 - a[:, None] ** 2 - a[None, :] ** 2 + a[:, None] * a[None, :])
        np.testing.assert_allclose(f, (an[:, None] + an[None, :]) / (a[:, None] + a[None, :]), rtol=1e-14)
        a = an


def test_telescoped_form_is_no_further_from_fp64_than_the_product():
    wp, wt, wd = worst_errors()
    print(f"worst relative error of K vs the fp64 product: product form {wp:.2e}, telescoped {wt:.2e}; between the two fp32 forms {wd:.2e}")
    assert wt <= wp, (wt, wp)
    assert wt < 1e-6  # a handful of roundings: a^0, ten steps of a^10 (contracting towards 1), two sums, the quotient, the scale


def test_iterates_stay_positive_and_denominators_nonzero():
    for r in spectra():
        its, aN, _ = iterates32(r)
        assert np.all(its[0] > 0) and np.all(aN > 0) and np.all(its[0] <= 1.0)
        assert np.all(np.isfinite(k_telescoped32(r)))


# ------------------------------------------------------------------------------------------------------------------ the kernel on the emulator
def relF(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("D", [12, 33])
def test_backward_cell_on_the_emulator_vs_oracle(emul, D):
    """One backward cell (NT = 1 with padded rows; NT = 2, one row past the first tile) against oracle/glad_exact.py's cell backward, at the
    tolerances of test_single_cell_d64_vs_oracle."""
    from uglad_amd import _lib
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    p = ex.params64(np.load(os.path.join(GOLDEN, "params_trained.npz")))
    pk = torch.tensor(np.concatenate([p[k].ravel() for k in ex.PARAM_KEYS]), dtype=torch.float32)
    S = torch.from_numpy(synthetic_covariance_batch(1, D, seed=70 + D).astype(np.float32))
    Z = torch.from_numpy(ex.init_theta(S.double().numpy(), float(p["theta_init_offset"][0]), 0).astype(np.float32))
    lam = torch.tensor([ex.lambda_nn(p, 1.0, 0.0)], dtype=torch.float32)
    for mode in ("ns10", "exact"):
        Zo, half, U = (torch.empty(1, D, D) for _ in range(3))
        beta, nf = torch.empty(1, D), torch.empty(1)
        emul.cell_fwd(S, Z, lam, pk, Zo, half, U, beta, nf, emul.workspace(1, D, S), _lib.SQRT_MODES[mode])
        # upstream gradient: the loss gradient at the oracle's own Z_next, symmetrised.  (Under a random G the terms of dL/dlam cancel, at D = 12
        # to 1e-5 of their absolute sum, and the relative tolerance below then measures the cancellation and not the kernel.)
        Zr = ex.cell_fwd(S.double().numpy(), Z.double().numpy(), float(lam), p, mode)[0]
        Gn = ex.loss_bwd(Zr, S.double().numpy())
        Gn = torch.from_numpy(np.ascontiguousarray(0.5 * (Gn + Gn.transpose(0, 2, 1)), dtype=np.float32))
        Go, grho, glam = torch.empty(1, D, D), torch.zeros(1, 28), torch.empty(1)
        emul.cell_bwd(Gn, S, Z, half, U, beta, lam, pk, Go, grho, glam, _lib.SQRT_MODES[mode])
        grads = {k: np.zeros_like(p[k]) for k in ex.PARAM_KEYS}
        Gr, glr = ex.cell_bwd(Gn.double().numpy(), S.double().numpy(), Z.double().numpy(), float(lam), p, grads, mode)
        assert torch.equal(Go, Go.transpose(1, 2)), mode
        assert relF(Go.numpy(), Gr) < 2e-5, mode
        assert abs(glam.item() - glr) < 1e-3 * abs(glr), mode
        ref_rho = np.concatenate([grads[k].ravel() for k in ex.PARAM_KEYS[1:7]])
        assert relF(grho.numpy()[0], ref_rho) < 1e-4, mode
