"""The entrywise phases of the backward cell (csrc/cell_bwd.h, the kEpiDivDiff epilogue of csrc/wide_bwd.h) on the GPU against the fp64 oracle:
uglad_cell_bwd (one step) and uglad_glad_backward (L = 3: every step of the pass in one launch for D <= 128, so whatever a workgroup sets up before
its step loop has to hold for all of them), with and without dL/dS (cell_bwd_gs_kernel / cell_bwd_kernel), square-root modes ns10 and exact, at the
smallest sizes that reach each instantiation and path (CASES).

The bound of every output is TWICE the error that the commit before the NS10 divided difference became one quotient (glad_device.h:
ns_divided_difference) had against the same oracle on the same inputs: tests/golden/cell_bwd_entrywise_parent_errors.json, measured with this
file's errors_of() on an MI355X with that commit's library.  The two differ by the fp32 rounding of K_ij only (<= 1e-6 relative, and the quotient is
the more accurate form: tests/test_ns_divided_difference.py), so an error beyond twice the earlier one is a defect, not noise."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import glad_exact as ex
from oracle import glad_ns as ns

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
L = 3
# name: (D, M, wide mode, graded)        what it reaches
CASES = {
    "d3": (3, 2, -1, False),            # NT = 1, most of a thread's entry slots empty
    "d33": (33, 3, -1, False),          # NT = 2, padded rows
    "d128": (128, 2, -1, False),        # NT = 4, the benchmark's instantiation: D = DP, every slot of the last full pass taken
    "d127": (127, 2, -1, False),        # D < DP at NT = 4
    "d160_one_workgroup": (160, 1, 0, False),  # big matrices in the workspace, one workgroup per matrix
    "d160_wide": (160, 1, 1, False),    # many workgroups per matrix: the tile epilogue of wide_bwd.h
    "d33_graded": (33, 1, -1, True),    # one eigenvalue of S about 1e3 times the rest
}
MODES = ("ns10", "exact")
_cache = {}


def relF(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def inputs(D, M, graded):
    from uglad_amd.utils.prepare_data import synthetic_covariance_batch

    if not graded:
        return synthetic_covariance_batch(M, D, seed=90 + D).astype(np.float64)
    rng = np.random.default_rng(7)
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    w = rng.uniform(0.05, 0.1, D)
    w[-1] = 1e3 * w[:-1].mean()
    S = (Q * w) @ Q.T
    return (0.5 * (S + S.T))[None].astype(np.float32).astype(np.float64)


def oracle_pass(S64, p, mode):
    """The fp64 pass, step by step: dL/dZ_0, the six rhoNN gradient blocks as 28 numbers, dL/dlam of every (step, matrix); and the same for
    the last step alone.  G_L is the oracle's own loss gradient at its Theta_L."""
    M = S64.shape[0]
    _, tr = ex.glad_forward(S64, p, L, 0, mode=mode)
    G_L = ex.loss_bwd(tr["theta_L"], S64)
    G_L = 0.5 * (G_L + G_L.transpose(0, 2, 1))  # (symmetric to the last bit, also after rounding to fp32)
    grads = {k: np.zeros_like(p[k]) for k in ex.PARAM_KEYS}
    glam = np.zeros((L, M))
    G, one = G_L, None
    for k in range(L - 1, -1, -1):
        Gk = np.empty_like(G)
        for m in range(M):
            Gk[m:m + 1], glam[k, m] = ex.cell_bwd(G[m:m + 1], S64[m:m + 1], tr["Z_in"][k][m:m + 1], tr["lambdas"][k], p, grads, mode)
        G = Gk
        if one is None:
            one = dict(G_out=G.copy(), grad_rho=np.concatenate([grads[q].ravel() for q in ex.PARAM_KEYS[1:7]]), glam=glam[k].copy())
    full = dict(G_out=G, grad_rho=np.concatenate([grads[q].ravel() for q in ex.PARAM_KEYS[1:7]]), glam=glam)
    return G_L, one, full


def oracle_gs(S64, p, G_L):
    """sym(d <G_L, Theta_L(S)> / dS) of the NS-faithful fp64 oracle (ns10 only: oracle/glad_ns.py is the reference's own iteration)."""
    St = torch.tensor(S64, dtype=torch.float64, requires_grad=True)
    p64 = {k: torch.tensor(p[k], dtype=torch.float64) for k in ns.PARAM_KEYS}
    (ns.glad(St, p64, L=L, INIT_DIAG=0) * torch.as_tensor(G_L)).sum().backward()
    g = St.grad.numpy()
    return 0.5 * (g + g.transpose(0, 2, 1))


def errors_of(case, mode):
    """Every output's relative Frobenius error against the oracle: {"<call>/<output>": error}.  Also asserts what holds exactly: every output
    identical between two calls, dL/dZ symmetric (with many workgroups per matrix it is symmetric to rounding only: there the relative
    asymmetry is one more figure, bounded like the errors).  Computed once per (case, mode)."""
    if (case, mode) in _cache:
        return _cache[case, mode]
    from uglad_amd import _lib

    D, M, wide, graded = CASES[case]
    lib, dev = _lib.get_lib(), _lib.device()
    f32 = dict(dtype=torch.float32, device=dev)
    p = ex.params64(np.load(os.path.join(GOLDEN, "params_trained.npz")))
    params = torch.tensor(np.concatenate([p[k].ravel() for k in ex.PARAM_KEYS]), **f32)
    S64 = inputs(D, M, graded)
    S = torch.from_numpy(S64.astype(np.float32)).to(dev)
    G_L64, ref_one, ref_full = oracle_pass(S64, p, mode)
    G_L = torch.from_numpy(np.ascontiguousarray(G_L64, dtype=np.float32)).to(dev)
    sq = _lib.SQRT_MODES[mode]
    err = {}
    lib.set_wide_mode(wide)
    lib.set_matrix_iteration(0)  # (a single matrix of 128 < D <= 256 would otherwise leave the spectral path)
    try:
        wsp = lib.workspace(M, D, S)
        Z, half, U = torch.empty(L + 1, M, D, D, **f32), torch.empty(L, M, D, D, **f32), torch.empty(L, M, D, D, **f32)
        beta, lam, lam_in = torch.empty(L, M, D, **f32), torch.empty(L + 1, **f32), torch.empty(L + 1, 2, **f32)
        lib.glad_forward(S, params, 1.0, 0, L, Z, half, U, beta, lam, lam_in, torch.empty(M, **f32), torch.empty(1, **f32), wsp, sq)

        def one_step():
            Go, grp, glp = torch.empty(M, D, D, **f32), torch.zeros(M, _lib.NRHO, **f32), torch.empty(M, **f32)
            lib.cell_bwd(G_L, S, Z[L - 1], half[L - 1], U[L - 1], beta[L - 1], lam[L - 1:L], params, Go, grp, glp, sq, workspace=wsp)
            return dict(G_out=Go.cpu(), grad_rho=grp.sum(0).cpu(), glam=glp.cpu())

        def whole_pass(with_gs):
            bufs = (torch.zeros(M, D, D, **f32), torch.zeros(M, D, D, **f32))
            grp, glp, gtp = torch.empty(M, _lib.NRHO, **f32), torch.empty(L, M, **f32), torch.empty(M, **f32)
            grad = torch.empty(_lib.NPARAM, **f32)
            gS = torch.empty(M, D, D, **f32) if with_gs else None
            lib.glad_backward(G_L, S, params, 0, L, Z, half, U, beta, lam, lam_in, bufs[0], bufs[1], grp, glp, gtp, grad, wsp, sq, gS=gS)
            out = dict(G_out=bufs[0].cpu(), grad_rho=grp.sum(0).cpu(), glam=glp.cpu())  # (dL/dZ_0 ends up in the first buffer on every route)
            if with_gs:
                out["gS"] = gS.cpu()
            return out

        for call, run, ref in (("cell_bwd", one_step, ref_one), ("glad_backward", lambda: whole_pass(False), ref_full),
                               ("glad_backward_gs", lambda: whole_pass(True), ref_full)):
            a, b = run(), run()
            for k in a:
                assert torch.equal(a[k], b[k]), f"{case} {mode} {call}: {k} differs between two calls"
            if wide == 1:  # one workgroup per tile: (i, j) and (j, i) are computed apart and agree to rounding only, here and before this change
                err[f"{call}/G_out_asymmetry"] = relF(a["G_out"].numpy(), a["G_out"].transpose(1, 2).numpy())
            else:  # one workgroup per matrix: every entry of the upper triangle is stored twice
                assert torch.equal(a["G_out"], a["G_out"].transpose(1, 2)), f"{case} {mode} {call}: dL/dZ is not symmetric"
            for k in ("G_out", "grad_rho", "glam"):
                err[f"{call}/{k}"] = relF(a[k].numpy(), ref[k])
            if "gS" in a:
                assert torch.equal(a["gS"], a["gS"].transpose(1, 2)), f"{case} {mode}: dL/dS is not symmetric"
                if mode == "ns10":  # (the only oracle of dL/dS, oracle/glad_ns.py, is the reference's own iteration: there is no exact mode of it)
                    err[f"{call}/gS"] = relF(a["gS"].numpy(), oracle_gs(S64, p, G_L64))
    finally:
        lib.set_wide_mode(-1)
        lib.set_matrix_iteration(-1)
    _cache[case, mode] = err
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_backward_entrywise_within_twice_the_parent_error(case, mode):
    parent = json.load(open(os.path.join(GOLDEN, "cell_bwd_entrywise_parent_errors.json")))["errors"][f"{case}/{mode}"]
    err = errors_of(case, mode)
    assert set(err) == set(parent)
    for k in sorted(err):
        print(f"{case} {mode} {k}: error {err[k]:.3e}, parent {parent[k]:.3e}")
    for k in sorted(err):
        assert err[k] <= 2.0 * parent[k], (case, mode, k, err[k], parent[k])
