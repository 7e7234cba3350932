"""Phase A of the backward cell with the rhoNN backward packed across pairs of entries (csrc/cell_bwd.h: rho_backward2 on the RhoAct2 of
rho_forward2, the 28 sums kept as pairs, masking by g_rho = 0 and weight 0 instead of a branch per entry), at the sizes that
tests/test_cell_bwd_entrywise.py does not reach (CASES).  The method is that file's: errors_of() there, against oracle/glad_exact.py in fp64, through
uglad_cell_bwd and uglad_glad_backward, with and without dL/dS, in modes ns10 and exact; it also asserts that two calls give identical outputs
and that dL/dZ is symmetric to the last bit.

The bound of every figure is TWICE the error that the commit before the packed phase A (rho_backward entry by entry) had against the same oracle
on the same inputs: tests/golden/cell_bwd_packed_parent_errors.json, measured with errors_of() below on an MI355X with that commit's library.
The two differ in the association of fp32 sums only (a thread's even and odd entries are summed apart and added once; multiply-adds fused
otherwise), so an error beyond twice the earlier one is a defect, not noise.

What holds exactly is checked exactly (uglad_cell_bwd, D = 128 and D = 33, M = 2): a matrix whose entries are all inactive has 28 rhoNN sums
of exactly 0 and leaves the other matrix's outputs what a launch of that matrix alone gives, bit for bit; dL/dZ equals its transpose; two
launches give the same bytes."""
import json
import os

import numpy as np
import pytest
import torch

import test_cell_bwd_entrywise as ew
from oracle import glad_exact as ex

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
# name: (D, M, L, wide mode)             what it reaches
CASES = {
    "d2": (2, 2, 3, -1),                 # one entry slot per thread: the single-entry "pair"
    "d64": (64, 2, 3, -1),               # NT = 2 with D = DP, 5 entry slots: odd
    "d65": (65, 2, 3, -1),               # NT = 3, 10 entry slots: even; 6 upper tiles
    "d96": (96, 2, 3, -1),               # NT = 3 with D = DP
    "d129": (129, 1, 3, 0),              # NT = 5, one workgroup per matrix: passes of eight entries, the last one short
    "d128_L5": (128, 3, 5, -1),          # the sums of five steps of one launch in registers; 10 upper tiles on 8 waves
}
MODES = ("ns10", "exact")


def errors_of(case, mode):
    """ew.errors_of() on this file's case: the same calls, oracle and error function, with this case's L."""
    D, M, L, wide = CASES[case]
    saved = ew.L, ew.CASES
    ew.L, ew.CASES = L, {case: (D, M, wide, False)}
    try:
        return ew.errors_of(case, mode)
    finally:
        ew.L, ew.CASES = saved


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_packed_phase_a_within_twice_the_parent_error(case, mode):
    parent = json.load(open(os.path.join(GOLDEN, "cell_bwd_packed_parent_errors.json")))["errors"][f"{case}/{mode}"]
    err = errors_of(case, mode)
    assert set(err) == set(parent)
    for k in sorted(err):
        print(f"{case} {mode} {k}: error {err[k]:.3e}, parent {parent[k]:.3e}")
    for k in sorted(err):
        assert err[k] <= 2.0 * parent[k], (case, mode, k, err[k], parent[k])


_step = {}


def last_step(D):
    """The inputs of the last step's uglad_cell_bwd for M = 2 matrices (forward pass of L = 2 on the device), computed once per D."""
    if D in _step:
        return _step[D]
    from uglad_amd import _lib

    M, L = 2, 2
    lib, dev = _lib.get_lib(), _lib.device()
    f32 = dict(dtype=torch.float32, device=dev)
    p = ex.params64(np.load(os.path.join(GOLDEN, "params_trained.npz")))
    params = torch.tensor(np.concatenate([p[k].ravel() for k in ex.PARAM_KEYS]), **f32)
    S = torch.from_numpy(ew.inputs(D, M, False).astype(np.float32)).to(dev)
    wsp = lib.workspace(M, D, S)
    Z, half, U = torch.empty(L + 1, M, D, D, **f32), torch.empty(L, M, D, D, **f32), torch.empty(L, M, D, D, **f32)
    beta, lam, lam_in = torch.empty(L, M, D, **f32), torch.empty(L + 1, **f32), torch.empty(L + 1, 2, **f32)
    lib.glad_forward(S, params, 1.0, 0, L, Z, half, U, beta, lam, lam_in, torch.empty(M, **f32), torch.empty(1, **f32), wsp, 1)
    G = torch.randn(M, D, D, generator=torch.Generator(device="cpu").manual_seed(3)).to(dev)
    G = (G + G.transpose(1, 2)).contiguous()
    _step[D] = dict(G=G, S=S, Z=Z[L - 1].contiguous(), half=half[L - 1].contiguous(), U=U[L - 1].contiguous(), beta=beta[L - 1].contiguous(),
                    lam=lam[L - 1:L].contiguous(), params=params)
    return _step[D]


def cell_bwd(t, half, rows=slice(None)):
    """uglad_cell_bwd (ns10) on the matrices `rows` of the step's inputs: G_out, the 28 rhoNN sums per matrix, dL/dlam per matrix."""
    from uglad_amd import _lib

    lib = _lib.get_lib()
    a = {k: t[k][rows].contiguous() for k in ("G", "S", "Z", "U", "beta")}
    half = half[rows].contiguous()
    M, D, _ = a["S"].shape
    f32 = dict(dtype=torch.float32, device=a["S"].device)
    Go, grp, glp = torch.empty(M, D, D, **f32), torch.zeros(M, _lib.NRHO, **f32), torch.empty(M, **f32)
    lib.cell_bwd(a["G"], a["S"], a["Z"], half, a["U"], a["beta"], t["lam"], t["params"], Go, grp, glp, 1, workspace=lib.workspace(M, D, a["S"]))
    return Go.cpu(), grp.cpu(), glp.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("D", (128, 33))
def test_all_entries_inactive_adds_exact_zeros(D):
    t = last_step(D)
    half = t["half"].clone()
    half[0] = 0.0  # |x| > rho never holds: every entry of matrix 0 is inactive
    Go, grp, glp = cell_bwd(t, half)
    assert torch.isfinite(Go).all() and torch.isfinite(glp).all()
    assert torch.equal(grp[0], torch.zeros(grp.shape[1])), grp[0]
    Go1, grp1, glp1 = cell_bwd(t, half, slice(1, 2))
    assert torch.equal(Go[1], Go1[0]) and torch.equal(grp[1], grp1[0]) and torch.equal(glp[1], glp1[0])
    assert grp[1].abs().max() > 0  # (the other matrix does have active entries)


@pytest.mark.gpu
@pytest.mark.parametrize("D", (128, 33))
def test_g_out_is_symmetric_and_two_launches_agree(D):
    t = last_step(D)
    a, b = cell_bwd(t, t["half"]), cell_bwd(t, t["half"])
    assert torch.equal(a[0], a[0].transpose(1, 2))
    for x, y in zip(a, b):
        assert x.numpy().tobytes() == y.numpy().tobytes()
