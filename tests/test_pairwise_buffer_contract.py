"""uglad_pairwise_covariance held to its buffers (buffer_contract.py: guard bands, three fills, four runs from the same inputs): every
optional output with the repair, none of them without it, and a batch with flagged tables -- on the SIMT emulator and on the GPU."""
import numpy as np
import pytest
import torch

import buffer_contract as bc
from buffer_contract_cases import Case, _lib, _t


def _tables(rng, K, N, D, p):
    X = rng.standard_normal((K, N, 3)) @ rng.standard_normal((3, D)) + rng.standard_normal((K, N, D)) + 50.0
    X[rng.random((K, N, D)) < p] = np.nan
    return X


def every_output(K, N, D, device):
    def call(inp):
        r = _lib().pairwise_covariance(inp["X"], normalize=True, min_pairs=2, eval_offset=0.1, repair=True, want_f64=True, want_counts=True)
        return r._asdict()

    return Case("pairwise_covariance", f"K{K}_N{N}_D{D}", lambda rng, dev: {"X": _t(_tables(rng, K, N, D, 0.2), dev)}, call, "all repair", device=device)


def no_optional_output(K, N, D, device):
    """S_out alone: S64_out, counts_out, info_out and min_eig_out NULL, through the C entry point (HipLib always asks for info)."""
    def call(inp):
        lib = _lib()
        X = inp["X"]
        wsp = lib._wide_workspace("uglad_pairwise_covariance", X.device, K, D)
        S = torch.empty(K, D, D, dtype=torch.float32, device=X.device)
        lib._call("uglad_pairwise_covariance", lib._vp(X), K, N, D, 0, 2, 0.1, lib._p(S), None, None, None, None, lib._p(wsp))
        return {"S": S}

    return Case("pairwise_covariance", f"K{K}_N{N}_D{D}", lambda rng, dev: {"X": _t(_tables(rng, K, N, D, 0.25), dev)}, call, "plain", device=device)


def flagged_batch(K, N, D, device):
    """An all-NaN column in the first table, a pair below min_pairs in the last, a clean table between them."""
    def make(rng, dev):
        X = _tables(rng, K, N, D, 0.1)
        X[0, :, D // 3] = np.nan
        X[K - 1, 0::2, 1] = np.nan
        X[K - 1, 1::2, D - 1] = np.nan
        return {"X": _t(X, dev)}

    def call(inp):
        r = _lib().pairwise_covariance(inp["X"], normalize=False, min_pairs=2, eval_offset=0.1, repair=True, want_f64=True, want_counts=True)
        return r._asdict()

    return Case("pairwise_covariance", f"K{K}_N{N}_D{D}", make, call, "all repair flagged", device=device)


def cases(device):
    return [every_output(2, 20, 40, device), no_optional_output(1, 30, 70, device), flagged_batch(3, 24, 40, device)]


EMULATED, GPU = cases("cpu"), cases("cuda")


def _check_tables(case):
    """The case is what its name says: the flagged batch has flags in its first and last table only (their min_eig NaN); every table of
    the other cases has min n_ij >= min_pairs = 2 and finite columns, so that a changed seed cannot turn them into flag cases unnoticed."""
    inputs = case.inputs()
    X = inputs["X"].cpu().numpy()
    seen = (~np.isnan(X)).astype(np.int64)
    clean = [int((seen[k].T @ seen[k]).min()) >= 2 and not np.isinf(X[k]).any() for k in range(len(X))]
    if "flagged" not in case.id:
        assert all(clean)
        return
    out = case.call(inputs)
    info, mn = out["info"].cpu().numpy(), out["min_eig"].cpu().numpy()
    assert clean == [False, True, False]
    assert info[0].any() and not info[1].any() and info[2].any() and np.isnan(mn[0]) and not np.isnan(mn[1]) and np.isnan(mn[2])


@pytest.mark.parametrize("case", EMULATED, ids=[c.id for c in EMULATED])
def test_emulated(emul, case):
    bc.run_case(case)
    _check_tables(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU, ids=[c.id for c in GPU])
def test_gpu(case):
    bc.run_case(case)
    _check_tables(case)
