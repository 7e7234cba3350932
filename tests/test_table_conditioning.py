"""process_table's conditioning loop on the device: the ranking of highly correlated features (uglad_correlated_features,
csrc/corr_wide.h) and process_table / analyse_condition_number / get_highly_correlated_features with device=True
(uglad_amd/utils/prepare_data.py), which stand on uglad_table_spectrum (csrc/eigvals_wide.h; its eigenvalues are tested in
tests/test_eigvals_wide.py).  CPU: the unmodified kernel sources on the SIMT emulator.  GPU: the same checkers on the device, with
D = 288 added.

The ranking's oracle is the host get_highly_correlated_features, which restates the reference; its answer is integers, so the comparison
is exact.  That is legitimate only where a last-bit difference between the two Gram products cannot move the threshold: the sorted
|cov2| values around the threshold's place floor(0.1 n) must differ by more than 1e-9 relative (the products agree to about 1e-13).  The
seeds below were chosen so that this holds, and every case asserts it on the oracle's side.  The exact-tie case needs no such margin:
its matrix holds small integers and D = 64 is a power of two, so cov2 is exact in fp64 on both sides and full of equal magnitudes.

The goldens tests/golden/table_cond_*.npz were made by the reference's own process_table (tests/golden/make_table_goldens.py), with
margins: every eigenvalue of every round is < 1e-5 or > 1e-2 against eigval_th = 1e-3, and COND_NUM is 10 x away from every round's
condition number; both are asserted here on the recorded values."""
import os
import re

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


# ============================================================================================ 1. the ranking
RANK_SEEDS = {3: 0, 25: 0, 64: 0, 65: 0, 130: 0, 288: 0}


def collinear_covariance(D, seed):
    """The covariance of a table of N = 2 D rows: independent uniform columns, and about a tenth of the columns near-collinear combinations
    of two earlier ones (noise 1e-3)."""
    rng = np.random.default_rng(1000 * D + seed)
    X = rng.random((2 * D, D))
    for c in rng.choice(np.arange(2, D), size=max(D // 10, 1), replace=False) if D > 2 else []:
        a, b = rng.choice(c, size=2, replace=False)
        X[:, c] = rng.uniform(0.5, 1.0) * X[:, a] - rng.uniform(0.5, 1.0) * X[:, b] + 1e-3 * rng.standard_normal(2 * D)
    return np.cov(X.T, bias=1).reshape(D, D)


def ranking_oracle(S):
    """(list, counts (D,), the sorted magnitudes around the threshold's place) by the host restatement's own steps."""
    from uglad_amd.utils import prepare_data

    cov2 = prepare_data.empirical_covariance(S)
    np.fill_diagonal(cov2, 0.0)
    a = np.abs(cov2)
    upper = np.sort(a[np.triu_indices(len(S), 1)])[::-1]
    r = int(0.1 * len(upper))
    counts = (a >= upper[r]).sum(axis=1)
    return prepare_data.get_highly_correlated_features(S), counts, upper[max(r - 1, 0):r + 2]


def device_ranking(S):
    from uglad_amd import _lib

    order, counts, n_listed = _lib.get_lib().correlated_features(torch.from_numpy(np.array(S, dtype=np.float64)).to(_lib.device()))
    assert order.dtype == counts.dtype == n_listed.dtype == torch.int32
    return order.cpu().numpy(), counts.cpu().numpy(), n_listed.cpu().numpy()


def check_ranking(D):
    from uglad_amd.utils import prepare_data

    S = np.stack([collinear_covariance(D, RANK_SEEDS[D] + k) for k in range(2)])
    order, counts, n_listed = device_ranking(S)
    for k in range(2):
        want, want_counts, around = ranking_oracle(S[k])
        rel = np.abs(np.diff(around)) / around[:-1]
        print(f"D {D}[{k}]: {len(want)} features listed, the values around the threshold differ by {rel} relative")
        assert (rel > 1e-9).all(), "precondition: the threshold's neighbours are apart"
        assert n_listed[k] == len(want) and np.array_equal(order[k, :n_listed[k]], want)
        assert np.array_equal(counts[k], want_counts)
        assert sorted(order[k]) == list(range(D))  # a permutation: the features with count 0 behind the list
    solo = device_ranking(S[1:])  # K = 1: the bits of the slab in the batch
    assert np.array_equal(solo[0][0], order[1]) and np.array_equal(solo[1][0], counts[1])
    assert np.array_equal(prepare_data.get_highly_correlated_features(S[0], device=True), ranking_oracle(S[0])[0])


def check_exact_ties(D=64):
    """Small integers: cov2 is exact on both sides and holds many equal magnitudes; pins `>= th` and the tie rule (index ascending)."""
    rng = np.random.default_rng(64)
    B = rng.integers(0, 3, size=(2, D, D))
    S = (B + np.swapaxes(B, 1, 2)).astype(np.float64)
    S[1, :, 5] = S[1, :, 9]  # two identical columns: identical rows of cov2 but for their own places
    order, counts, n_listed = device_ranking(S)
    for k in range(2):
        want, want_counts, around = ranking_oracle(S[k])
        ties = int((want_counts[:, None] == want_counts[None, :]).sum() - D) // 2
        print(f"exact[{k}]: {len(want)} listed, {ties} pairs of equal counts, values around the threshold {around}")
        assert ties > 0
        assert n_listed[k] == len(want) and np.array_equal(order[k, :n_listed[k]], want) and np.array_equal(counts[k], want_counts)
    Z = np.zeros((1, 8, 8))  # th = 0: every entry counts, the zero diagonal too; every count ties
    order, counts, n_listed = device_ranking(Z)
    assert np.array_equal(counts[0], np.full(8, 8)) and np.array_equal(order[0], np.arange(8)) and n_listed[0] == 8
    assert np.array_equal(ranking_oracle(Z[0])[0], np.arange(8))


def check_ranking_c_entry(lib, device):
    import ctypes

    from uglad_amd._lib import UgladError

    size = lib._dll.uglad_correlated_features_workspace_floats
    assert size(1, 1) == -2 and size(1, 0) == -2 and size(1, 2049) == -2 and size(0, 8) == -2
    assert 0 < size(1, 2) <= size(1, 65) <= size(1, 2048) and size(2, 65) == 2 * size(1, 65)
    D = 8
    S = torch.eye(D, dtype=torch.float64, device=device)[None].contiguous()
    ints = [torch.zeros(n, dtype=torch.int32, device=device) for n in (D, D, 1)]
    wsp = torch.empty(size(1, D), dtype=torch.float32, device=device)
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(S_=S, o=ints[0], c=ints[1], n=ints[2], w=lib._p(wsp), D_=D):
        lib._call("uglad_correlated_features", vp(S_), 1, D_, vp(o), vp(c), vp(n), w)

    for kw in (dict(S_=None), dict(o=None), dict(c=None), dict(n=None), dict(w=None)):
        with pytest.raises(UgladError, match="NULL"):
            call(**kw)
    for bad in (0, 1, 2049):
        with pytest.raises(UgladError, match="dimension"):
            call(D_=bad)
    call()


@pytest.mark.parametrize("D", [3, 25, 64, 65, 130])
def test_emulated_ranking(emul, D):
    check_ranking(D)


def test_emulated_ranking_exact_ties(emul):
    check_exact_ties()


def test_emulated_ranking_c_entry(emul):
    check_ranking_c_entry(emul, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("D", [3, 25, 64, 65, 130, 288])
def test_gpu_ranking(D):
    check_ranking(D)


@pytest.mark.gpu
def test_gpu_ranking_exact_ties():
    check_exact_ties()


@pytest.mark.gpu
def test_gpu_ranking_c_entry():
    from uglad_amd import _lib

    check_ranking_c_entry(_lib.get_lib(), "cuda")


# ============================================================================================ 2. process_table(device=True)
def check_golden(name):
    import pandas as pd

    from uglad_amd.utils import prepare_data

    g = np.load(os.path.join(GOLDEN, f"table_cond_{name}.npz"))
    cond_num, th = float(g["cond_num"]), float(g["eigval_th"])
    con_ref, below_ref = g["round_con"], g["round_below"]
    # the margins the comparison relies on, on the recorded values
    assert (g["round_gap_lo"] < 1e-5).all() and (g["round_gap_hi"] > 1e-2).all() and th == 1e-3
    assert ((con_ref > 10 * cond_num) | (con_ref < cond_num / 10)).all() and con_ref[-1] < cond_num and len(con_ref) >= 2
    df = pd.DataFrame(g["table"].astype(np.float64))
    host_rounds, dev_rounds = [], []
    host = prepare_data.process_table(df.copy(), COND_NUM=cond_num, eigval_th=th, VERBOSE=False, rounds=host_rounds)
    dev = prepare_data.process_table(df.copy(), COND_NUM=cond_num, eigval_th=th, VERBOSE=False, device=True, rounds=dev_rounds)
    for r, (cols, con, below) in enumerate(dev_rounds):
        print(f"{name} round {r}: {cols} columns, con {con:.9e} (reference {con_ref[r] if r < len(con_ref) else float('nan'):.9e}), below {below}")
    assert dev.equals(host) and list(dev.columns) == list(g["kept"]) and dev.index.equals(host.index)
    assert len(dev_rounds) == len(host_rounds) == len(con_ref)
    for r, (cols, con, below) in enumerate(dev_rounds):
        assert cols == g["round_cols"][r] and below == below_ref[r]
        if con_ref[r] < 1e12:
            assert abs(con - con_ref[r]) <= 1e-6 * con_ref[r], (r, con, con_ref[r])
        else:
            assert con > cond_num and con_ref[r] > cond_num


def check_no_rounds(lib):
    """COND_NUM = inf: zero rounds, one spectrum call, no ranking; D = 2049: UgladError, and nothing falls back to the host."""
    from uglad_amd._lib import UgladError
    from uglad_amd.utils import prepare_data

    g = np.load(os.path.join(GOLDEN, "table_cond_n400_d96.npz"))
    table = g["table"].astype(np.float64)
    calls = {"spectrum": 0, "ranking": 0}
    spectrum, ranking = lib.table_spectrum, lib.correlated_features

    def counted_spectrum(*a, **kw):
        calls["spectrum"] += 1
        return spectrum(*a, **kw)

    def counted_ranking(*a, **kw):
        calls["ranking"] += 1
        return ranking(*a, **kw)

    lib.table_spectrum, lib.correlated_features = counted_spectrum, counted_ranking
    try:
        rounds = []
        dev = prepare_data.process_table(table, VERBOSE=False, device=True, rounds=rounds)
        assert calls == {"spectrum": 1, "ranking": 0} and len(rounds) == 1
        assert dev.equals(prepare_data.process_table(table, VERBOSE=False)) and dev.shape == table.shape
        assert abs(rounds[0][1] - g["round_con"][0]) <= 1e-6 * g["round_con"][0] and rounds[0][2] == g["round_below"][0]
        wide = np.random.default_rng(1).random((4, 2049))
        with pytest.raises(UgladError, match="2049 columns"):
            prepare_data.process_table(wide, VERBOSE=False, device=True)
        with pytest.raises(UgladError, match="2049 columns"):
            prepare_data.analyse_condition_number(wide, VERBOSE=False, device=True)
        assert calls == {"spectrum": 1, "ranking": 0}
        assert prepare_data.process_table(wide, VERBOSE=False).shape == (4, 2049)  # the host path takes it, as before
    finally:
        del lib.table_spectrum, lib.correlated_features


def check_verbose_text(capsys):
    """device=True prints the host path's lines; only the numbers' last digits may differ."""
    from uglad_amd.utils import prepare_data

    table = np.random.default_rng(2).random((30, 6))
    prepare_data.process_table(table, msg="t", VERBOSE=True)
    host = capsys.readouterr().out.splitlines()
    prepare_data.process_table(table, msg="t", VERBOSE=True, device=True)
    dev = capsys.readouterr().out.splitlines()
    strip = lambda line: re.sub(r"[-+]?\d+\.?\d*(e[-+]?\d+)?", "#", line)  # noqa: E731
    assert len(host) == len(dev) == 6 and [strip(a) for a in host] == [strip(b) for b in dev]


def test_emulated_process_table_golden(emul):
    check_golden("n400_d96")


def test_emulated_process_table_without_rounds_and_too_wide(emul):
    check_no_rounds(emul)


def test_emulated_process_table_prints_the_same_lines(emul, capsys):
    check_verbose_text(capsys)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n400_d96", "n900_d288"])
def test_gpu_process_table_golden(name):
    check_golden(name)


@pytest.mark.gpu
def test_gpu_process_table_without_rounds_and_too_wide():
    from uglad_amd import _lib

    check_no_rounds(_lib.get_lib())


@pytest.mark.gpu
def test_gpu_process_table_prints_the_same_lines(capsys):
    check_verbose_text(capsys)
