"""The association matrix of a table that mixes categorical and real columns (uglad_association, csrc/assoc_wide.h; the host layer in
uglad_amd/utils/prepare_data.py), against goldens made by the real reference (tests/golden/make_assoc_goldens.py: pairwise_cov_matrix,
the eigvals minimum and the repair of get_covariance).  CPU: the host formulation, and the unmodified kernel sources on the SIMT
emulator.  GPU: the same goldens (with the D = 288 one, which the emulator would take minutes for), a grid of 33 tiles, fit_mixed.

Tolerances, none of them measured on the code under test:
  entries   BOUND = 256 x the largest d_ref of tests/golden/assoc_deviation.json, d_ref = the deviation of the package's host
            formulation from the reference as the generator measured it (device and host formulation differ in summation order only;
            256 is the multiple the reference's own rounding is given).  Entries of r/r pairs are compared directly, the SQUARES of the
            entries that involve a categorical: V and eta are square roots of quantities that may sit at a max(0, .) clamp, where an
            error e in the radicand is sqrt(e) in the root.  BOUND must stay below 1e-12.
  min eig   |device - reference| <= ||A||_inf 2^-40 (the bisection's bracket ends at ||A||_inf 2^-48).
  fp32      every entry of the fp32 output within one fp32 ulp of the float32 rounding of the golden's repaired matrix."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from uglad_amd.utils import prepare_data as pd_

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ["n97_d12", "n400_d40", "n300_d288", "allreal_n200_d20"]
with open(os.path.join(GOLDEN, "assoc_deviation.json")) as _f:
    DEVIATION = json.load(_f)
BOUND = 256 * max(v["d_ref"] for v in DEVIATION.values())

_cache = {}


def golden(name):
    """(table fp64, kinds, cards, names, A, min eig, offset, repaired) of a golden, loaded once and never modified."""
    if name not in _cache:
        g = np.load(os.path.join(GOLDEN, f"assoc_{name}.npz"))
        D = g["cards"].shape[0]
        iu = np.triu_indices(D)
        A = np.zeros((D, D))
        A[iu] = g["A_triu"]
        A.T[iu] = g["A_triu"]
        R = A.copy()
        R[np.diag_indices(D)] = g["repaired_diag"]
        out = (g["table"].astype(np.float64), g["kinds"], g["cards"], [str(n) for n in g["names"]], A, float(g["min_eig"]),
               float(g["offset"]), R)
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = out
    return _cache[name]


def frame(table, kinds, names=None):
    import pandas as pd

    names = names or [f"f{i}" for i in range(table.shape[1])]
    df = pd.DataFrame({n: (table[:, i].astype(np.int64) if kinds[i] == "c" else table[:, i]) for i, n in enumerate(names)})
    return df, dict(zip(names, kinds))


def deviation(A, ref, kinds):
    """max |A - ref| over the r/r entries and max |A^2 - ref^2| over the entries that involve a categorical."""
    kinds = np.asarray(kinds)
    anycat = (kinds[:, None] == "c") | (kinds[None, :] == "c")
    return float(np.abs(np.where(anycat, A * A, A) - np.where(anycat, ref * ref, ref)).max())


def run(lib, tables, maps, device, **kw):
    A, mn, A64 = lib.association(torch.from_numpy(np.array(tables, dtype=np.float64)).to(device), maps, **kw)
    if device != "cpu":
        torch.cuda.synchronize()
    return A.cpu().numpy(), None if mn is None else mn.cpu().numpy(), None if A64 is None else A64.cpu().numpy()


def check_golden(lib, name, device):
    """A golden through the device entry: the fp64 matrix, the repair's eigenvalue and the fp32 output, under the rules above."""
    table, kinds, cards, names, A, min_eig, offset, R = golden(name)
    maps = pd_._expanded_layout(names, kinds, cards)
    Af, mn, A64 = run(lib, table[None], maps, device, eval_offset=offset, repair=True, want_f64=True)
    dev = deviation(A64[0], A, kinds)
    norm = float(np.abs(A).sum(axis=1).max())
    print(f"{name}: W {maps.W}; deviation from the reference {dev:.2e} (bound {BOUND:.2e}); min eig {min_eig!r}, device {mn[0]!r}, "
          f"bound {norm * 2.0 ** -40:.2e}")
    assert np.array_equal(A64[0], A64[0].T) and np.array_equal(Af[0], Af[0].T)  # the mirror is a copy
    assert dev <= BOUND
    if min_eig <= 1e-6:
        assert abs(mn[0] - min_eig) <= norm * 2.0 ** -40
    else:
        assert np.isposinf(mn[0])  # passed the test at 1e-6: never computed, not repaired
        assert np.array_equal(Af[0], A64[0].astype(np.float32))
    R32 = R.astype(np.float32)
    assert (np.abs(Af[0].astype(np.float64) - R32.astype(np.float64)) <= np.spacing(np.abs(R32)).astype(np.float64)).all()


# ============================================================================================ synthetic tables at the shapes that matter
def synthetic(N, cards, seed, K=1):
    """(K, N, D) encoded tables, column i categorical with cards[i] levels (0: real), every column tied to a shared latent factor."""
    rng = np.random.default_rng(seed)
    cards = np.asarray(cards)
    out = np.empty((K, N, len(cards)))
    for k in range(K):
        lat = rng.standard_normal(N)
        for i, c in enumerate(cards):
            v = lat * rng.uniform(0.2, 1.0) + rng.standard_normal(N)
            if c:  # quantile cuts of its own values: every level occurs
                out[k, :, i] = np.digitize(v, np.quantile(v, np.linspace(0, 1, c + 1)[1:-1]))
            else:
                out[k, :, i] = v * rng.uniform(0.5, 20.0) + rng.uniform(-5, 5)
    return out, np.where(cards > 0, "c", "r"), cards.astype(np.int32)


SHAPES = {
    # W < 64: r/r, c/r and c/c pairs in one diagonal tile, two binary columns (their pair is 2 x 2: Yates); N ragged against the 32-row chunks
    "one_tile": (45, [2, 0, 5, 2, 0, 3, 0]),
    # a categorical of exactly 64 levels fills tile 0; the rest lands in tile 1, its pairs with the first in the off-diagonal tile (0, 1)
    "full_tile_64_levels": (150, [64, 0, 3, 2, 0, 2]),
    # 40 + 30 levels would straddle column 64: the second categorical starts at 64 (24 padding columns in the middle of the layout)
    "forced_padding": (77, [40, 30, 0, 2, 0, 7]),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_emulated_shapes_match_the_host_formulation(emul, shape):
    N, cards = SHAPES[shape]
    tables, kinds, cards = synthetic(N, cards, seed=len(shape))
    df, dtype = frame(tables[0], kinds)
    enc, maps = pd_.encode_mixed_table(df, dtype)
    if shape == "one_tile":
        assert maps.W == 64 and list(maps.tile_first) == [0, 7]
    if shape == "full_tile_64_levels":
        assert maps.W == 128 and list(maps.feat_offset[:2]) == [0, 64] and list(maps.tile_first) == [0, 1, 6]
    if shape == "forced_padding":
        assert list(maps.feat_offset[:3]) == [0, 64, 94] and (maps.col_level[40:64] == pd_.ASSOC_PAD).all() and maps.W == 128
    assert all(o // 64 == (o + w - 1) // 64 for o, w in zip(maps.feat_offset, maps.feat_width))  # the layout rule
    host = np.array(pd_.pairwise_cov_matrix(df, dtype))
    Af, mn, A64 = run(emul, enc[None], maps, "cpu", repair=False, want_f64=True)
    assert mn is None and np.array_equal(A64[0], A64[0].T)
    dev = deviation(A64[0], host, kinds)
    print(f"{shape}: deviation from the host formulation {dev:.2e} (bound {BOUND:.2e})")
    assert dev <= BOUND
    assert np.array_equal(Af[0], A64[0].astype(np.float32))


def two_tables_one_without_a_level():
    """K = 2 tables under one layout; table 1 has no row at level 2 of column 0 (5 levels) nor at level 1 of column 3 (3 levels), so the
    numbers of rows and columns of their contingency tables differ between the tables -- and the pair (3, 5) is 2 x 2 in table 1 only."""
    tables, kinds, cards = synthetic(83, [5, 0, 4, 3, 0, 2], seed=7, K=2)
    t1 = tables[1]
    t1[t1[:, 0] == 2, 0] = 3
    t1[t1[:, 3] == 1, 3] = 0
    return tables, kinds, cards


def check_two_tables(lib, device):
    tables, kinds, cards = two_tables_one_without_a_level()
    maps = pd_._expanded_layout([f"f{i}" for i in range(len(cards))], kinds, cards)
    _, _, A64 = run(lib, tables, maps, device, repair=False, want_f64=True)
    for k in range(2):
        df, dtype = frame(tables[k], kinds)
        host = np.array(pd_.pairwise_cov_matrix(df, dtype))  # (its own encoding of this table alone: the empty levels do not exist)
        dev = deviation(A64[k], host, kinds)
        print(f"table {k}: deviation from the host formulation run on it alone {dev:.2e} (bound {BOUND:.2e})")
        assert dev <= BOUND
    assert not np.array_equal(A64[0], A64[1])


def test_emulated_two_tables_one_without_a_level(emul):
    check_two_tables(emul, "cpu")


# ============================================================================================ CPU: host formulation, goldens on the emulator
def test_bound_is_derived_and_goldens_are_small():
    assert sorted(DEVIATION) == sorted(NAMES)
    assert BOUND < 1e-12
    for name in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, f"assoc_{name}.npz")) < 1 << 20
    _, kinds, cards, *_ = golden("n97_d12")
    assert (cards == 2).sum() == 2  # two binary columns
    assert all(golden(n)[5] <= 1e-6 for n in NAMES[:3]) and golden(NAMES[3])[5] > 1e-6 and (golden(NAMES[3])[1] == "r").all()


@pytest.mark.parametrize("name", NAMES)
def test_host_formulation_matches_the_reference_goldens(name):
    import pandas as pd

    table, kinds, cards, names, A, *_ = golden(name)
    df, dtype = frame(table, kinds, names)
    out = pd_.pairwise_cov_matrix(df, dtype)
    assert isinstance(out, pd.DataFrame) and list(out.index) == names and list(out.columns) == names
    dev = deviation(np.array(out), A, kinds)
    print(f"{name}: host formulation, deviation from the reference {dev:.2e} (bound {BOUND:.2e})")
    assert dev <= BOUND
    enc, maps = pd_.encode_mixed_table(df, dtype)
    assert np.array_equal(enc, table) and np.array_equal(maps.cards, cards) and maps.W == DEVIATION[name]["W"]


def test_cramers_v_and_correlation_ratio_match_golden_entries():
    table, kinds, cards, names, A, *_ = golden("n97_d12")
    cat, real = np.nonzero(kinds == "c")[0], np.nonzero(kinds == "r")[0]
    binary = [i for i in cat if cards[i] == 2]
    pairs_cc = [(binary[0], binary[1]), (cat[0], cat[-1]), (cat[1], cat[1])]  # the 2 x 2 pair, a larger one, a diagonal entry
    for i, j in pairs_cc:
        v = pd_.cramers_v(table[:, i].astype(int), table[:, j].astype(int))
        assert isinstance(v, float) and abs(v * v - A[i, j] ** 2) <= BOUND
    assert A[binary[0], binary[0]] < 1.0  # the diagonal goes through the same formula: below 1 for a binary column
    for i, j in [(cat[0], real[0]), (cat[-1], real[-1])]:
        e = pd_.correlation_ratio(table[:, i].astype(int), table[:, j])
        assert isinstance(e, float) and abs(e * e - A[i, j] ** 2) <= BOUND


@pytest.mark.parametrize("name", ["n97_d12", "n400_d40", "allreal_n200_d20"])
def test_emulated_goldens_matrix_repair_and_fp32_output(emul, name):
    check_golden(emul, name, "cpu")


# ============================================================================================ arguments and host-side checks
def test_encode_mixed_table_refuses_what_the_device_cannot_take():
    import pandas as pd

    n = 130
    base = pd.DataFrame({"a": np.arange(n) % 3, "x": np.linspace(0.0, 1.0, n)})
    ok = {"a": "c", "x": "r"}
    pd_.encode_mixed_table(base, ok)
    with pytest.raises(ValueError, match="'wide'"):
        pd_.encode_mixed_table(base.assign(wide=np.arange(n) % 65), {**ok, "wide": "c"})
    pd_.encode_mixed_table(base.assign(wide=np.arange(n) % 64), {**ok, "wide": "c"})  # 64 levels are taken
    with pytest.raises(ValueError, match="'one'"):
        pd_.encode_mixed_table(base.assign(one="k"), {**ok, "one": "c"})
    with pytest.raises(ValueError, match="'flat'"):
        pd_.encode_mixed_table(base.assign(flat=2.5), {**ok, "flat": "r"})
    with pytest.raises(ValueError, match="'gap'"):
        pd_.encode_mixed_table(base.assign(gap=np.where(np.arange(n) == 5, None, "u")), {**ok, "gap": "c"})
    with pytest.raises(ValueError, match="'x'"):
        pd_.encode_mixed_table(base, {"a": "c", "x": "n"})
    many = pd.DataFrame(np.arange(2 * (pd_.ASSOC_MAX_DIM + 1), dtype=np.float64).reshape(2, -1))
    with pytest.raises(ValueError, match=str(pd_.ASSOC_MAX_DIM)):
        pd_.encode_mixed_table(many, {c: "r" for c in many.columns})
    levels64 = pd.DataFrame({f"c{i}": np.roll(np.arange(64), i) for i in range(pd_.ASSOC_MAX_WIDTH // 64 + 1)})
    with pytest.raises(ValueError, match=str(pd_.ASSOC_MAX_WIDTH)):
        pd_.encode_mixed_table(levels64, {c: "c" for c in levels64.columns})


def test_emulated_c_entry_error_codes(emul):
    from uglad_amd._lib import UgladError

    dll = emul._dll
    assert dll.uglad_association_max_width() == pd_.ASSOC_MAX_WIDTH == 16384 and emul.max_dim == pd_.ASSOC_MAX_DIM
    size = dll.uglad_association_workspace_floats
    assert size(1, 12, 64) == 2 * (2 * 64 * 64 + 3 * 64 + 8 + 2 * 64)
    assert size(1, 1, 64) == -2 and size(1, 12, 16384 + 64) == -2 and size(1, 12, 100) == -2 and size(0, 12, 64) == -2
    assert size(1, emul.max_dim + 1, 4096) == -2 and size(1, 100, 64) == -2
    assert size(200, 2048, 16384) == -2  # beyond 2^31 - 1 floats
    table, kinds, cards, names, *_ = golden("n97_d12")
    maps = pd_._expanded_layout(names, kinds, cards)
    N, D = table.shape
    X = torch.from_numpy(table.copy())
    ints = [torch.from_numpy(np.ascontiguousarray(a)) for a in (maps.col_feature, maps.col_level, maps.feat_offset, maps.feat_width, maps.tile_first)]
    A = torch.empty(1, D, D)
    wsp = torch.empty(size(1, D, maps.W) + 2, dtype=torch.float32)
    assert wsp.data_ptr() % 8 == 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(table_p=p(X), D_=D, W_=maps.W, A_p=p(A), wsp_p=p(wsp), maps_p=None, N_=N):
        mp = maps_p or [p(a) for a in ints]
        emul._call("uglad_association", table_p, 1, N_, D_, *mp, W_, 0.1, A_p, None, None, wsp_p)

    call()  # (the arguments are good)
    with pytest.raises(UgladError, match="NULL"):
        call(table_p=None)
    with pytest.raises(UgladError, match="NULL"):
        call(A_p=None)
    with pytest.raises(UgladError, match="NULL"):
        call(maps_p=[p(a) for a in ints[:4]] + [None])
    with pytest.raises(UgladError, match="NULL"):
        call(wsp_p=ctypes.c_void_p(wsp.data_ptr() + 4))  # misaligned
    with pytest.raises(UgladError, match="dimension"):
        call(D_=1)
    with pytest.raises(UgladError, match="dimension"):
        call(W_=pd_.ASSOC_MAX_WIDTH + 64)
    with pytest.raises(UgladError, match="dimension"):
        call(N_=1)
    with pytest.raises(UgladError):
        emul.association(torch.zeros(1, 4, D), maps)  # fp32 tables are refused


def test_emulated_nan_in_a_real_column_stays_in_its_row_and_column(emul):
    table, kinds, cards, names, *_ = golden("n97_d12")
    maps = pd_._expanded_layout(names, kinds, cards)
    clean, _, _ = run(emul, table[None], maps, "cpu", repair=False)
    j = int(np.nonzero(kinds == "r")[0][1])
    bad = table.copy()
    bad[11, j] = np.nan
    A, _, _ = run(emul, bad[None], maps, "cpu", repair=False)
    assert np.isnan(A[0, j, :]).all() and np.isnan(A[0, :, j]).all()
    keep = np.ones(len(kinds), dtype=bool)
    keep[j] = False
    assert np.array_equal(A[0][np.ix_(keep, keep)], clean[0][np.ix_(keep, keep)])


# ============================================================================================ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_goldens_matrix_repair_and_fp32_output(name):
    from uglad_amd import _lib

    check_golden(_lib.get_lib(), name, "cuda")


@pytest.mark.gpu
def test_gpu_two_tables_one_without_a_level():
    from uglad_amd import _lib

    check_two_tables(_lib.get_lib(), "cuda")


@pytest.mark.gpu
def test_gpu_33_tiles_of_expanded_width_match_the_host_formulation():
    """W = 2112: 561 tile pairs per table, a grid beyond the goldens' (W = 1152).  Every tile holds 9 categoricals (12 .. 2 levels) and 12
    real columns, 64 expanded columns exactly."""
    from uglad_amd import _lib

    tables, kinds, cards = synthetic(150, ([12, 10, 8, 6, 5, 4, 3, 2, 2] + [0] * 12) * 33, seed=5)
    df, dtype = frame(tables[0], kinds)
    enc, maps = pd_.encode_mixed_table(df, dtype)
    assert maps.W == 2112 and len(cards) == 693
    host = np.array(pd_.pairwise_cov_matrix(df, dtype))
    Af, _, A64 = run(_lib.get_lib(), enc[None], maps, "cuda", repair=False, want_f64=True)
    dev = deviation(A64[0], host, kinds)
    print(f"W 2112: deviation from the host formulation {dev:.2e} (bound {BOUND:.2e})")
    assert np.array_equal(A64[0], A64[0].T) and dev <= BOUND
    assert np.array_equal(Af[0], A64[0].astype(np.float32))


@pytest.mark.gpu
def test_gpu_fit_mixed_trains_on_the_repaired_association_matrix(tmp_path):
    import uglad_amd
    from uglad_amd import main

    FIT_TOL = 1e-4  # relative Frobenius, the project's contract for a fit (tests/test_gpu_parity.py)
    table, kinds, cards, names, A, min_eig, offset, R = golden("n97_d12")
    df, dtype = frame(table, kinds, names)
    Ad, mn = uglad_amd.mixed_association(df, dtype, repair=True, eval_offset=offset)
    assert Ad.is_cuda and Ad.dtype == torch.float32 and abs(mn - min_eig) <= np.abs(A).sum(axis=1).max() * 2.0 ** -40
    torch.manual_seed(0)
    est = uglad_amd.uGLAD_GL()
    est.fit_mixed(df, dtype, eval_offset=offset, epochs=20, L=6, verbose=False)
    P = est.precision_
    assert P.shape == (12, 12) and np.isfinite(P).all()
    assert np.abs(P - P.T).max() <= 2.0 ** -20 * np.abs(P).max()  # symmetric to fp32 rounding
    torch.manual_seed(0)
    Sb = torch.from_numpy(R.astype(np.float32))[None].cuda()
    ref, _, _ = main.run_uGLAD_direct(None, eval_offset=offset, EPOCHS=20, L=6, VERBOSE=False, Sb=Sb)
    ref = ref[0].detach().cpu().numpy().astype(np.float64)
    err = float(np.linalg.norm(P - ref) / np.linalg.norm(ref))
    print(f"fit_mixed against run_uGLAD_direct on the golden's repaired matrix: rel-Frobenius {err:.2e}")
    assert err < FIT_TOL
    assert deviation(est.covariance_, A, kinds) <= BOUND and est.covariance_.dtype == np.float64  # unrepaired
    assert est.node_names_ == names and np.isnan(est.location_[kinds == "c"]).all()
    assert np.allclose(est.location_[kinds == "r"], table[:, kinds == "r"].mean(axis=0), rtol=1e-12)
    assert est.model_glad is not None and np.isfinite(est.cond_max_)
    R = R.copy()
    out = est.predict(S=R)
    assert out.shape == (12, 12) and np.isfinite(out).all()
    graph = est.recovered_graph()
    assert len(graph.edges) >= 1
    main.save_uGLAD_model(est, str(tmp_path / "mixed"))
    back = main.load_uGLAD_model(str(tmp_path / "mixed"))
    assert np.array_equal(back.precision_, P) and np.array_equal(back.predict(S=R), out)


@pytest.mark.gpu
def test_gpu_covariance_wide_is_bit_identical_around_an_association_call():
    from uglad_amd import _lib

    lib = _lib.get_lib()
    X = torch.from_numpy(np.random.default_rng(3).standard_normal((1, 40, 70))).cuda()  # N < D: singular, repaired

    def cov():
        S, mn, rep = lib.covariance_wide(X, normalize=True, eval_offset=0.1, repair=True, return_min_eig=True)
        torch.cuda.synchronize()
        return S.cpu().numpy(), mn.cpu().numpy(), rep.cpu().numpy()

    before = cov()
    check_golden(lib, "n97_d12", "cuda")
    after = cov()
    assert before[2].all() and np.isfinite(before[1]).all()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
