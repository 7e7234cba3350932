"""CPU suite: host-side logic, the C-ABI library's exports, the no-fallback rule, and the sharded (world_size 2, gloo) path."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ----------------------------------------------------------------------------------------------- C ABI
def test_library_builds_loads_and_exports_every_declared_symbol():
    import ctypes

    import __graft_entry__ as ge
    from uglad_amd import _lib

    ge.build()  # hipcc cross-compiles gfx950 without a GPU; a no-op when up to date
    header = open(os.path.join(ROOT, "include", "uglad_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|float)\s+(uglad_\w+)\s*\(", header))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(dll, name), name
    assert dll.uglad_max_dim() >= 128 and dll.uglad_version() >= 1  # pure host calls, no GPU needed
    csrc = os.path.join(ROOT, "uglad_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))]
    assert "glad_kernels.hip" in sources and "host_route.h" in sources
    for f in sources:  # gfx950 only, no dual path -- in the kernels and in the host layer's headers
        src = open(os.path.join(csrc, f)).read()
        assert "__HIP_PLATFORM" not in src and "cuda" not in src.lower(), f


def test_product_has_no_cpu_fallback_and_never_touches_the_oracle(monkeypatch):
    import uglad_amd
    from uglad_amd import _lib

    for dirpath, _, files in os.walk(os.path.join(ROOT, "uglad_amd")):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, re.M), f
    if not torch.cuda.is_available():
        monkeypatch.setattr(_lib, "_instance", None)
        with pytest.raises(_lib.UgladError):
            uglad_amd.glad(torch.eye(4)[None], uglad_amd.GladParams(1.0))
        with pytest.raises(_lib.UgladError):
            uglad_amd.loss_uGLAD(torch.eye(4)[None], torch.eye(4)[None])
    with pytest.raises(_lib.UgladError):
        _lib.HipLib("/nonexistent/libuglad_hip.so")


def test_gladparams_is_state_dict_compatible_with_the_reference():
    import uglad_amd
    from uglad_amd.glad.glad_params import PARAM_KEYS

    g = np.load(os.path.join(ROOT, "tests", "golden", "params_trained.npz"))
    m = uglad_amd.GladParams(1.0)
    assert tuple(m.state_dict().keys()) == PARAM_KEYS == tuple(g.files)
    m.load_state_dict({k: torch.from_numpy(g[k]) for k in g.files})
    pk = m.packed()
    assert pk.shape == (42,) and pk.requires_grad
    np.testing.assert_array_equal(pk.detach().numpy(), np.concatenate([g[k].ravel() for k in g.files]))
    with pytest.raises(ValueError):
        uglad_amd.GladParams(1.0, nF=4)
    # same construction order as the reference => same draw from the same seed (checked against the captured init)
    torch.manual_seed(123)
    fresh = uglad_amd.GladParams(1.0)
    gf = np.load(os.path.join(ROOT, "tests", "golden", "params_fresh.npz"))
    for k in gf.files:
        np.testing.assert_array_equal(fresh.state_dict()[k].numpy(), gf[k])
    # API-parity helpers
    X = torch.randn(2, 5, 5)
    out = m.eta_forward(X, torch.randn(2, 5, 5), 0, torch.randn(2, 5, 5))
    assert out.shape == X.shape and float(m.lambda_forward(0.3, 0.2).detach()) > 0


# ----------------------------------------------------------------------------------------------- host data utilities
def test_process_table_and_covariance_semantics():
    from uglad_amd.utils import prepare_data as pd_

    rng = np.random.default_rng(0)
    X = rng.standard_normal((50, 6))
    X[5, 2] = np.nan  # filled with the column mean
    X = np.column_stack([X, np.full(50, 7.0), X[:, 0]])  # constant column and duplicate column: dropped
    X[3] = 0.0  # all-zero row: dropped
    T = pd_.process_table(X, NORM="min_max", VERBOSE=False)
    assert T.shape == (49, 6)
    assert np.allclose(T.min().values, 0) and np.allclose(T.max().values, 1) and not np.isnan(T.values).any()
    S = pd_.get_covariance([T.values])[0]
    np.testing.assert_allclose(S, np.cov(T.values.T, bias=1), rtol=1e-12)
    Xs = np.ones((10, 3)) * np.arange(3)  # singular covariance -> eigenvalue repair to `offset`
    Xs[:, 0] += rng.standard_normal(10)
    Sr = pd_.get_covariance([Xs], offset=0.1)[0]
    assert abs(np.linalg.eigvalsh(Sr).min() - 0.1) < 1e-9
    t = pd_.convert_to_torch(S)
    assert t.dtype == torch.float32 and not t.requires_grad
    Xb, P = pd_.get_data(12, (0.1, 0.2), 40, batch_size=2, eig_offset=1.0, rng=5)
    assert Xb.shape == (2, 40, 12) and abs(np.linalg.eigvalsh(P[0]).min() - 1.0) < 1e-9
    Sb = pd_.synthetic_covariance_batch(3, 10, seed=1)
    np.testing.assert_array_equal(Sb[1:], pd_.synthetic_covariance_batch(2, 10, seed=1, task_offset=1))  # shardable


def test_kfold_and_imputation_match_sklearn_and_the_reference():
    from sklearn.model_selection import KFold

    from uglad_amd import main

    for n, k in ((10, 3), (400, 3), (17, 5)):
        ours = list(main._kfold_indices(n, k))
        theirs = list(KFold(n_splits=k).split(np.zeros((n, 1))))
        for (a, b), (c, d) in zip(ours, theirs):
            np.testing.assert_array_equal(a, c)
            np.testing.assert_array_equal(b, d)
    X = np.array([[1.0, np.nan], [3.0, 4.0], [np.nan, 8.0]])
    np.testing.assert_allclose(main.mean_imputation(X[None])[0], [[1, 6], [3, 4], [2, 8]])
    with pytest.raises(ValueError):
        main.mean_imputation(np.array([[[np.nan, 1.0], [np.nan, 2.0]]]))


def test_metrics_match_sklearn():
    from sklearn import metrics as skm

    from uglad_amd.utils.metrics import get_auc, report_metrics_all

    rng = np.random.default_rng(2)
    y = rng.integers(0, 2, 200)
    s = np.round(rng.random(200), 2)  # ties on purpose
    fpr, tpr, _ = skm.roc_curve(y, s)
    auc, aupr = get_auc(y, s)
    assert abs(auc - skm.auc(fpr, tpr)) < 1e-12 and abs(aupr - skm.average_precision_score(y, s)) < 1e-12
    T = np.triu((rng.random((9, 9)) < 0.3).astype(float), 1)
    T = T + T.T + np.eye(9)
    G = T * rng.random((9, 9)) + np.triu((rng.random((9, 9)) < 0.1).astype(float), 1)
    G = (G + G.T) / 2
    m = report_metrics_all(T, G)
    assert set(m) == {"FDR", "TPR", "FPR", "SHD", "nnzTrue", "nnzPred", "precision", "recall", "Fbeta", "aupr", "auc"}
    assert m["nnzTrue"] == float(np.count_nonzero(np.triu(T, 1)))


# ----------------------------------------------------------------------------------------------- sharded path
_WORKER = r"""
import os, sys, json
import numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import conftest
import torch.distributed as dist
rank = int(sys.argv[1]); world = int(sys.argv[2])
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[3], RANK=str(rank), WORLD_SIZE=str(world))
assert conftest.install_emulated_lib() is not None
if world > 1:
    dist.init_process_group("gloo", rank=rank, world_size=world)
import uglad_amd
from uglad_amd import main
from uglad_amd.utils import prepare_data as pd_
rng = np.random.default_rng(11)
n_tasks = int(sys.argv[5]) if len(sys.argv) > 5 else 4
k_fold = int(sys.argv[6]) if len(sys.argv) > 6 else 4
Xb = [pd_.get_data(8, (0.2, 0.4), 60, 1, eig_offset=1.0, rng=rng)[0][0] for _ in range(n_tasks)]
init = np.load(os.path.join({root!r}, "tests", "golden", "params_trained.npz"))
real = main.init_uGLAD
def init_fixed(*a, **k):
    m, _ = real(*a, **k)
    m.load_state_dict({{key: torch.from_numpy(init[key]) for key in init.files}})
    return m, main.glad.get_optimizers(m, lr_glad=k.get("lr", 0.002))
main.init_uGLAD = init_fixed
est = uglad_amd.uGLAD_multitask()
est.fit(Xb, epochs=2, lr=0.01, L=3, verbose=False)
out = dict(precision=est.precision_.tolist(), params=est.model_glad.packed().detach().numpy().tolist())
# missing-data mode: K sub-sample covariances sharded, loss against the replicated full covariance, consensus all-reduce
X = Xb[0].copy(); X[rng.random(X.shape) < 0.2] = np.nan
g = uglad_amd.uGLAD_GL()
g.fit(X, epochs=2, lr=0.01, L=3, verbose=False, k_fold=k_fold, mode="missing")
out["missing_precision"] = g.precision_.tolist()
out["missing_params"] = g.model_glad.packed().detach().numpy().tolist()
if rank == 0:
    json.dump(out, open(sys.argv[4], "w"))
if world > 1:
    dist.destroy_process_group()
"""


def _run_world(world, port, tmp_path, n_tasks=4, k_fold=4):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT))
    outf = str(tmp_path / f"out_w{world}.json")
    env = dict(os.environ, OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")  # (up to eight ranks share this container's eight cores)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(world), str(port), outf, str(n_tasks), str(k_fold)], env=env)
             for r in range(world)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    import json

    return json.load(open(outf))


def test_sharded_world2_gloo_equals_single_process(tmp_path):
    """One process per 'GPU' (here: CPU + emulated kernels), gloo, world_size 2: multitask fit and missing-data fit must give
    the single-process precision matrices and trained parameters (exchanges i-iii of uglad_amd/dist.py)."""
    import conftest

    if conftest.build_emulated_lib() is None:
        pytest.skip("host clang++ not available")
    single = _run_world(1, 29611, tmp_path)
    double = _run_world(2, 29612, tmp_path)
    for key in ("precision", "params", "missing_precision", "missing_params"):
        a, b = np.array(single[key]), np.array(double[key])
        assert a.shape == b.shape
        np.testing.assert_allclose(b, a, rtol=2e-5, atol=2e-6, err_msg=key)


@pytest.mark.parametrize("world,n_tasks,k_fold,port", [(4, 6, 5, 29621), (8, 11, 9, 29631)])
def test_sharded_uneven_shards_gloo_world4_and_world8(tmp_path, world, n_tasks, k_fold, port):
    """Rehearsal of more ranks than this round's hardware offers (gloo, CPU, emulated kernels): world_size 4 with 6 tasks / 5 sub-sample
    covariances (shards 2,2,1,1 / 2,1,1,1) and world_size 8 with 11 tasks / 9 sub-samples (2,2,2,1,1,1,1,1 / 2,1,...,1) -- the batch does
    NOT divide evenly, so the divisor of the batch mean is the global count handed to glad(), the gradient message sums unequal shards and
    all_gather_cat pads.  Same precision matrices and trained parameters as one process."""
    import conftest

    if conftest.build_emulated_lib() is None:
        pytest.skip("host clang++ not available")
    single = _run_world(1, port, tmp_path, n_tasks, k_fold)
    many = _run_world(world, port + 1, tmp_path, n_tasks, k_fold)
    for key in ("precision", "params", "missing_precision", "missing_params"):
        a, b = np.array(single[key]), np.array(many[key])
        assert a.shape == b.shape
        np.testing.assert_allclose(b, a, rtol=2e-5, atol=2e-6, err_msg=key)


def test_sharded_glad_requires_the_global_batch():
    import uglad_amd
    from uglad_amd import dist
    from uglad_amd.glad import glad as gmod

    class Two(dist.Collective):
        world_size, rank = 2, 0

    with pytest.raises(ValueError, match="global_batch"):
        gmod.glad(torch.eye(4)[None], uglad_amd.GladParams(1.0), L=2, collective=Two())


def test_ranks_without_a_matrix_fail_everywhere_before_any_exchange():
    """world_size > K: every rank raises the same ValueError before the first collective (none may hang in an all-reduce)."""
    import uglad_amd
    from uglad_amd import dist, main

    class Eight(dist.Collective):
        world_size, rank = 8, 5

        def all_reduce_sum(self, t):
            raise AssertionError("a collective was reached")

        all_reduce_min = all_gather_cat = all_reduce_sum

    dist.set_collective(Eight())
    try:
        rng = np.random.default_rng(0)
        with pytest.raises(ValueError, match="cannot be sharded over 8 ranks"):
            main.run_uGLAD_multitask([rng.standard_normal((30, 5)) for _ in range(3)], EPOCHS=1, VERBOSE=False)
        with pytest.raises(ValueError, match="cannot be sharded over 8 ranks"):
            main.run_uGLAD_missing(rng.standard_normal((1, 30, 5)), EPOCHS=1, VERBOSE=False, K_batch=3)
    finally:
        dist.set_collective(None)
