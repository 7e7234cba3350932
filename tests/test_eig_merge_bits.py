"""GPU: the merges of the divide & conquer (csrc/eig_lean.h, and the handed-over last merge of csrc/wide_fwd.h) give the bits they gave before
their phases got one statement each for the wave-local and the workgroup-wide levels.

On the sizes, inputs and calls of eig_merge_cases.py, against golden/eig_parent_bits.npz, recorded on an MI355X from the build of the parent commit
(golden/make_eig_goldens.py):
  0. the CRC32 of every input batch is the recorded one: an input that came out differently on this machine is told apart from a kernel that did;
  1. beta and U of uglad_symeig, bit for bit: in full up to D = 33, by CRC32 per matrix beyond; Z_out, U_out, beta_out and normF_partial of
     uglad_cell_fwd on the eigensolver route, with and without the handed-over last merge, by CRC32 per matrix;
  2. independent of the bits: every decomposition meets the bounds of eigensolver_cases.check.
Which calls launch wide_secular_kernel and wide_merge_kernel is asserted on the CPU from the emulator's launch record, the way test_launch_routes.py
does it, at the padded sizes the emulator build has (D = 129, 160: NT = 5)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import eig_merge_cases as ec
import eigensolver_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "eig_parent_bits.npz"))


@pytest.fixture(scope="module")
def lib():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from uglad_amd import _lib

    return _lib.get_lib()


@pytest.mark.gpu
@pytest.mark.parametrize("D", ec.SYMEIG_SIZES)
def test_symeig_bits_are_the_parents(lib, golden, D):
    names, A32 = list(ec.symeig_inputs(D)), ec.symeig_batch(D)
    key = f"symeig/D{D}/"
    assert ec.crc(A32) == int(golden[key + "input_crc"][0]), key + "the INPUT differs from the recorded one (not the kernel)"
    beta, U = ec.run_symeig(lib, "cuda", A32)
    if D <= ec.FULL_UP_TO:
        differ = [n for m, n in enumerate(names) if beta[m].tobytes() != golden[key + "beta"][m].tobytes() or U[m].tobytes() != golden[key + "U"][m].tobytes()]
    else:
        same = (ec.crc_per_matrix(beta) == golden[key + "beta_crc"]) & (ec.crc_per_matrix(U) == golden[key + "U_crc"])
        differ = [n for m, n in enumerate(names) if not same[m]]
    failures = []
    for m, name in enumerate(names):
        try:
            eig, res, orth = cases.check(A32[m], beta[m], U[m], ec.bound_kind(name), name)
            print(f"D={D:3d} {name:36s} eig {eig:.2e} res {res:.2e} (bound {cases.bound(ec.bound_kind(name), D):.2e}) orth {orth:.2e}")
        except AssertionError as err:
            failures.append(err.args[0])
    assert not differ, (key, "beta or U differ from the parent's bits", differ)
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ec.CELL_SHAPES, ids=lambda s: f"D{s[0]}_M{s[1]}")
def test_cell_bits_are_the_parents_with_and_without_the_handed_over_merge(lib, golden, shape):
    D, M = shape
    inputs = ec.cell_inputs(D, M, ec.trained_params())
    key = f"cell/D{D}_M{M}/"
    assert [ec.crc(x) for x in inputs] == [int(c) for c in golden[key + "input_crc"]], key + "an INPUT differs from the recorded one (not the kernel)"
    differ = []
    for wide in (1, 0):
        got = ec.run_cell(lib, "cuda", inputs, wide)  # (restores both settings to -1 in a finally)
        differ += [f"wide{wide}/{name}" for name in ec.CELL_OUTPUTS if not np.array_equal(ec.crc_per_matrix(got[name]), golden[f"{key}wide{wide}/{name}"])]
    assert not differ, (key, "differ from the parent's bits (CRC32 per matrix)", differ)


ROUTE_WORKER = """
import ctypes, os, sys
sys.path.insert(0, %r)
import eig_merge_cases as ec
dll = ctypes.CDLL(%r)
dll.uglad_cell_fwd.argtypes = [ctypes.c_void_p] * 11 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
dll.uglad_symeig.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
def launched(fn, *args):
    open(os.environ["UGLAD_EMUL_LAUNCH_LOG"], "w").close()
    rc = fn(*args, None)
    with open(os.environ["UGLAD_EMUL_LAUNCH_LOG"]) as f:
        names = [ln.split("(")[0].replace("void ", "").split("<")[0] for ln in f.read().splitlines()]
    return rc, ",".join(sorted(set(names)))
buf = [(i + 1) << 36 for i in range(11)]
assert dll.uglad_set_matrix_iteration(0) == 0
for D, M in ec.CELL_SHAPES:
    if (D + 31) // 32 not in (1, 2, 4, 5):
        continue
    for wide in (1, 0):
        assert dll.uglad_set_wide_mode(wide) == 0
        print("ROUTE", f"cell_D{D}_M{M}_wide{wide}", *launched(dll.uglad_cell_fwd, *buf, M, D, ec.SQRT_NS10))
assert dll.uglad_set_wide_mode(-1) == 0 and dll.uglad_set_matrix_iteration(-1) == 0
for D in ec.SYMEIG_SIZES:
    if (D + 31) // 32 in (1, 2, 4, 5):
        print("ROUTE", f"symeig_D{D}", *launched(dll.uglad_symeig, *buf[:4], len(ec.PLAIN_FAMILIES) + 3, D))
"""


def test_only_the_wide_calls_hand_the_last_merge_over():
    """The launch record of a record-only emulator run (no kernel executes; the pointers are made-up addresses)."""
    from conftest import build_emulated_lib

    path = build_emulated_lib()
    if path is None:
        pytest.skip("host clang++ not available for the SIMT-emulator build")
    with tempfile.TemporaryDirectory() as tmp:
        env = {k: v for k, v in os.environ.items() if k not in ("UGLAD_WIDE_BWD", "UGLAD_MATRIX_ITERATION")}
        env.update(UGLAD_EMUL_LAUNCH_LOG=os.path.join(tmp, "launches.txt"), UGLAD_EMUL_RECORD_ONLY="1")
        out = subprocess.run([sys.executable, "-c", ROUTE_WORKER % (HERE, path)], env=env, capture_output=True, text=True, check=True)
    got = {ln.split()[1]: (int(ln.split()[2]), set(ln.split()[3].split(","))) for ln in out.stdout.splitlines() if ln.startswith("ROUTE")}
    handed_over = {"uglad::wide_secular_kernel", "uglad::wide_merge_kernel"}
    wide = [f"cell_D{D}_M{M}_wide1" for D, M in ec.CELL_SHAPES if D <= 160]
    assert sorted(wide) == ["cell_D129_M2_wide1", "cell_D160_M2_wide1"] and set(wide) < set(got)
    assert {k for k in got if k.startswith("symeig_")} == {f"symeig_D{D}" for D in ec.SYMEIG_SIZES if (D + 31) // 32 in (1, 2, 4, 5)}
    for call, (rc, kernels) in got.items():
        assert rc == 0 and kernels, (call, rc, kernels)
        if call in wide:
            assert handed_over <= kernels, (call, kernels)
        else:
            assert not (handed_over & kernels), (call, kernels)
        assert not any(k.startswith("uglad::ns_") for k in kernels), (call, kernels)  # (the eigensolver, not the matrix iteration of wide_ns.h)
