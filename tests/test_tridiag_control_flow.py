"""GPU: tridiag_kernel (csrc/tridiag.h) masks its lanes and column slots without changing a bit of what it computes.

Through lib.tridiagonalize, the entry point bench.py times, on the shapes, routes and inputs of tridiag_control_flow_cases.py:
  1. tri (d, e, tau) and every row of R equal golden/tridiag_parent_bits.npz, recorded on an MI355X from the build of the commit before the masks
     were rewritten (golden/make_tridiag_goldens.py): in full where the golden keeps the arrays, by CRC32 per matrix where it keeps those.
  2. independent of the golden's bits: Q rebuilt from (R, tau) in fp64 -- ||Q^T A Q - T||_F / ||A||_F and ||Q^T Q - I||_F are each at most twice
     what the parent build gave on the same input (stored next to the bits).  The arithmetic is unchanged, so equality is expected; the factor
     absorbs a moved contraction only.
The route of every case (which instantiation the host layer launches) is asserted on the CPU from the emulator's launch record, the way
test_launch_routes.py does it, for the padded sizes the emulator build has (NT = 1, 2, 4, 5)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import tridiag_control_flow_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "tridiag_parent_bits.npz"))


@pytest.fixture(scope="module")
def lib():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from uglad_amd import _lib

    return _lib.get_lib()


@pytest.mark.gpu
@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_bits_and_residuals_are_the_parents(lib, golden, case):
    for name, launch in tc.inputs(case).items():
        key = f"{tc.case_id(case)}/{name}/"
        tri, R = tc.run(lib, "cuda", case, launch)
        res = tc.all_residuals(launch, tri, R)
        want = golden[key + "res"]
        print(f"{key:28s} ||Q^T A Q - T|| / ||A|| {res[:, 0].max():.3e} (parent {want[:, 0].max():.3e})   ||Q^T Q - I|| {res[:, 1].max():.3e} "
              f"(parent {want[:, 1].max():.3e})")
        # 1. the parent's bits
        if key + "tri_crc" in golden.files:
            assert np.array_equal(tc.crc_per_matrix(tri), golden[key + "tri_crc"]), key + "tri (CRC32 per matrix)"
            tri = tri[list(tc.checked_matrices(launch))]
        assert tri.tobytes() == golden[key + "tri"].tobytes(), key + "tri"
        if key + "R" in golden.files:
            assert R.tobytes() == golden[key + "R"].tobytes(), key + "R"
        else:
            assert np.array_equal(tc.crc_per_matrix(R), golden[key + "R_crc"]), key + "R (CRC32 per matrix)"
        # 2. independent of them
        assert np.all(res <= 2 * want), (key, res, want)


ROUTE_WORKER = """
import ctypes, os, sys
sys.path.insert(0, %r)
import tridiag_control_flow_cases as tc
dll = ctypes.CDLL(%r)
dll.uglad_tridiagonalize.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
for case in tc.CASES:
    D, M, env = case
    if (D + 31) // 32 not in (1, 2, 4, 5):
        continue
    for k in tc.SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    open(os.environ["UGLAD_EMUL_LAUNCH_LOG"], "w").close()
    rc = dll.uglad_tridiagonalize(1 << 36, 2 << 36, 3 << 36, 4 << 36, 5 << 36, M, D, None)
    with open(os.environ["UGLAD_EMUL_LAUNCH_LOG"]) as f:
        print("ROUTE", tc.case_id(case), rc, f.read().strip().split("(")[0].replace("void ", ""))
"""


def test_every_case_takes_the_route_it_is_meant_to_cover():
    """The launch record of a record-only emulator run (no kernel executes; the pointers are made-up addresses)."""
    from conftest import build_emulated_lib

    path = build_emulated_lib()
    if path is None:
        pytest.skip("host clang++ not available for the SIMT-emulator build")
    with tempfile.TemporaryDirectory() as tmp:
        env = {k: v for k, v in os.environ.items() if k not in tc.SWITCHES}
        env.update(UGLAD_EMUL_LAUNCH_LOG=os.path.join(tmp, "launches.txt"), UGLAD_EMUL_RECORD_ONLY="1")
        out = subprocess.run([sys.executable, "-c", ROUTE_WORKER % (HERE, path)], env=env, capture_output=True, text=True, check=True)
    got = {ln.split()[1]: (int(ln.split()[2]), " ".join(ln.split()[3:])) for ln in out.stdout.splitlines() if ln.startswith("ROUTE")}
    want = {tc.case_id(c): (0, tc.expected_kernel(c)) for c in tc.CASES if (c[0] + 31) // 32 in (1, 2, 4, 5)}
    assert got == want
    # both routes beyond D = 128, and every instantiation family of the kernel, are among the cases (NT = 3 and 8 included: host_route.h sends
    # them by the same two comparisons, nt <= 3 and nt > 4 && M <= 256, that the recorded ones went through)
    kernels = {tc.expected_kernel(c) for c in tc.CASES}
    for k in ("tridiag_kernel<4, 512>", "tridiag_kernel<3, 384>", "tridiag_kernel<2, 256>", "tridiag_kernel<1, 512>", "tridiag_kernel<3, 512>",
              "tridiag_kernel<5, 1024>", "tridiag_kernel<5, 512>", "tridiag_kernel<8, 1024>", "tridiag_kernel<8, 512>"):
        assert "uglad::" + k in kernels, k
