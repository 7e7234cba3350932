"""CPU: the two kernel forms of the L D L^T inverse (csrc/ldl_wide.h: ns_ldl_kernel, one workgroup per matrix; ns_ldl_phase_kernel, one launch per
phase) on the SIMT emulator, through lib.init_theta and lib.loss_fwd on the cases of ldl_cases.py the CPU can afford.

  (a) the two forms return the same bits where finite and NaN in the same places: they are one phase function walked by one schedule.
  (b) ||X - X64||_F / ||X64||_F against numpy fp64 and |logdet - slogdet| are each at most twice what the emulator run of the code BEFORE the two
      hand-kept copies were merged gave, golden/ldl_parent_emul_residuals.json (`python tests/test_ldl_forms_emulated.py --record` wrote it from that
      commit; it is the parent's and is not regenerated for a change that keeps the arithmetic).  null there = NaN: not finite at the parent either.
  (c) from a record-only run (no kernel executes): every case of the table, the GPU-only ones included, launches the kernel family and layout it is
      meant to cover -- ns_ldl_kernel<1024 | 2048> once, or ns_ldl_phase_kernel<...> once per step of the schedule, 5 nt times."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import ldl_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
PARENT = os.path.join(HERE, "golden", "ldl_parent_emul_residuals.json")


def errors_of(lib, case):
    """({form: (X, loss)}, {form name: [[inverse error, logdet error] per matrix]}) of both forms."""
    outs = {form: lc.run(lib, "cpu", case, form) for form in ("0", "1")}
    return outs, {lc.form_id(form): lc.forward_errors(case, *out).tolist() for form, out in outs.items()}


def record():
    sys.path.insert(0, os.path.join(HERE, ".."))
    from conftest import install_emulated_lib

    lib = install_emulated_lib()
    table = {}
    for case in lc.EMUL_CASES:
        outs, errs = errors_of(lib, case)
        assert lc.same_bits(outs["0"][0], outs["1"][0]), case
        table[lc.case_id(case)] = {f: [[None if np.isnan(v) else v for v in row] for row in rows] for f, rows in errs.items()}
        print(lc.case_id(case), table[lc.case_id(case)], flush=True)
    with open(PARENT, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in table.items()) + "\n}\n")


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    record()
    sys.exit(0)

import pytest  # noqa: E402


@pytest.fixture(scope="module")
def parent():
    with open(PARENT) as f:
        return json.load(f)


@pytest.mark.parametrize("case", lc.EMUL_CASES, ids=lc.case_id)
def test_both_forms_give_the_same_bits_and_the_parents_accuracy(emul, parent, case):
    outs, errs = errors_of(emul, case)
    (X0, loss0), (X1, loss1) = outs["0"], outs["1"]
    print(lc.case_id(case), errs, "parent", parent[lc.case_id(case)])
    # (a)
    assert lc.same_bits(X0, X1)
    assert (loss0 is None and loss1 is None) or lc.same_bits(loss0, loss1)
    # (b)
    for form, got in errs.items():
        want = [[np.nan if v is None else v for v in row] for row in parent[lc.case_id(case)][form]]
        assert lc.within_twice(got, want), (form, got, want)


ROUTE_WORKER = """
import ctypes, os, sys
sys.path.insert(0, %r)
import ldl_cases as lc
dll = ctypes.CDLL(%r)
dll.uglad_init_theta.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
dll.uglad_loss_fwd.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
for case in lc.GPU_CASES + lc.EMUL_CASES:
    entry, M, D, _ = case
    for form in lc.forms(case):
        os.environ.pop(lc.SWITCH, None)
        if form is not None:
            os.environ[lc.SWITCH] = form
        open(os.environ["UGLAD_EMUL_LAUNCH_LOG"], "w").close()
        if entry == "init":
            rc = dll.uglad_init_theta(1 << 36, 2 << 36, 0, 3 << 36, 4 << 36, M, D, None)
        else:
            rc = dll.uglad_loss_fwd(1 << 36, 2 << 36, 1, None, 5 << 36, 3 << 36, 4 << 36, M, D, None)
        with open(os.environ["UGLAD_EMUL_LAUNCH_LOG"]) as f:
            names = [ln.split("(")[0].replace("void ", "") for ln in f.read().splitlines()]
        ldl = [n for n in names if "ns_ldl" in n]
        print("ROUTE", lc.case_id(case), lc.form_id(form), rc, len(ldl), " ".join(sorted(set(ldl))))
"""


def test_every_case_launches_the_form_and_layout_it_is_meant_to_cover():
    """The launch record of a record-only emulator run (no kernel executes; the pointers are made-up addresses)."""
    from conftest import build_emulated_lib

    path = build_emulated_lib()
    if path is None:
        pytest.skip("host clang++ not available for the SIMT-emulator build")
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, UGLAD_EMUL_LAUNCH_LOG=os.path.join(tmp, "launches.txt"), UGLAD_EMUL_RECORD_ONLY="1")
        out = subprocess.run([sys.executable, "-c", ROUTE_WORKER % (HERE, path)], env=env, capture_output=True, text=True, check=True)
    got = {(t[1], t[2]): (int(t[3]), " ".join(t[5:]), int(t[4])) for t in (ln.split() for ln in out.stdout.splitlines() if ln.startswith("ROUTE"))}
    want = {(lc.case_id(c), lc.form_id(f)): (0,) + lc.expected_launches(c, f) for c in lc.GPU_CASES + lc.EMUL_CASES for f in lc.forms(c)}
    assert got == want
    # both layouts in both forms, and the default on either side of the crossover, are among the cases
    kernels = {v[1] for v in want.values()}
    assert kernels == {f"uglad::ns_ldl_{k}kernel<{fd}>" for k in ("", "phase_") for fd in (1024, 2048)}
    assert want[("init_M1_D256", "default")][1:] == ("uglad::ns_ldl_kernel<1024>", 1)
    assert want[("init_M1_D288", "default")][1:] == ("uglad::ns_ldl_phase_kernel<1024>", 45)
