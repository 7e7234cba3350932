"""CPU twin of test_tridiag_control_flow.py: the unmodified tridiag_kernel on the SIMT emulator, under its three schedules.

The shapes of tridiag_control_flow_cases.py up to D = 129 that the emulator build instantiates (NT = 1, 2, 4, 5: D = 65 and 96 are GPU-only), every
input, both entry forms.  Check: Q rebuilt from (R, tau) in fp64 tridiagonalises A and is orthogonal.  The emulator's bits are not the GPU's, so
the GPU golden does not apply; the bounds are absolute, per case, launch and MATRIX: twice (the factor the GPU test allows over its parent) what the
emulator run of the kernel BEFORE its masks were rewritten gave under the fair schedule, golden/tridiag_parent_emul_residuals.json
(`python tests/test_tridiag_control_flow_emulated.py --worker` prints the table; it is the parent's and is not regenerated for a change that keeps
the arithmetic).  The launches with the matrix scaled by 1e-17 stand at 3e-3 .. 2e-2 there: kNegligibleSig is an absolute threshold, and columns
of norm below 3e-18 get no reflector.  One process per schedule: the policy is read once per process."""
import json
import os
import subprocess
import sys

import pytest

import tridiag_control_flow_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
EMULATED = [c for c in tc.CASES if c[0] <= 129 and c[1] <= 3 and (c[0] + 31) // 32 != 3]


def worker():
    sys.path.insert(0, os.path.join(HERE, ".."))
    from conftest import install_emulated_lib

    lib = install_emulated_lib()
    for case in EMULATED:
        for name, launch in tc.inputs(case).items():
            tri, R = tc.run(lib, "cpu", case, launch)
            res = tc.all_residuals(launch, tri, R)
            print(f"RES {tc.case_id(case)} {name} " + " ".join(f"{v:.3e}" for v in res.ravel()), flush=True)  # (r_t, r_o) of matrix 0, 1, ...


@pytest.mark.parametrize("schedule", ["fair", "ahead", "behind"])
def test_reflectors_of_the_emulated_kernel_tridiagonalise_and_are_orthogonal(schedule):
    from conftest import build_emulated_lib

    if build_emulated_lib() is None:
        pytest.skip("host clang++ not available for the SIMT-emulator build")
    with open(os.path.join(HERE, "golden", "tridiag_parent_emul_residuals.json")) as f:
        parent = json.load(f)
    env = {k: v for k, v in os.environ.items() if k not in tc.SWITCHES}
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=dict(env, UGLAD_EMUL_SCHED=schedule), capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    rows = {f"{ln.split()[1]}/{ln.split()[2]}": [float(v) for v in ln.split()[3:]] for ln in out.stdout.splitlines() if ln.startswith("RES")}
    assert sorted(rows) == sorted(parent) and len(rows) == 3 * len(EMULATED)
    for key, got in rows.items():
        assert len(got) == len(parent[key])
        for j, (g, w) in enumerate(zip(got, parent[key])):  # (even j: ||Q^T A Q - T|| / ||A|| of matrix j / 2, odd j: its ||Q^T Q - I||)
            assert g <= 2 * w, (schedule, key, "matrix", j // 2, "||Q^T Q - I||" if j % 2 else "||Q^T A Q - T|| / ||A||", g, w)


if __name__ == "__main__" and sys.argv[1:] == ["--worker"]:
    worker()
