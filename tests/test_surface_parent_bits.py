"""The Python surface against the bits of the commit before it was consolidated (tests/golden/surface_parent_bits.npz, recorded on an
MI355X by tests/golden/make_surface_parent_goldens.py): glad.py's one autograd node, GladParams.load_packed_, the shared epoch loop, the
estimators' base, the one conversion helper and the split of main.py into inputs.py and after.py change no bit of any pass, fit, prediction,
score, graph, report or conditional Gaussian.  The cases are tests/surface_cases.py."""
import os

import numpy as np
import pytest

import surface_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "surface_parent_bits.npz")) as z:
        return {k: z[k] for k in z.files}


_seen = set()


@pytest.mark.parametrize("case", sc.cases())
def test_surface_equals_parent_bits(case, golden):
    out = sc.run(case)
    _seen.update(out)
    expected = {k for k in golden if k.startswith(case + ":") and not k.endswith("|spread")}
    assert set(out) == expected, f"{case}: outputs {sorted(set(out) ^ expected)} are not in both"
    wrong = []
    for key, a in out.items():
        spread = golden.get(key + "|spread")
        if spread is None:
            if not sc.same_bits(a, golden[key]):
                wrong.append(key)
        else:  # (the parent did not repeat itself here: twice its own spread)
            a64, g64 = np.asarray(a, dtype=np.float64), golden[key].astype(np.float64)
            dist = np.linalg.norm(a64 - g64) / max(np.linalg.norm(g64), 1e-300)
            print(f"{key}: {dist:.3e} from the parent, whose two recordings are {float(spread):.3e} apart")
            if not dist <= 2.0 * float(spread):
                wrong.append(key)
    assert not wrong, f"{case}: differs from the parent in {wrong}"


def test_no_case_dropped_out(golden):
    """The key set of the golden is the key set of the cases (this runs after them: it checks what they produced)."""
    keys = {k for k in golden if not k.endswith("|spread")}
    assert {k.split(":")[0] for k in keys} == set(sc.cases())
    if _seen:  # (the whole module ran)
        assert _seen == keys


def test_grouped_pass_of_one_group_is_glad_bit_for_bit():
    for what, a, b in sc.grouped_of_one_equals_glad():
        assert sc.same_bits(b, sc.stored(a)), what
