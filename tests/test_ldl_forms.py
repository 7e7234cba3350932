"""GPU: the L D L^T inverse beyond the eigensolver (csrc/ldl_wide.h) returns what it returned when its two kernel forms were two hand-kept copies.

Through lib.init_theta and lib.loss_fwd on the cases of ldl_cases.py, every case under both forms (UGLAD_LDL_LAUNCHES=0 / 1) and, on either side of
the crossover, with the switch unset:
  1. the inverse and the loss equal golden/ldl_parent_bits.npz, recorded on an MI355X from the build of the commit before the copies were merged
     (golden/make_ldl_goldens.py): the parent's bits where the parent is finite, NaN exactly where it has NaN (payloads are not compared); in full
     where the golden keeps the arrays, by CRC32 per matrix where it keeps those.
  2. independent of the golden's bits: ||A X - I||_F / sqrt(D) and |logdet - slogdet| in fp64 are each at most twice what the parent build gave on
     the same input (stored next to the bits).  The arithmetic is unchanged, so equality is expected; the factor absorbs a moved contraction only.
Which kernel and layout every case launches is asserted on the CPU from the emulator's launch record (test_ldl_forms_emulated.py)."""
import os

import numpy as np
import pytest

import ldl_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "ldl_parent_bits.npz"))


@pytest.fixture(scope="module")
def lib():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from uglad_amd import _lib

    return _lib.get_lib()


@pytest.mark.gpu
@pytest.mark.parametrize("case", lc.GPU_CASES, ids=lc.case_id)
def test_bits_and_residuals_are_the_parents(lib, golden, case):
    for form in lc.forms(case):
        key = f"{lc.case_id(case)}/{lc.form_id(form)}/"
        X, loss = lc.run(lib, "cuda", case, form)
        res, want = lc.backward_errors(case, X, loss), golden[key + "res"]
        print(f"{key:40s} ||A X - I|| / sqrt(D) {res[:, 0].max():.3e} (parent {want[:, 0].max():.3e})   |logdet - slogdet| {res[:, 1].max():.3e} "
              f"(parent {want[:, 1].max():.3e})")
        # 1. the parent's bits
        if key + "X" in golden.files:
            assert lc.same_bits(X, golden[key + "X"]), key + "X"
        else:
            assert np.array_equal(lc.crc_per_matrix(lc.canonical(X)), golden[key + "X_crc"]), key + "X (CRC32 per matrix)"
        if loss is not None:
            assert lc.same_bits(loss, golden[key + "loss"]), key + "loss"
        # 2. independent of them
        assert lc.within_twice(res, want), (key, res, want)
