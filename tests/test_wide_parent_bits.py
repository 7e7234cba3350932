"""GPU: the nine many-workgroup fp64 utilities (csrc/host_wide.h: covariance_wide, association, conditional_mean_wide, sample_scores,
support_metrics_wide, graph_wide, eigvalsh_wide, table_spectrum, correlated_features) return what they returned before their shared pieces
got one owner each -- the shift bisection, the reduction helpers and the symmetriser in chol_wide.h, the radix sort in sort_wide.h, the
centred Gram product in cov_wide.h.

Through the HipLib wrappers on the cases of wide_cases.py, every output equals golden/wide_parent_bits.npz (the first six) or
golden/wide_parent_bits_eigw.npz (the last three), each recorded on an MI355X from the build of the commit before the change that touched its
entry points (golden/make_wide_parent_goldens.py): the parent's bits where the parent is finite, NaN exactly where it has NaN (payloads
are not compared); in full for the first case of each entry point, by CRC32 per problem for the others.  Which kernels every call launches is
pinned on the CPU (test_launch_routes_wide.py)."""
import os

import numpy as np
import pytest

import wide_cases as wc

HERE = os.path.dirname(os.path.abspath(__file__))


class _Goldens:
    """The golden files as one: `files` and [key], as of one of them."""

    def __init__(self, parts):
        self.where = {key: part for part in parts for key in part.files}
        self.files = list(self.where)

    def __getitem__(self, key):
        return self.where[key][key]


@pytest.fixture(scope="module")
def golden():
    return _Goldens([np.load(os.path.join(HERE, "golden", name)) for name in wc.GOLDENS])


@pytest.fixture(scope="module")
def lib():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from uglad_amd import _lib

    return _lib.get_lib()


@pytest.mark.gpu
@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_every_output_has_the_parents_bits(lib, golden, case):
    got = wc.run(lib, "cuda", case)
    prefix = wc.case_id(case) + "/"
    assert {prefix + name for name in got} == {key.rsplit("/", 1)[0] for key in golden.files if key.startswith(prefix)}
    print(f"{prefix:24s} NaN per problem: { {n: c for n, c in wc.nan_counts(got).items() if any(c)} }")
    for name, per in got.items():
        key = prefix + name + "/"
        if wc.kept_in_full(case):
            for k, x in enumerate(per):
                assert wc.same_bits(x, golden[key + str(k)]), key + str(k)
            assert key + str(len(per)) not in golden.files
        else:
            assert np.array_equal(np.array([wc.crc(x) for x in per], dtype=np.uint32), golden[key + "crc"]), key + "(CRC32 per problem)"
