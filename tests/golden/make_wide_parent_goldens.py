#!/usr/bin/env python3
"""Records tests/golden/wide_parent_bits.npz or wide_parent_bits_eigw.npz ON THE GPU from the library under UGLAD_LIB (default: the in-tree
build): what the HipLib wrappers of the many-workgroup fp64 utilities return, bit for bit, on the cases of tests/wide_cases.py.  Which entry
points a file holds is wide_cases.GOLDENS.

wide_parent_bits.npz was recorded on an MI355X from the build of the commit BEFORE the utilities' shared pieces got one owner each (the shift
bisection and two reduction helpers in csrc/chol_wide.h, the radix sort in csrc/sort_wide.h, the entry points in csrc/host_wide.h; same
arithmetic, same launches).  wide_parent_bits_eigw.npz (eigvalsh_wide, table_spectrum, correlated_features) was recorded the same way from
the build of the commit before their feeders got one owner each (the centred Gram product in csrc/cov_wide.h, the symmetriser in
csrc/chol_wide.h).  Both are the parent's bits and are not to be regenerated for a change that claims to keep them.

    UGLAD_LIB=<parent build> python tests/golden/make_wide_parent_goldens.py <file name in wide_cases.GOLDENS> [out.npz]

Per case and output (keys "<case>/<output>/..."): the first case of every entry point in full, ".../<k>" the array of problem k (NaN canonical);
the others ".../crc", a CRC32 per problem of the same.  Reads nothing outside the repository."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import wide_cases as wc  # noqa: E402


def record(lib, dev, entries):
    out = {}
    for case in wc.CASES:
        if case[0] not in entries:
            continue
        got = wc.run(lib, dev, case)
        for name, per in got.items():
            key = f"{wc.case_id(case)}/{name}/"
            if wc.kept_in_full(case):
                out.update({key + str(k): wc.canonical(x) for k, x in enumerate(per)})
            else:
                out[key + "crc"] = np.array([wc.crc(x) for x in per], dtype=np.uint32)
        nans = {n: c for n, c in wc.nan_counts(got).items() if any(c)}
        print(f"{wc.case_id(case):24s} {len(got):3d} outputs   NaN per problem: {nans}", flush=True)
    return out


if __name__ == "__main__":
    from uglad_amd import _lib

    name = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, name)
    lib = _lib.get_lib()
    print("recording", wc.GOLDENS[name], "from", lib.path, flush=True)
    np.savez_compressed(path, **record(lib, "cuda", wc.GOLDENS[name]))
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
