#!/usr/bin/env python3
"""Records tests/golden/wide_parent_bits.npz ON THE GPU from the library under UGLAD_LIB (default: the in-tree build): what the HipLib wrappers
of the many-workgroup fp64 utilities return, bit for bit, on the cases of tests/wide_cases.py.

The committed file was recorded on an MI355X from the build of the commit BEFORE the utilities' shared pieces got one owner each (the shift
bisection and two reduction helpers in csrc/chol_wide.h, the radix sort in csrc/sort_wide.h, the entry points in csrc/host_wide.h; same
arithmetic, same launches): it is the parent's bits and is not to be regenerated for a change that claims to keep them.

    UGLAD_LIB=<parent build> python tests/golden/make_wide_parent_goldens.py [out.npz]

Per case and output (keys "<case>/<output>/..."): the first case of every entry point in full, ".../<k>" the array of problem k (NaN canonical);
the others ".../crc", a CRC32 per problem of the same.  Reads nothing outside the repository."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import wide_cases as wc  # noqa: E402


def record(lib, dev):
    out = {}
    for case in wc.CASES:
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

    lib = _lib.get_lib()
    print("recording from", lib.path, flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "wide_parent_bits.npz")
    np.savez_compressed(path, **record(lib, "cuda"))
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
