#!/usr/bin/env python3
"""Records tests/golden/tridiag_parent_bits.npz ON THE GPU from the library under UGLAD_LIB (default: the in-tree build): what
lib.tridiagonalize returns, bit for bit, on the cases of tests/tridiag_control_flow_cases.py, and the fp64 residuals of the (Q, T) it stands for.

The committed file was recorded on an MI355X from the build of the commit BEFORE tridiag_kernel's lane and slot masks were rewritten (same
arithmetic, selects instead of branches): it is the parent's bits and is not to be regenerated for a change that claims to keep them.

    UGLAD_LIB=<parent build> python tests/golden/make_tridiag_goldens.py [out.npz]

Per case and launch (keys "<case>/<launch>/..."):
  tri      (M, 3, DP) in full for the launches of up to three matrices; for the batches of 257 only the matrices whose Q is rebuilt (a committed
           file stays below 1 MiB), and tri_crc, a CRC32 per matrix, for all of them
  R        (M, D, D) in full up to D = 33, else R_crc, a CRC32 per matrix
  res      (matrices checked, 2): ||Q^T A Q - T||_F / ||A||_F and ||Q^T Q - I||_F in fp64
Reads nothing outside the repository."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import tridiag_control_flow_cases as tc  # noqa: E402


def record(lib, dev):
    out = {}
    for case in tc.CASES:
        for name, launch in tc.inputs(case).items():
            tri, R = tc.run(lib, dev, case, launch)
            key = f"{tc.case_id(case)}/{name}/"
            if tri.shape[0] <= 3:
                out[key + "tri"] = tri
            else:
                out[key + "tri"] = tri[list(tc.checked_matrices(launch))]
                out[key + "tri_crc"] = tc.crc_per_matrix(tri)
            if case[0] <= tc.FULL_R_UP_TO:
                out[key + "R"] = R
            else:
                out[key + "R_crc"] = tc.crc_per_matrix(R)
            out[key + "res"] = tc.all_residuals(launch, tri, R)
            print(f"{key:28s} worst ||Q^T A Q - T|| / ||A|| {out[key + 'res'][:, 0].max():.3e}   ||Q^T Q - I|| {out[key + 'res'][:, 1].max():.3e}",
                  flush=True)
    return out


if __name__ == "__main__":
    from uglad_amd import _lib

    lib = _lib.get_lib()
    print("recording from", lib.path, flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "tridiag_parent_bits.npz")
    np.savez_compressed(path, **record(lib, "cuda"))
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
