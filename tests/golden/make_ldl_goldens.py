#!/usr/bin/env python3
"""Records tests/golden/ldl_parent_bits.npz ON THE GPU from the library under UGLAD_LIB (default: the in-tree build): what lib.init_theta and
lib.loss_fwd return, bit for bit, on the cases of tests/ldl_cases.py under every form of the L D L^T inverse, and their fp64 residuals.

The committed file was recorded on an MI355X from the build of the commit BEFORE the two hand-kept copies of the factorisation (ldl_inverse in
chol.h, the phase switch in wide_ns.h) became one phase function and one schedule (csrc/ldl_wide.h; same arithmetic): it is the parent's bits and
is not to be regenerated for a change that claims to keep them.

    UGLAD_LIB=<parent build> python tests/golden/make_ldl_goldens.py [out.npz]

Per case and form (keys "<case>/<form>/..."):
  X        (M, D, D) in full up to D = 160 (NaN canonical), else X_crc, a CRC32 per matrix of the same
  loss     (M,) for the loss_fwd cases
  res      (M, 2): ||A X - I||_F / sqrt(D) and |logdet - slogdet| in fp64, NaN where not finite
Reads nothing outside the repository."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import ldl_cases as lc  # noqa: E402


def record(lib, dev):
    out = {}
    for case in lc.GPU_CASES:
        for form in lc.forms(case):
            X, loss = lc.run(lib, dev, case, form)
            key = f"{lc.case_id(case)}/{lc.form_id(form)}/"
            if case[2] <= lc.FULL_UP_TO:
                out[key + "X"] = lc.canonical(X)
            else:
                out[key + "X_crc"] = lc.crc_per_matrix(lc.canonical(X))
            if loss is not None:
                out[key + "loss"] = lc.canonical(loss)
            out[key + "res"] = lc.backward_errors(case, X, loss)
            print(f"{key:40s} ||A X - I|| / sqrt(D) {out[key + 'res'][:, 0].max():.3e}   |logdet - slogdet| {out[key + 'res'][:, 1].max():.3e}"
                  f"   crc {lc.crc_per_matrix(lc.canonical(X))}", flush=True)
    return out


if __name__ == "__main__":
    from uglad_amd import _lib

    lib = _lib.get_lib()
    print("recording from", lib.path, flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ldl_parent_bits.npz")
    np.savez_compressed(path, **record(lib, "cuda"))
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
