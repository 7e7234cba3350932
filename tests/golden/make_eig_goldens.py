#!/usr/bin/env python3
"""Records tests/golden/eig_parent_bits.npz ON THE GPU from the library under UGLAD_LIB (default: the in-tree build): what uglad_symeig and the
eigensolver route of uglad_cell_fwd return, bit for bit, on the cases of tests/eig_merge_cases.py.

The committed file was recorded on an MI355X from the build of the commit BEFORE the merge phases of csrc/eig_lean.h got one statement each for
the wave-local and the workgroup-wide levels (same arithmetic, same launches): it is the parent's bits and is not to be regenerated for a change
that claims to keep them.

    UGLAD_LIB=<parent build> python tests/golden/make_eig_goldens.py [out.npz]

Keys:
  symeig/D<D>/input_crc           CRC32 of the fp32 input batch
  symeig/D<D>/beta, U             in full up to D = 33, else beta_crc, U_crc: a CRC32 per matrix
  cell/D<D>_M<M>/input_crc        CRC32 of S, Z_in, lam and the parameters, in this order
  cell/D<D>_M<M>/wide<w>/<out>    a CRC32 per matrix of Z_out, U_out, beta_out and normF_partial
Every call runs twice and has to give the same bits both times.  Reads nothing outside the repository."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import eig_merge_cases as ec  # noqa: E402
import eigensolver_cases as cases  # noqa: E402


def record(lib, dev):
    out = {}
    for D in ec.SYMEIG_SIZES:
        names, A32 = list(ec.symeig_inputs(D)), ec.symeig_batch(D)
        beta, U = ec.run_symeig(lib, dev, A32)
        again = ec.run_symeig(lib, dev, A32)
        assert beta.tobytes() == again[0].tobytes() and U.tobytes() == again[1].tobytes(), f"D={D}: two runs differ"
        key = f"symeig/D{D}/"
        out[key + "input_crc"] = np.array([ec.crc(A32)], dtype=np.uint32)
        if D <= ec.FULL_UP_TO:
            out[key + "beta"], out[key + "U"] = beta, U
        else:
            out[key + "beta_crc"], out[key + "U_crc"] = ec.crc_per_matrix(beta), ec.crc_per_matrix(U)
        worst = np.zeros(3)
        for m, name in enumerate(names):
            worst = np.maximum(worst, cases.check(A32[m], beta[m], U[m], ec.bound_kind(name), name))
        print(f"{key:16s} {len(names):2d} matrices   worst eig {worst[0]:.2e} res {worst[1]:.2e} orth {worst[2]:.2e}", flush=True)
    params = ec.trained_params()
    for D, M in ec.CELL_SHAPES:
        inputs = ec.cell_inputs(D, M, params)
        key = f"cell/D{D}_M{M}/"
        out[key + "input_crc"] = np.array([ec.crc(x) for x in inputs], dtype=np.uint32)
        for wide in (1, 0):
            got, again = ec.run_cell(lib, dev, inputs, wide), ec.run_cell(lib, dev, inputs, wide)
            for name in ec.CELL_OUTPUTS:
                assert got[name].tobytes() == again[name].tobytes(), f"{key}wide{wide}/{name}: two runs differ"
                assert np.isfinite(got[name]).all(), f"{key}wide{wide}/{name}"
                out[f"{key}wide{wide}/{name}"] = ec.crc_per_matrix(got[name])
            print(f"{key}wide{wide}  beta in [{got['beta_out'].min():.3e}, {got['beta_out'].max():.3e}]  normF_partial {got['normF_partial']}", flush=True)
    return out


if __name__ == "__main__":
    from uglad_amd import _lib

    lib = _lib.get_lib()
    print("recording from", lib.path, flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "eig_parent_bits.npz")
    np.savez_compressed(path, **record(lib, "cuda"))
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
