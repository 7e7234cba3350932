"""The masks of tridiag_kernel (csrc/tridiag.h): shapes, inputs and checks shared by the GPU test (test_tridiag_control_flow.py), its CPU twin on
the emulator (test_tridiag_control_flow_emulated.py) and the generator of the golden (golden/make_tridiag_goldens.py).  `lib` is the HipLib
under test, `dev` where its tensors live; everything goes through lib.tridiagonalize, the entry point bench.py times.

A CASE is one shape and one route: (D, M, environment switches).  Per case three launches:
  "plain3":  A0 = [seeded random symmetric, diagonal, block matrix], A1 = nullptr
  "plain2":  A0 = [random * 1e-17, random * 1e+15], A1 = nullptr
  "slz":     S / lam - Z, two matrices sharing one lambda
and for the cases with M > 3 (the 512-thread route beyond D = 128 needs M > 256) one launch "plainM" of M matrices: the five above, then seeded
random ones.
  diagonal: every column's squared norm below the sub-diagonal is 0 <= kNegligibleSig: no reflector at all.
  block:    A[:6, 6:] = 0, so columns 4 and 5 ARE zero below the sub-diagonal when the chain reaches them (zeroing column 5 of the input alone does
            not survive the first reflector).
  1e-17:    nrm2 <= 1e-30: the library square root and divisions of the tiny-norm path.
Rows n - 2 and n - 1 of R are not written by the kernel; R is zero-filled before every launch so that the whole slab compares."""
import os
import zlib

import numpy as np
import torch

# (D, M, switches): the smallest shapes at which each mask of the kernel can go wrong
W0 = {"UGLAD_TRIDIAG_WAVE": "0"}
CASES = [
    (128, 3, {}),   # 16-byte load path, three LDS slots, no padding
    (127, 3, {}),   # dword path, n < DP in the last lanes
    (97, 3, {}),    # NT = 4 with 31 padded rows and dead slots from step 0
    (96, 3, {}), (65, 3, {}),   # NT = 3: all slots in registers (128 NT threads)
    (64, 3, {}), (33, 3, {}),   # NT = 2
    (25, 3, W0), (32, 3, W0),   # NT = 1 on the workgroup kernel
    (2, 3, W0), (3, 3, W0), (4, 3, W0),   # zero, one, two reflectors: the k1 > n - 3 exits and the trailing 2 x 2 block
    (96, 3, {"UGLAD_TRIDIAG_SMALL": "0"}), (25, 3, {"UGLAD_TRIDIAG_SMALL": "0", "UGLAD_TRIDIAG_WAVE": "0"}),   # <3, 512>, <1, 512>
    # NS = 3, 4; M <= 256: tridiag_kernel<NT, 1024>, above: <NT, 512> (host_route.h)
    (129, 2, {}), (129, 257, {}), (160, 2, {}), (160, 257, {}), (256, 2, {}), (256, 257, {}),
]
SWITCHES = ("UGLAD_TRIDIAG_WAVE", "UGLAD_TRIDIAG_SMALL")
FULL_R_UP_TO = 33  # the golden keeps R itself up to this D, a CRC32 per matrix beyond
Q_CHECKED_OF_A_LARGE_BATCH = 6  # matrices of a "plainM" launch whose Q is rebuilt in fp64 (the five special inputs and one more)


def case_id(case):
    D, M, env = case
    return f"D{D}_M{M}" + "".join("_" + k.replace("UGLAD_TRIDIAG_", "").lower() + v for k, v in sorted(env.items()))


def expected_kernel(case):
    """The instantiation host_route.h sends this case to (asserted against the emulator's launch record where the emulator build has the NT)."""
    D, M, env = case
    nt = (D + 31) // 32
    if nt == 1 and env.get("UGLAD_TRIDIAG_WAVE", "1") != "0":
        return f"uglad::tridiag_wave_kernel<{nt}>"
    if nt <= 3 and env.get("UGLAD_TRIDIAG_SMALL", "1") != "0":
        return f"uglad::tridiag_kernel<{nt}, {128 * nt}>"
    return f"uglad::tridiag_kernel<{nt}, {1024 if nt > 4 and M <= 256 else 512}>"


def random_symmetric(D, seed):
    a = np.random.default_rng(seed).standard_normal((D, D))
    return ((a + a.T) / 2).astype(np.float32)


def inputs(case):
    """{launch: (A0, A1 or None, lam or None)} as float32 numpy arrays."""
    D, M, _ = case
    rnd = random_symmetric(D, 1000 + D)
    diag = np.diag(np.random.default_rng(2000 + D).standard_normal(D)).astype(np.float32)
    block = random_symmetric(D, 3000 + D)
    block[:6, 6:] = 0.0
    block[6:, :6] = 0.0
    tiny, huge = rnd * np.float32(1e-17), rnd * np.float32(1e15)
    S = np.stack([random_symmetric(D, 4000 + D), random_symmetric(D, 4001 + D)])
    Z = np.stack([random_symmetric(D, 5000 + D), random_symmetric(D, 5001 + D)])
    out = {"plain3": (np.stack([rnd, diag, block]), None, None), "plain2": (np.stack([tiny, huge]), None, None),
           "slz": (S, Z, np.array([0.5], dtype=np.float32))}
    if M > 3:
        out = {"plainM": (np.stack([rnd, diag, block, tiny, huge] + [random_symmetric(D, 6000 + D + i) for i in range(M - 5)]), None, None)}
    return out


def run(lib, dev, case, launch):
    """(tri (M, 3, DP), R (M, D, D)) of one launch, as numpy."""
    D = case[0]
    A0, A1, lam = launch
    M, DP = A0.shape[0], 32 * ((D + 31) // 32)
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}  # (the host layer reads its switches on every call)
    os.environ.update(case[2])
    try:
        a0 = torch.from_numpy(A0).to(dev).contiguous()
        a1 = torch.from_numpy(A1).to(dev).contiguous() if A1 is not None else None
        lm = torch.from_numpy(lam).to(dev) if lam is not None else None
        R = torch.zeros_like(a0)
        wsp = lib.workspace(M, D, a0)
        wsp.zero_()
        lib.tridiagonalize(a0, a1, lm, R, wsp)
        if dev != "cpu":
            torch.cuda.synchronize()
        return wsp[:M * 3 * DP].reshape(M, 3, DP).cpu().numpy().copy(), R.cpu().numpy().copy()
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def crc_per_matrix(R):
    return np.array([zlib.crc32(np.ascontiguousarray(r).tobytes()) for r in R], dtype=np.uint32)


def residuals(A, tri, R):
    """(||Q^T A Q - T||_F / ||A||_F, ||Q^T Q - I||_F) of one matrix in fp64: Q = H_0 ... H_{n-3}, H_k = I - tau_k v_k v_k^T, v_k = row k of R
    (0 up to column k, 1 at k + 1), T from d = tri[0], e = tri[1], tau = tri[2]."""
    n = A.shape[0]
    A = A.astype(np.float64)
    d, e, tau = (tri[i, :n].astype(np.float64) for i in range(3))
    Q = np.eye(n)
    for k in range(n - 2):
        v = R[k].astype(np.float64)
        Q -= tau[k] * np.outer(Q @ v, v)
    T = np.diag(d) + np.diag(e[:n - 1], 1) + np.diag(e[:n - 1], -1)
    return (float(np.linalg.norm(Q.T @ A @ Q - T) / max(np.linalg.norm(A), 1e-300)), float(np.linalg.norm(Q.T @ Q - np.eye(n))))


def matrix_of(launch, m):
    """The matrix the kernel factors, in fp64 from the fp32 inputs (the kernel's own rounding of S / lam - Z is part of what is measured)."""
    A0, A1, lam = launch
    return A0[m].astype(np.float64) if A1 is None else A0[m].astype(np.float64) / float(lam[0]) - A1[m].astype(np.float64)


def checked_matrices(launch):
    M = launch[0].shape[0]
    return range(M) if M <= 3 else list(range(Q_CHECKED_OF_A_LARGE_BATCH - 1)) + [M - 1]


def all_residuals(launch, tri, R):
    return np.array([residuals(matrix_of(launch, m), tri[m], R[m]) for m in checked_matrices(launch)])
