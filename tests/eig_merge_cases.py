"""The merges of the divide & conquer (csrc/eig_lean.h, csrc/wide_fwd.h): sizes, inputs and runs shared by the GPU test (test_eig_merge_bits.py)
and the generator of its golden (golden/make_eig_goldens.py).  `lib` is the HipLib under test.

Two groups of calls:
  symeig   uglad_symeig through batch_symeig's entry point, one call per D of SYMEIG_SIZES on the batch symeig_inputs(D): every NT from 1 to 8,
           every 2^k and 2^k + 1 split, an odd leaf, the padded sizes 96 / 160 whose pole loads read past the merge, four and two lanes per root,
           the paired update at NT = 4 and the 8-lane secular pass at bs = 256.
  cell     uglad_cell_fwd (NS10) at CELL_SHAPES with the matrix iteration switched off, once with many workgroups per matrix (the last merge handed
           over to wide_secular_kernel / wide_merge_kernel) and once without.
Every input comes from np.random.default_rng(seed) and elementwise arithmetic (no BLAS, no LAPACK), so that it is the same array on every machine;
the golden keeps a CRC32 of each input batch all the same."""
import os
import zlib

import numpy as np
import torch

import eigensolver_cases as cases

SYMEIG_SIZES = [3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 224, 255, 256]
FULL_UP_TO = 33  # the golden keeps beta and U themselves up to this D, a CRC32 per matrix beyond
# the families of eigensolver_cases.families built without LAPACK (no random orthogonal basis)
PLAIN_FAMILIES = ["wilkinson", "glued wilkinson", "toeplitz 1-2-1", "weak coupling", "tridiag random", "decaying tridiagonal", "ones", "0.37 ones",
                  "ones block + zero block", "two ones blocks", "kms", "arrowhead", "identity + rank one", "near-diagonal 1e-6"]
CLUSTER = "repeated diagonal + 1e-7 symmetric"  # in place of the clusters eigensolver_cases makes with a QR factor
DENSE = ["dense random 0", "dense random 1"]
CELL_SHAPES = [(129, 2), (160, 2), (256, 2)]  # (D, M): NT = 5 (two lanes per root at the 64- and 128-pole merges), the padded 160, NT = 8
CELL_OUTPUTS = ("Z_out", "U_out", "beta_out", "normF_partial")
SQRT_NS10 = 1


def random_symmetric(D, seed):
    a = np.random.default_rng(seed).standard_normal((D, D))
    return (a + a.T) / 2


def symeig_inputs(D):
    """name -> fp64 symmetric D x D matrix, in a fixed order."""
    fam = cases.families(D)
    out = {k: fam[k] for k in PLAIN_FAMILIES if k in fam}
    out[CLUSTER] = np.diag(np.repeat(np.linspace(-1.0, 1.0, (D + 3) // 4), 4)[:D]) + 1e-7 * random_symmetric(D, 7000 + D)
    for s, name in enumerate(DENSE):
        out[name] = random_symmetric(D, 8000 + 2 * D + s)
    return out


def bound_kind(name):
    """Which bound of eigensolver_cases a family has to meet: runs of coinciding poles are pushed apart (C), everything else is general (G)."""
    return "C" if name == CLUSTER else "G" if name in DENSE else cases.bound_kind(name)


def symeig_batch(D):
    return np.stack(list(symeig_inputs(D).values())).astype(np.float32)


def run_symeig(lib, dev, A32):
    """(beta (M, D), U (M, D, D)) as numpy."""
    A = torch.from_numpy(A32).to(dev).contiguous()
    U = torch.empty_like(A)
    beta = torch.empty(A.shape[:2], dtype=A.dtype, device=A.device)
    lib.symeig(A, U, beta)
    if dev != "cpu":
        torch.cuda.synchronize()
    return beta.cpu().numpy().copy(), U.cpu().numpy().copy()


def trained_params():
    """The 42 parameters of golden/params_trained.npz in the order the kernels take them."""
    pz = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "params_trained.npz"))
    return np.concatenate([pz[k].ravel() for k in pz.files]).astype(np.float32)


def cell_inputs(D, M, params):
    """(S, Z_in, lam, params) as float32 numpy: b = S / lam - Z_in is what the cell decomposes."""
    i = np.arange(D)
    S = np.stack([0.5 ** np.abs(i[:, None] - i[None, :]) + 0.05 * random_symmetric(D, 9000 + D + m) for m in range(M)])
    Z = np.stack([0.5 * np.eye(D) + 0.02 * random_symmetric(D, 9500 + D + m) for m in range(M)])
    return S.astype(np.float32), Z.astype(np.float32), np.array([1.0], dtype=np.float32), np.asarray(params, dtype=np.float32)


def run_cell(lib, dev, inputs, wide):
    """{output: numpy array} of one uglad_cell_fwd call on the eigensolver route, with (wide = 1) or without (0) the handed-over last merge."""
    S, Z, lam, params = (torch.from_numpy(x).to(dev).contiguous() for x in inputs)
    M, D, _ = S.shape
    lib.set_matrix_iteration(0)
    lib.set_wide_mode(wide)
    try:
        Z_out, half, U = (torch.zeros_like(S) for _ in range(3))
        beta = torch.zeros(M, D, dtype=S.dtype, device=S.device)
        nfp = torch.zeros(M, dtype=S.dtype, device=S.device)
        wsp = lib.workspace(M, D, S)
        wsp.zero_()
        lib.cell_fwd(S, Z, lam, params, Z_out, half, U, beta, nfp, wsp, SQRT_NS10)
        if dev != "cpu":
            torch.cuda.synchronize()
        return {"Z_out": Z_out.cpu().numpy().copy(), "U_out": U.cpu().numpy().copy(), "beta_out": beta.cpu().numpy().copy(),
                "normF_partial": nfp.cpu().numpy().copy()}
    finally:
        lib.set_wide_mode(-1)
        lib.set_matrix_iteration(-1)


def crc(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes())


def crc_per_matrix(x):
    return np.array([crc(r) for r in x], dtype=np.uint32)
