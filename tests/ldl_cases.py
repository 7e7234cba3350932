"""The L D L^T inverse beyond the eigensolver (csrc/ldl_wide.h) in its two kernel forms: shapes, inputs and checks shared by the GPU test
(test_ldl_forms.py), its CPU twin on the emulator (test_ldl_forms_emulated.py) and the generator of the golden (golden/make_ldl_goldens.py).
`lib` is the HipLib under test, `dev` where its tensors live.

A CASE is (entry point, M, D, input):
  "init": lib.init_theta of synthetic_covariance_batch(M, D, 4 D, seed=D) with golden/params_trained.npz -> Theta_0 = (S + t I)^-1
  "loss": lib.loss_fwd of Q diag(w) Q^T, w = linspace(0.5, 5, D), S = I -> the loss (-logdet + trace) and the inverse; the inputs
          "spd"    as it stands
          "neg2"   two negative eigenvalues: finite logdet, finite inverse
          "neg3"   three: NaN loss (torch.logdet of a negative determinant), finite inverse
          "pivot0" A[0, 0] = 0: the first pivot is zero, NaN everywhere (the not-ok path)
A FORM is the value of UGLAD_LDL_LAUNCHES: "0" one workgroup per matrix (ns_ldl_kernel), "1" one launch per phase (ns_ldl_phase_kernel), None unset
(host_route.h decides: launches from nt = ceil(D / 32) = 9)."""
import os
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCH = "UGLAD_LDL_LAUNCHES"
LOSS_INPUTS = ("spd", "neg2", "neg3", "pivot0")
# (entry, M, D, input) -- why this shape
GPU_CASES = [
    ("init", 1, 129, None),    # nt = 5, ragged last tile, first size on this path
    ("init", 3, 150, None),    # a batch: slab stride, blockIdx -> matrix
    ("init", 1, 160, None),    # D = padded size exactly
    ("init", 1, 256, None),    # config 5's own route (default: one workgroup)
    ("init", 1, 288, None),    # first size past the crossover (default: launches)
    ("init", 1, 577, None),    # nt = 19 > 16 waves: the one-workgroup walk wraps its tile loops; dp^2 > 512 * 256: the capped element grids wrap
    ("init", 1, 1025, None),   # the 2048 x 2049 layout (FD = 2048), nt = 33
] + [("loss", 1, 200, k) for k in LOSS_INPUTS]  # sign count, logdet rules, the not-ok path
DEFAULT_TOO = (256, 288)  # the sizes on either side of the crossover also run with the switch unset
# the emulator build's eigensolver ends at D = 160 and every work-item is a fiber: 161 and 170 stand in for 129 .. 160, 1025 is GPU-only
EMUL_CASES = [("init", 1, 161, None), ("init", 2, 170, None)] + [("loss", 1, 200, k) for k in LOSS_INPUTS] + [("init", 1, 577, None)]
FULL_UP_TO = 160  # the golden keeps the outputs themselves up to this D, a CRC32 per matrix beyond


def case_id(case):
    entry, M, D, kind = case
    return f"{entry}_M{M}_D{D}" + (f"_{kind}" if kind else "")


def forms(case):
    return ("0", "1") + ((None,) if case[2] in DEFAULT_TOO else ())


def form_id(form):
    return {"0": "one_workgroup", "1": "launches", None: "default"}[form]


def expected_launches(case, form):
    """(kernel instantiation, number of its launches) host_launch.h sends this case to.  The schedule of nt block columns has 5 nt steps:
    Init, nt Diag, nt - 1 Panel and Trail each, nt - 1 WSum and WMul each, Scale, X, Finish."""
    D = case[2]
    nt, fd = (D + 31) // 32, 1024 if D <= 1024 else 2048
    launches = form == "1" if form is not None else nt >= 9
    return (f"uglad::ns_ldl_phase_kernel<{fd}>", 5 * nt) if launches else (f"uglad::ns_ldl_kernel<{fd}>", 1)


_cache = {}


def packed_params():
    """((42,) float32 tensor the kernels read, t = theta_init_offset) of golden/params_trained.npz."""
    if "params" not in _cache:
        import uglad_amd

        pz = np.load(os.path.join(HERE, "golden", "params_trained.npz"))
        m = uglad_amd.GladParams(1.0)
        m.load_state_dict({k: torch.from_numpy(np.array(pz[k])) for k in pz.files})
        _cache["params"] = (m.packed().detach().contiguous(), float(m.state_dict()["theta_init_offset"].item()))
    return _cache["params"]


def matrices(case):
    """(M, D, D) float32: what the entry point is given.  Computed once per case and left unchanged."""
    if case not in _cache:
        entry, M, D, kind = case
        if entry == "init":
            from uglad_amd.utils.prepare_data import synthetic_covariance_batch

            a = synthetic_covariance_batch(M, D, 4 * D, seed=D)
        else:
            Q, _ = np.linalg.qr(np.random.default_rng(1).standard_normal((D, D)))
            w = np.linspace(0.5, 5.0, D)
            negatives = {"neg2": 2, "neg3": 3}.get(kind, 0)
            w[:negatives] = [-1.0, -3.0, -0.7][:negatives]
            a = ((Q * w) @ Q.T)[None]
            if kind == "pivot0":
                a[0, 0, 0] = 0.0
        _cache[case] = np.ascontiguousarray(a, dtype=np.float32)
        _cache[case].setflags(write=False)
    return _cache[case]


def factored(case):
    """(M, D, D) float64: the matrices the kernels invert, from the fp32 inputs."""
    A = matrices(case).astype(np.float64)
    return A + packed_params()[1] * np.eye(case[2]) if case[0] == "init" else A


def run(lib, dev, case, form):
    """(X (M, D, D), loss (M,) or None) of one call under one form, as numpy float32."""
    entry, M, D, _ = case
    saved = os.environ.pop(SWITCH, None)  # (the host layer reads its switches on every call)
    if form is not None:
        os.environ[SWITCH] = form
    try:
        A = torch.from_numpy(matrices(case).copy()).to(dev)
        X = torch.zeros_like(A)
        wsp = lib.workspace(M, D, A)
        loss = None
        if entry == "init":
            lib.init_theta(A, packed_params()[0].to(dev), 0, X, wsp)
        else:
            loss = torch.zeros(M, dtype=torch.float32, device=dev)
            lib.loss_fwd(A, torch.eye(D, dtype=torch.float32, device=dev)[None].contiguous(), None, loss, X, wsp)
        if dev != "cpu":
            torch.cuda.synchronize()
        return X.cpu().numpy().copy(), None if loss is None else loss.cpu().numpy().copy()
    finally:
        os.environ.pop(SWITCH, None)
        if saved is not None:
            os.environ[SWITCH] = saved


def crc_per_matrix(X):
    return np.array([zlib.crc32(np.ascontiguousarray(x).tobytes()) for x in X], dtype=np.uint32)


def same_bits(a, b):
    """Equal bits where finite, NaN in the same places (NaN payloads are not compared)."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.where(na, np.float32(0), a).tobytes() == np.where(nb, np.float32(0), b).tobytes()


def canonical(X):
    """X with every NaN replaced by the one quiet NaN, so that a CRC32 compares bits where finite and NaN-ness elsewhere."""
    X = np.array(X, dtype=np.float32)
    X[np.isnan(X)] = np.float32(np.nan)
    return X


def logdet_of(case, loss):
    """The device's log-determinant out of its loss: loss = -logdet + trace(A S), S = I (the trace in fp64 from the fp32 input)."""
    return np.trace(factored(case), axis1=1, axis2=2) - loss.astype(np.float64)


def slogdet(case):
    """fp64 log|det|, NaN for a negative determinant (torch.logdet's rule)."""
    sign, val = np.linalg.slogdet(factored(case))
    return np.where(sign > 0, val, np.nan)


def forward_errors(case, X, loss):
    """Per matrix (||X - X64||_F / ||X64||_F, |logdet - slogdet|) against numpy fp64; NaN where the device or the reference has none."""
    A = factored(case)
    with np.errstate(all="ignore"):
        ref = np.linalg.inv(A)
        ex = np.array([np.linalg.norm(x.astype(np.float64) - r) / np.linalg.norm(r) for x, r in zip(X, ref)])
        el = np.abs(logdet_of(case, loss) - slogdet(case)) if loss is not None else np.full(len(X), np.nan)
    return np.stack([ex, el], axis=1)


def backward_errors(case, X, loss):
    """Per matrix (||A X - I||_F / sqrt(D), |logdet - slogdet|) in fp64; NaN where not finite."""
    A, D = factored(case), case[2]
    with np.errstate(all="ignore"):
        rx = np.array([np.linalg.norm(a @ x.astype(np.float64) - np.eye(D)) / np.sqrt(D) for a, x in zip(A, X)])
        rl = np.abs(logdet_of(case, loss) - slogdet(case)) if loss is not None else np.full(len(X), np.nan)
    return np.stack([rx, rl], axis=1)


def within_twice(got, parent):
    """got <= 2 parent wherever the parent is finite; NaN exactly where the parent has NaN."""
    got, parent = np.asarray(got, dtype=np.float64), np.asarray(parent, dtype=np.float64)
    nan = np.isnan(parent)
    return np.array_equal(np.isnan(got), nan) and bool(np.all(got[~nan] <= 2 * parent[~nan]))
