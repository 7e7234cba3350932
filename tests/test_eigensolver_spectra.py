"""uglad_symeig (eig_lean.h behind tridiag.h / tridiag_wave.h) on the classic adversarial spectra of tests/eigensolver_cases.py: Wilkinson and glued
Wilkinson matrices, couplings around the skip threshold, clusters, repeated eigenvalues, and the matrices whose tridiagonal form has blocks far
below ||A|| (the constant matrix and its relatives) -- every one against numpy's fp64 eigvalsh of the fp32 input, with the bounds of that module.
The CPU tests run the kernel sources on the SIMT emulator (NT = 1, 2, 4, 5: all its build has); their GPU twins add NT = 3, 6, 7, 8, every
2^k + 1 split and the padded sizes 96 / 160, whose pole loads read past the merge.  One batch_symeig call per D."""
import json
import os

import numpy as np
import pytest
import torch

import eigensolver_cases as cases

EMUL_SIZES = [3, 5, 16, 17, 21, 32, 33, 64, 100, 128, 129, 160]
GPU_SIZES = EMUL_SIZES + [65, 96, 97, 161, 192, 193, 225, 255, 256]


def decompose_and_check(D, device, names=None, label=""):
    """All families of size D (or those in `names`) in one batch; every figure is printed, every violation reported at once."""
    import uglad_amd

    mats = cases.families(D)
    if names is not None:
        mats = {k: v for k, v in mats.items() if k in names}
    A32 = torch.from_numpy(np.stack(list(mats.values()))).float().contiguous()
    beta, U = uglad_amd.batch_symeig(A32.to(device))
    beta, U = beta.cpu().numpy(), U.cpu().numpy()
    failures, figures = [], {}
    for m, name in enumerate(mats):
        kind = cases.bound_kind(name)
        _, _, eig, res, orth = cases.measure(A32[m].numpy(), beta[m], U[m])
        figures[name] = (eig, res, orth)
        print(f"D={D:3d} {label}{name:24s} eig {eig:.2e} res {res:.2e} (bound {cases.bound(kind, D):.2e}) orth {orth:.2e}")
        try:
            cases.check(A32[m].numpy(), beta[m], U[m], kind, name)
        except AssertionError as err:
            failures.append(err.args[0])
    assert not failures, failures
    return figures


def emulated_names(D):
    return cases.REDUCED if D >= 129 else None


@pytest.mark.parametrize("D", EMUL_SIZES)
def test_adversarial_spectra(emul, D):
    decompose_and_check(D, torch.device("cpu"), emulated_names(D))


@pytest.mark.parametrize("D", [16, 21, 32])
def test_adversarial_spectra_workgroup_tridiagonalisation(emul, monkeypatch, D):
    """D <= 32 behind the workgroup kernels instead of the one-wave tridiagonalisation (on the constant matrix the two used to fail differently)."""
    monkeypatch.setenv("UGLAD_TRIDIAG_WAVE", "0")
    decompose_and_check(D, torch.device("cpu"))


def test_adversarial_spectra_512_thread_tridiagonalisation(emul, monkeypatch):
    monkeypatch.setenv("UGLAD_TRIDIAG_SMALL", "0")
    decompose_and_check(64, torch.device("cpu"))


# ----------------------------------------------------------------------------------------------- GPU twins
def record(D, label, figures):
    """Side output, for the record only (profiles/eigensolver_spectra.txt): with UGLAD_RECORD_DIR set, the worst figure per family group goes
    into eigensolver_spectra.json in that directory."""
    out_dir = os.environ.get("UGLAD_RECORD_DIR")
    if not out_dir:
        return
    try:
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, "eigensolver_spectra.json")
        data = json.load(open(path)) if os.path.exists(path) else {}
        row = {}
        for name, (eig, res, orth) in figures.items():
            g = row.setdefault(cases.group_of(name), {"eig": 0.0, "res": 0.0, "orth": 0.0, "bound": cases.bound(cases.bound_kind(name), D)})
            g["eig"], g["res"], g["orth"] = max(g["eig"], eig), max(g["res"], res), max(g["orth"], orth)
        data[f"{D:03d} {label}".strip()] = row
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def gpu_device():
    from uglad_amd import _lib

    h = _lib.get_lib()
    assert h.path.endswith("libuglad_hip.so") and h.require_gpu  # the native gfx950 build, nothing else
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("D", GPU_SIZES)
def test_adversarial_spectra_gpu(D):
    record(D, "", decompose_and_check(D, gpu_device()))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [21, 32])
def test_adversarial_spectra_workgroup_tridiagonalisation_gpu(monkeypatch, D):
    monkeypatch.setenv("UGLAD_TRIDIAG_WAVE", "0")
    record(D, "wave=0", decompose_and_check(D, gpu_device(), label="wave=0 "))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 96])
def test_adversarial_spectra_512_thread_tridiagonalisation_gpu(monkeypatch, D):
    monkeypatch.setenv("UGLAD_TRIDIAG_SMALL", "0")
    record(D, "small=0", decompose_and_check(D, gpu_device(), label="small=0 "))
