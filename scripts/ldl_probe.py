#!/usr/bin/env python3
"""Diagnostic (GPU box): time of Theta_0 = (S + t I)^-1 beyond the eigensolver (uglad_init_theta: the L D L^T inverse of csrc/ldl_wide.h, as
ns_ldl_kernel or as the launches of ns_ldl_phase_kernel, + two Newton steps) per size, and its accuracy against numpy fp64.
python scripts/ldl_probe.py [--reps N] [D ...]   (N HIP-event timings after a warm-up, default 5; their median is printed last on the line.
UGLAD_LIB selects the build, UGLAD_LDL_LAUNCHES the form.)"""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import uglad_amd
from uglad_amd import _lib
from uglad_amd.utils.prepare_data import synthetic_covariance_batch
args = sys.argv[1:]
reps = 5
if "--reps" in args:
    reps = int(args[args.index("--reps") + 1]); del args[args.index("--reps"):args.index("--reps") + 2]
lib = _lib.get_lib()
pz = np.load(os.path.join(ROOT, "tests", "golden", "params_trained.npz"))
m = uglad_amd.GladParams(1.0, device="cuda"); m.load_state_dict({k: torch.from_numpy(np.array(pz[k])) for k in pz.files})
pk = m.packed().detach().contiguous()
t_off = float(m.state_dict()["theta_init_offset"].item())
for D in [int(a) for a in args] or [320, 512, 1024, 2048]:
    Snp = synthetic_covariance_batch(1, D, 4 * D, seed=D)
    S = torch.from_numpy(Snp).cuda(); Z = torch.empty_like(S); wsp = lib.workspace(1, D, S)
    for _ in range(3): lib.init_theta(S, pk, 0, Z, wsp)
    torch.cuda.synchronize()
    ref = np.linalg.inv(Snp[0].astype(np.float64) + t_off * np.eye(D))
    err = np.linalg.norm(Z[0].cpu().numpy() - ref) / np.linalg.norm(ref)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record(); lib.init_theta(S, pk, 0, Z, wsp); b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in evs]
    print(f"D={D:5d}: rel-Frobenius vs fp64 inverse {err:.2e}; per call, HIP events (ms): " + " ".join(f"{v:.3f}" for v in ms)
          + f"; median {float(np.median(ms)):.4f}", flush=True)
