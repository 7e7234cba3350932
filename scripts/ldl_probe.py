#!/usr/bin/env python3
"""Diagnostic (GPU box): time of Theta_0 = (S + t I)^-1 beyond the eigensolver (uglad_init_theta: the L D L^T inverse of csrc/ldl_wide.h, as
ns_ldl_kernel or as the launches of ns_ldl_phase_kernel, + two Newton steps) per size, and its accuracy against numpy fp64.
python scripts/ldl_probe.py [--reps N] [D ...]   (N HIP-event timings after a warm-up, default 5; their median is printed last on the line.
UGLAD_LIB selects the build, UGLAD_LDL_LAUNCHES the form.)
python scripts/ldl_probe.py --hard [D ...]       the error table of the hard matrices of tests/ldl_cases.py (default D = 161 577) against numpy fp64, the
device next to torch.linalg.inv / torch.logdet in fp32 on the CPU, with the bounds tests/test_ldl_hard.py asserts; also written to
profiles/ldl_hard_errors.txt.  A record: no tolerance is taken from it."""
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


def hard_table(sizes):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ldl_cases as lc

    form = os.environ.get(lc.SWITCH)
    lines = [f"# scripts/ldl_probe.py --hard {' '.join(map(str, sizes))}   ({lc.SWITCH} = {form if form is not None else 'unset: the default form'})",
             "# ex = ||X - X64||_F / ||X64||_F, el = |logdet - slogdet|, res = ||A X - I||_F / sqrt(D), all against numpy fp64 on the fp32 input; unit = u || |X64| |A| |X64| ||_F / ||X64||_F;",
             "# growth = max(|L| |d| |L|^T) / max |A| of the fp64 unpivoted factorisation; t32 = torch.linalg.inv / torch.logdet, fp32, CPU.  init kinds: the logdet through the loss of S + t I",
             f"# {'D':>4s} {'kind':12s} {'cond':>8s} {'growth':>8s} | {'ex dev':>8s} {'ex t32':>8s} {'unit':>8s} {'dev/unit':>8s} {'t32/unit':>8s} | {'el dev':>8s} {'el t32':>8s} {'bound 2':>8s} | {'res dev':>8s} {'res t32':>8s}"]
    for D in sizes:
        for kind in lc.FAMILIES:
            a = lc.hard_matrix(kind, D, 0)
            A, ref = lc.inverted(kind, a), lc.hard_reference(kind, D, 0)
            a_in = lc.shifted32(a) if lc.entry_of(kind) == "init" else a  # what the factorisation starts from
            X = lc.run_on(lib, "cuda", lc.entry_of(kind), a[None], form)[0][0]
            logdet = -float(lc.run_on(lib, "cuda", "loss", a_in[None], form)[1][0])
            ref_in = ref if a_in is a else lc.reference64(a_in.astype(np.float64))
            t_inv, t_logdet = lc.torch32(a_in)
            ex, et = lc.inverse_error(X, ref), lc.inverse_error(t_inv, ref)
            lines.append(f"  {D:4d} {kind:12s} {np.linalg.cond(A):8.1e} {ref['growth']:8.1e} | {ex:8.1e} {et:8.1e} {ref['inv_unit']:8.1e} {ex / ref['inv_unit']:8.3f} "
                         f"{et / ref['inv_unit']:8.3f} | {abs(logdet - ref_in['logdet']):8.1e} {abs(t_logdet - ref_in['logdet']):8.1e} {ref_in['ld_bound']:8.1e} | "
                         f"{lc.residual(A, X):8.1e} {lc.residual(A, t_inv):8.1e}")
            print(lines[-1], flush=True)
    with open(os.path.join(ROOT, "profiles", "ldl_hard_errors.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if "--hard" in args:
    args.remove("--hard")
    hard_table([int(a) for a in args] or [161, 577])
    sys.exit(0)
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
