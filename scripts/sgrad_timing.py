"""Cost of the gradient with respect to S: one training pass (forward_uGLAD + backward) with and without S.requires_grad, alternating in
one process on the same GPU.  Configs: 3 (M = 1024, D = 128, L = 30), 1 (M = 1, D = 25, L = 15) and one D = 512 matrix, L = 15.
    python scripts/sgrad_timing.py [--reps 5] > profiles/sgrad_timing.txt"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import uglad_amd  # noqa: E402
from uglad_amd.utils.prepare_data import synthetic_covariance_batch  # noqa: E402


def one_pass(S, model, L, want):
    St = S.detach().clone().requires_grad_(want)
    model.zero_grad()
    _, loss = uglad_amd.forward_uGLAD(St, model, L=L)
    loss.backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for name, M, D, L in (("config 3", 1024, 128, 30), ("config 1", 1, 25, 15), ("D = 512", 1, 512, 15)):
        S = torch.from_numpy(synthetic_covariance_batch(M, D, seed=1)).cuda()
        torch.manual_seed(0)
        model = uglad_amd.GladParams(1.0, device="cuda")
        for want in (False, True):  # warm-up
            one_pass(S, model, L, want)
        times = {False: [], True: []}
        for _ in range(a.reps):
            for want in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(3):
                    one_pass(S, model, L, want)
                e1.record()
                torch.cuda.synchronize()
                times[want].append(e0.elapsed_time(e1) / 3)
        off, on = np.median(times[False]), np.median(times[True])
        print(f"{name:9s} M={M:5d} D={D:4d} L={L:2d}: without S.grad {off:8.3f} ms  with {on:8.3f} ms  ratio {on / off:.3f}  "
              f"(medians of {a.reps}; spread without {min(times[False]):.3f}-{max(times[False]):.3f}, with {min(times[True]):.3f}-{max(times[True]):.3f})",
              flush=True)


if __name__ == "__main__":
    main()
