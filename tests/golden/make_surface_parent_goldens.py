"""Records tests/golden/surface_parent_bits.npz: every output of tests/surface_cases.py, as the commit BEFORE the Python surface was
consolidated computes it on an MI355X (outputs of up to surface_cases.FULL_UP_TO elements in full, a CRC32 beyond).

    PYTHONPATH=<built checkout of that commit> python tests/golden/make_surface_parent_goldens.py [OUT.npz]

(without PYTHONPATH the package of this checkout is recorded: that is how a golden is checked against itself, not how it is made.)

Every case runs twice and must repeat itself bit for bit.  An output that does not is kept in full with the relative Frobenius distance of
its two recordings under "<output>|spread", which the test doubles into its tolerance; no output of a pass may need that, and the outputs
of at most two other cases.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.append(os.path.join(HERE, "..", ".."))

import surface_cases as sc  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "surface_parent_bits.npz")
    import uglad_amd

    print(f"recording the package at {os.path.dirname(os.path.abspath(uglad_amd.__file__))}", flush=True)
    golden, loose = {}, set()
    for case in sc.cases():
        first, second = sc.run(case), sc.run(case)
        assert sorted(first) == sorted(second)
        for key, a in first.items():
            if sc.same_bits(second[key], sc.stored(a)):
                golden[key] = sc.stored(a)
                continue
            a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(second[key], dtype=np.float64)
            golden[key] = sc.canonical(a)
            golden[key + "|spread"] = np.float64(np.linalg.norm(a64 - b64) / max(np.linalg.norm(a64), 1e-300))
            loose.add(case)
            print(f"NOT REPEATED  {key}: spread {golden[key + '|spread']:.3e}", flush=True)
        print(f"{case}: {len(first)} outputs", flush=True)
    assert not any(c.startswith("pass/") for c in loose), f"a pass does not repeat itself: {sorted(loose)}"
    assert len(loose) <= 2, f"more than two cases do not repeat themselves -- shorten them: {sorted(loose)}"
    np.savez_compressed(out, **golden)
    print(f"{out}: {len(golden)} entries, {os.path.getsize(out)} bytes; not repeated: {sorted(loose) or 'none'}")


if __name__ == "__main__":
    main()
