#!/usr/bin/env python3
"""What every entry point touches of its buffers: the GPU cases of tests/test_buffer_contract.py through the same run_case
(tests/buffer_contract.py), one row per case.

    python scripts/buffer_contract_probe.py [--out profiles/buffer_contract.txt] [--only SUBSTRING]

Per case: the entry point, shape and route switches; the four verdicts (confined, independent, inputs, rc); the wall time of the case (four
calls and their checks); then one line per buffer of the call in allocation order:
  ws   a workspace: the floats uglad_workspace_floats / uglad_*_workspace_floats returned, and the first and last float the call changed
  out  an output: its size in bytes and the first and last byte the call changed
  scr  an argument the header declares as scratch: as an output
`changed` is the union over the three fills (0x00, 0xFF, 0x7F): a byte counts where it differs from the fill after the call, so a word the
call sets to zero shows under 0xFF and 0x7F.  `-` = the call changed nothing of it.  The extent shows where a sizing function asks for far
more than is used, or exactly as much, which leaves no slack.  Nothing asserts on it."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import buffer_contract as bc  # noqa: E402
import buffer_contract_cases as cases_  # noqa: E402


def rows(res):
    yield f"{res.id}  {res.verdicts()}  {res.seconds * 1e3:.0f} ms"
    for key, (nbytes, lo, hi, scratch) in res.touched.items():
        name = key.split(":", 1)[1]
        if scratch and name.startswith(("workspace", "_wide_workspace")):
            ext = "-" if lo is None else f"{lo // 4} .. {hi // 4}"
            slack = "" if hi is None else f"  ({nbytes // 4 - 1 - hi // 4} floats behind the last)"
            yield f"    ws   {nbytes // 4} floats, changed {ext}{slack}"
        else:
            ext = "-" if lo is None else f"{lo} .. {hi}"
            yield f"    {'scr' if scratch else 'out'}  {name}: {nbytes} bytes, changed {ext}"
    for p in res.problems[:12]:
        yield "    ! " + p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "buffer_contract.txt"))
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    from uglad_amd import _lib

    lib = _lib.get_lib()
    t0 = time.perf_counter()
    lines, bad = [], 0
    todo = [c for c in cases_.cases("cuda") if args.only in c.id]
    for case in todo:
        res = bc.run_case(case, raise_on_failure=False)
        bad += not res.ok
        lines += list(rows(res))
        print(lines[-1 - len(res.touched) - len(res.problems[:12])], flush=True)
    head = [f"buffer contract of {len(todo)} cases on {torch.cuda.get_device_name(0)}, library version {lib.version}: guards of {bc.GUARD_BYTES} bytes, "
            f"fills {', '.join(f'0x{f:02X}' for f in bc.FILLS)}", f"{bad} cases fail a verdict; {time.perf_counter() - t0:.1f} s in all", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    print(head[1])


if __name__ == "__main__":
    main()
