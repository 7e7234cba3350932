#!/usr/bin/env python3
"""Per-kernel resource table of the built library: VGPRs, AGPRs, SGPRs, spills, scratch bytes per lane, LDS, workgroup size and the
scratch instructions that sit inside loops (a backward branch spans them) -- read from the gfx950 code object inside
uglad_amd/csrc/libuglad_hip.so with the ROCm LLVM tools; nothing is run on a GPU.

    python scripts/kernel_meta.py [--so PATH] [--filter SUBSTR] [--loops] > profiles/rNN_kernel_meta.txt
        (--loops disassembles every kernel of the table: about a minute for the whole library, seconds with --filter)
    python scripts/kernel_meta.py [--so PATH] --diff OTHER.so [--alias OLD=NEW ...]

--loops disassembles every kernel and counts scratch_load / scratch_store instructions inside backward-branch spans, the global load
instructions (gld) and the s_waitcnt with vmcnt <= 1 (vmwait): a kernel that waits about as often as it loads fetches its data one round
trip at a time (an `inside ? load : 0` that became a branch per entry, a load whose register another load's address was allocated into).
--diff compares the two libraries function by function (kernels and the device functions they call): the resource figures of the table and
the instruction encodings of the disassembly, addresses left out.  Exit status 1 on any difference -- what a refactor has to leave at 0.
--alias OLD=NEW (repeatable; exact symbols, as the "only in" lines print them): a function the refactor renamed -- OTHER.so's OLD is compared
with --so's NEW.
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def extract_code_object(so: str, out_dir: str) -> str:
    """The gfx950 ELF bundled into the host library."""
    co = os.path.join(out_dir, "gfx950.co")
    r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--list", "--type=o", f"--input={so}"], capture_output=True, text=True)
    targets = [t for t in r.stdout.split() if "gfx950" in t]
    if targets:
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={so}", f"--targets={targets[0]}",
                        f"--output={co}"], check=True, capture_output=True)
        if os.path.getsize(co) > 0:
            return co
    # a linked .so keeps the fat binary in section .hip_fatbin: cut it out and unbundle that
    fat = os.path.join(out_dir, "fatbin")
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
    data = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    objs = []
    pos = 0
    while True:
        i = data.find(magic, pos)
        if i < 0:
            break
        n = int.from_bytes(data[i + 24:i + 32], "little")
        p = i + 32
        for _ in range(n):
            off = int.from_bytes(data[p:p + 8], "little")
            size = int.from_bytes(data[p + 8:p + 16], "little")
            tlen = int.from_bytes(data[p + 16:p + 24], "little")
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                objs.append(data[i + off:i + off + size])
        pos = i + 24
    if not objs:
        raise SystemExit(f"no gfx950 code object in {so}")
    paths = []
    for k, o in enumerate(objs):
        pk = os.path.join(out_dir, f"gfx950_{k}.co")
        open(pk, "wb").write(o)
        paths.append(pk)
    return paths


def notes(co: str):
    """Kernel descriptors' metadata (msgpack rendered as YAML by llvm-readelf --notes)."""
    txt = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    kernels = []
    cur = None
    for line in txt.splitlines():
        m = re.match(r"\s+-?\s*\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip()
        if key == "agpr_count" or (key == "args" and cur is None):
            pass
        if line.lstrip().startswith("- .") and key in ("agpr_count", "args"):
            cur = {}
            kernels.append(cur)
        if cur is not None and key in ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                       "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size",
                                       "name", "uses_dynamic_stack"):
            cur[key] = val.strip("'\"")
    return [k for k in kernels if "name" in k]


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    out = r.stdout.splitlines()
    return dict(zip(names, out)) if len(out) == len(names) else {n: n for n in names}


def kernel_instr_stats(co: str, sym: str):
    """(scratch instructions, of them inside a backward-branch span, instructions, global loads, s_waitcnt with vmcnt <= 1) for one kernel
    symbol."""
    txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", f"--disassemble-symbols={sym}", co], capture_output=True, text=True).stdout
    ins = []  # (addr, mnemonic, target or None)
    loads = waits = 0
    for line in txt.splitlines():
        m = re.match(r"\s+(\S+)\s+(.*?)//\s*([0-9A-Fa-f]+):", line)
        if not m:
            continue
        addr = int(m.group(3), 16)
        mn = m.group(1)
        if mn.startswith(("global_load", "flat_load", "buffer_load")):
            loads += 1
        elif mn == "s_waitcnt":
            mv = re.search(r"vmcnt\((\d+)\)", m.group(2))
            if mv and int(mv.group(1)) <= 1:
                waits += 1
        tgt = None
        if mn.startswith("s_cbranch") or mn == "s_branch":
            mt = re.search(r"<[^>+]+\+0x([0-9a-fA-F]+)>", line)
            if mt:
                tgt = int(mt.group(1), 16)
        ins.append((addr, mn, tgt))
    if not ins:
        return 0, 0, 0, 0, 0
    base = ins[0][0]
    spans = [(base + t, a) for a, mn, t in ins if t is not None and base + t <= a]
    scr = [a for a, mn, _ in ins if mn.startswith("scratch_")]
    inside = sum(1 for a in scr if any(lo <= a <= hi for lo, hi in spans))
    return len(scr), inside, len(ins), loads, waits


def functions(so: str, td: str):
    """({symbol: resource figures} of the kernels, {symbol: [(encoding, text)]} of every function) over all code objects of a library."""
    os.makedirs(td)
    cos = extract_code_object(so, td)
    meta, code = {}, {}
    for co in [cos] if isinstance(cos, str) else cos:
        for k in notes(co):
            meta[k["name"]] = {f: v for f, v in k.items() if f != "name"}
        cur = None
        for line in subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout.splitlines():
            m = re.match(r"[0-9a-fA-F]+ <(.+)>:$", line)
            if m:
                cur = code.setdefault(m.group(1), [])
                continue
            m = re.match(r"\s+(.*?)\s*//\s*[0-9A-Fa-f]+:\s*(.*)$", line)  # text // address: encoding
            if m and cur is not None:
                cur.append((m.group(2).strip(), m.group(1)))
    return meta, code


def diff(so_a: str, so_b: str, aliases=()) -> int:
    with tempfile.TemporaryDirectory() as td:
        meta_a, code_a = functions(so_a, os.path.join(td, "a"))
        meta_b, code_b = functions(so_b, os.path.join(td, "b"))
    for old, new in (a.split("=", 1) for a in aliases):  # so_b's OLD goes by so_a's name NEW
        if old not in code_b or new not in code_a:
            raise SystemExit(f"--alias {old}={new}: {old} is not in {so_b} or {new} is not in {so_a}")
        code_b[new] = [(enc.replace(old, new), text) for enc, text in code_b.pop(old)]  # (a branch prints its target as <function+offset>)
        if old in meta_b:
            meta_b[new] = meta_b.pop(old)
    bad = 0
    for sym in sorted(set(code_a) ^ set(code_b)):
        print(f"only in {so_a if sym in code_a else so_b}: {sym}")
        bad += 1
    same = {True: 0, False: 0}  # by "is a kernel"
    for sym in sorted(set(code_a) & set(code_b)):
        why = None
        if meta_a.get(sym) != meta_b.get(sym):
            ma, mb = meta_a.get(sym) or {}, meta_b.get(sym) or {}
            why = "resources " + ", ".join(f"{f} {ma.get(f)} != {mb.get(f)}" for f in sorted(set(ma) | set(mb)) if ma.get(f) != mb.get(f))
        elif [e for e, _ in code_a[sym]] != [e for e, _ in code_b[sym]]:
            at = next((i for i, (x, y) in enumerate(zip(code_a[sym], code_b[sym])) if x[0] != y[0]), min(len(code_a[sym]), len(code_b[sym])))
            why = (f"{len(code_a[sym])} / {len(code_b[sym])} instructions, first difference at instruction {at}: "
                   f"{code_a[sym][at:at + 1]} != {code_b[sym][at:at + 1]}")
        if why:
            print(f"DIFFERENT {sym}: {why}")
            bad += 1
        else:
            same[sym in meta_a] += 1
    print(f"# {so_a} vs {so_b}: {same[True]} of {len(set(meta_a) | set(meta_b))} kernels and {same[False]} of "
          f"{len((set(code_a) | set(code_b)) - set(meta_a) - set(meta_b))} device functions identical "
          f"(resource figures and instruction encodings); {bad} differ")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--so", default=os.path.join(ROOT, "uglad_amd", "csrc", "libuglad_hip.so"))
    ap.add_argument("--filter", default="")
    ap.add_argument("--loops", action="store_true")
    ap.add_argument("--diff", metavar="OTHER.so", help="compare --so with this library instead of printing the table")
    ap.add_argument("--alias", metavar="OLD=NEW", action="append", default=[], help="with --diff: OTHER.so's function OLD is --so's NEW")
    a = ap.parse_args()
    if a.diff:
        return diff(a.so, a.diff, a.alias)
    with tempfile.TemporaryDirectory() as td:
        cos = extract_code_object(a.so, td)
        if isinstance(cos, str):
            cos = [cos]
        rows = []
        for co in cos:
            ks = notes(co)
            dm = demangle([k["name"] for k in ks])
            for k in ks:
                k["pretty"] = re.sub(r"\(.*$", "", dm[k["name"]]).replace("void ", "")
                k["co"] = co
                rows.append(k)
        rows = [k for k in rows if a.filter in k["pretty"]]
        rows.sort(key=lambda k: k["pretty"])
        print(f"# {os.path.relpath(a.so, ROOT)}: {len(rows)} kernels in {len(cos)} gfx950 code object(s)")
        hdr = f"{'kernel':58s} {'wg':>5s} {'vgpr':>5s} {'agpr':>5s} {'sgpr':>5s} {'vspill':>6s} {'sspill':>6s} {'scratchB':>8s} {'ldsB':>7s}"
        if a.loops:
            hdr += f" {'scr_ins':>7s} {'in_loops':>8s} {'gld':>5s} {'vmwait':>6s}"
        print(hdr)
        for k in rows:
            line = (f"{k['pretty'][:58]:58s} {k.get('max_flat_workgroup_size', '?'):>5s} {k.get('vgpr_count', '?'):>5s} "
                    f"{k.get('agpr_count', '?'):>5s} {k.get('sgpr_count', '?'):>5s} {k.get('vgpr_spill_count', '0'):>6s} "
                    f"{k.get('sgpr_spill_count', '0'):>6s} {k.get('private_segment_fixed_size', '0'):>8s} "
                    f"{k.get('group_segment_fixed_size', '0'):>7s}")
            if a.loops:
                n, inside, tot, loads, waits = kernel_instr_stats(k["co"], k["name"])
                line += f" {n:7d} {inside:8d} {loads:5d} {waits:6d}"
            print(line)


if __name__ == "__main__":
    sys.exit(main())
