"""Every entry point held to its buffers: no store outside them, no load of a word the call did not define (include/uglad_hip.h: the caller
owns the workspace, inputs are const, outputs have stated extents).  A helper module like wide_cases.py: no conftest, no pytest setting.

`guarded_buffers(device, fill)` replaces torch.empty / torch.empty_like for its duration: every buffer the wrappers (uglad_amd/_lib.py,
glad/glad.py, main.py) allocate on the library's device comes out of a uint8 tensor with `guard_bytes` on either side, every byte of it
set to `fill`.  `check()` says what became of the guards and which part of the interior the call changed.  `run_case(case)` runs one call
four times from the same inputs -- plain, then under each of the three fills -- and asserts

  1. confinement     every guard of every buffer intact under every fill;
  2. independence    every output bit-equal across the four runs: an element the call never writes differs between the fills, and so does
                     one computed from scratch the call read before it wrote it;
  3. inputs          every input tensor bit-equal to its clone from before the call;
  4. return code 0.

The fills: 0x00; 0xFF, a NaN as fp32 and fp64 and -1 as int32; 0x7F, 3.39e38 as fp32 and 1.38e306 as fp64 -- finite, because a stale NaN is
swallowed by fmaxf and by an integer atomicMax on float bits (eig_lean.h has one), a huge finite value is not.

A CASE is any object with
  id        str
  device    where the library's tensors live ("cuda", or "cpu" on the emulator)
  inputs()  -> {name: tensor}, seeded; called once, the same tensors go into all four calls
  call(inputs) -> {name: tensor}: the outputs the wrappers return.  They name the buffers they are (by address) and are compared like them;
            a nonzero return code arrives as UgladError
  exempt    {buffer name: key of EXEMPTIONS}, for the two buffers the header leaves partly undefined
Buffers are matched across the runs in allocation order.  A buffer is an OUTPUT unless its allocation site is one of SCRATCH_SITES: the
workspace, and the arguments the header declares as scratch (guarded, their touched extent recorded, their contents not compared).
"""
import linecache
import os
import re
import sys
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import torch

FILLS = (0x00, 0xFF, 0x7F)
GUARD_BYTES = 65536  # twice the largest single tile the wide kernels store (64 x 64 fp64 = 32 KiB); a multiple of 512: the interior keeps the allocator's alignment

# ---- what is guarded but not compared: (file, function, assigned name) of the allocation -> the header's word for it
SCRATCH_SITES = {
    ("_lib.py", "workspace", None): "workspace: caller-owned scratch of uglad_workspace_floats(M, D) floats",
    ("_lib.py", "_wide_workspace", None): "workspace: caller-owned scratch of uglad_*_workspace_floats floats",
    ("_lib.py", "covariance", "scratch"): "eig_scratch (K*D*D + K*D floats); its eigenvalue tail is compared through HipLib.covariance's min_eig",
    ("_lib.py", "conditional_mean", "scratch"): "scratch (K*D*D floats) of uglad_conditional_mean",
    ("glad.py", "backward", "bufs"): "gbuf0 / gbuf1 of uglad_glad_backward*: scratch",
}


# ---- the two outputs the header leaves partly undefined.  Nothing is added here: anything else that turns out partly written is a finding.
def _edges_up_to_count(t: torch.Tensor, outputs: Dict[str, torch.Tensor]) -> torch.Tensor:
    """The first edge_count[k] entries of every problem of edge_ij (K, E, 2) / edge_w (K, E), one after the other."""
    m = outputs["edge_count"].cpu().tolist()
    return torch.cat([t[k, :m[k]].reshape(-1) for k in range(t.shape[0])]) if t.shape[0] else t.reshape(-1)


def _nothing(t: torch.Tensor, outputs: Dict[str, torch.Tensor]) -> torch.Tensor:
    return t.reshape(-1)[:0]


@dataclass(frozen=True)
class Exemption:
    header: str  # the sentence of include/uglad_hip.h that grants it
    defined: Callable  # (buffer, the run's outputs) -> the part that is compared


EXEMPTIONS = {
    "graph_wide.edges": Exemption(
        "uglad_graph_wide: \"edge_ij (K, E, 2) int32 and edge_w (K, E) fp32, the first m entries of a problem in the reference's order, the "
        "rest undefined\"", _edges_up_to_count),
    "matrix_iteration.beta": Exemption(
        "the matrix-iteration path: \"U's slot of the saved tensors carries the square root, beta's stays unused\"", _nothing),
}


# ---------------------------------------------------------------------------------------------------------------- the guarded allocator
@dataclass
class Buffer:
    index: int
    site: str  # file:function:line of the torch.empty call
    name: str  # the name it is assigned to there (or site#k); a returned output's name wins
    scratch: Optional[str]  # SCRATCH_SITES' word, or None for an output
    dtype: torch.dtype
    shape: Tuple[int, ...]
    nbytes: int
    view: torch.Tensor  # what the caller received
    raw: Optional[torch.Tensor]  # the uint8 tensor with its guards (None in a plain run)
    k: int = 0  # which torch.empty of its statement it is


@dataclass
class BufferReport:
    """check() of one buffer.  Byte offsets count from the start of the interior: negative in the left guard, >= nbytes in the right one."""
    index: int
    name: str
    site: str
    scratch: Optional[str]
    nbytes: int
    left_ok: bool
    right_ok: bool
    left: Optional[Tuple[int, int, int]]  # (first, last, count) of the changed bytes of the left guard, None when intact
    right: Optional[Tuple[int, int, int]]
    touched: Optional[Tuple[int, int]]  # first and last interior byte that differs from the fill, None when none does

    @property
    def confined(self) -> bool:
        return self.left_ok and self.right_ok


_ASSIGN = re.compile(r"(\w+)\s*=\s*\(?\s*torch\.empty(?:_like)?\(")
_TARGETS = re.compile(r"^\s*([\w\s,]+?)\s*=[^=]")
_CALLS = re.compile(r"torch\.empty(?:_like)?\(")


def _extent(mask: torch.Tensor) -> Optional[Tuple[int, int, int]]:
    """(first, last, count) of the set entries of a 1-D bool tensor, None when none is set."""
    n = int(mask.sum().item())
    if n == 0:
        return None
    m8 = mask.to(torch.uint8)
    first = int(torch.argmax(m8).item())
    last = mask.numel() - 1 - int(torch.argmax(m8.flip(0)).item())
    return first, last, n


class guarded_buffers:
    """Context manager (see the module's docstring).  fill = None: the plain run -- the real functions, only recorded."""

    def __init__(self, device, fill: Optional[int], guard_bytes: int = GUARD_BYTES):
        if guard_bytes % 512 or guard_bytes <= 0:
            raise ValueError("guard_bytes must be a positive multiple of 512 (the interior keeps the allocator's alignment)")
        if fill is not None and not 0 <= fill <= 255:
            raise ValueError("fill is one byte")
        self.device = torch.device(device)
        self.fill = fill
        self.guard = guard_bytes
        self.buffers: List[Buffer] = []
        self._saved = None

    # -- the patch
    def __enter__(self):
        self._saved = (torch.empty, torch.empty_like)
        real_empty, real_like = self._saved
        me = self

        def empty(*size, **kw):
            dev = torch.device(kw["device"]) if kw.get("device") is not None else torch.device("cpu")
            if dev.type != me.device.type or not me._plain_kwargs(kw):
                return real_empty(*size, **kw)
            shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(int(s) for s in size)
            return me._allocate(shape, kw.get("dtype") or torch.get_default_dtype(), dev, sys._getframe(1), lambda: real_empty(*size, **kw))

        def empty_like(inp, **kw):
            dev = torch.device(kw["device"]) if kw.get("device") is not None else inp.device
            if dev.type != me.device.type or not me._plain_kwargs(kw):
                return real_like(inp, **kw)
            return me._allocate(tuple(inp.shape), kw.get("dtype") or inp.dtype, dev, sys._getframe(1), lambda: real_like(inp, **kw))

        torch.empty, torch.empty_like = empty, empty_like
        return self

    def __exit__(self, *exc):
        torch.empty, torch.empty_like = self._saved
        return False

    @staticmethod
    def _plain_kwargs(kw) -> bool:
        """Only allocations the wrappers make are guarded: shape, dtype, device.  `out=`, pinned memory, strides and the like go through."""
        return all(k in ("dtype", "device") or (k == "requires_grad" and not v) for k, v in kw.items())

    def _allocate(self, shape, dtype, dev, frame, real):
        n = 1
        for s in shape:
            n *= int(s)
        nbytes = n * torch.zeros(0, dtype=dtype).element_size()
        if self.fill is None:
            raw, view = None, real()
        else:
            raw = torch.full((nbytes + 2 * self.guard,), self.fill, dtype=torch.uint8, device=dev)
            view = raw[self.guard:self.guard + nbytes].view(dtype).view(shape)
        site, name, scratch, k = self._site(frame)
        self.buffers.append(Buffer(len(self.buffers), site, name, scratch, dtype, tuple(shape), nbytes, view, raw, k))
        return view

    def _site(self, frame):
        code, line = frame.f_code, frame.f_lineno
        fname = os.path.basename(code.co_filename)
        site = f"{fname}:{code.co_name}:{line}"
        text = linecache.getline(code.co_filename, line)
        # the k-th torch.empty of this line: the calls of one statement follow one another
        ncalls = len(_CALLS.findall(text))
        k = (self.buffers[-1].k + 1) % max(1, ncalls) if self.buffers and self.buffers[-1].site == site else 0
        direct = _ASSIGN.findall(text)
        targets = _TARGETS.match(text)
        targets = [t.strip() for t in targets.group(1).split(",")] if targets else []
        if len(direct) == ncalls and ncalls:
            name = direct[k]
        elif len(targets) == ncalls and ncalls:
            name = targets[k]
        elif len(targets) == 1:
            name = targets[0] if ncalls <= 1 else f"{targets[0]}[{k}]"
        else:
            name = f"{code.co_name}:{line}#{k}"
        base = name.split("[")[0]
        scratch = SCRATCH_SITES.get((fname, code.co_name, None)) or SCRATCH_SITES.get((fname, code.co_name, base))
        return site, name, scratch, k

    # -- the verdict
    def check(self) -> List[BufferReport]:
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        out = []
        for b in self.buffers:
            if b.raw is None:
                out.append(BufferReport(b.index, b.name, b.site, b.scratch, b.nbytes, True, True, None, None, None))
                continue
            g, n = self.guard, b.nbytes
            left = _extent(b.raw[:g] != self.fill)
            right = _extent(b.raw[g + n:] != self.fill)
            inner = _extent(b.raw[g:g + n] != self.fill) if n else None
            out.append(BufferReport(
                b.index, b.name, b.site, b.scratch, n, left is None, right is None,
                None if left is None else (left[0] - g, left[1] - g, left[2]),
                None if right is None else (right[0] + n, right[1] + n, right[2]),
                None if inner is None else inner[:2]))
        return out

    def release_scratch(self):
        """Drops what is not compared (the workspaces are the large ones); check() has been called."""
        for b in self.buffers:
            if b.scratch is not None:
                b.view = b.raw = None


# ---------------------------------------------------------------------------------------------------------------- one case, four runs
def bits(t: torch.Tensor) -> torch.Tensor:
    """The bytes of a tensor, 1-D uint8: what `torch.equal` compares here (NaN payloads and signed zeros count)."""
    x = t.detach().reshape(-1)
    if x.numel() and x.stride(0) != 1:  # (one element of a strided slice keeps its stride)
        x = x.new_zeros(x.shape).copy_(x)
    return x.view(torch.uint8)


def _diff(a: torch.Tensor, b: torch.Tensor) -> Optional[Tuple[int, int, int]]:
    a, b = bits(a), bits(b)
    if a.numel() != b.numel():
        return (0, max(a.numel(), b.numel()) - 1, abs(a.numel() - b.numel()))
    if torch.equal(a, b):
        return None
    return _extent(a != b)


@dataclass
class CaseResult:
    id: str
    confinement: bool = True
    independence: bool = True
    inputs_untouched: bool = True
    rc: object = 0
    problems: List[str] = field(default_factory=list)
    # per buffer name: (nbytes, first touched byte, last touched byte) -- the union over the three fills; scratch flagged
    touched: Dict[str, Tuple[int, Optional[int], Optional[int], bool]] = field(default_factory=dict)
    seconds: float = 0.0

    @property
    def ok(self) -> bool:
        return self.confinement and self.independence and self.inputs_untouched and self.rc == 0

    def verdicts(self) -> str:
        f = lambda v: "ok" if v else "FAIL"  # noqa: E731
        return f"confined={f(self.confinement)} independent={f(self.independence)} inputs={f(self.inputs_untouched)} rc={self.rc}"


def _one_run(case, inputs, fill, guard_bytes):
    """(outputs, buffers, reports, rc) of one call under one fill (None: plain)."""
    from uglad_amd._lib import UgladError

    rc = 0
    with guarded_buffers(case.device, fill, guard_bytes) as gb:
        try:
            outputs = dict(case.call(inputs) or {})
        except UgladError as e:  # a nonzero return code of the C entry point
            outputs, rc = {}, str(e)
    rc = outputs.pop("rc", rc)
    reports = gb.check()
    # a returned output that IS a guarded buffer gives it its name; the others (clones, sums) are compared as they are
    by_ptr = {b.view.data_ptr(): b for b in gb.buffers if b.nbytes}
    extra = {}
    for name, t in outputs.items():
        if t is None:
            continue
        b = by_ptr.get(t.data_ptr()) if t.numel() else None
        if b is not None and b.nbytes == t.numel() * t.element_size():
            b.name = name
            reports[b.index].name = name
        else:
            extra[name] = t.detach().clone()
    named = {name: t for name, t in outputs.items() if t is not None}
    return named, extra, gb, reports, rc


def run_case(case, guard_bytes: int = GUARD_BYTES, raise_on_failure: bool = True) -> CaseResult:
    t0 = time.perf_counter()
    res = CaseResult(case.id)
    inputs = case.inputs()
    before = {k: v.detach().clone() for k, v in inputs.items() if torch.is_tensor(v)}
    exempt = dict(getattr(case, "exempt", None) or {})
    runs = []
    for fill in (None,) + FILLS:
        tag = "plain" if fill is None else f"fill 0x{fill:02X}"
        named, extra, gb, reports, rc = _one_run(case, inputs, fill, guard_bytes)
        # 4. return code
        if rc != 0:
            res.rc = rc
            res.problems.append(f"return code [{tag}]: {rc}")
        # 1. confinement
        for r in reports:
            if not r.confined:
                res.confinement = False
                for side, ext in (("left", r.left), ("right", r.right)):
                    if ext is not None:
                        res.problems.append(f"confinement [{tag}]: buffer {r.index} {r.name} ({r.site}, {r.nbytes} bytes): {side} guard changed at "
                                            f"bytes {ext[0]} .. {ext[1]} ({ext[2]} bytes) from the interior's start")
            if fill is not None:
                key = f"{r.index}:{r.name}"
                n, lo, hi, s = res.touched.get(key, (r.nbytes, None, None, r.scratch is not None))
                if r.touched is not None:
                    lo = r.touched[0] if lo is None else min(lo, r.touched[0])
                    hi = r.touched[1] if hi is None else max(hi, r.touched[1])
                res.touched[key] = (r.nbytes, lo, hi, r.scratch is not None)
        # 3. inputs
        if gb.device.type == "cuda":
            torch.cuda.synchronize()
        for k, v in before.items():
            d = _diff(inputs[k], v)
            if d is not None:
                res.inputs_untouched = False
                res.problems.append(f"inputs [{tag}]: {k} changed at bytes {d[0]} .. {d[1]} ({d[2]} bytes)")
                inputs[k].detach().copy_(v)  # (the next run starts from the same inputs)
        # what this run leaves to compare: every output buffer (the part the header defines) and every other returned tensor
        compare = {}
        for b, r in zip(gb.buffers, reports):
            if b.scratch is None:
                key = f"{b.index}:{r.name}"
                ex = exempt.get(r.name)
                compare[key] = EXEMPTIONS[ex].defined(b.view, named).clone() if ex else b.view
        for name, t in extra.items():
            compare[f"returned:{name}"] = t
        gb.release_scratch()
        runs.append((tag, compare, [(b.site, b.nbytes) for b in gb.buffers]))
    # 2. independence
    tag0, ref, sites0 = runs[0]
    for tag, compare, sites in runs[1:]:
        if sites != sites0:
            res.independence = False
            res.problems.append(f"independence [{tag}]: the call allocated other buffers than the plain run ({len(sites)} vs {len(sites0)})")
            continue
        for key, t in compare.items():
            d = _diff(t, ref[key])
            if d is not None:
                res.independence = False
                res.problems.append(f"independence [{tag} vs {tag0}]: output {key} ({tuple(t.shape)}, {t.dtype}) differs at bytes {d[0]} .. {d[1]} "
                                    f"({d[2]} bytes)")
    res.seconds = time.perf_counter() - t0
    if raise_on_failure:
        assert res.ok, f"{case.id}: {res.verdicts()}\n  " + "\n  ".join(res.problems[:40])
    return res
