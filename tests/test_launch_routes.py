"""CPU: which kernels every C-ABI call launches -- kernel instantiation, grid, block, scalar and pointer arguments -- pinned against
tests/golden/launch_routes.json.

The SIMT emulator's hipLaunchKernelGGL (tests/simt_emul/hip/hip_runtime.h) appends one line per launch to the file UGLAD_EMUL_LAUNCH_LOG
names and, under UGLAD_EMUL_RECORD_ONLY=1, does not execute.  The host layer never reads a device result back, so a record-only run takes every
host decision of a real run; the pointers handed in are made-up addresses, one 64 GiB range per buffer, which makes every workspace offset
part of the record.  Every process configuration (environment switches, uglad_set_* calls) runs in a process of its own: a value set through the
API cannot be unset.

The fixture (per group of calls the numbers, the return codes and a digest of the whole record: summarise()) was recorded from the host layer as
it stood BEFORE it was split into routing / launch / entry-point headers (same emulator hook, nothing else changed) with
`python tests/test_launch_routes.py --record <library>`; it is not to be regenerated for a refactoring.

The emulator build has NT = ceil(D / 32) in {1, 2, 4, 5}; the dispatch of NT = 3, 6, 7, 8 (D = 65..96, 161..256) through the one-workgroup and wide
paths, and tridiag_kernel<3, 384>, are reached on the GPU only (tests/test_gpu_parity.py: the goldens at D = 96, 200, 256)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "launch_routes.json")

# ---------------------------------------------------------------------------------------------------------------- the table
L = 2
FULL = "full"      # whole passes + per-step entry points + numbers
PASSES = "passes"  # whole passes + numbers
DEFAULT_SHAPES = [  # (M, D, groups)
    (1, 25, 1), (4, 25, 2), (4, 25, 4), (3, 33, 1), (2, 64, 1), (2, 128, 1),
    # matrix-iteration crossover: M ceil(D / 64)^2 <= 96 and M <= 8 training, <= 256 forward-only (9 tiles per matrix at D = 129, 160)
    (1, 129, 1), (8, 129, 1), (9, 129, 1), (28, 129, 1), (29, 129, 1),
    (8, 160, 1), (9, 160, 1), (28, 160, 1), (29, 160, 1), (4, 160, 2), (4, 160, 4),
    # wide: D > 192 or M <= 128; the 1024-thread tridiagonalisation: M <= 256
    (128, 160, 1), (129, 160, 1), (256, 160, 1), (257, 160, 1),
    # no eigensolver in this build: the matrix iteration; its 32 / 64 fp64 tile at 256 tiles of 64 x 64
    (1, 161, 1), (28, 161, 1), (29, 161, 1), (1, 288, 1), (2, 288, 2),
]
SMALL = [(1, 25, 1), (4, 25, 4), (3, 33, 1), (2, 64, 1), (2, 128, 1)]
LARGE = [(1, 129, 1), (9, 160, 1), (129, 160, 1)]
NS = [(1, 129, 1), (1, 161, 1), (29, 161, 1), (1, 288, 1)]
# (name, environment, setter calls, shapes, what to run)
CONFIGS = [
    ("default", {}, [], DEFAULT_SHAPES, FULL),
    ("UGLAD_TRIDIAG_WAVE=0", {"UGLAD_TRIDIAG_WAVE": "0"}, [], SMALL, FULL),
    ("UGLAD_TRIDIAG_WAVE=1", {"UGLAD_TRIDIAG_WAVE": "1"}, [], SMALL[:2], PASSES),
    ("UGLAD_NO_FUSED_LAMBDA=1", {"UGLAD_NO_FUSED_LAMBDA": "1"}, [], SMALL + LARGE, PASSES),
    ("UGLAD_TRIDIAG_SMALL=0", {"UGLAD_TRIDIAG_SMALL": "0"}, [], SMALL, FULL),
    ("UGLAD_TRIDIAG_SMALL=1", {"UGLAD_TRIDIAG_SMALL": "1"}, [], SMALL[:2], PASSES),
    ("UGLAD_TRIDIAG_SMALL=0,UGLAD_TRIDIAG_WAVE=0", {"UGLAD_TRIDIAG_SMALL": "0", "UGLAD_TRIDIAG_WAVE": "0"}, [], SMALL, PASSES),
    ("UGLAD_CHOLESKY=0", {"UGLAD_CHOLESKY": "0"}, [], SMALL + LARGE, FULL),
    ("UGLAD_CHOLESKY=1", {"UGLAD_CHOLESKY": "1"}, [], SMALL[:2], PASSES),
    ("UGLAD_PERSISTENT_BWD=0", {"UGLAD_PERSISTENT_BWD": "0"}, [], SMALL + [(4, 25, 2)], PASSES),
    ("UGLAD_PERSISTENT_BWD=1", {"UGLAD_PERSISTENT_BWD": "1"}, [], SMALL[:2], PASSES),
    ("UGLAD_NS_PREFETCH_ALL=0", {"UGLAD_NS_PREFETCH_ALL": "0"}, [], NS, FULL),
    ("UGLAD_NS_PREFETCH_ALL=1", {"UGLAD_NS_PREFETCH_ALL": "1"}, [], NS[:2], PASSES),
    ("UGLAD_LDL_LAUNCHES=0", {"UGLAD_LDL_LAUNCHES": "0"}, [], NS, FULL),
    ("UGLAD_LDL_LAUNCHES=1", {"UGLAD_LDL_LAUNCHES": "1"}, [], NS, FULL),
    ("UGLAD_NS_TILE=64", {"UGLAD_NS_TILE": "64"}, [], NS, FULL),
    ("UGLAD_NS_TILE=32", {"UGLAD_NS_TILE": "32"}, [], NS, PASSES),
    ("UGLAD_WIDE_BWD=0", {"UGLAD_WIDE_BWD": "0"}, [], LARGE + [(8, 160, 1)], FULL),
    ("UGLAD_WIDE_BWD=1", {"UGLAD_WIDE_BWD": "1"}, [], LARGE + [(8, 160, 1), (257, 160, 1), (2, 128, 1)], FULL),
    ("UGLAD_MATRIX_ITERATION=0", {"UGLAD_MATRIX_ITERATION": "0"}, [], LARGE + [(1, 25, 1), (1, 161, 1)], FULL),
    ("UGLAD_MATRIX_ITERATION=1", {"UGLAD_MATRIX_ITERATION": "1"}, [], LARGE + [(1, 25, 1), (4, 25, 2), (255, 64, 1), (256, 64, 1), (1, 161, 1)], FULL),
    # a value set through the API wins over the environment
    ("set_wide_mode(0)", {"UGLAD_WIDE_BWD": "1"}, [("uglad_set_wide_mode", 0)], LARGE, PASSES),
    ("set_wide_mode(1)", {"UGLAD_WIDE_BWD": "0"}, [("uglad_set_wide_mode", 1)], LARGE + [(257, 160, 1)], PASSES),
    ("set_wide_mode(-1)", {"UGLAD_WIDE_BWD": "1"}, [("uglad_set_wide_mode", -1)], LARGE, PASSES),
    ("set_matrix_iteration(0)", {"UGLAD_MATRIX_ITERATION": "1"}, [("uglad_set_matrix_iteration", 0)], LARGE + [(1, 25, 1)], PASSES),
    ("set_matrix_iteration(1)", {"UGLAD_MATRIX_ITERATION": "0"}, [("uglad_set_matrix_iteration", 1)], LARGE + [(1, 25, 1)], PASSES),
    ("set_matrix_iteration(-1)", {"UGLAD_MATRIX_ITERATION": "1"}, [("uglad_set_matrix_iteration", -1)], LARGE + [(1, 25, 1)], PASSES),
    ("set_wide_mode(2),set_matrix_iteration(-2)", {}, [("uglad_set_wide_mode", 2), ("uglad_set_matrix_iteration", -2)], [(1, 129, 1)], PASSES),
]
# not in the fixture: compared with the default configuration's record (`=0` means "not disabled", like every other switch)
NOT_DISABLED = ("UGLAD_NO_FUSED_LAMBDA=0", {"UGLAD_NO_FUSED_LAMBDA": "0"}, [], SMALL, PASSES)
SWITCHES = ("UGLAD_TRIDIAG_WAVE", "UGLAD_NO_FUSED_LAMBDA", "UGLAD_TRIDIAG_SMALL", "UGLAD_CHOLESKY", "UGLAD_PERSISTENT_BWD", "UGLAD_NS_PREFETCH_ALL",
            "UGLAD_LDL_LAUNCHES", "UGLAD_NS_TILE", "UGLAD_WIDE_BWD", "UGLAD_MATRIX_ITERATION")

# ---------------------------------------------------------------------------------------------------------------- the worker
BUFFERS = ["S", "params", "Z", "half", "U", "beta", "lam", "lam_in", "nf_partial", "nf_sum", "cond_max", "ws", "G_L", "gbuf0", "gbuf1", "grp", "glam",
           "gt", "grad", "gS", "Zin", "Zout", "theta_inv", "loss", "struct", "ctx", "X", "scratch", "a", "b", "c", "d"]
SIGS = {
    "uglad_init_theta": "ppippii", "uglad_init_theta_bwd": "ppippii", "uglad_lambda_init": "pfpp", "uglad_cell_fwd": "p" * 11 + "iii",
    "uglad_cell_fwd_stage2": "p" * 11 + "iii", "uglad_sum_partials": "pip", "uglad_lambda_step": "pfpppp", "uglad_cell_bwd": "p" * 12 + "iii",
    "uglad_loss_fwd": "ppippppii", "uglad_loss_bwd": "pppippfpii", "uglad_loss_bwd_wrt_s": "pppippfppii", "uglad_finish_grads": "ppppppii",
    "uglad_glad_forward": "ppfiipi" + "p" * 9 + "iii", "uglad_glad_backward": "pppii" + "p" * 13 + "iii",
    "uglad_glad_forward_grouped": "ppfiipi" + "p" * 9 + "iiii", "uglad_glad_backward_grouped": "pppii" + "p" * 13 + "iiii",
    "uglad_glad_backward_wrt_s": "pppii" + "p" * 13 + "iiiip", "uglad_glad_forward_sharded": "ppfiipi" + "p" * 9 + "iiiipp",
    "uglad_symeig": "ppppii", "uglad_covariance": "piiiifppp", "uglad_tridiagonalize": "pppppii", "uglad_symeig_jacobi": "pppii",
    "uglad_conditional_mean": "p" * 9 + "iii", "uglad_support_metrics": "pppiii",
}
CT = {"p": ctypes.c_void_p, "i": ctypes.c_int, "f": ctypes.c_float}
EXCHANGE = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)


def short(line):
    """'void uglad::k<1>(float const*, int) [grid] [block] args' -> 'uglad::k<1> [grid] [block] args': the instantiation names the kernel."""
    head, rest = line.split(" [", 1)
    depth, i = 0, len(head) - 1
    while i >= 0:  # the parameter list: the balanced parentheses the symbol ends with
        depth += (head[i] == ")") - (head[i] == "(")
        if depth == 0:
            break
        i -= 1
    head = head[:i] if head.endswith(")") and i > 0 else head
    return head.replace("void ", "", 1) + " [" + rest


class Recorder:
    def __init__(self, lib_path, log_path):
        self.dll = ctypes.CDLL(lib_path)
        self.log = log_path
        for name, sig in SIGS.items():
            fn = getattr(self.dll, name)
            fn.argtypes = [CT[c] for c in sig] + [ctypes.c_void_p]
            fn.restype = ctypes.c_int
        self.exchange = EXCHANGE(lambda buf, n, ctx, stream: 0)
        self.out = {}

    def call(self, key, name, *args):
        vals = []
        for a in args:
            if isinstance(a, str):  # a buffer: its made-up address (never dereferenced in a record-only run)
                a = (BUFFERS.index(a) + 1) << 36
            vals.append(a)
        open(self.log, "w").close()
        rc = getattr(self.dll, name)(*vals, None)
        with open(self.log) as f:
            self.out[key] = {"rc": rc, "launches": [short(line) for line in f.read().splitlines()]}

    def numbers(self, key, M, D):
        d = self.dll
        self.out[key] = {"workspace_floats": d.uglad_workspace_floats(M, D),
                         "cond_is_upper_bound": [d.uglad_cond_is_upper_bound(M, D, t, s) for t in (0, 1) for s in (0, 1, 2)]}

    def passes(self, M, D, G):
        k = f"M{M} D{D} G{G}"
        self.numbers(k + " numbers", M, D)
        state = ("half", "U", "beta")
        nostate = (None, None, None)
        tail = ("lam", "lam_in", "nf_partial", "nf_sum")
        bwd = ("G_L", "S", "params", 0, L, "Z", "half", "U", "beta", "lam", "lam_in", "gbuf0", "gbuf1", "grp", "glam", "gt", "grad", "ws", M, D)
        for sq in (1, 0):
            for st, tag in ((state, "train"), (nostate, "fwdonly")):
                self.call(f"{k} forward {tag} sqrt{sq}", "uglad_glad_forward_grouped", "S", "params", 1.0, 0, L, "Z", L + 1 if st[0] else 2, *st, *tail,
                          "cond_max" if sq else None, "ws", M, D, G, sq)
            self.call(f"{k} backward sqrt{sq}", "uglad_glad_backward_grouped", *bwd, G, sq)
            self.call(f"{k} backward gS sqrt{sq}", "uglad_glad_backward_wrt_s", *bwd, G, sq, "gS")
        self.call(f"{k} forward init_diag1", "uglad_glad_forward_grouped", "S", "params", 1.0, 1, L, "Z", L + 1, *state, *tail, None, "ws", M, D, G, 1)
        self.call(f"{k} backward init_diag1 gS", "uglad_glad_backward_wrt_s", *bwd[:3], 1, *bwd[4:], G, 1, "gS")
        self.call(f"{k} backward init_diag1", "uglad_glad_backward_grouped", *bwd[:3], 1, *bwd[4:], G, 1)
        if G == 1:  # the entry points without a group count, and the sharded pass with an injected exchange
            self.call(f"{k} forward ungrouped", "uglad_glad_forward", "S", "params", 1.0, 0, L, "Z", L + 1, *state, *tail, "cond_max", "ws", M, D, 1)
            self.call(f"{k} backward ungrouped", "uglad_glad_backward", *bwd, 1)
            for st, tag in ((state, "train"), (nostate, "fwdonly")):
                self.call(f"{k} sharded {tag}", "uglad_glad_forward_sharded", "S", "params", 1.0, 0, L, "Z", 2, *st, *tail, "cond_max", "ws", M, D, 3 * M, 1,
                          ctypes.cast(self.exchange, ctypes.c_void_p).value, "ctx")

    def steps(self, M, D):
        k = f"M{M} D{D} step"
        for idg in (0, 1, 2):
            self.call(f"{k} init_theta {idg}", "uglad_init_theta", "S", "params", idg, "Z", "ws", M, D)
            self.call(f"{k} init_theta_bwd {idg}", "uglad_init_theta_bwd", "Z", "gbuf0", idg, "gt", "ws", M, D)
        cell = ("S", "Zin", "lam", "params", "Zout")
        for sq in (0, 1, 2):
            self.call(f"{k} cell_fwd train sqrt{sq}", "uglad_cell_fwd", *cell, "half", "U", "beta", "nf_partial", "cond_max", "ws", M, D, sq)
            self.call(f"{k} cell_fwd fwdonly sqrt{sq}", "uglad_cell_fwd", *cell, None, None, None, "nf_partial", None, "ws", M, D, sq)
            self.call(f"{k} cell_fwd_stage2 sqrt{sq}", "uglad_cell_fwd_stage2", *cell, "half", "U", "beta", "nf_partial", "cond_max", "ws", M, D, sq)
            self.call(f"{k} cell_bwd sqrt{sq}", "uglad_cell_bwd", "G_L", "S", "Zin", "half", "U", "beta", "lam", "params", "gbuf0", "grp", "glam", "ws", M, D, sq)
        self.call(f"{k} loss_fwd", "uglad_loss_fwd", "Z", "S", M, "struct", "loss", "theta_inv", "ws", M, D)
        self.call(f"{k} loss_fwd shared S", "uglad_loss_fwd", "Z", "S", 1, None, "loss", "theta_inv", "ws", M, D)
        self.call(f"{k} loss_bwd_wrt_s", "uglad_loss_bwd_wrt_s", "Z", "theta_inv", "S", M, None, "a", 0.5, "gbuf0", "gS", M, D)
        self.call(f"{k} lambda_init", "uglad_lambda_init", "params", 1.0, "lam", "lam_in")
        self.call(f"{k} sum_partials", "uglad_sum_partials", "nf_partial", M, "nf_sum")
        self.call(f"{k} lambda_step", "uglad_lambda_step", "nf_sum", 0.25, "lam", "params", "a", "b")
        self.call(f"{k} finish_grads", "uglad_finish_grads", "gt", "grp", "glam", "lam_in", "params", "grad", L, M)
        # the utilities that share the dispatch on NT and the tridiagonalisation launch
        self.call(f"{k} symeig", "uglad_symeig", "a", "U", "beta", "ws", M, D)
        self.call(f"{k} covariance", "uglad_covariance", "X", M, 40, D, 1, 0.1, "S", "scratch", "ws")
        self.call(f"{k} covariance plain", "uglad_covariance", "X", M, 40, D, 0, 0.0, "S", None, None)
        self.call(f"{k} tridiagonalize", "uglad_tridiagonalize", "a", "b", "lam", "c", "ws", M, D)
        self.call(f"{k} tridiagonalize one", "uglad_tridiagonalize", "a", None, None, "c", "ws", M, D)
        self.call(f"{k} symeig_jacobi", "uglad_symeig_jacobi", "a", "U", "beta", M, D)
        self.call(f"{k} conditional_mean", "uglad_conditional_mean", "a", "b", "c", "d", "X", "Z", "loss", "scratch", "ws", M, D, 1)
        self.call(f"{k} support_metrics", "uglad_support_metrics", "a", "b", "c", M, D, 1)

    def refusals(self):
        cell = ("S", "Zin", "lam", "params", "Zout", "half", "U", "beta", "nf_partial", "cond_max", "ws")
        for M, D in ((1, 0), (0, 25), (1, 96), (1, 2049), (21846, 161), (21845, 161), (21846, 160)):  # (NT = 3 is masked out of this build)
            self.numbers(f"refuse M{M} D{D} numbers", M, D)
            self.call(f"refuse M{M} D{D} cell_fwd", "uglad_cell_fwd", *cell, M, D, 1)
            self.call(f"refuse M{M} D{D} init_theta", "uglad_init_theta", "S", "params", 0, "Z", "ws", M, D)
            self.call(f"refuse M{M} D{D} symeig", "uglad_symeig", "a", "U", "beta", "ws", M, D)
        self.numbers("numbers M4096 D2048", 4096, 2048)
        self.call("refuse null cell_fwd", "uglad_cell_fwd", *cell[:-1], None, 1, 25, 1)
        self.call("refuse null init_theta", "uglad_init_theta", "S", "params", 0, "Z", None, 1, 25)
        self.call("null workspace init_theta init_diag1", "uglad_init_theta", "S", "params", 1, "Z", None, 1, 25)
        self.call("null workspace cell_bwd D25", "uglad_cell_bwd", "G_L", "S", "Zin", "half", "U", "beta", "lam", "params", "gbuf0", "grp", "glam", None, 1, 25, 1)
        self.call("refuse null cell_bwd D129", "uglad_cell_bwd", "G_L", "S", "Zin", "half", "U", "beta", "lam", "params", "gbuf0", "grp", "glam", None, 1, 129, 1)
        self.call("refuse loss_fwd s_batch", "uglad_loss_fwd", "Z", "S", 2, None, "loss", "theta_inv", "ws", 3, 25)
        fwd = ("S", "params", 1.0, 0, L, "Z", L + 1, "half", "U", "beta", "lam", "lam_in", "nf_partial", "nf_sum", None, "ws")
        bwd = ("G_L", "S", "params", 0, L, "Z", "half", "U", "beta", "lam", "lam_in", "gbuf0", "gbuf1", "grp", "glam", "gt", "grad", "ws")
        for M, G in ((4, 3), (2, 4), (4, 0)):
            self.call(f"refuse groups M{M} G{G} forward", "uglad_glad_forward_grouped", *fwd, M, 25, G, 1)
            self.call(f"refuse groups M{M} G{G} backward", "uglad_glad_backward_grouped", *bwd, M, 25, G, 1)
            self.call(f"refuse groups M{M} G{G} backward gS", "uglad_glad_backward_wrt_s", *bwd, M, 25, G, 1, "gS")
        self.call("refuse L0 forward", "uglad_glad_forward", *fwd[:4], 0, *fwd[5:], 1, 25, 1)
        self.call("refuse z_slabs forward", "uglad_glad_forward", *fwd[:6], 1, *fwd[7:], 1, 25, 1)
        self.call("refuse sharded no exchange", "uglad_glad_forward_sharded", *fwd, 1, 25, 2, 1, None, "ctx")
        self.call("refuse sharded m_global", "uglad_glad_forward_sharded", *fwd, 2, 25, 1, 1, ctypes.cast(self.exchange, ctypes.c_void_p).value, "ctx")
        self.call("refuse gS null", "uglad_glad_backward_wrt_s", *bwd, 1, 25, 1, 1, None)
        self.call("refuse gS init_diag", "uglad_glad_backward_wrt_s", *bwd[:3], 2, *bwd[4:], 1, 25, 1, 1, "gS")
        self.call("refuse gS sqrt", "uglad_glad_backward_wrt_s", *bwd, 1, 25, 1, 2, "gS")


def worker(lib_path, config_name):
    name, _env, setters, shapes, what = next(c for c in CONFIGS + [NOT_DISABLED] if c[0] == config_name)
    with tempfile.TemporaryDirectory() as tmp:
        os.environ["UGLAD_EMUL_LAUNCH_LOG"] = os.path.join(tmp, "launches.txt")
        os.environ["UGLAD_EMUL_RECORD_ONLY"] = "1"
        rec = Recorder(lib_path, os.environ["UGLAD_EMUL_LAUNCH_LOG"])
        rec.out["setters"] = [getattr(rec.dll, fn)(mode) for fn, mode in setters]
        for M, D, G in shapes:
            rec.passes(M, D, G)
            if what == FULL and G == 1:
                rec.steps(M, D)
        if name == "default":
            rec.refusals()
    return rec.out


def run_config(lib_path, config):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(config[1])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", lib_path, config[0]], env=env, capture_output=True, text=True, check=True)
    return json.loads(r.stdout)


# The fixture keeps, per configuration and per group of calls (the passes of a shape, its per-step calls, the refusals): the numbers as they
# are, every return code that is not 0, the count of calls and of launches, and the SHA-256 of the group's whole record (every call's return
# code and launch lines) -- equal digests are equal records.  `--dump <library> <configuration>` prints a whole record, to diff two builds.
def group_of(key):
    t = key.split()
    return " ".join(t[:3]) if t[0].startswith("M") and t[1].startswith("D") else "refusals"


def summarise(calls):
    out, groups = {"setters": calls["setters"]}, {}
    for key, v in calls.items():
        if key != "setters":
            groups.setdefault(group_of(key), {})[key] = v
    for g, members in groups.items():
        launched = [v for v in members.values() if "launches" in v]
        out[g] = {"calls": len(launched), "launches": sum(len(v["launches"]) for v in launched),
                  "sha256": hashlib.sha256(json.dumps(members, sort_keys=True).encode()).hexdigest()[:20],
                  "errors": {k[len(g) + 1:] if k.startswith(g) else k: v["rc"] for k, v in members.items() if v.get("rc")}}
        out[g].update({k: v for m in members.values() if "launches" not in m for k, v in m.items()} if g != "refusals" else
                      {"numbers": {k: v for k, v in members.items() if "launches" not in v}})
    return out


if __name__ == "__main__":
    if sys.argv[1] == "--worker":
        json.dump(worker(sys.argv[2], sys.argv[3]), sys.stdout)
    elif sys.argv[1] == "--dump":
        json.dump(run_config(sys.argv[2], next(c for c in CONFIGS if c[0] == sys.argv[3])), sys.stdout, indent=1)
    elif sys.argv[1] == "--record":
        with open(FIXTURE, "w") as f:
            body = []  # one line per group
            for c in CONFIGS:
                groups = summarise(run_config(sys.argv[2], c))
                body.append(json.dumps(c[0]) + ": {\n" + ",\n".join(f"  {json.dumps(g)}: {json.dumps(v)}" for g, v in groups.items()) + "\n }")
            f.write("{\n " + ",\n ".join(body) + "\n}\n")
    sys.exit(0)

import pytest  # noqa: E402


@pytest.fixture(scope="module")
def emul_lib_path():
    from conftest import build_emulated_lib

    path = build_emulated_lib()
    if path is None:
        pytest.skip("host clang++ not available for the SIMT-emulator build")
    return path


@pytest.fixture(scope="module")
def golden_routes():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_table_covers_every_switch_of_the_toggle_matrix():
    import re

    with open(os.path.join(HERE, "..", "scripts", "gpu_toggle_matrix.sh")) as f:
        toggles = set(re.findall(r'"(UGLAD_[A-Z_0-9]+=\w+)"', f.read()))
    assert toggles and toggles <= {c[0] for c in CONFIGS}
    assert {t.split("=")[0] for t in toggles} <= set(SWITCHES)


@pytest.mark.parametrize("config", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_call_launches_what_it_launched(emul_lib_path, golden_routes, config):
    got = summarise(run_config(emul_lib_path, config))
    want = golden_routes[config[0]]
    assert sorted(got) == sorted(want)
    for group in want:  # (numbers, return codes and counts first: they say more than a digest that differs)
        assert got[group] == want[group], (f"{config[0]} / {group}: the record differs from the pinned one; "
                                           f"`python tests/test_launch_routes.py --dump <library> '{config[0]}'` prints it whole")


def test_no_fused_lambda_0_leaves_the_fusion_on(emul_lib_path, golden_routes):
    got = summarise(run_config(emul_lib_path, NOT_DISABLED))
    assert any(got[g] != golden_routes["UGLAD_NO_FUSED_LAMBDA=1"].get(g) for g in got if g != "setters")  # (the switch matters in these passes)
    for group, value in got.items():
        assert value == golden_routes["default"][group], group
