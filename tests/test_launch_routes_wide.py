"""CPU: which kernels the nine many-workgroup fp64 utilities launch (csrc/host_wide.h: covariance_wide, association, conditional_mean_wide,
sample_scores, support_metrics_wide, graph_wide, eigvalsh_wide, table_spectrum, correlated_features) and what their *_workspace_floats return,
pinned against tests/golden/launch_routes_wide.json.

The machinery is test_launch_routes.py's: the emulator's launch hook under UGLAD_EMUL_RECORD_ONLY=1 in a worker process, made-up addresses for every
buffer (one 64 GiB range each, so every workspace offset is part of the record), `short` for the kernel's name, per group of calls the counts, the
return codes that are not 0 and a SHA-256 of the whole record.  uglad_graph_wide reads n_keep on the host: that one array is real.

The fixture's first six groups were recorded from the host layer as it stood BEFORE the wide utilities' shared pieces got one owner each (the
shift bisection in chol_wide.h, the radix sort in sort_wide.h, the entry points in host_wide.h), with `python tests/test_launch_routes_wide.py
--record <library>` on a build of that commit; its last three (eigvalsh_wide, table_spectrum, correlated_features) with `--record <library>
<group> ...`, which leaves the other groups as they are, on a build of the commit before the centred Gram product (cov_wide.h) and the
symmetriser (chol_wide.h) got one owner each.  It is not to be regenerated for a refactoring.  Two normalisations stand between a record and the fixture, both below:
RENAMED (a kernel that moved to its owner under a new name -> the name it was recorded under) and a by-value struct argument's size `{n}` -> `{}`
(a view that holds less than the one it was cut from is a smaller argument; what the kernels read of it is pinned by their results)."""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_launch_routes as tlr  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "launch_routes_wide.json")

# ---------------------------------------------------------------------------------------------------------------- the two normalisations
RENAMED = {  # the kernel as it is now -> as the fixture names it
    "uglad::cholw_bisect_kernel<uglad::CovwBracket>": "uglad::covw_control_kernel",
    "uglad::cholw_bisect_kernel<uglad::AssocBracket>": "uglad::assoc_control_kernel",
    "uglad::cholw_repair_kernel": "uglad::covw_repair_kernel",
    "uglad::sortw_hist_kernel": "uglad::mw_hist_kernel",
    "uglad::sortw_scan_kernel": "uglad::mw_scan_kernel",
    "uglad::sortw_scatter_kernel": "uglad::mw_scatter_kernel",
    "uglad::covw_gram_kernel<uglad::CovwSink>": "uglad::covw_gram_kernel",
    "uglad::covw_gram_kernel<uglad::EigwGramSink>": "uglad::eigw_gram_kernel",
}
STRUCT_SIZE = re.compile(r"\{\d+\}")


def normalised(line):
    name, rest = tlr.short(line).split(" [", 1)
    return RENAMED.get(name, name) + " [" + STRUCT_SIZE.sub("{}", rest)


# ---------------------------------------------------------------------------------------------------------------- the table
CT = dict(tlr.CT, d=ctypes.c_double)
SIGS = {  # (the stream, last, is added by the recorder)
    "uglad_covariance_wide": "piiiidppp", "uglad_association": "piii" + "p" * 5 + "id" + "pppp", "uglad_conditional_mean_wide": "p" * 8 + "iii",
    "uglad_sample_scores": "pi" + "p" * 6 + "iii", "uglad_support_metrics_wide": "ppppiii", "uglad_graph_wide": "pipp" + "p" * 7 + "iiip",
    "uglad_eigvalsh_wide": "piidppp", "uglad_table_spectrum": "piiidpppp", "uglad_correlated_features": "piipppp",
}
SIZES = {"uglad_covariance_wide": 2, "uglad_association": 3, "uglad_conditional_mean_wide": 2, "uglad_sample_scores": 3,
         "uglad_support_metrics_wide": 2, "uglad_graph_wide": 2, "uglad_eigvalsh_wide": 2, "uglad_correlated_features": 2}
# (arguments of <name>_workspace_floats; uglad_table_spectrum takes uglad_eigvalsh_wide's workspace)
COV = [(1, 1), (2, 40), (1, 64), (1, 65), (3, 129)]          # (K, D): one tile, ragged, exactly one tile, two tiles, a batch of three tiles
ASSOC = [(2, 12, 64), (1, 40, 128)]                          # (K, D, W)
AFTER = [(2, 40), (1, 129)]
SCORES = [(2, 1, 1), (2, 100, 70), (1, 257, 129)]            # (K, N, D)
METRICS = [(2, 2), (1, 70), (1, 129)]
GRAPH = [(2, 2), (2, 70), (65, 40)]                          # (65 problems: two threshold launches)
EIGVALS = COV                                                # (also table_spectrum's)
CORR = [(1, 2)] + COV[1:]
UNALIGNED = ((tlr.BUFFERS.index("ws") + 1) << 36) + 4


class Recorder(tlr.Recorder):
    def __init__(self, lib_path, log_path):
        super().__init__(lib_path, log_path)
        for name, sig in SIGS.items():
            fn = getattr(self.dll, name)
            fn.argtypes = [CT[c] for c in sig] + [ctypes.c_void_p]
            fn.restype = ctypes.c_int
        for name, n in SIZES.items():
            size = getattr(self.dll, name + "_workspace_floats")
            size.argtypes, size.restype = [ctypes.c_int] * n, ctypes.c_int
        self.keep = []  # the host arrays handed in

    def call(self, key, name, *args):
        super().call(key, name, *args)
        self.out[key]["launches"] = [normalised(line) for line in self.out[key]["launches"]]

    def size(self, name, *dims):
        self.out[f"{name} size {' '.join(map(str, dims))}"] = {"workspace_floats": getattr(self.dll, name + "_workspace_floats")(*dims)}

    def host_ints(self, values):
        a = (ctypes.c_int * len(values))(*values)
        self.keep.append(a)
        return ctypes.addressof(a)

    # -- one method per entry point: (key, the call with every argument in place); `ws` lets a refusal hand in another workspace
    def covariance(self, key, K, D, N=30, normalize=1, X="X", S="S", mn="a", ws="ws"):
        self.call(f"uglad_covariance_wide {key}", "uglad_covariance_wide", X, K, N, D, normalize, 0.1, S, mn, ws)

    def association(self, key, K, D, W, N=50, table="X", maps=("a", "b", "c", "d", "grp"), A="S", A64="Z", mn="lam", ws="ws"):
        self.call(f"uglad_association {key}", "uglad_association", table, K, N, D, *maps, W, 0.1, A, A64, mn, ws)

    def after(self, key, K, D, clip01=0, P="a", cov="S", ws="ws"):
        self.call(f"uglad_conditional_mean_wide {key}", "uglad_conditional_mean_wide", P, "b", "c", "d", "X", cov, "loss", ws, K, D, clip01)

    def scores(self, key, K, N, D, x_batch, X="X", dens="b", logdet="c", ws="ws"):
        self.call(f"uglad_sample_scores {key}", "uglad_sample_scores", X, x_batch, "S", "a", "Z", dens, logdet, ws, K, N, D)

    def metrics(self, key, K, D, true="a", ws="ws"):
        self.call(f"uglad_support_metrics_wide {key}", "uglad_support_metrics_wide", true, "b", "c", ws, K, D, 1)

    def graph(self, key, K, D, keep, th_in="lam", want_stats=1, from_precision=1, values="a", tri="gt", stats="grad", ws="ws"):
        self.call(f"uglad_graph_wide {key}", "uglad_graph_wide", values, from_precision, self.host_ints(keep) if keep is not None else None, th_in,
                  "lam_in", "b", "c", "d", "U", tri, stats, want_stats, K, D, ws)

    def eigvals(self, key, K, D, A="a", eig="b", summary="c", ws="ws"):
        self.call(f"uglad_eigvalsh_wide {key}", "uglad_eigvalsh_wide", A, K, D, 0.25, eig, summary, ws)

    def spectrum(self, key, K, D, N=30, X="X", eig="b", summary="c", cov="Z", ws="ws"):
        self.call(f"uglad_table_spectrum {key}", "uglad_table_spectrum", X, K, N, D, 0.25, eig, summary, cov, ws)

    def corr(self, key, K, D, S="a", order="b", counts="c", n_listed="d", ws="ws"):
        self.call(f"uglad_correlated_features {key}", "uglad_correlated_features", S, K, D, order, counts, n_listed, ws)

    def everything(self):
        for name, n in SIZES.items():  # the numbers: every shape below, and the ends of every range
            for K in (0, 1, 65535, 65536):
                for D in (0, 1, 2, 64, 65, 2048, 2049):
                    dims = {"uglad_association": [(K, D, 64), (K, D, 16384)], "uglad_sample_scores": [(K, 1, D), (K, 100000, D)]}.get(name, [(K, D)])
                    for d in dims:
                        self.size(name, *d)
        for W in (0, 63, 11, 128, 16384, 16448):
            self.size("uglad_association", 1, 12, W)
        for N in (0, 1, 2 ** 31 - 1):
            self.size("uglad_sample_scores", 1, N, 70)
        self.size("uglad_sample_scores", 4096, 2 ** 20, 2048)  # past 2^31 - 1 floats
        for K, D in COV:
            self.size("uglad_covariance_wide", K, D)
            self.covariance(f"K{K} D{D} repair", K, D)
            self.covariance(f"K{K} D{D} plain", K, D, mn=None, normalize=0)
        for K, D, W in ASSOC:
            self.size("uglad_association", K, D, W)
            self.association(f"K{K} D{D} W{W} repair f64", K, D, W)
            self.association(f"K{K} D{D} W{W} repair", K, D, W, A64=None)
            self.association(f"K{K} D{D} W{W} plain", K, D, W, mn=None)
        for K, D in AFTER:
            self.size("uglad_conditional_mean_wide", K, D)
            self.after(f"K{K} D{D} cov", K, D)
            self.after(f"K{K} D{D} no cov clip01", K, D, clip01=1, cov=None)
        for K, N, D in SCORES:
            self.size("uglad_sample_scores", K, N, D)
            for xb in sorted({1, K}):
                self.scores(f"K{K} N{N} D{D} x_batch{xb} density", K, N, D, xb)
                self.scores(f"K{K} N{N} D{D} x_batch{xb} logdet only", K, N, D, xb, dens=None)
                self.scores(f"K{K} N{N} D{D} x_batch{xb} distances", K, N, D, xb, dens=None, logdet=None)
        for K, D in METRICS:
            self.size("uglad_support_metrics_wide", K, D)
            self.metrics(f"K{K} D{D}", K, D)
        for K, D in GRAPH:
            self.size("uglad_graph_wide", K, D)
            E = D * (D - 1) // 2
            ranked, mixed = [(k * 7) % (E + 1) for k in range(K)], [-1 if k % 2 else E for k in range(K)]
            for stats in (1, 0):
                self.graph(f"K{K} D{D} ranked stats{stats}", K, D, ranked, th_in=None, want_stats=stats)
                self.graph(f"K{K} D{D} given stats{stats}", K, D, [-1] * K, want_stats=stats, from_precision=0)
                self.graph(f"K{K} D{D} mixed stats{stats}", K, D, mixed, want_stats=stats)
            self.graph(f"K{K} D{D} ranked no stats buffers", K, D, ranked, th_in=None, want_stats=0, tri=None, stats=None)
        for K, D in EIGVALS:
            self.size("uglad_eigvalsh_wide", K, D)
            self.eigvals(f"K{K} D{D}", K, D)
            self.spectrum(f"K{K} D{D} cov", K, D)
            self.spectrum(f"K{K} D{D} no cov", K, D, cov=None)
        for K, D in CORR:
            self.size("uglad_correlated_features", K, D)
            self.corr(f"K{K} D{D}", K, D)
        self.refusals()

    def refusals(self):
        bad_KD = ((0, 40), (65536, 40), (1, 0), (1, 2049))
        for K, D in bad_KD + ((1, 40),):
            tag = f"refuse K{K} D{D}" if (K, D) != (1, 40) else "refuse"
            if (K, D) != (1, 40):
                self.covariance(tag, K, D)
                self.association(tag, K, D, 64)
                self.after(tag, K, D)
                self.scores(tag, K, 10, D, 1)
                self.metrics(tag, K, D)
                self.graph(tag, K, D, [0] * max(K, 1) if K < 65536 else [0])
                self.eigvals(tag, K, D)
                self.spectrum(tag, K, D)
                self.corr(tag, K, D)
                continue
            self.covariance(tag + " null X", K, D, X=None)
            self.covariance(tag + " null S", K, D, S=None)
            self.covariance(tag + " null workspace", K, D, ws=None)
            self.covariance(tag + " unaligned workspace", K, D, ws=UNALIGNED)
            self.covariance(tag + " N0", K, D, N=0)
            self.covariance(tag + " normalize2", K, D, normalize=2)
            self.association(tag + " null table", K, D, 64, table=None)
            self.association(tag + " null map", K, D, 64, maps=("a", "b", None, "d", "grp"))
            self.association(tag + " null A", K, D, 64, A=None)
            self.association(tag + " unaligned workspace", K, D, 64, ws=UNALIGNED)
            self.association(tag + " D1", K, 1, 64)
            self.association(tag + " N1", K, D, 64, N=1)
            for W in (0, 32, 100, 16448):
                self.association(tag + f" W{W}", K, D, W)
            self.after(tag + " null P", K, D, P=None)
            self.after(tag + " null workspace", K, D, ws=None)
            self.after(tag + " unaligned workspace", K, D, ws=UNALIGNED)
            self.scores(tag + " null X", K, 10, D, 1, X=None)
            self.scores(tag + " unaligned workspace", K, 10, D, 1, ws=UNALIGNED)
            self.scores(tag + " N0", K, 0, D, 1)
            self.scores(tag + " x_batch2", K, 10, D, 2)
            self.scores(tag + " x_batch0", 3, 10, D, 0)
            self.metrics(tag + " null true", K, D, true=None)
            self.metrics(tag + " unaligned workspace", K, D, ws=UNALIGNED)
            self.metrics(tag + " D1", K, 1)
            self.graph(tag + " null values", K, D, [0], values=None)
            self.graph(tag + " null n_keep", K, D, None)
            self.graph(tag + " unaligned workspace", K, D, [0], ws=UNALIGNED)
            self.graph(tag + " D1", K, 1, [0])
            self.graph(tag + " from_precision2", K, D, [0], from_precision=2)
            self.graph(tag + " want_stats2", K, D, [0], want_stats=2)
            self.graph(tag + " stats without buffers", K, D, [0], tri=None)
            self.graph(tag + " n_keep past E", K, D, [D * (D - 1) // 2 + 1])
            self.graph(tag + " n_keep -2", K, D, [-2])
            self.graph(tag + " given without thresholds", K, D, [-1], th_in=None)
            for arg in ("A", "eig", "summary", "ws"):
                self.eigvals(tag + f" null {arg}", K, D, **{arg: None})
            self.eigvals(tag + " unaligned workspace", K, D, ws=UNALIGNED)
            for arg in ("X", "eig", "summary", "ws"):
                self.spectrum(tag + f" null {arg}", K, D, **{arg: None})
            self.spectrum(tag + " unaligned workspace", K, D, ws=UNALIGNED)
            self.spectrum(tag + " N0", K, D, N=0)
            for arg in ("S", "order", "counts", "n_listed", "ws"):
                self.corr(tag + f" null {arg}", K, D, **{arg: None})
            self.corr(tag + " unaligned workspace", K, D, ws=UNALIGNED)
            self.corr(tag + " D1", K, 1)


def worker(lib_path):
    with tempfile.TemporaryDirectory() as tmp:
        os.environ["UGLAD_EMUL_LAUNCH_LOG"] = os.path.join(tmp, "launches.txt")
        os.environ["UGLAD_EMUL_RECORD_ONLY"] = "1"
        rec = Recorder(lib_path, os.environ["UGLAD_EMUL_LAUNCH_LOG"])
        rec.everything()
    return rec.out


def run(lib_path):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", lib_path], capture_output=True, text=True, check=True)
    return json.loads(r.stdout)


def summarise(calls):
    """Per entry point (the key's first word): the workspace numbers as they are, every return code that is not 0, the counts of calls and
    launches, and test_launch_routes.py's digest of the group's whole record."""
    groups = {}
    for key, v in calls.items():
        groups.setdefault(key.split()[0], {})[key] = v
    out = {}
    for g, members in groups.items():
        launched = {k: v for k, v in members.items() if "launches" in v}
        out[g] = {"calls": len(launched), "launches": sum(len(v["launches"]) for v in launched.values()),
                  "sha256": hashlib.sha256(json.dumps(members, sort_keys=True).encode()).hexdigest()[:20],
                  "launches_per_call": {k[len(g) + 1:]: len(v["launches"]) for k, v in launched.items() if not v["rc"]},
                  "errors": {k[len(g) + 1:]: v["rc"] for k, v in launched.items() if v["rc"]},
                  "workspace_floats": {k[len(g) + 6:]: v["workspace_floats"] for k, v in members.items() if "launches" not in v}}
    return out


if __name__ == "__main__":
    if sys.argv[1] == "--worker":
        json.dump(worker(sys.argv[2]), sys.stdout)
    elif sys.argv[1] == "--dump":
        json.dump(run(sys.argv[2]), sys.stdout, indent=1)
    elif sys.argv[1] == "--record":  # <library> [group ...]: the groups named, the fixture's other lines as they are; none named: all
        new = summarise(run(sys.argv[2]))
        lines = [f"{json.dumps(g)}: {json.dumps(v)}" for g, v in new.items() if g in sys.argv[3:] or not sys.argv[3:]]
        if sys.argv[3:]:
            with open(FIXTURE) as f:
                kept = [line.strip().rstrip(",") for line in f.read().splitlines()[1:-1]]
            # (in front: a line that stays, the last one too, stays byte for byte)
            lines += [line for line in kept if json.loads("{" + line + "}").keys().isdisjoint(sys.argv[3:])]
        with open(FIXTURE, "w") as f:
            f.write("{\n " + ",\n ".join(lines) + "\n}\n")
    sys.exit(0)

import pytest  # noqa: E402

from test_launch_routes import emul_lib_path  # noqa: E402,F401  (the fixture that builds the emulator library)


@pytest.fixture(scope="module")
def record(emul_lib_path):  # noqa: F811
    return summarise(run(emul_lib_path))


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_normalisation_names_only_what_moved():
    line = "void uglad::sortw_scan_kernel(uglad::SortwView) [2 1 1] [256 1 1] {24}"
    assert normalised(line) == "uglad::mw_scan_kernel [2 1 1] [256 1 1] {}"
    line = "void uglad::cholw_bisect_kernel<uglad::CovwBracket>(int, int, uglad::CholwView) [1 1 1] [64 1 1] -1 40 {24}"
    assert normalised(line) == "uglad::covw_control_kernel [1 1 1] [64 1 1] -1 40 {}"
    line = "void uglad::cholw_update_kernel(int, uglad::CholwView) [1 1 1] [256 1 1] 0 {24}"
    assert normalised(line) == "uglad::cholw_update_kernel [1 1 1] [256 1 1] 0 {}"


@pytest.mark.parametrize("entry", sorted(SIGS))
def test_every_wide_call_launches_what_it_launched(record, golden, entry):
    assert sorted(record) == sorted(golden) == sorted(SIGS)
    got, want = record[entry], golden[entry]
    for field in ("workspace_floats", "errors", "calls", "launches_per_call", "launches", "sha256"):  # (the digest last: the others say more)
        assert got[field] == want[field], (f"{entry} / {field}: the record differs from the pinned one; "
                                           f"`python tests/test_launch_routes_wide.py --dump <library>` prints it whole")
