"""ctypes binding of libuglad_hip.so (C ABI: include/uglad_hip.h).

There is no CPU fallback: `get_lib()` raises if the gfx950 shared object is missing or no GPU is visible, and every
wrapper insists on contiguous fp32 tensors on the GPU.  PyTorch is only the owner of device memory and of the stream.
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# UGLAD_LIB: development / profiling builds of the same library (e.g. with phase stamps); the product loads the in-tree build
LIB_PATH = os.environ.get("UGLAD_LIB") or os.path.join(_HERE, "csrc", "libuglad_hip.so")

SQRT_MODES = {"exact": 0, "ns10": 1}
NPARAM = 42
NRHO = 28

_c_float_p = ctypes.c_void_p
_SIGS = {
    "uglad_version": ([], ctypes.c_int),
    "uglad_max_dim": ([], ctypes.c_int),
    "uglad_max_eig_dim": ([], ctypes.c_int),
    "uglad_set_matrix_iteration": ([ctypes.c_int], ctypes.c_int),
    "uglad_validated_cond": ([], ctypes.c_float),
    "uglad_cond_is_upper_bound": ([ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "uglad_workspace_floats": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "uglad_init_theta": ([_c_float_p, _c_float_p, ctypes.c_int, _c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_init_theta_bwd": ([_c_float_p, _c_float_p, ctypes.c_int, _c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_lambda_init": ([_c_float_p, ctypes.c_float, _c_float_p, _c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_cell_fwd": ([_c_float_p] * 11 + [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_cell_fwd_stage2": ([_c_float_p] * 11 + [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_sum_partials": ([_c_float_p, ctypes.c_int, _c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_lambda_step": ([_c_float_p, ctypes.c_float, _c_float_p, _c_float_p, _c_float_p, _c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_cell_bwd": ([_c_float_p] * 12 + [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_loss_fwd": ([_c_float_p, _c_float_p, ctypes.c_int, _c_float_p, _c_float_p, _c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_loss_bwd": ([_c_float_p, _c_float_p, _c_float_p, ctypes.c_int, _c_float_p, _c_float_p, ctypes.c_float, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_finish_grads": ([_c_float_p] * 6 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_glad_forward": ([_c_float_p, _c_float_p, ctypes.c_float, ctypes.c_int, ctypes.c_int, _c_float_p, ctypes.c_int] + [_c_float_p] * 9
                           + [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_glad_backward": ([_c_float_p, _c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int] + [_c_float_p] * 13
                            + [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_glad_forward_grouped": ([_c_float_p, _c_float_p, ctypes.c_float, ctypes.c_int, ctypes.c_int, _c_float_p, ctypes.c_int]
                                   + [_c_float_p] * 9 + [ctypes.c_int] * 4 + [ctypes.c_void_p], ctypes.c_int),
    "uglad_glad_backward_grouped": ([_c_float_p, _c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int] + [_c_float_p] * 13
                                    + [ctypes.c_int] * 4 + [ctypes.c_void_p], ctypes.c_int),
    "uglad_glad_forward_sharded": ([_c_float_p, _c_float_p, ctypes.c_float, ctypes.c_int, ctypes.c_int, _c_float_p, ctypes.c_int] + [_c_float_p] * 9
                                   + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_rccl_unique_id": ([ctypes.c_void_p], ctypes.c_int),
    "uglad_rccl_comm_init": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_rccl_comm_destroy": ([ctypes.c_void_p], ctypes.c_int),
    "uglad_rccl_comm_count": ([ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_rccl_allreduce_sum": ([_c_float_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_consensus_partial": ([_c_float_p, ctypes.c_int, ctypes.c_int, _c_float_p, _c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_consensus_combine": ([_c_float_p, _c_float_p, ctypes.c_int, _c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_symeig": ([_c_float_p, _c_float_p, _c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_covariance": ([_c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, _c_float_p, _c_float_p,
                          _c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_covariance_wide_workspace_floats": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "uglad_covariance_wide": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, _c_float_p,
                               ctypes.c_void_p, _c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_association_max_width": ([], ctypes.c_int),
    "uglad_association_workspace_floats": ([ctypes.c_int, ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "uglad_association": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_double,
                           _c_float_p, ctypes.c_void_p, ctypes.c_void_p, _c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_rank_correlation_workspace_floats": ([ctypes.c_int] * 4, ctypes.c_int),
    "uglad_rank_correlation_pair_chunks": ([ctypes.c_int] * 3, ctypes.c_int),
    "uglad_rank_correlation": ([ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_double, _c_float_p] + [ctypes.c_void_p] * 4
                               + [_c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_pairwise_covariance_workspace_floats": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "uglad_pairwise_covariance": ([ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_double, _c_float_p] + [ctypes.c_void_p] * 4
                                  + [_c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_weighted_covariance_workspace_floats": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "uglad_weighted_covariance": ([ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_double, _c_float_p] + [ctypes.c_void_p] * 4
                                  + [_c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_edge_frequency": ([ctypes.c_void_p, ctypes.c_void_p, _c_float_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4, ctypes.c_int),
    "uglad_tridiagonalize": ([_c_float_p, _c_float_p, _c_float_p, _c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_symeig_jacobi": ([_c_float_p, _c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_conditional_mean": ([_c_float_p] * 9 + [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_conditional_mean_wide_workspace_floats": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "uglad_conditional_mean_wide": ([ctypes.c_void_p] * 8 + [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_sample_scores_workspace_floats": ([ctypes.c_int, ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "uglad_sample_scores": ([ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5 + [_c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                             ctypes.c_void_p], ctypes.c_int),
    "uglad_partial_correlations": ([_c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "uglad_support_metrics": ([_c_float_p, _c_float_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p],
                              ctypes.c_int),
    "uglad_support_metrics_wide_workspace_floats": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "uglad_support_metrics_wide": ([_c_float_p, _c_float_p, ctypes.c_void_p, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_void_p], ctypes.c_int),
    "uglad_graph_wide_workspace_floats": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "uglad_graph_wide": ([_c_float_p, ctypes.c_int, ctypes.c_void_p, _c_float_p] + [ctypes.c_void_p] * 7 + [ctypes.c_int, ctypes.c_int, ctypes.c_int,
                         _c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_eigvalsh_wide_workspace_floats": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "uglad_eigvalsh_wide": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, _c_float_p,
                             ctypes.c_void_p], ctypes.c_int),
    "uglad_table_spectrum": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double] + [ctypes.c_void_p] * 3
                             + [_c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_correlated_features_workspace_floats": ([ctypes.c_int, ctypes.c_int], ctypes.c_int),
    "uglad_correlated_features": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3 + [_c_float_p, ctypes.c_void_p],
                                  ctypes.c_int),
    "uglad_set_wide_mode": ([ctypes.c_int], ctypes.c_int),
    "uglad_glad_backward_wrt_s": ([_c_float_p, _c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int] + [_c_float_p] * 13
                                  + [ctypes.c_int] * 4 + [_c_float_p, ctypes.c_void_p], ctypes.c_int),
    "uglad_loss_bwd_wrt_s": ([_c_float_p, _c_float_p, _c_float_p, ctypes.c_int, _c_float_p, _c_float_p, ctypes.c_float, _c_float_p,
                              _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
}
EXPORTS = tuple(_SIGS)


class UgladError(RuntimeError):
    pass


class GraphWide(NamedTuple):
    """What uglad_graph_wide leaves on the device for K problems (include/uglad_hip.h)."""
    threshold: torch.Tensor            # (K,) float32
    edge_count: torch.Tensor           # (K,) int32: m
    edge_ij: torch.Tensor              # (K, E, 2) int32, the first m rows defined
    edge_w: torch.Tensor               # (K, E) float32, the first m defined
    degree: torch.Tensor               # (K, D) int32
    triangles2: Optional[torch.Tensor]  # (K, D) int32: twice the triangles at every node
    stats: Optional[torch.Tensor]      # (K, 6) float64: num_nodes, num_edges, avg_degree, density, avg_clustering, transitivity


RANK_METHODS = {"spearman": 0, "kendall": 1, "scores": 2}  # UGLAD_RANK_*


class RankCorrelation(NamedTuple):
    """What uglad_rank_correlation leaves on the device for K tables (include/uglad_hip.h)."""
    A: torch.Tensor                   # (K, D, D) float32, repaired when asked
    min_eig: Optional[torch.Tensor]   # (K,) float64, +inf for a table that needed no repair
    A64: Optional[torch.Tensor]       # (K, D, D) float64, unrepaired
    gram: Optional[torch.Tensor]      # (K, D, D) float64
    info: torch.Tensor                # (K, D) int32: bit 0 NaN, bit 1 constant


class PairwiseCovariance(NamedTuple):
    """What uglad_pairwise_covariance leaves on the device for K tables (include/uglad_hip.h)."""
    S: torch.Tensor                   # (K, D, D) float32, repaired when asked
    S64: Optional[torch.Tensor]       # (K, D, D) float64, unrepaired
    counts: Optional[torch.Tensor]    # (K, D, D) int32: the jointly observed rows of every pair
    info: torch.Tensor                # (K, D) int32: PAIRWISE_FLAGS
    min_eig: Optional[torch.Tensor]   # (K,) float64, +inf for a table that needed no repair, NaN for a flagged one


class WeightedCovariance(NamedTuple):
    """What uglad_weighted_covariance leaves on the device for R weightings of one table's rows (include/uglad_hip.h)."""
    S: torch.Tensor                   # (R, D, D) float32, repaired when asked
    S64: Optional[torch.Tensor]       # (R, D, D) float64, unrepaired
    mean: Optional[torch.Tensor]      # (R, D) float64: the weighted column means
    info: torch.Tensor                # (R,) int32: WEIGHT_FLAGS
    min_eig: Optional[torch.Tensor]   # (R,) float64, +inf for a weighting that needed no repair, NaN for a flagged one


WEIGHT_FLAGS = {1: "a weight is negative, NaN or infinite", 2: "the weights sum to zero"}


class EdgeFrequency(NamedTuple):
    """What uglad_edge_frequency leaves on the device for R recovered graphs (include/uglad_hip.h)."""
    count: torch.Tensor               # (D, D) int32: the graphs that hold edge {i, j}
    positive: torch.Tensor            # (D, D) int32: ... with a weight > 0
    totals: torch.Tensor              # (2,) int64: sum_{i<j} c_ij, sum_{i<j} c_ij (R - c_ij)


PAIRWISE_FLAGS = {1: "no observed entry", 2: "in a pair with fewer than min_pairs jointly observed rows",
                  4: "constant observed values under normalize", 8: "holds an infinity"}


class HipLib:
    """Thin typed wrapper over the C ABI.  `require_gpu=False` exists only so that tests can point the same wrapper at the
    host build of the kernels under tests/simt_emul (CPU tensors, no stream); the package itself never does that."""

    def __init__(self, path: str = LIB_PATH, require_gpu: bool = True):
        if not os.path.exists(path):
            raise UgladError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  uglad_amd has no CPU fallback."
            )
        self.path = path
        self.require_gpu = require_gpu
        self._dll = ctypes.CDLL(path)
        for name, (argtypes, restype) in _SIGS.items():
            fn = getattr(self._dll, name)
            fn.argtypes = argtypes
            fn.restype = restype
        self.max_dim = int(self._dll.uglad_max_dim())
        self.max_eig_dim = int(self._dll.uglad_max_eig_dim())
        self.validated_cond = float(self._dll.uglad_validated_cond())
        self.version = int(self._dll.uglad_version())

    # ------------------------------------------------------------------ helpers
    def _p(self, t: Optional[torch.Tensor]):
        if t is None:
            return None
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise UgladError("uglad_amd kernels take contiguous float32 tensors")
        if self.require_gpu and not t.is_cuda:
            raise UgladError("uglad_amd kernels take GPU tensors (no CPU fallback)")
        return ctypes.c_void_p(t.data_ptr())

    @staticmethod
    def _vp(t: Optional[torch.Tensor]):
        """Pointer of a tensor that is not fp32 (fp64 tables, results); its dtype and placement are the caller's to check."""
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def _require_f64(self, t: torch.Tensor, ndim: int, what: str) -> None:
        if t.dtype != torch.float64 or not t.is_contiguous() or t.dim() != ndim:
            raise UgladError(what)
        if self.require_gpu and not t.is_cuda:
            raise UgladError("uglad_amd kernels take GPU tensors (no CPU fallback)")

    def _wide_workspace(self, name: str, device, *dims: int) -> torch.Tensor:
        """Scratch of <name>_workspace_floats(*dims) floats for one call of the wide entry point `name`; must outlive the enqueue."""
        n = int(getattr(self._dll, name + "_workspace_floats")(*map(int, dims)))
        if n < 0:
            self._check(name + "_workspace_floats", n)
        return torch.empty(n, dtype=torch.float32, device=device)

    def _stream(self):
        if not self.require_gpu:
            return None
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _check(name: str, rc: int):
        if rc != 0:
            kind = {-1: "NULL pointer", -2: "unsupported dimension", -3: "unknown mode",
                    -4: "RCCL not loadable / an RCCL call failed"}.get(rc, f"hipError {rc}")
            raise UgladError(f"{name} failed: {kind}")

    def _call(self, name, *args):
        self._check(name, getattr(self._dll, name)(*args, self._stream()))

    def cond_is_upper_bound(self, M: int, D: int, training: bool, mode: int) -> bool:
        """Whether cond_max of a cell call of this shape is the Gershgorin upper bound (matrix-iteration path) or the condition number itself."""
        rc = int(self._dll.uglad_cond_is_upper_bound(int(M), int(D), int(bool(training)), int(mode)))
        if rc < 0:
            self._check("uglad_cond_is_upper_bound", rc)
        return rc == 1

    def set_wide_mode(self, mode: int) -> None:
        """-1 automatic, 0 never, 1 always (D > 128): many workgroups per matrix for few large matrices (include/uglad_hip.h)."""
        self._check("uglad_set_wide_mode", self._dll.uglad_set_wide_mode(int(mode)))

    def set_matrix_iteration(self, mode: int) -> None:
        """The cell as the reference's own Newton-Schulz matrix iteration on dense tile products (csrc/wide_ns.h): -1 (default) beyond
        max_eig_dim and for few matrices of 128 < D <= 256, 0 beyond max_eig_dim only, 1 for every D.  Size workspaces after setting it."""
        self._check("uglad_set_matrix_iteration", self._dll.uglad_set_matrix_iteration(int(mode)))

    def workspace(self, M: int, D: int, like: torch.Tensor) -> torch.Tensor:
        """Caller-owned scratch of uglad_workspace_floats(M, D) floats on `like`'s device."""
        n = int(self._dll.uglad_workspace_floats(int(M), int(D)))
        if n < 0:
            self._check("uglad_workspace_floats", n)
        return torch.empty(n, dtype=torch.float32, device=like.device)

    # ------------------------------------------------------------------ entry points
    def init_theta(self, S, params, init_diag, theta0, workspace):
        M, D, _ = S.shape
        self._call("uglad_init_theta", self._p(S), self._p(params), int(init_diag), self._p(theta0), self._p(workspace), M, D)

    def init_theta_bwd(self, theta0, G0, init_diag, gt_partial, workspace=None):
        M, D, _ = theta0.shape
        self._call("uglad_init_theta_bwd", self._p(theta0), self._p(G0), int(init_diag), self._p(gt_partial),
                   self._p(workspace), M, D)

    def lambda_init(self, params, lambda_init, lam_out, lam_in):
        self._call("uglad_lambda_init", self._p(params), float(lambda_init), self._p(lam_out), self._p(lam_in))

    def cell_fwd(self, S, Z_in, lam, params, Z_out, half_out, U_out, beta_out, normF_partial, workspace, mode, cond_max=None):
        """cond_max: (M,) running maximum of cond(b^T b + 4/lam I) per matrix, or None (include/uglad_hip.h)."""
        M, D, _ = S.shape
        self._call("uglad_cell_fwd", self._p(S), self._p(Z_in), self._p(lam), self._p(params), self._p(Z_out),
                   self._p(half_out), self._p(U_out), self._p(beta_out), self._p(normF_partial), self._p(cond_max),
                   self._p(workspace), M, D, int(mode))

    def cell_fwd_stage2(self, S, Z_in, lam, params, Z_out, half_out, U_out, beta_out, normF_partial, workspace, mode,
                        cond_max=None):
        M, D, _ = S.shape
        self._call("uglad_cell_fwd_stage2", self._p(S), self._p(Z_in), self._p(lam), self._p(params), self._p(Z_out),
                   self._p(half_out), self._p(U_out), self._p(beta_out), self._p(normF_partial), self._p(cond_max),
                   self._p(workspace), M, D, int(mode))

    def sum_partials(self, partials, out):
        self._call("uglad_sum_partials", self._p(partials), partials.numel(), self._p(out))

    def lambda_step(self, normF_sum, inv_M, lam_prev, params, lam_next, lam_in_next):
        self._call("uglad_lambda_step", self._p(normF_sum), float(inv_M), self._p(lam_prev), self._p(params),
                   self._p(lam_next), self._p(lam_in_next))

    def cell_bwd(self, G_next, S, Z_in, half, U, beta, lam, params, G_out, grad_rho_partial, glam_partial, mode,
                 workspace=None):
        M, D, _ = S.shape
        self._call("uglad_cell_bwd", self._p(G_next), self._p(S), self._p(Z_in), self._p(half), self._p(U), self._p(beta),
                   self._p(lam), self._p(params), self._p(G_out), self._p(grad_rho_partial), self._p(glam_partial),
                   self._p(workspace), M, D, int(mode))

    def loss_fwd(self, theta, S, struct, loss_partial, theta_inv, workspace):
        M, D, _ = theta.shape
        self._call("uglad_loss_fwd", self._p(theta), self._p(S), S.shape[0], self._p(struct), self._p(loss_partial),
                   self._p(theta_inv), self._p(workspace), M, D)

    def loss_bwd(self, theta, theta_inv, S, struct, g_up, scale, G_out):
        M, D, _ = theta.shape
        self._call("uglad_loss_bwd", self._p(theta), self._p(theta_inv), self._p(S), S.shape[0], self._p(struct),
                   self._p(g_up), float(scale), self._p(G_out), M, D)

    def loss_bwd_wrt_s(self, theta, theta_inv, S, struct, g_up, scale, G_out, gS):
        """loss_bwd that also overwrites gS (S's shape) with dL/dS, symmetric part (include/uglad_hip.h)."""
        M, D, _ = theta.shape
        self._call("uglad_loss_bwd_wrt_s", self._p(theta), self._p(theta_inv), self._p(S), S.shape[0], self._p(struct),
                   self._p(g_up), float(scale), self._p(G_out), self._p(gS), M, D)

    def finish_grads(self, gt_partial, grad_rho_partial, glam_partial, lam_in, params, grad, L, M):
        self._call("uglad_finish_grads", self._p(gt_partial), self._p(grad_rho_partial), self._p(glam_partial),
                   self._p(lam_in), self._p(params), self._p(grad), int(L), int(M))

    def glad_forward(self, S, params, lambda_init, init_diag, L, Z, half, U, beta, lam, lam_in, nf_partial, nf_sum, workspace,
                     mode, groups: int = 1, cond_max=None):
        M, D, _ = S.shape
        if groups == 1:
            self._call("uglad_glad_forward", self._p(S), self._p(params), float(lambda_init), int(init_diag), int(L), self._p(Z),
                       int(Z.shape[0]), self._p(half), self._p(U), self._p(beta), self._p(lam), self._p(lam_in),
                       self._p(nf_partial), self._p(nf_sum), self._p(cond_max), self._p(workspace), M, D, int(mode))
        else:
            self._call("uglad_glad_forward_grouped", self._p(S), self._p(params), float(lambda_init), int(init_diag), int(L),
                       self._p(Z), int(Z.shape[0]), self._p(half), self._p(U), self._p(beta), self._p(lam), self._p(lam_in),
                       self._p(nf_partial), self._p(nf_sum), self._p(cond_max), self._p(workspace), M, D, int(groups), int(mode))

    # the sharded pass in one call: `exchange` = (function pointer, context) with the uglad_allreduce_fn signature (include/uglad_hip.h)
    ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)

    def glad_forward_sharded(self, S, params, lambda_init, init_diag, L, Z, half, U, beta, lam, lam_in, nf_partial, nf_sum, workspace,
                             mode, m_global: int, exchange, cond_max=None):
        M, D, _ = S.shape
        fn, ctx = exchange
        self._call("uglad_glad_forward_sharded", self._p(S), self._p(params), float(lambda_init), int(init_diag), int(L), self._p(Z),
                   int(Z.shape[0]), self._p(half), self._p(U), self._p(beta), self._p(lam), self._p(lam_in), self._p(nf_partial),
                   self._p(nf_sum), self._p(cond_max), self._p(workspace), M, D, int(m_global), int(mode),
                   ctypes.cast(fn, ctypes.c_void_p), ctypes.c_void_p(ctx) if isinstance(ctx, int) else ctx)

    def rccl_unique_id(self) -> bytes:
        buf = ctypes.create_string_buffer(128)
        self._check("uglad_rccl_unique_id", self._dll.uglad_rccl_unique_id(ctypes.cast(buf, ctypes.c_void_p)))
        return buf.raw

    def rccl_comm_init(self, unique_id: bytes, nranks: int, rank: int) -> int:
        """ncclCommInitRank on the current device; returns the communicator as an integer handle."""
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        comm = ctypes.c_void_p()
        self._check("uglad_rccl_comm_init", self._dll.uglad_rccl_comm_init(ctypes.cast(buf, ctypes.c_void_p), int(nranks), int(rank),
                                                                           ctypes.cast(ctypes.byref(comm), ctypes.c_void_p)))
        return int(comm.value)

    def rccl_comm_destroy(self, comm: int) -> None:
        self._check("uglad_rccl_comm_destroy", self._dll.uglad_rccl_comm_destroy(ctypes.c_void_p(comm)))

    def rccl_comm_count(self, comm: int) -> int:
        """ncclCommCount of a communicator made by rccl_comm_init."""
        n = ctypes.c_int(0)
        self._check("uglad_rccl_comm_count", self._dll.uglad_rccl_comm_count(ctypes.c_void_p(comm), ctypes.cast(ctypes.byref(n), ctypes.c_void_p)))
        return int(n.value)

    def rccl_exchange(self, comm: int):
        """(function pointer, context) for glad_forward_sharded: ncclAllReduce issued from the library on the compute stream."""
        return ctypes.cast(self._dll.uglad_rccl_allreduce_sum, ctypes.c_void_p), int(comm)

    def glad_backward(self, G_L, S, params, init_diag, L, Z, half, U, beta, lam, lam_in, gbuf0, gbuf1, grad_rho_partial,
                      glam_partial, gt_partial, grad, workspace, mode, groups: int = 1, gS=None):
        """gS (M,D,D) or None: when given, also dL/dS of the pass (uglad_glad_backward_wrt_s), overwritten."""
        M, D, _ = S.shape
        args = (self._p(G_L), self._p(S), self._p(params), int(init_diag), int(L), self._p(Z), self._p(half), self._p(U),
                self._p(beta), self._p(lam), self._p(lam_in), self._p(gbuf0), self._p(gbuf1), self._p(grad_rho_partial),
                self._p(glam_partial), self._p(gt_partial), self._p(grad), self._p(workspace), M, D)
        if gS is not None:
            self._call("uglad_glad_backward_wrt_s", *args, int(groups), int(mode), self._p(gS))
        elif groups == 1:
            self._call("uglad_glad_backward", *args, int(mode))
        else:
            self._call("uglad_glad_backward_grouped", *args, int(groups), int(mode))

    def consensus_partial(self, theta_K, absmin, signsum):
        K, D, _ = theta_K.shape
        self._call("uglad_consensus_partial", self._p(theta_K), K, D, self._p(absmin), self._p(signsum))

    def consensus_combine(self, absmin, signsum, out):
        D = absmin.shape[-1]
        self._call("uglad_consensus_combine", self._p(absmin), self._p(signsum), D, self._p(out))

    def tridiagonalize(self, A0, A1, lam, R, workspace):
        M, D, _ = A0.shape
        self._call("uglad_tridiagonalize", self._p(A0), self._p(A1), self._p(lam), self._p(R), self._p(workspace), M, D)

    def covariance(self, X, normalize: bool = False, eval_offset: float = 0.1, repair: bool = True,
                   return_min_eig: bool = False):
        """(K,N,D) tables on the device -> (K,D,D) covariances (uglad_covariance).  With `return_min_eig` also the smallest
        eigenvalue of every covariance BEFORE the repair, as the device's fp32 solver saw it ((K,) tensor)."""
        K, N, D = X.shape
        S = torch.empty(K, D, D, dtype=torch.float32, device=X.device)
        scratch = torch.empty(K * D * D + K * D, dtype=torch.float32, device=X.device) if repair else None
        wsp = self.workspace(K, D, X) if repair else None  # both must outlive the enqueue
        self._call("uglad_covariance", self._p(X), K, N, D, int(bool(normalize)), float(eval_offset), self._p(S), self._p(scratch),
                   self._p(wsp))
        if return_min_eig:
            if not repair:
                raise UgladError("return_min_eig needs repair=True (the eigenvalues come from the repair's solver run)")
            return S, scratch[K * D * D:].reshape(K, D)[:, 0].clone()
        return S

    def covariance_wide(self, X64, normalize: bool = False, eval_offset: float = 0.1, repair: bool = True,
                        return_min_eig: bool = False):
        """(K,N,D) FLOAT64 tables on the device -> (K,D,D) fp32 covariances for every D <= max_dim (uglad_covariance_wide): fp64
        throughout, the repair decided by a Cholesky bisection instead of an eigensolver.  With `return_min_eig` also the (K,) fp64
        smallest eigenvalues before the repair (+inf for a table that needed none) and the (K,) bool mask of the repaired tables."""
        self._require_f64(X64, 3, "covariance_wide takes a contiguous (K, N, D) float64 tensor")
        if return_min_eig and not repair:
            raise UgladError("return_min_eig needs repair=True (the eigenvalue comes from the repair's bisection)")
        K, N, D = X64.shape
        wsp = self._wide_workspace("uglad_covariance_wide", X64.device, K, D)
        S = torch.empty(K, D, D, dtype=torch.float32, device=X64.device)
        mn = torch.empty(K, dtype=torch.float64, device=X64.device) if repair else None
        self._call("uglad_covariance_wide", self._vp(X64), K, N, D, int(bool(normalize)), float(eval_offset), self._p(S), self._vp(mn),
                   self._p(wsp))
        if return_min_eig:
            return S, mn, ~torch.isinf(mn)
        return S

    def association(self, table64, maps, eval_offset: float = 0.1, repair: bool = True, want_f64: bool = False):
        """(K,N,D) FLOAT64 encoded mixed tables on the device + the MixedMaps of their expanded layout
        (utils.prepare_data.encode_mixed_table) -> (A, min_eig, A64) (uglad_association): A (K,D,D) fp32 -- Cramer's V, the correlation
        ratio and Pearson's r, repaired like a covariance when `repair` --, min_eig (K,) fp64 (the smallest eigenvalue before the repair,
        +inf for a table that needed none; None without `repair`), A64 (K,D,D) fp64 unrepaired (None without `want_f64`)."""
        self._require_f64(table64, 3, "association takes a contiguous (K, N, D) float64 tensor")
        K, N, D = table64.shape
        W = int(maps.W)
        if len(maps.feat_offset) != D:
            raise UgladError(f"association: the maps describe {len(maps.feat_offset)} features, the table has {D}")
        dev = table64.device
        wsp = self._wide_workspace("uglad_association", dev, K, D, W)
        ints = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
                for a in (maps.col_feature, maps.col_level, maps.feat_offset, maps.feat_width, maps.tile_first)]
        A = torch.empty(K, D, D, dtype=torch.float32, device=dev)
        A64 = torch.empty(K, D, D, dtype=torch.float64, device=dev) if want_f64 else None
        mn = torch.empty(K, dtype=torch.float64, device=dev) if repair else None
        self._call("uglad_association", self._vp(table64), K, N, D, *[self._vp(a) for a in ints], W, float(eval_offset), self._p(A),
                   self._vp(A64), self._vp(mn), self._p(wsp))
        return A, mn, A64

    def rank_correlation(self, X64, method, transform: bool = True, eval_offset: float = 0.1, repair: bool = True, want_f64: bool = False,
                         want_gram: bool = False) -> "RankCorrelation":
        """(K,N,D) FLOAT64 tables on the device -> RankCorrelation (uglad_rank_correlation): the rank-based correlation matrix of the
        nonparanormal model by `method` ("spearman", "kendall", "scores" or its UGLAD_RANK_* number): A (K,D,D) fp32 -- with `transform`
        2 sin(pi rho / 6) or sin(pi tau / 2) --, repaired like a covariance when `repair`; min_eig (K,) fp64 (the smallest eigenvalue
        before the repair, +inf for a table that needed none; None without `repair`); A64 (K,D,D) fp64 unrepaired (None without
        `want_f64`); gram (K,D,D) fp64, the integer Gram matrix the coefficients are ratios of (None without `want_gram`); info (K,D)
        int32, bit 0: the column holds a NaN, bit 1: it is constant -- NaN in that feature's row and column of A."""
        self._require_f64(X64, 3, "rank_correlation takes a contiguous (K, N, D) float64 tensor")
        if method not in RANK_METHODS and method not in RANK_METHODS.values():
            raise UgladError(f"rank_correlation: method {method!r} is none of {sorted(RANK_METHODS)}")
        m = RANK_METHODS.get(method, method)
        K, N, D = X64.shape
        dev = X64.device
        wsp = self._wide_workspace("uglad_rank_correlation", dev, K, N, D, m)
        A = torch.empty(K, D, D, dtype=torch.float32, device=dev)
        A64 = torch.empty(K, D, D, dtype=torch.float64, device=dev) if want_f64 else None
        gram = torch.empty(K, D, D, dtype=torch.float64, device=dev) if want_gram else None
        info = torch.empty(K, D, dtype=torch.int32, device=dev)
        mn = torch.empty(K, dtype=torch.float64, device=dev) if repair else None
        self._call("uglad_rank_correlation", self._vp(X64), K, N, D, int(m), int(bool(transform)), float(eval_offset), self._p(A),
                   self._vp(A64), self._vp(gram), self._vp(info), self._vp(mn), self._p(wsp))
        return RankCorrelation(A, mn, A64, gram, info)

    def pairwise_covariance(self, X64, normalize: bool = False, min_pairs: int = 2, eval_offset: float = 0.1, repair: bool = True,
                            want_f64: bool = False, want_counts: bool = False) -> "PairwiseCovariance":
        """(K,N,D) FLOAT64 tables on the device, NaN = missing -> PairwiseCovariance (uglad_pairwise_covariance): the available-case
        covariance, every entry over the rows where both its columns are observed (divided by their number n_ij), of the columns as they
        are or, with `normalize`, min-max normalised over their observed entries.  S (K,D,D) fp32, repaired like a covariance when
        `repair`; S64 (K,D,D) fp64 unrepaired (None without `want_f64`); counts (K,D,D) int32, n_ij (None without `want_counts`); info
        (K,D) int32, the bits of PAIRWISE_FLAGS -- an entry with n_ij < min_pairs and the row and column of a column flagged 1, 4 or 8
        are NaN --; min_eig (K,) fp64: the smallest eigenvalue before the repair, +inf for a table that needed none, NaN for a table with
        any flag set, which is not repaired (None without `repair`)."""
        self._require_f64(X64, 3, "pairwise_covariance takes a contiguous (K, N, D) float64 tensor")
        K, N, D = X64.shape
        dev = X64.device
        wsp = self._wide_workspace("uglad_pairwise_covariance", dev, K, D)
        S = torch.empty(K, D, D, dtype=torch.float32, device=dev)
        S64 = torch.empty(K, D, D, dtype=torch.float64, device=dev) if want_f64 else None
        counts = torch.empty(K, D, D, dtype=torch.int32, device=dev) if want_counts else None
        info = torch.empty(K, D, dtype=torch.int32, device=dev)
        mn = torch.empty(K, dtype=torch.float64, device=dev) if repair else None
        self._call("uglad_pairwise_covariance", self._vp(X64), K, N, D, int(bool(normalize)), int(min_pairs), float(eval_offset), self._p(S),
                   self._vp(S64), self._vp(counts), self._vp(info), self._vp(mn), self._p(wsp))
        return PairwiseCovariance(S, S64, counts, info, mn)

    def weighted_covariance(self, X64, W64, eval_offset: float = 0.1, repair: bool = True, want_f64: bool = False,
                            want_mean: bool = False) -> "WeightedCovariance":
        """ONE (N,D) FLOAT64 table and (R,N) FLOAT64 row weights on the device -> WeightedCovariance (uglad_weighted_covariance): per
        weighting the covariance sum_n w_n (x_n - mu)(x_n - mu)^T / sum_n w_n about its own weighted mean mu -- a bootstrap resample for
        integer multiplicities, a subsample for 0 / 1 -- with the table uploaded and staged once for all of them.  S (R,D,D) fp32,
        repaired like a covariance when `repair`; S64 (R,D,D) fp64 unrepaired (None without `want_f64`); mean (R,D) fp64 (None without
        `want_mean`); info (R,) int32, the bits of WEIGHT_FLAGS -- a flagged weighting is NaN throughout --; min_eig (R,) fp64: the
        smallest eigenvalue before the repair, +inf for a weighting that needed none, NaN for a flagged one (None without `repair`)."""
        self._require_f64(X64, 2, "weighted_covariance takes a contiguous (N, D) float64 table")
        self._require_f64(W64, 2, "weighted_covariance takes contiguous (R, N) float64 weights")
        N, D = X64.shape
        R = W64.shape[0]
        if W64.shape[1] != N or W64.device != X64.device:
            raise UgladError(f"weighted_covariance: weights of shape {tuple(W64.shape)} for a table of {N} rows (one device)")
        dev = X64.device
        wsp = self._wide_workspace("uglad_weighted_covariance", dev, R, D)
        S = torch.empty(R, D, D, dtype=torch.float32, device=dev)
        S64 = torch.empty(R, D, D, dtype=torch.float64, device=dev) if want_f64 else None
        mean = torch.empty(R, D, dtype=torch.float64, device=dev) if want_mean else None
        info = torch.empty(R, dtype=torch.int32, device=dev)
        mn = torch.empty(R, dtype=torch.float64, device=dev) if repair else None
        self._call("uglad_weighted_covariance", self._vp(X64), self._vp(W64), R, N, D, float(eval_offset), self._p(S), self._vp(S64),
                   self._vp(mean), self._vp(info), self._vp(mn), self._p(wsp))
        return WeightedCovariance(S, S64, mean, info, mn)

    def edge_frequency(self, graph: "GraphWide", D: int) -> "EdgeFrequency":
        """The GraphWide of R problems of dimension D (graph_wide) -> EdgeFrequency (uglad_edge_frequency): per edge the number of the R
        graphs that hold it, the same over the edges with a positive weight, and the two integer totals StARS' instability is made of."""
        R, E = graph.edge_w.shape
        if E != D * (D - 1) // 2 or tuple(graph.edge_ij.shape) != (R, E, 2) or tuple(graph.edge_count.shape) != (R,):
            raise UgladError(f"edge_frequency: the edge lists are not those of {R} graphs of dimension {D}")
        for t, dt in ((graph.edge_count, torch.int32), (graph.edge_ij, torch.int32)):
            if t.dtype != dt or not t.is_contiguous() or (self.require_gpu and not t.is_cuda):
                raise UgladError("edge_frequency takes the contiguous int32 device tensors graph_wide returns")
        dev = graph.edge_w.device
        count = torch.empty(D, D, dtype=torch.int32, device=dev)
        positive = torch.empty(D, D, dtype=torch.int32, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        self._call("uglad_edge_frequency", self._vp(graph.edge_count), self._vp(graph.edge_ij), self._p(graph.edge_w), R, D, self._vp(count),
                   self._vp(positive), self._vp(totals))
        return EdgeFrequency(count, positive, totals)

    def rank_pair_chunks(self, K: int, N: int, D: int) -> int:
        """The number of chunks a Kendall call of this shape deals the row pairs of a tile over (uglad_rank_correlation_pair_chunks)."""
        n = int(self._dll.uglad_rank_correlation_pair_chunks(int(K), int(N), int(D)))
        if n < 0:
            self._check("uglad_rank_correlation_pair_chunks", n)
        return n

    def conditional_mean(self, precision, mean, observed, values, clip01: bool = False):
        """uglad_conditional_mean: (K,D,D), (K,D), (K,D) mask, (K,D) -> full_mean (K,D), cond_cov (K,D,D), log_pdf (K)."""
        K, D, _ = precision.shape
        f32 = dict(dtype=torch.float32, device=precision.device)
        full_mean, cond_cov, log_pdf = torch.empty(K, D, **f32), torch.empty(K, D, D, **f32), torch.empty(K, **f32)
        scratch = torch.empty(K, D, D, **f32)
        wsp = self.workspace(K, D, precision)
        self._call("uglad_conditional_mean", self._p(precision), self._p(mean), self._p(observed), self._p(values),
                   self._p(full_mean), self._p(cond_cov), self._p(log_pdf), self._p(scratch), self._p(wsp), K, D, int(bool(clip01)))
        return full_mean, cond_cov, log_pdf

    def conditional_mean_wide(self, P64, mean64, observed, values64, clip01: bool = False, want_cov: bool = True):
        """uglad_conditional_mean_wide, every D <= max_dim: (K,D,D), (K,D) FLOAT64, (K,D) fp32 mask, (K,D) FLOAT64 -> full_mean (K,D)
        float64, cond_cov (K,D,D) fp32 (None without `want_cov`: the product is skipped), log_pdf (K) float64.  A problem whose L_uu is
        not positive definite comes back with NaN in log_pdf, in the unobserved entries of full_mean and in the (u, u) block of cond_cov."""
        for a, ndim in ((P64, 3), (mean64, 2), (values64, 2)):
            self._require_f64(a, ndim, "conditional_mean_wide takes contiguous float64 tensors (K, D, D), (K, D), (K, D) and a float32 mask")
        K, D, _ = P64.shape
        if P64.shape[2] != D or tuple(mean64.shape) != (K, D) or tuple(values64.shape) != (K, D) or tuple(observed.shape) != (K, D):
            raise UgladError("conditional_mean_wide: shapes (K, D, D), (K, D), (K, D), (K, D)")
        dev = P64.device
        wsp = self._wide_workspace("uglad_conditional_mean_wide", dev, K, D)
        full_mean = torch.empty(K, D, dtype=torch.float64, device=dev)
        log_pdf = torch.empty(K, dtype=torch.float64, device=dev)
        cond_cov = torch.empty(K, D, D, dtype=torch.float32, device=dev) if want_cov else None
        self._call("uglad_conditional_mean_wide", self._vp(P64), self._vp(mean64), self._p(observed), self._vp(values64), self._vp(full_mean),
                   self._p(cond_cov), self._vp(log_pdf), self._p(wsp), K, D, int(bool(clip01)))
        return full_mean, cond_cov, log_pdf

    def sample_scores(self, X64, P64, mean64, want_density: bool = True):
        """uglad_sample_scores, every D <= max_dim: X (K,N,D) or (1,N,D) (one table for every model), precision (K,D,D), mean (K,D), all
        FLOAT64 -> (mahalanobis (K,N): the squared distances xc^T P xc with P the symmetric part of the precision, log_density (K,N),
        logdet (K)), float64 on the device; the last two are None without `want_density` (the factorisation is skipped).  A model that is
        not positive definite comes back with NaN in logdet and log_density.  Bit for bit, a row's numbers do not depend on N, on its
        position, or on K (csrc/score_wide.h)."""
        what = "sample_scores takes contiguous float64 tensors (K or 1, N, D), (K, D, D), (K, D)"
        for a, ndim in ((X64, 3), (P64, 3), (mean64, 2)):
            self._require_f64(a, ndim, what)
        K, D, _ = P64.shape
        xb, N, _ = X64.shape
        if P64.shape[2] != D or X64.shape[2] != D or tuple(mean64.shape) != (K, D) or xb not in (1, K):
            raise UgladError(what)
        dev = P64.device
        wsp = self._wide_workspace("uglad_sample_scores", dev, K, N, D)
        maha = torch.empty(K, N, dtype=torch.float64, device=dev)
        dens = torch.empty(K, N, dtype=torch.float64, device=dev) if want_density else None
        logdet = torch.empty(K, dtype=torch.float64, device=dev) if want_density else None
        self._call("uglad_sample_scores", self._vp(X64), int(xb), self._vp(P64), self._vp(mean64), self._vp(maha), self._vp(dens),
                   self._vp(logdet), self._p(wsp), K, N, D)
        return maha, dens, logdet

    def _eigw_buffers(self, K: int, D: int, device):
        """(workspace, eig (K,D), summary (K,6)) of one uglad_eigvalsh_wide or uglad_table_spectrum call: they share the slab layout."""
        return (self._wide_workspace("uglad_eigvalsh_wide", device, K, D), torch.empty(K, D, dtype=torch.float64, device=device),
                torch.empty(K, 6, dtype=torch.float64, device=device))

    def eigvalsh_wide(self, A64, th: float = 0.0):
        """uglad_eigvalsh_wide, every D <= max_dim: (K,D,D) FLOAT64 matrices -> (eig (K,D) float64 ASCENDING, summary (K,6) float64: min,
        max, min |.|, max |.|, con = max |.| / min |.|, the number of eigenvalues < th), on the device.  The symmetric part is what is
        solved; a matrix with a non-finite entry comes back as NaN in all places (csrc/eigvals_wide.h)."""
        self._require_f64(A64, 3, "eigvalsh_wide takes a contiguous (K, D, D) float64 tensor")
        K, D, D2 = A64.shape
        if D2 != D:
            raise UgladError("eigvalsh_wide takes a contiguous (K, D, D) float64 tensor")
        wsp, eig, summary = self._eigw_buffers(K, D, A64.device)
        self._call("uglad_eigvalsh_wide", self._vp(A64), K, D, float(th), self._vp(eig), self._vp(summary), self._p(wsp))
        return eig, summary

    def table_spectrum(self, X64, th: float = 0.0, want_cov: bool = False):
        """uglad_table_spectrum: (K,N,D) FLOAT64 tables -> (eig, summary, cov) of their empirical covariances (centred, / N) as
        eigvalsh_wide returns them; cov (K,D,D) float64 with `want_cov`, else None."""
        self._require_f64(X64, 3, "table_spectrum takes a contiguous (K, N, D) float64 tensor")
        K, N, D = X64.shape
        dev = X64.device
        wsp, eig, summary = self._eigw_buffers(K, D, dev)
        cov = torch.empty(K, D, D, dtype=torch.float64, device=dev) if want_cov else None
        self._call("uglad_table_spectrum", self._vp(X64), K, N, D, float(th), self._vp(eig), self._vp(summary), self._vp(cov), self._p(wsp))
        return eig, summary, cov

    def correlated_features(self, S64):
        """uglad_correlated_features, every 2 <= D <= max_dim: (K,D,D) FLOAT64 covariance matrices -> (order (K,D), counts (K,D),
        n_listed (K)) int32 on the device: order[k][:n_listed[k]] is get_highly_correlated_features of matrix k (csrc/corr_wide.h)."""
        self._require_f64(S64, 3, "correlated_features takes a contiguous (K, D, D) float64 tensor")
        K, D, D2 = S64.shape
        if D2 != D:
            raise UgladError("correlated_features takes a contiguous (K, D, D) float64 tensor")
        dev = S64.device
        wsp = self._wide_workspace("uglad_correlated_features", dev, K, D)
        order = torch.empty(K, D, dtype=torch.int32, device=dev)
        counts = torch.empty(K, D, dtype=torch.int32, device=dev)
        n_listed = torch.empty(K, dtype=torch.int32, device=dev)
        self._call("uglad_correlated_features", self._vp(S64), K, D, self._vp(order), self._vp(counts), self._vp(n_listed), self._p(wsp))
        return order, counts, n_listed

    def partial_correlations(self, precision):
        K, D, _ = precision.shape
        rho = torch.empty_like(precision)
        self._call("uglad_partial_correlations", self._p(precision), self._p(rho), K, D)
        return rho

    def support_metrics(self, true_theta, pred_theta, beta: int = 1):
        """uglad_support_metrics: two (K,D,D) fp32 tensors -> (K, 11) float64 tensor on the device."""
        K, D, _ = pred_theta.shape
        out = torch.empty(K, 11, dtype=torch.float64, device=pred_theta.device)
        self._call("uglad_support_metrics", self._p(true_theta), self._p(pred_theta), ctypes.c_void_p(out.data_ptr()), K, D,
                   int(beta))
        return out

    def support_metrics_wide(self, true_theta, pred_theta, beta: int = 1):
        """uglad_support_metrics_wide, every 2 <= D <= max_dim: two (K,D,D) fp32 tensors -> (K, 11) float64 tensor on the device.  The
        edges of every pair are sorted by score on the device (csrc/metrics_wide.h); all but aupr is bit-equal to support_metrics."""
        if true_theta.dim() != 3 or true_theta.shape != pred_theta.shape or true_theta.shape[1] != true_theta.shape[2]:
            raise UgladError("support_metrics_wide: two tensors of shape (K, D, D)")
        K, D, _ = pred_theta.shape
        tp, pp = self._p(true_theta), self._p(pred_theta)
        wsp = self._wide_workspace("uglad_support_metrics_wide", pred_theta.device, K, D)
        out = torch.empty(K, 11, dtype=torch.float64, device=pred_theta.device)
        self._call("uglad_support_metrics_wide", tp, pp, self._vp(out), self._p(wsp), K, D, int(beta))
        return out

    def graph_wide(self, values, n_keep=None, threshold=None, from_precision: bool = True, want_stats: bool = True) -> "GraphWide":
        """uglad_graph_wide, every 2 <= D <= max_dim: (K,D,D) fp32 precision matrices (or partial correlations with `from_precision=False`)
        -> the recovered graphs as device tensors (GraphWide).  Per problem either `n_keep` (an int or K of them: the number of largest
        |rho| the threshold is ranked by, 0 <= n_keep <= E) or `threshold` (a float, K of them or a (K,) tensor); with both, the problems
        whose n_keep is -1 take the threshold.  Only the first edge_count[k] rows of edge_ij[k] / edge_w[k] are defined."""
        if values.dim() != 3 or values.shape[1] != values.shape[2]:
            raise UgladError("graph_wide: a tensor of shape (K, D, D)")
        K, D, _ = values.shape
        vp = self._p(values)
        dev = values.device
        E = D * (D - 1) // 2
        if n_keep is None:
            if threshold is None:
                raise UgladError("graph_wide: n_keep or threshold")
            keep = [-1] * K
        else:
            keep = [int(n_keep)] * K if isinstance(n_keep, int) else [int(n) for n in n_keep]
        if len(keep) != K:
            raise UgladError("graph_wide: one n_keep per problem")
        th_in = None
        if threshold is not None:
            th_in = torch.as_tensor(threshold, dtype=torch.float32).reshape(-1).expand(K) if not torch.is_tensor(threshold) or threshold.numel() == 1 \
                else threshold.reshape(-1)
            if th_in.numel() != K:
                raise UgladError("graph_wide: one threshold per problem")
            th_in = th_in.to(device=dev, dtype=torch.float32).contiguous()
        wsp = self._wide_workspace("uglad_graph_wide", dev, K, D)
        i32 = dict(dtype=torch.int32, device=dev)
        out = GraphWide(threshold=torch.empty(K, dtype=torch.float32, device=dev), edge_count=torch.empty(K, **i32),
                        edge_ij=torch.empty(K, E, 2, **i32), edge_w=torch.empty(K, E, dtype=torch.float32, device=dev),
                        degree=torch.empty(K, D, **i32), triangles2=torch.empty(K, D, **i32) if want_stats else None,
                        stats=torch.empty(K, 6, dtype=torch.float64, device=dev) if want_stats else None)
        self._call("uglad_graph_wide", vp, int(bool(from_precision)), (ctypes.c_int * K)(*keep), self._p(th_in), self._p(out.threshold),
                   self._vp(out.edge_count), self._vp(out.edge_ij), self._p(out.edge_w), self._vp(out.degree), self._vp(out.triangles2),
                   self._vp(out.stats), int(bool(want_stats)), K, D, self._p(wsp))
        return out

    def symeig(self, A, U, beta, jacobi: bool = False):
        M, D, _ = A.shape
        if jacobi:
            self._call("uglad_symeig_jacobi", self._p(A), self._p(U), self._p(beta), M, D)
        else:
            wsp = self.workspace(M, D, A)  # must outlive the enqueue (the caching allocator keeps it valid for the stream)
            self._call("uglad_symeig", self._p(A), self._p(U), self._p(beta), self._p(wsp), M, D)


_instance: Optional[HipLib] = None


def get_lib() -> HipLib:
    """The process-wide library handle.  Fails loudly when the HIP build or the GPU is missing."""
    global _instance
    if _instance is None:
        if not torch.cuda.is_available():
            raise UgladError("uglad_amd needs an MI355X visible to PyTorch-ROCm; there is no CPU fallback")
        _instance = HipLib(LIB_PATH, require_gpu=True)
    return _instance


def device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())
