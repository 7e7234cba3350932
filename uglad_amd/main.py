"""uGLAD's training/inference surface on MI355X.  Mirrors the hot-path half of `uglad/main.py`:

    uGLAD_GL / uGLAD_multitask        main.py:34-226    sklearn-GraphicalLassoCV-style wrappers (covariance_, precision_, location_)
    init_uGLAD / forward_uGLAD / loss_uGLAD   main.py:233-335
    run_uGLAD_direct / _CV / _missing / _multitask   main.py:338-789   epoch loops (host Python, as in the reference)
    mean_imputation / get_final_precision_from_batch main.py:647-716

Same names, argument meaning, defaults and return shapes.  Deliberate differences: invalid arguments raise ValueError
instead of sys.exit(0) (main.py:137,667,708); epochs < 10 works (the reference divides by zero, main.py:386); nothing is
plotted (main.py:416 writes ./loss_curve.png); tensors live on the GPU until `fit` stores numpy attributes.  Additive
only: `sqrt_mode=`, `predict()`, and sharding of the multi-task / missing-data batch over the ranks of an initialised
torch.distributed process group (one process per GPU, RCCL).
"""
from __future__ import annotations

import contextlib
import copy
from time import time
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .dist import Collective, get_collective
from .glad import glad
from .glad.glad_params import GladParams
from .utils import prepare_data
from .utils.metrics import report_metrics_all  # noqa: F401  (host-side API parity; the drivers count on the device)


# ============================================================================================ loss
class _GlassoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, S, struct, divisor):
        lib = _lib.get_lib()
        M, D, _ = theta.shape
        f32 = dict(dtype=torch.float32, device=theta.device)
        theta = theta.contiguous()
        partial = torch.empty(M, **f32)
        theta_inv = torch.empty(M, D, D, **f32)
        wsp = lib.workspace(M, D, theta)
        lib.loss_fwd(theta, S, struct, partial, theta_inv, wsp)
        total = torch.empty(1, **f32)
        lib.sum_partials(partial, total)
        ctx.save_for_backward(theta, theta_inv, S, struct if struct is not None else torch.empty(0, **f32))
        ctx.has_struct = struct is not None
        ctx.scale = 1.0 / float(divisor)
        return (total * ctx.scale).reshape(())

    @staticmethod
    def backward(ctx, g):
        lib = _lib.get_lib()
        theta, theta_inv, S, struct = ctx.saved_tensors
        G = torch.empty_like(theta)
        g_up = g.detach().to(torch.float32).reshape(1).contiguous()
        if ctx.needs_input_grad[1]:  # dL/dS, symmetric part (include/uglad_hip.h, uglad_loss_bwd_wrt_s)
            gS = torch.empty_like(S)
            lib.loss_bwd_wrt_s(theta, theta_inv, S, struct if ctx.has_struct else None, g_up, ctx.scale, G, gS)
            return G, gS, None, None
        lib.loss_bwd(theta, theta_inv, S, struct if ctx.has_struct else None, g_up, ctx.scale, G)
        return G, None, None, None


def loss_uGLAD(theta: torch.Tensor, S: torch.Tensor, struct_theta: Optional[torch.Tensor] = None,
               batch_divisor: Optional[int] = None) -> torch.Tensor:
    """Glasso objective sum_b(-logdet Theta_b + tr(S_b Theta_b)) / B with B = S.shape[0] (ref main.py:289-335), plus the
    log-cosh structure penalty when `struct_theta` is given.  S may be (1, D, D) against Theta (K, D, D) (the
    missing-data call, main.py:620-622; the divisor is then 1).  `batch_divisor` overrides B for a sharded batch.
    S stays in the autograd graph when it requires grad (and grad mode is on): S.grad is the symmetric part of the reference's
    gradient, (Theta + Theta^T) / 2 per matrix, summed over the batch when one S is broadcast.  Otherwise S is detached as before."""
    dev = theta.device
    if not (S.requires_grad and torch.is_grad_enabled()):
        S = S.detach()
    S = S.to(device=dev, dtype=torch.float32).contiguous()
    if S.dim() == 2:
        S = S[None]
    if S.shape[0] not in (1, theta.shape[0]):
        raise ValueError("S must hold one matrix or one per precision matrix")
    if struct_theta is not None:
        struct_theta = struct_theta.detach().to(device=dev, dtype=torch.float32)
        if struct_theta.dim() == 2:
            struct_theta = struct_theta[None]
        if struct_theta.shape[0] == 1 and S.shape[0] > 1:  # one prior for the whole batch: the reference's (1 - struct) - eye broadcasts it (main.py:327-328)
            struct_theta = struct_theta.expand(S.shape[0], -1, -1)
        struct_theta = struct_theta.contiguous()
        if struct_theta.shape != S.shape:
            raise ValueError("struct_theta must have the shape of S (or hold one matrix for the whole batch)")
    B = S.shape[0] if batch_divisor is None else batch_divisor
    return _GlassoLoss.apply(theta, S, struct_theta, B)


def _loss_per_matrix(theta: torch.Tensor, S: torch.Tensor) -> torch.Tensor:
    """-logdet Theta_b + tr(S_b Theta_b) for every matrix of the batch, (M,) on the device, no autograd (the test-fold losses
    of the batched CV driver)."""
    lib = _lib.get_lib()
    M, D, _ = theta.shape
    theta = theta.detach().contiguous()
    S = S.detach().to(device=theta.device, dtype=torch.float32).contiguous()
    partial = torch.empty(M, dtype=torch.float32, device=theta.device)
    theta_inv = torch.empty_like(theta)
    wsp = lib.workspace(M, D, theta)
    lib.loss_fwd(theta, S, None, partial, theta_inv, wsp)
    return partial


# ============================================================================================ model / forward
def init_uGLAD(lr: float, theta_init_offset: float = 1.0, nF: int = 3, H: int = 3):
    """GladParams on the GPU + Adam (ref main.py:233-249)."""
    model = GladParams(theta_init_offset=theta_init_offset, nF=nF, H=H, device=_lib.device())
    optimizer = glad.get_optimizers(model, lr_glad=lr)
    return model, optimizer


def forward_uGLAD(Sb, model_glad, L: int = 15, INIT_DIAG: int = 0, loss_Sb=None, struct_theta=None,
                  sqrt_mode: Optional[str] = None, collective: Optional[Collective] = None,
                  global_batch: Optional[int] = None):
    """predTheta = glad(Sb), loss = glasso loss on Sb (or on loss_Sb) -- ref main.py:252-286."""
    dev = next(model_glad.parameters()).device
    Sb = Sb.to(dev)
    predTheta = glad.glad(Sb, model_glad, L=L, INIT_DIAG=INIT_DIAG, sqrt_mode=sqrt_mode, collective=collective,
                          global_batch=global_batch)
    if loss_Sb is None:
        # divisor = number of matrices in the WHOLE batch (main.py:306,315), also when this rank holds a shard of it
        loss = loss_uGLAD(predTheta, Sb, struct_theta=struct_theta, batch_divisor=global_batch)
    else:
        loss = loss_uGLAD(predTheta, loss_Sb, struct_theta=struct_theta)
    return predTheta, loss


def _to_dev(x):
    return prepare_data.convert_to_torch(x, req_grad=False, device=_lib.device())


_DEVICE_COVARIANCE = False  # set for the duration of a fit()/predict() by uGLAD_GL / uGLAD_multitask(device_covariance=True)


@contextlib.contextmanager
def device_covariance(enabled: bool = True):
    """Within this context the drivers form the covariances (and the reference's eigenvalue repair) on the GPU
    (`uglad_covariance`, beyond the eigensolver's size `uglad_covariance_wide`) instead of in fp64 numpy on the host
    (prepare_data.py:328-356)."""
    global _DEVICE_COVARIANCE
    saved, _DEVICE_COVARIANCE = _DEVICE_COVARIANCE, bool(enabled)
    try:
        yield
    finally:
        _DEVICE_COVARIANCE = saved


REPAIR_THRESHOLD = 1e-6  # prepare_data.py:347: "min eig <= 1e-6 -> S += (offset - min eig) I"
REPAIR_BAND = 1e-4       # fp32 eigenvalues within this (relative to ||S||_2-ish scale) of the threshold are re-decided in fp64


def _device_covariance_group(X: np.ndarray, eval_offset: float) -> torch.Tensor:
    """(K, N, D) equally-shaped tables -> (K, D, D) repaired covariances on the device.

    The reference decides its repair from fp64 eigenvalues (prepare_data.py:343-352); the device sees fp32 eigenvalues of an
    fp32 covariance, whose absolute error is ~1e-7 ||S||.  Where the device's smallest eigenvalue lies within REPAIR_BAND of
    the threshold the decision could flip -- an O(offset) discontinuity -- so exactly those matrices (rare: nearly singular
    with a minimum eigenvalue of ~1e-6) are re-decided from an fp64 eigvalsh on the host and corrected in place.
    Tables wider than the eigensolver's size go to the fp64 front-end, which needs no such band."""
    lib = _lib.get_lib()
    if X.shape[-1] > lib.max_eig_dim:
        # beyond the eigensolver's size: the fp64 front-end (csrc/cov_wide.h) takes the reference's decision itself, in fp64
        return lib.covariance_wide(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(_lib.device()), normalize=False,
                                   eval_offset=eval_offset, repair=True)
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(_lib.device())
    S, mn = lib.covariance(Xd, normalize=False, eval_offset=eval_offset, repair=True, return_min_eig=True)
    mn = mn.cpu().numpy().astype(np.float64)
    scale = np.maximum(1.0, S.diagonal(dim1=1, dim2=2).abs().sum(1).cpu().numpy())  # trace >= ||S||_2 for a PSD matrix
    for k in np.nonzero(np.abs(mn - REPAIR_THRESHOLD) <= REPAIR_BAND * scale)[0]:
        applied = mn[k] <= REPAIR_THRESHOLD
        Sk = S[k].double().cpu().numpy()
        if applied:
            Sk = Sk - (eval_offset - mn[k]) * np.eye(Sk.shape[0])  # undo the device's shift, decide again
        mn64 = float(np.linalg.eigvalsh(0.5 * (Sk + Sk.T)).min())
        if mn64 <= REPAIR_THRESHOLD:
            Sk = Sk + (eval_offset - mn64) * np.eye(Sk.shape[0])
        S[k] = torch.from_numpy(Sk.astype(np.float32)).to(S.device)
    return S


def _covariance(Xb, eval_offset):
    """Tables (K,N,D) -> (K,D,D) fp32 covariances on the device, repaired as prepare_data.get_covariance does.
    Under device_covariance the tables are grouped by shape (missing mode's row-subsampled folds and multitask tables may
    differ in length) and every group of equal shape is one launch of the device front-end."""
    if _DEVICE_COVARIANCE:
        tables = [np.asarray(x) for x in Xb]
        max_dim = _lib.get_lib().max_dim  # (what the cell covers; wider tables take the host path below, and fail at the cell)
        if tables and all(t.ndim == 2 and t.shape[1] <= max_dim and t.dtype != object for t in tables):
            groups = {}
            for i, t in enumerate(tables):
                groups.setdefault(t.shape, []).append(i)
            D = tables[0].shape[1]
            if all(shape[1] == D for shape in groups):
                out = torch.empty(len(tables), D, D, dtype=torch.float32, device=_lib.device())
                for idx in groups.values():
                    out[idx] = _device_covariance_group(np.stack([tables[i] for i in idx]), eval_offset)
                return out
    return _to_dev(prepare_data.get_covariance(Xb, offset=eval_offset))


def mixed_association(df, dtype, repair: bool = True, eval_offset: float = 0.1):
    """The association matrix of a table that mixes categorical ('c') and real ('r') columns, on the device (uglad_association,
    csrc/assoc_wide.h; the reference's pairwise_cov_matrix, prepare_data.py:253-285): `dtype` maps column name -> 'c' | 'r'.  Returns
    (A, min_eig): A the (D, D) fp32 matrix on the device, with `repair` shifted like a covariance (min eig <= 1e-6: A += (eval_offset -
    min eig) I, prepare_data.py:347-352), and min_eig the smallest eigenvalue before the repair as a float (+inf where none was needed;
    None without `repair`)."""
    table, maps = prepare_data.encode_mixed_table(df, dtype)
    A, mn, _ = _lib.get_lib().association(torch.from_numpy(table[None]).to(_lib.device()), maps, eval_offset=eval_offset, repair=repair)
    return A[0], (None if mn is None else float(mn[0]))


def _rank_tables(X):
    """(tables (K, N, D) float64 contiguous, single, names): an (N, D) array or DataFrame, or a list / (K, N, D) array of tables."""
    names = [str(c) for c in X.columns] if hasattr(X, "columns") else None
    single = hasattr(X, "columns") or (not isinstance(X, (list, tuple)) and np.ndim(X) == 2)
    tables = np.array(X, dtype=np.float64, order="C")  # (a copy of its own: the caller's array may be read-only)
    tables = tables[None] if single else tables
    if tables.ndim != 3:
        raise ValueError("rank_correlation takes an (N, D) table, or a list / (K, N, D) array of tables of one shape")
    if np.isnan(tables).any():
        raise ValueError("rank_correlation: the table holds NaN; impute or drop those rows first")
    return tables, single, names


def rank_correlation(X, method: str = "kendall", transform: bool = True, repair: bool = True, eval_offset: float = 0.1):
    """The rank-based correlation matrix of the nonparanormal (Gaussian copula) model, on the device (uglad_rank_correlation,
    csrc/rank_wide.h; additive, what R's huge.npn offers): `method` "spearman" (with `transform` 2 sin(pi rho / 6)), "kendall" (tau-b,
    sin(pi tau / 2): the SKEPTIC estimator) or "scores" (the correlation of Phi^-1(rank / (N + 1))).  X is an (N, D) array or DataFrame,
    or a list / (K, N, D) array of tables of one shape.  Returns (A, min_eig) like mixed_association: A the (D, D) -- or (K, D, D) -- fp32
    matrix on the device, with `repair` shifted like a covariance (min eig <= 1e-6: A += (eval_offset - min eig) I), and min_eig the
    smallest eigenvalue before the repair as a float -- or a (K,) float64 array -- (+inf where none was needed; None without `repair`).
    A constant column gives NaN in its row and column; a NaN raises ValueError."""
    tables, single, _ = _rank_tables(X)
    out = _lib.get_lib().rank_correlation(torch.from_numpy(tables).to(_lib.device()), method, transform=transform,
                                          eval_offset=eval_offset, repair=repair)
    mn = None if out.min_eig is None else out.min_eig.cpu().numpy()
    if single:
        return out.A[0], (None if mn is None else float(mn[0]))
    return out.A, mn


def _print_every(EPOCHS: int) -> int:
    return max(1, int(EPOCHS / 10))


def _allreduce_grads(model, loss, coll: Collective):
    """Exchange (ii): SUM of the 42 gradients and of the loss over ranks, in one 43-float message."""
    if coll.world_size == 1:
        return loss.detach()
    flat = torch.cat([p.grad.reshape(-1) for p in model.parameters()] + [loss.detach().reshape(1)])
    coll.all_reduce_sum(flat)
    off = 0
    for p in model.parameters():
        n = p.numel()
        p.grad.copy_(flat[off:off + n].reshape(p.shape))
        off += n
    return flat[off]


# ============================================================================================ drivers
def run_uGLAD_direct(Xb, trueTheta=None, eval_offset=0.1, EPOCHS=250, lr=0.002, INIT_DIAG=0, L=15, VERBOSE=True,
                     sqrt_mode=None, Sb=None):
    """Direct mode: one table, one covariance, EPOCHS Adam steps on the glasso loss (ref main.py:338-425).
    Passing trueTheta adds the reference's log-cosh structure penalty to the loss (main.py:398).
    Sb (additive): the (B, D, D) fp32 input matrices already on the device -- Xb is then not looked at (fit_mixed: the association
    matrix of a mixed table takes the covariance's place)."""
    if Sb is None:
        Sb = _covariance(Xb, eval_offset)
    if trueTheta is not None:
        trueTheta = _to_dev(trueTheta)
    B = Sb.shape[0]
    model_glad, optimizer_glad = init_uGLAD(lr=lr, theta_init_offset=1.0, nF=3, H=3)
    PRINT_EVERY = _print_every(EPOCHS)
    predTheta = None
    # The reference stops at the first NaN loss BEFORE that epoch's backward/step (main.py:401-406).  Asking the device for
    # the loss every epoch would stall the host behind the GPU, so the NaN flag of an epoch travels to pinned host memory
    # asynchronously and is looked at one epoch later; the speculative epoch is then undone (the 42 parameters are snapshotted
    # before every step), which leaves exactly the model the reference returns.
    lagged = Sb.is_cuda
    params = list(model_glad.parameters())
    pending = None  # (epoch, event, pinned flag, predTheta of that epoch, snapshot taken before that epoch's step)

    def snapshot():  # one launch: the 42 parameters packed (the optimiser is not returned, its state needs no rescue)
        return torch.cat([p.detach().reshape(-1) for p in params])

    def restore(snap):
        with torch.no_grad():
            off = 0
            for p in params:
                p.copy_(snap[off:off + p.numel()].reshape(p.shape))
                off += p.numel()

    def nan_epoch(p):
        p[1].synchronize()
        return bool(p[2].item())

    stopped = None
    for e in range(EPOCHS):
        optimizer_glad.zero_grad()
        predTheta_e, loss = forward_uGLAD(Sb, model_glad, L=L, INIT_DIAG=INIT_DIAG, struct_theta=trueTheta,
                                          sqrt_mode=sqrt_mode, collective=Collective())
        if lagged:
            if pending is not None and nan_epoch(pending):
                stopped = pending
                break
            flag = torch.empty(1, dtype=torch.bool).pin_memory()
            flag.copy_(torch.isnan(loss.detach()).reshape(1), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            pending = (e, ev, flag, predTheta_e, snapshot())
        elif torch.isnan(loss):
            print(f"Warning: NaN loss encountered at epoch {e}. Try updating the parameters and train.")
            predTheta = predTheta_e
            break
        predTheta = predTheta_e
        loss.backward()
        if not e % PRINT_EVERY and VERBOSE:
            print(f"epoch:{e}/{EPOCHS} loss:{loss.item()}")
        optimizer_glad.step()
    if lagged and stopped is None and pending is not None and nan_epoch(pending):
        stopped = pending  # the very last epoch was the NaN one
    if stopped is not None:
        print(f"Warning: NaN loss encountered at epoch {stopped[0]}. Try updating the parameters and train.")
        restore(stopped[4])
        predTheta = stopped[3]
    compare_theta = None
    if trueTheta is not None and predTheta is not None:
        compare_theta = device_report_metrics(trueTheta, predTheta)[B - 1]  # (the reference keeps the last matrix's dict)
        if VERBOSE:
            print(f"Compare - {compare_theta}")
    return predTheta, compare_theta, model_glad


def _kfold_indices(n: int, k: int):
    """sklearn KFold(n_splits=k) without shuffling: (train, test) index pairs."""
    if k < 2 or k > n:
        raise ValueError(f"k_fold must be in [2, n_samples], got {k}")
    sizes = np.full(k, n // k, dtype=int)
    sizes[: n % k] += 1
    idx = np.arange(n)
    cur = 0
    for s in sizes:
        test = idx[cur:cur + s]
        yield np.concatenate([idx[:cur], idx[cur + s:]]), test
        cur += s


def _cv_fold(_k, Sb_train, Sb_test, model_glad, optimizer_glad, EPOCHS, INIT_DIAG, L, VERBOSE, sqrt_mode):
    """One fold of run_uGLAD_CV: EPOCHS x {training step on the train-fold covariance, no_grad forward on the test fold}.
    The best-so-far test loss and the parameters that go with it are tracked ON THE DEVICE (a select per parameter tensor
    instead of the reference's host-side comparison + deepcopy, main.py:506-518), so an epoch needs no device-to-host copy
    and the host can run ahead of the GPU; the selection is the reference's: strictly smaller test loss, snapshot taken
    AFTER this epoch's optimiser step, NaN never wins."""
    one = Collective()
    params = list(model_glad.parameters())
    best_loss = torch.full((), float("inf"), dtype=torch.float32, device=Sb_train.device)
    best_state = torch.cat([p.detach().reshape(-1) for p in params])  # the 42 parameters, packed
    PRINT_EVERY = _print_every(EPOCHS)
    for e in range(EPOCHS):
        optimizer_glad.zero_grad()
        _, loss_train = forward_uGLAD(Sb_train, model_glad, L=L, INIT_DIAG=INIT_DIAG, sqrt_mode=sqrt_mode, collective=one)
        with torch.no_grad():
            _, loss_test = forward_uGLAD(Sb_test, model_glad, L=L, INIT_DIAG=INIT_DIAG, sqrt_mode=sqrt_mode, collective=one)
        loss_train.backward()
        optimizer_glad.step()
        with torch.no_grad():
            lt = loss_test.reshape(())
            improved = lt < best_loss
            best_loss = torch.where(improved, lt, best_loss)
            best_state = torch.where(improved, torch.cat([p.reshape(-1) for p in params]), best_state)
        if not e % PRINT_EVERY and VERBOSE:
            print(f"Fold {_k}: epoch:{e}/{EPOCHS} test-loss:{float(loss_test.item())}")
    best = float(best_loss.item())
    best_model = None
    if best < np.inf:
        best_model = copy.deepcopy(model_glad)
        with torch.no_grad():
            off = 0
            for p in best_model.parameters():
                p.copy_(best_state[off:off + p.numel()].reshape(p.shape))
                off += p.numel()
    return {"test_loss": best, "model": best_model}


def _cv_folds_batched(folds, EPOCHS, lr, INIT_DIAG, L, VERBOSE, sqrt_mode):
    """All folds of CV mode as ONE batch: fold k = group k of a grouped pass, with its own 42 parameters and
    its own lambda sequence (glad_grouped); one Adam over the (k, 42) parameter table (Adam is entrywise, so every fold gets
    exactly the updates of its own optimiser); the best test loss per fold and the parameters that go with it are selected on
    the device.  Per epoch: one grouped training pass, one grouped no_grad pass on the test folds, no host synchronisation."""
    from .glad.glad import glad_grouped

    k = len(folds)
    S_train = torch.cat([f[1] for f in folds])  # (k, D, D): one train-fold covariance per group
    S_test = torch.cat([f[2] for f in folds])
    S_both = torch.cat([S_train, S_test])
    P = torch.nn.Parameter(torch.stack([f[3].packed().detach() for f in folds]))  # models were initialised in fold order
    opt = glad.get_optimizers(_ParamTable(P), lr_glad=lr)
    best_loss = torch.full((k,), float("inf"), dtype=torch.float32, device=P.device)
    best_P = P.detach().clone()
    PRINT_EVERY = _print_every(EPOCHS)
    for e in range(EPOCHS):
        opt.zero_grad()
        # train folds and test folds ride in ONE grouped pass of 2k groups (a small pass is bound by the latency of its
        # kernels, not by how many matrices it carries); the test groups see the same parameters, detached
        theta = glad_grouped(S_both, torch.cat([P, P.detach()]), L=L, INIT_DIAG=INIT_DIAG, sqrt_mode=sqrt_mode)
        loss_train = loss_uGLAD(theta[:k], S_train, batch_divisor=1)  # sum of the folds' losses: d/dP[k] is fold k's own gradient
        with torch.no_grad():
            loss_test = _loss_per_matrix(theta[k:], S_test)
        loss_train.backward()
        opt.step()
        with torch.no_grad():
            improved = loss_test < best_loss  # (NaN never wins; snapshot AFTER this epoch's step, as in main.py:506,518)
            best_loss = torch.where(improved, loss_test, best_loss)
            best_P = torch.where(improved[:, None], P.detach(), best_P)
        if not e % PRINT_EVERY and VERBOSE:
            print(f"epoch:{e}/{EPOCHS} test-loss per fold: {[float(v) for v in loss_test.cpu()]}")
    results = {}
    bl = best_loss.cpu().numpy()
    for i, f in enumerate(folds):
        model = None
        if bl[i] < np.inf:
            model = copy.deepcopy(f[3])
            with torch.no_grad():
                off = 0
                for p in model.parameters():
                    p.copy_(best_P[i, off:off + p.numel()].reshape(p.shape))
                    off += p.numel()
        results[f[0]] = {"test_loss": float(bl[i]), "model": model}
    return results


class _ParamTable(torch.nn.Module):
    """A module around one (G, 42) parameter table, so that get_optimizers() can be handed the usual `.parameters()`."""

    def __init__(self, table: torch.nn.Parameter):
        super().__init__()
        self.table = table


def run_uGLAD_CV(Xb, trueTheta=None, eval_offset=0.1, EPOCHS=250, lr=0.002, INIT_DIAG=0, L=15, VERBOSE=True, k_fold=5,
                 sqrt_mode=None, parallel_folds: bool = False, batched_folds: bool = False):
    """k-fold CV mode (ref main.py:428-550): per fold a fresh model, per epoch one training step on the train-fold
    covariance and one no_grad forward on the test fold; the model with the best test loss over all folds is run on the
    full covariance.

    batched_folds (additive): all folds in ONE grouped batch -- per-fold parameters and lambda sequences inside
    the kernels (`_cv_folds_batched`), no host synchronisation per epoch.

    parallel_folds (additive): the folds are independent problems of one matrix each -- a single small matrix
    keeps one CU busy for a few hundred microseconds per kernel -- so each fold trains in its own host thread on its own HIP
    stream and the GPU runs them side by side.  The arithmetic of a fold is untouched (same kernels, same order), so the
    result is bit-identical to the sequential run; the models are still initialised in fold order, which keeps the draws
    from torch's global RNG those of the reference."""
    Sb = _covariance(Xb, eval_offset)
    if trueTheta is not None:
        trueTheta = _to_dev(trueTheta)
    one = Collective()
    B = 1
    folds = []
    for _k, (train, test) in enumerate(_kfold_indices(Xb[0].shape[0], k_fold)):
        Sb_train = _covariance(Xb[0][train][None], eval_offset)
        Sb_test = _covariance(Xb[0][test][None], eval_offset)
        model_glad, optimizer_glad = init_uGLAD(lr=lr, theta_init_offset=1.0, nF=3, H=3)
        folds.append((_k, Sb_train, Sb_test, model_glad, optimizer_glad))
    results = {}
    if batched_folds and len(folds) > 1:
        results = _cv_folds_batched(folds, EPOCHS, lr, INIT_DIAG, L, VERBOSE, sqrt_mode)
    elif parallel_folds and Sb.is_cuda and len(folds) > 1:
        import threading

        main_stream = torch.cuda.current_stream()
        streams = [torch.cuda.Stream(device=Sb.device) for _ in folds]
        errors = []

        def work(fold, stream):
            try:
                torch.cuda.set_device(Sb.device)
                with torch.cuda.stream(stream):
                    results[fold[0]] = _cv_fold(*fold, EPOCHS, INIT_DIAG, L, VERBOSE, sqrt_mode)
            except BaseException as exc:  # surfaced in the caller's thread below
                errors.append(exc)

        for s in streams:
            s.wait_stream(main_stream)  # the covariances and the initial parameters were produced on the caller's stream
        threads = [threading.Thread(target=work, args=(f, s)) for f, s in zip(folds, streams)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for s in streams:
            main_stream.wait_stream(s)
        if errors:
            raise errors[0]
    else:
        for fold in folds:
            if VERBOSE:
                print(f"Fold num {fold[0]}")
            results[fold[0]] = _cv_fold(*fold, EPOCHS, INIT_DIAG, L, VERBOSE, sqrt_mode)
    results = {k: results[k] for k in sorted(results)}
    best_loss = np.inf
    model_glad = None
    for _k in results:
        if results[_k]["test_loss"] < best_loss:
            model_glad = results[_k]["model"]
            best_loss = results[_k]["test_loss"]
    if model_glad is None:
        raise ValueError("cross-validation produced no finite test loss")
    with torch.no_grad():
        predTheta, _ = forward_uGLAD(Sb, model_glad, L=L, INIT_DIAG=INIT_DIAG, sqrt_mode=sqrt_mode, collective=one)
    compare_theta = None
    if trueTheta is not None:
        compare_theta = device_report_metrics(trueTheta, predTheta)[B - 1]
        if VERBOSE:
            print(f"Comparison - {compare_theta}")
    return predTheta, compare_theta, model_glad


def mean_imputation(Xb: np.ndarray) -> np.ndarray:
    """NaN -> column mean; an all-NaN column is an error (ref main.py:647-670; ValueError instead of sys.exit)."""
    X = np.array(Xb[0], dtype=np.float64)
    with np.errstate(all="ignore"):
        col_mean = np.nanmean(X, axis=0)
    if np.isnan(col_mean).any():
        raise ValueError("One or more columns have all NaNs")
    r, c = np.where(np.isnan(X))
    X[r, c] = col_mean[c]
    return X[None]


def get_final_precision_from_batch(predTheta: torch.Tensor, type: str = "min",
                                   collective: Optional[Collective] = None) -> torch.Tensor:
    """Consensus over K precision matrices: sign by majority (ties -> +), magnitude = min_k |Theta_k| (ref main.py:673-716).
    With a sharded batch the two partial results are all-reduced (MIN, SUM) before being combined.
    type="mean" -- buggy in the reference (it broadcasts row 0 of the mean, main.py:705) -- is implemented as the
    entrywise mean of |Theta_k| and is a labelled deviation."""
    lib = _lib.get_lib()
    coll = collective if collective is not None else Collective()
    predTheta = predTheta.detach().contiguous()
    K, D, _ = predTheta.shape
    f32 = dict(dtype=torch.float32, device=predTheta.device)
    absmin = torch.empty(D, D, **f32)
    signsum = torch.empty(D, D, **f32)
    lib.consensus_partial(predTheta, absmin, signsum)
    coll.all_reduce_min(absmin)
    coll.all_reduce_sum(signsum)
    if type == "min":
        value = absmin
    elif type == "mean":
        tot = predTheta.abs().sum(0)
        cnt = torch.tensor([float(K)], **f32)
        coll.all_reduce_sum(tot)
        coll.all_reduce_sum(cnt)
        value = (tot / cnt).contiguous()
    else:
        raise ValueError(f"Enter valid type min/mean, currently {type}")
    out = torch.empty(D, D, **f32)
    lib.consensus_combine(value, signsum, out)
    return out.reshape(1, D, D)


def run_uGLAD_missing(Xb, trueTheta=None, eval_offset=0.1, EPOCHS=250, lr=0.002, INIT_DIAG=0, L=15, VERBOSE=True,
                      K_batch=3, sqrt_mode=None):
    """Missing-data mode (ref main.py:553-644): mean imputation, K row-subsampled covariances as one multi-task batch whose
    loss is taken against the single full-data covariance (divisor 1), consensus at the end.  Under torch.distributed the K
    sub-batches are sharded over the ranks (config 5: one per GPU)."""
    if K_batch == 0:
        K_batch = 3
    coll = get_collective()
    _check_shardable(K_batch, coll, "K_batch sub-sample covariances")
    Xb = mean_imputation(Xb)
    Sb = _covariance(Xb, eval_offset)
    folds = [tr for tr, _ in _kfold_indices(Xb[0].shape[0], K_batch)]
    lo, hi = coll.shard(K_batch)
    X_K = [Xb[0][idx] for idx in folds[lo:hi]]
    S_K = _covariance(X_K, eval_offset)
    if trueTheta is not None:
        trueTheta = _to_dev(trueTheta)
    model_glad, optimizer_glad = init_uGLAD(lr=lr, theta_init_offset=1.0, nF=3, H=3)
    _broadcast_model(model_glad, coll)
    PRINT_EVERY = _print_every(EPOCHS)
    predTheta = None
    for e in range(EPOCHS):
        optimizer_glad.zero_grad()
        predTheta, loss = forward_uGLAD(S_K, model_glad, L=L, INIT_DIAG=INIT_DIAG, loss_Sb=Sb, sqrt_mode=sqrt_mode,
                                        collective=coll, global_batch=K_batch)
        loss.backward()
        total = _allreduce_grads(model_glad, loss, coll)
        optimizer_glad.step()
        if not e % PRINT_EVERY and VERBOSE:
            print(f"epoch:{e}/{EPOCHS} loss:{float(total)}")
    predTheta = get_final_precision_from_batch(predTheta, type="min", collective=coll)
    compare_theta = None
    if trueTheta is not None:
        compare_theta = device_report_metrics(trueTheta[:1], predTheta[:1])[0]
        if VERBOSE:
            print(f"Comparison - {compare_theta}")
    return predTheta, compare_theta, model_glad


def _check_shardable(K: int, coll: Collective, what: str) -> None:
    """Every rank must own at least one matrix: an empty shard would fail locally while the other ranks wait in the first
    collective.  K and world_size are known everywhere, so every rank raises the same error before any exchange."""
    if K < coll.world_size:
        raise ValueError(f"{K} {what} cannot be sharded over {coll.world_size} ranks (need at least one per rank)")


def _broadcast_model(model, coll: Collective):
    """Replicate rank 0's freshly initialised 42 parameters (each rank draws its own otherwise)."""
    if coll.world_size == 1:
        return
    with torch.no_grad():
        flat = torch.cat([p.reshape(-1) for p in model.parameters()])
        if coll.rank != 0:
            flat.zero_()
        coll.all_reduce_sum(flat)
        off = 0
        for p in model.parameters():
            n = p.numel()
            p.copy_(flat[off:off + n].reshape(p.shape))
            off += n


def run_uGLAD_multitask(Xb, trueTheta=None, eval_offset=0.1, EPOCHS=250, lr=0.002, INIT_DIAG=0, L=15, VERBOSE=True,
                        sqrt_mode=None):
    """Multi-task mode (ref main.py:719-789): K tables -> K covariances -> ONE shared 42-parameter model trained on the
    batch.  Under torch.distributed every rank passes the full list and works on its contiguous slice; the per-step
    norm, the gradients and the final precision matrices are exchanged over RCCL, so every rank returns all K."""
    K = len(Xb)
    coll = get_collective()
    _check_shardable(K, coll, "tasks")
    lo, hi = coll.shard(K)
    Sb = _covariance(Xb[lo:hi], eval_offset)
    model_glad, optimizer_glad = init_uGLAD(lr=lr, theta_init_offset=1.0, nF=3, H=3)
    _broadcast_model(model_glad, coll)
    PRINT_EVERY = _print_every(EPOCHS)
    predTheta = None
    for e in range(EPOCHS):
        optimizer_glad.zero_grad()
        predTheta, loss = forward_uGLAD(Sb, model_glad, L=L, INIT_DIAG=INIT_DIAG, sqrt_mode=sqrt_mode, collective=coll,
                                        global_batch=K)
        loss.backward()
        total = _allreduce_grads(model_glad, loss, coll)
        optimizer_glad.step()
        if not e % PRINT_EVERY and VERBOSE:
            print(f"epoch:{e}/{EPOCHS} loss:{float(total)}")
    predTheta = coll.all_gather_cat(predTheta.detach())
    compare_theta = []
    if trueTheta is not None:
        compare_theta = device_report_metrics(np.asarray(trueTheta), predTheta)  # all K graphs in one launch
        if VERBOSE:
            for b, rM in enumerate(compare_theta):
                print(f"Metrics for graph {b}: {rM}\n")
    return predTheta, compare_theta, model_glad


# ============================================================================================ public classes
class uGLAD_GL(object):
    """Drop-in for the reference's `uGLAD_GL` (main.py:34-151): `fit` sets covariance_ (float64), precision_ (float32),
    location_, node_names_, model_glad and returns the metrics dict (or None) -- not self, like the reference."""

    def __init__(self, device_covariance: bool = False):
        """device_covariance (additive): form the input covariances + eigenvalue repair on the GPU."""
        super().__init__()
        self.device_covariance = bool(device_covariance)
        self.covariance_: Optional[np.ndarray] = None
        self.precision_: Optional[np.ndarray] = None
        self.location_: Optional[np.ndarray] = None
        self.data_min_: Optional[np.ndarray] = None    # (additive) column minima and ranges of the table fit() normalised: what
        self.data_range_: Optional[np.ndarray] = None  # places a new row in the model's coordinates (mahalanobis, score_samples, score)
        self.model_glad: Optional[GladParams] = None
        self._fit_cfg = None

    def fit(self, X, true_theta=None, eval_offset=0.1, centered=False, epochs=250, lr=0.002, INIT_DIAG=0, L=15,
            verbose=True, k_fold=3, mode="direct", node_names=None, sqrt_mode=None, parallel_folds=False,
            batched_folds=False):
        start = time()
        if verbose:
            print("Running uGLAD")
        processed = prepare_data.process_table(X, NORM="min_max", VERBOSE=verbose)
        data_min, data_range = prepare_data.kept_min_range(X, processed)
        X = np.array(processed)
        M, D = X.shape
        Xb = X.reshape(1, M, D)
        true_theta_b = None if true_theta is None else np.asarray(true_theta).reshape(1, D, D)
        kw = dict(trueTheta=true_theta_b, eval_offset=eval_offset, EPOCHS=epochs, lr=lr, INIT_DIAG=INIT_DIAG, L=L,
                  VERBOSE=verbose, sqrt_mode=sqrt_mode)
        with device_covariance(self.device_covariance), glad.regime_monitor() as regime:
            if mode == "missing":
                pred_theta, compare_theta, model_glad = run_uGLAD_missing(Xb, K_batch=k_fold, **kw)
            elif mode == "cv" and k_fold >= 0:
                pred_theta, compare_theta, model_glad = run_uGLAD_CV(Xb, k_fold=k_fold, parallel_folds=parallel_folds,
                                                                         batched_folds=batched_folds, **kw)
            elif mode == "direct":
                pred_theta, compare_theta, model_glad = run_uGLAD_direct(Xb, **kw)
            else:
                raise ValueError(f"Please enter K-fold value in valid range [0, ), currently entered {k_fold}; check mode {mode}")
        self.covariance_ = prepare_data.empirical_covariance(X, assume_centered=centered)
        self.location_ = X.mean(axis=0)
        self.data_min_, self.data_range_ = data_min, data_range
        self.node_names_ = list(node_names) if node_names is not None else [f"node_{i}" for i in range(D)]
        if pred_theta is not None:
            self.precision_ = pred_theta[0].detach().cpu().numpy()
        if model_glad is not None:
            self.model_glad = model_glad
        self._fit_cfg = dict(L=L, INIT_DIAG=INIT_DIAG, eval_offset=eval_offset, sqrt_mode=sqrt_mode)
        # regime diagnostic (additive): the largest cond(b^T b + 4/lambda I) any pass of this fit saw; warns beyond the validated bound
        self.cond_max_ = regime.warn_if_outside("uGLAD_GL.fit", get_collective() if mode == "missing" else None)  # (the sharded mode)
        if verbose:
            print(f"Total runtime: {time() - start} secs\n")
        return compare_theta

    def fit_mixed(self, df, dtype, true_theta=None, eval_offset=0.1, epochs=250, lr=0.002, INIT_DIAG=0, L=15, verbose=True,
                  sqrt_mode=None):
        """`fit` for a table that mixes categorical and real columns (additive; the reference stops at pairwise_cov_matrix,
        prepare_data.py:253-285, and has no route from it into the model): `dtype` maps column name -> 'c' | 'r'.  The table is encoded
        on the host (prepare_data.encode_mixed_table), its association matrix -- Cramer's V, the correlation ratio, Pearson's r -- is
        formed and repaired on the device (uglad_association), and direct-mode training runs on that matrix.  Sets covariance_ (the
        UNREPAIRED association matrix, float64), precision_, location_ (the means of the 'r' columns, NaN for 'c'), node_names_ (the
        column names), model_glad, cond_max_ and association_min_eig_; predict(S=...), recovered_graph() and save / load work afterwards.
        Direct mode only: CV, missing and multitask modes are out of scope for mixed tables -- a fold can lose levels of a categorical,
        so every fold would need an encoding of its own."""
        start = time()
        if verbose:
            print("Running uGLAD on a mixed table")
        table, maps = prepare_data.encode_mixed_table(df, dtype)
        D = table.shape[1]
        A, mn, A64 = _lib.get_lib().association(torch.from_numpy(table[None]).to(_lib.device()), maps, eval_offset=eval_offset,
                                                repair=True, want_f64=True)
        true_theta_b = None if true_theta is None else np.asarray(true_theta).reshape(1, D, D)
        with glad.regime_monitor() as regime:
            pred_theta, compare_theta, model_glad = run_uGLAD_direct(None, trueTheta=true_theta_b, eval_offset=eval_offset, EPOCHS=epochs,
                                                                     lr=lr, INIT_DIAG=INIT_DIAG, L=L, VERBOSE=verbose,
                                                                     sqrt_mode=sqrt_mode, Sb=A)
        self.covariance_ = A64[0].cpu().numpy()
        self.association_min_eig_ = float(mn[0])
        self.location_ = np.where(maps.kinds == "r", table.mean(axis=0), np.nan)
        self.data_min_ = self.data_range_ = None  # (a mixed table is not normalised, and its rows cannot be scored)
        self.node_names_ = [str(n) for n in maps.names]
        if pred_theta is not None:
            self.precision_ = pred_theta[0].detach().cpu().numpy()
        if model_glad is not None:
            self.model_glad = model_glad
        self._fit_cfg = dict(L=L, INIT_DIAG=INIT_DIAG, eval_offset=eval_offset, sqrt_mode=sqrt_mode)
        self.cond_max_ = regime.warn_if_outside("uGLAD_GL.fit_mixed", None)
        if verbose:
            print(f"Total runtime: {time() - start} secs\n")
        return compare_theta

    def fit_copula(self, X, method="kendall", true_theta=None, eval_offset=0.1, epochs=250, lr=0.002, INIT_DIAG=0, L=15, verbose=True,
                   sqrt_mode=None):
        """`fit` under the nonparanormal (Gaussian copula) model (additive; the reference has no such option): for a table whose columns
        are not Gaussian after any normalisation -- counts, concentrations, skewed and heavy-tailed measurements -- the covariance is
        replaced by a rank-based correlation matrix, `method` "kendall", "spearman" or "scores" (rank_correlation), formed and repaired
        on the device (uglad_rank_correlation), and direct-mode training runs on that matrix.  X is an (N, D) array or DataFrame.  Sets
        covariance_ (the UNREPAIRED matrix, float64), precision_, location_ (the column means), node_names_ (a DataFrame's columns),
        model_glad, cond_max_ and copula_min_eig_; predict(S=...), recovered_graph() and save / load work afterwards.  Direct mode
        only: CV, missing and multitask modes are out of scope."""
        start = time()
        if verbose:
            print("Running uGLAD on a rank correlation matrix")
        tables, single, names = _rank_tables(X)
        if not single:
            raise ValueError("fit_copula takes one (N, D) table")
        D = tables.shape[2]
        names = names if names is not None else [f"node_{i}" for i in range(D)]
        out = _lib.get_lib().rank_correlation(torch.from_numpy(tables).to(_lib.device()), method, transform=True, eval_offset=eval_offset,
                                              repair=True, want_f64=True)
        constant = np.nonzero(out.info[0].cpu().numpy() & 2)[0]
        if len(constant):
            raise ValueError(f"fit_copula: constant columns have no rank correlation: {[names[i] for i in constant]}")
        true_theta_b = None if true_theta is None else np.asarray(true_theta).reshape(1, D, D)
        with glad.regime_monitor() as regime:
            pred_theta, compare_theta, model_glad = run_uGLAD_direct(None, trueTheta=true_theta_b, eval_offset=eval_offset, EPOCHS=epochs,
                                                                     lr=lr, INIT_DIAG=INIT_DIAG, L=L, VERBOSE=verbose,
                                                                     sqrt_mode=sqrt_mode, Sb=out.A)
        self.covariance_ = out.A64[0].cpu().numpy()
        self.copula_min_eig_ = float(out.min_eig[0])
        self.location_ = tables[0].mean(axis=0)
        self.data_min_ = self.data_range_ = None  # (rows of a copula fit are not scored)
        self.node_names_ = names
        if pred_theta is not None:
            self.precision_ = pred_theta[0].detach().cpu().numpy()
        if model_glad is not None:
            self.model_glad = model_glad
        self._fit_cfg = dict(L=L, INIT_DIAG=INIT_DIAG, eval_offset=eval_offset, sqrt_mode=sqrt_mode)
        self.cond_max_ = regime.warn_if_outside("uGLAD_GL.fit_copula", None)
        if verbose:
            print(f"Total runtime: {time() - start} secs\n")
        return compare_theta

    def recovered_graph(self, sparsity: float = 0.1):
        """The graph of the fitted precision_ (recovered_graph): the `sparsity` fraction of the edges with the largest |rho|."""
        if self.precision_ is None:
            raise ValueError("call fit() first")
        return recovered_graph(self.precision_, sparsity=sparsity)

    def predict(self, X=None, S=None) -> np.ndarray:
        """Inference-only pass: the trained 42 parameters applied to new data (no_grad forward, the reference's
        main.py:539-540 pattern).  Give a samples table X (processed like `fit` does) or covariance(s) S.
        Warns (UgladRegimeWarning) when the pass leaves the validated regime -- e.g. an un-normalised covariance given as S."""
        if self.model_glad is None:
            raise ValueError("call fit() first")
        cfg = self._fit_cfg
        if S is None:
            X = np.array(prepare_data.process_table(X, NORM="min_max", VERBOSE=False))
            S = prepare_data.get_covariance(X[None], offset=cfg["eval_offset"])
        S = np.asarray(S, dtype=np.float64)
        if S.ndim == 2:
            S = S[None]
        with torch.no_grad(), glad.regime_monitor() as regime:
            theta = glad.glad(_to_dev(S), self.model_glad, L=cfg["L"], INIT_DIAG=cfg["INIT_DIAG"],
                              sqrt_mode=cfg["sqrt_mode"], collective=Collective())
        self.predict_cond_max_ = regime.warn_if_outside("uGLAD_GL.predict")
        out = theta.cpu().numpy()
        return out[0] if out.shape[0] == 1 else out


    # ---- scoring rows (additive: sklearn's covariance estimators carry these three, the reference none)
    def _model_coordinates(self, X, normalized: bool) -> np.ndarray:
        if self.precision_ is None or self.location_ is None:
            raise ValueError("call fit() first")
        if np.isnan(self.location_).any():
            raise ValueError("location_ holds NaN for the categorical columns of a fit_mixed() table: its rows have no Gaussian score")
        return _to_model_coordinates(X, None if normalized else (self.data_min_, self.data_range_), len(self.location_))

    def mahalanobis(self, X, normalized: bool = False) -> np.ndarray:
        """SQUARED Mahalanobis distances (N,) of the rows of X to location_ under precision_ (as sklearn's `mahalanobis`), float64, on
        the device (uglad_sample_scores).  X has the D columns fit() kept, in node_names_ order, in the units of the training table:
        it is mapped by (X - data_min_) / data_range_ in fp64 and no row is dropped; `normalized=True` takes X as already mapped.  A
        NaN in a row gives NaN for that row only."""
        return sample_scores(self.precision_, self.location_, self._model_coordinates(X, normalized)).mahalanobis

    def score_samples(self, X, normalized: bool = False) -> np.ndarray:
        """Gaussian log-density (N,) of every row of X under (location_, precision_) (sklearn's `score_samples`); X as for mahalanobis."""
        return sample_scores(self.precision_, self.location_, self._model_coordinates(X, normalized)).log_density

    def score(self, X, normalized: bool = False) -> float:
        """The mean of score_samples(X) (sklearn's `score`)."""
        return float(np.mean(self.score_samples(X, normalized=normalized)))


class uGLAD_multitask(object):
    """Drop-in for the reference's `uGLAD_multitask` (main.py:155-226): K tables, one shared model, batched attributes."""

    def __init__(self, device_covariance: bool = False):
        super().__init__()
        self.device_covariance = bool(device_covariance)
        self.covariance_ = []
        self.precision_: Optional[np.ndarray] = None
        self.location_: Optional[np.ndarray] = None    # (additive) (K, D) each: the tasks' means, and the column minima and ranges of
        self.data_min_: Optional[np.ndarray] = None    # the tables fit() normalised (mahalanobis, score_samples, score)
        self.data_range_: Optional[np.ndarray] = None
        self.model_glad: Optional[GladParams] = None
        self._fit_cfg = None

    def fit(self, Xb, true_theta_b=None, eval_offset=0.1, centered=False, epochs=250, lr=0.002, INIT_DIAG=0, L=15,
            verbose=True, sqrt_mode=None):
        start = time()
        if verbose:
            print("Running uGLAD in multi-task mode")
        processed = [prepare_data.process_table(X, NORM="min_max", VERBOSE=verbose) for X in Xb]
        min_range = [prepare_data.kept_min_range(X, P) for X, P in zip(Xb, processed)]
        Xb = [np.array(P) for P in processed]
        with device_covariance(self.device_covariance), glad.regime_monitor() as regime:
            pred_theta, compare_theta, model_glad = run_uGLAD_multitask(
                Xb, trueTheta=true_theta_b, eval_offset=eval_offset, EPOCHS=epochs, lr=lr, INIT_DIAG=INIT_DIAG, L=L,
                VERBOSE=verbose, sqrt_mode=sqrt_mode)
        self.covariance_ = np.array([prepare_data.empirical_covariance(X, assume_centered=centered) for X in Xb])
        self.precision_ = pred_theta.detach().cpu().numpy()
        self.location_ = np.array([X.mean(axis=0) for X in Xb])
        self.data_min_, self.data_range_ = np.array([m for m, _ in min_range]), np.array([r for _, r in min_range])
        self.model_glad = model_glad
        self._fit_cfg = dict(L=L, INIT_DIAG=INIT_DIAG, eval_offset=eval_offset, sqrt_mode=sqrt_mode)
        self.cond_max_ = regime.warn_if_outside("uGLAD_multitask.fit", get_collective())
        if verbose:
            print(f"Total runtime: {time() - start} secs\n")
        return compare_theta

    def recovered_graph(self, sparsity: float = 0.1):
        """The K graphs of the fitted precision_ (recovered_graph): the `sparsity` fraction of the edges with the largest |rho|."""
        if self.precision_ is None:
            raise ValueError("call fit() first")
        return recovered_graph(self.precision_, sparsity=sparsity)

    def predict(self, Xb=None, S=None) -> np.ndarray:
        """no_grad forward of the trained model on new tables (list) or covariances (K, D, D)."""
        if self.model_glad is None:
            raise ValueError("call fit() first")
        cfg = self._fit_cfg
        if S is None:
            Xb = [np.array(prepare_data.process_table(X, NORM="min_max", VERBOSE=False)) for X in Xb]
            S = prepare_data.get_covariance(Xb, offset=cfg["eval_offset"])
        with torch.no_grad(), glad.regime_monitor() as regime:
            theta = glad.glad(_to_dev(np.asarray(S, dtype=np.float64)), self.model_glad, L=cfg["L"],
                              INIT_DIAG=cfg["INIT_DIAG"], sqrt_mode=cfg["sqrt_mode"], collective=Collective())
        self.predict_cond_max_ = regime.warn_if_outside("uGLAD_multitask.predict")
        return theta.cpu().numpy()


    # ---- scoring rows (additive, as uGLAD_GL's)
    def _scores(self, X, normalized: bool):
        if self.precision_ is None or self.location_ is None:
            raise ValueError("call fit() first")
        K, D = self.location_.shape
        tables = list(X) if isinstance(X, (list, tuple)) or np.ndim(X) == 3 else [X] * K  # K tables pairwise, or one for every task
        if len(tables) != K:
            raise ValueError(f"{len(tables)} tables for {K} tasks")
        mapped = [_to_model_coordinates(T, None if normalized else (self.data_min_[k], self.data_range_[k]), D) for k, T in enumerate(tables)]
        if len({len(T) for T in mapped}) == 1:
            return sample_scores(self.precision_, self.location_, np.stack(mapped))
        each = [sample_scores(self.precision_[k], self.location_[k], T) for k, T in enumerate(mapped)]  # (tables of different lengths)
        return SampleScores([e.mahalanobis for e in each], [e.log_density for e in each], np.array([e.logdet for e in each]))

    def mahalanobis(self, X, normalized: bool = False):
        """SQUARED Mahalanobis distances (K, N) of the rows of one (N, D) table to every task's location_ under its precision_, each task
        mapping X with its own data_min_ / data_range_ (`normalized=True`: X is already mapped); a list of K tables (or a (K, N, D)
        array) is scored pairwise, table k by task k -- a list of K arrays when their lengths differ.  See uGLAD_GL.mahalanobis."""
        return self._scores(X, normalized).mahalanobis

    def score_samples(self, X, normalized: bool = False):
        """Gaussian log-densities (K, N), X as for mahalanobis: for one table the argmax over K is the most likely task of every row."""
        return self._scores(X, normalized).log_density

    def score(self, X, normalized: bool = False) -> np.ndarray:
        """(K,) means of score_samples(X) per task."""
        return np.array([float(np.mean(d)) for d in self._scores(X, normalized).log_density])


# ============================================================================================ scoring rows against fitted models
class SampleScores(NamedTuple):
    """What sample_scores returns, float64 numpy arrays."""
    mahalanobis: np.ndarray   # (K, N) squared distances xc^T P xc ((N,) for a single (D, D) model)
    log_density: np.ndarray   # (K, N) (logdet P - D log 2 pi - q) / 2
    logdet: np.ndarray        # (K,)   (a float64 scalar for a single model); NaN where P is not positive definite


SCORE_ROW_CHUNK = 65536  # rows per call of uglad_sample_scores unless row_chunk says otherwise (halved while the workspace is refused)


def _to_model_coordinates(X, min_range, D: int) -> np.ndarray:
    """(N, D) float64: X as given (min_range None) or mapped by (X - min) / range, the normalisation fit() applied to its own table."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != D:
        raise ValueError(f"X must be (N, {D}): the columns fit() kept, in node_names_ order; got {X.shape}")
    if min_range is None:
        return X
    mn, rg = min_range
    if mn is None or rg is None:
        raise ValueError("this model carries no data_min_ / data_range_ (fitted before they were kept?): pass normalized=True")
    return (X - mn) / rg


def sample_scores(precision, location, X, row_chunk=None) -> SampleScores:
    """Squared Mahalanobis distance and Gaussian log-density of every row of X under every model, on the device in fp64
    (uglad_sample_scores, csrc/score_wide.h): precision (D, D) or (K, D, D) -- its symmetric part is used --, location (D,) or (K, D), X
    (N, D) (one table for every model) or (K, N, D); numpy arrays or device tensors.  Rows go through in chunks of `row_chunk` (default
    SCORE_ROW_CHUNK, less where the workspace demands it), so any N fits; a row's numbers do not depend on the chunking, bit for bit.  A
    model that is not positive definite gets NaN in logdet and log_density and keeps its distances; a NaN in a row stays in that row."""
    lib = _lib.get_lib()
    dev = _lib.device()

    def to(a):
        if torch.is_tensor(a):
            return a.detach().to(device=dev, dtype=torch.float64).contiguous()
        a = np.ascontiguousarray(a, dtype=np.float64)
        return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)

    single = np.ndim(precision) == 2
    if np.ndim(precision) not in (2, 3) or np.shape(precision)[-1] > lib.max_dim:
        raise ValueError(f"precision must be (D, D) or (K, D, D) with D <= max_dim = {lib.max_dim}; got {tuple(np.shape(precision))}")
    P, mu = to(precision), to(location)
    P = P[None] if P.dim() == 2 else P
    mu = mu[None] if mu.dim() == 1 else mu
    if P.dim() != 3 or P.shape[1] != P.shape[2] or tuple(mu.shape) != tuple(P.shape[:2]):
        raise ValueError(f"precision (K, D, D) and location (K, D); got {tuple(P.shape)} and {tuple(mu.shape)}")
    K, D = mu.shape
    if not torch.is_tensor(X):
        X = np.asarray(X, dtype=np.float64)
    X = X[None] if X.ndim == 2 else X
    if X.ndim != 3 or X.shape[2] != D or X.shape[0] not in (1, K) or X.shape[1] < 1:
        raise ValueError(f"X must be (N, {D}) or ({K}, N, {D}) with N >= 1; got {tuple(X.shape)}")
    N = X.shape[1]
    chunk = min(N, int(row_chunk) if row_chunk else SCORE_ROW_CHUNK)
    if chunk < 1:
        raise ValueError("row_chunk must be positive")
    while chunk > 1 and int(lib._dll.uglad_sample_scores_workspace_floats(K, chunk, D)) < 0:
        chunk = (chunk + 1) // 2
    maha, dens, logdet = np.empty((K, N)), np.empty((K, N)), None
    for a in range(0, N, chunk):
        q, ld, det = lib.sample_scores(to(X[:, a:a + chunk]), P, mu)
        maha[:, a:a + chunk], dens[:, a:a + chunk] = q.cpu().numpy(), ld.cpu().numpy()
        logdet = det.cpu().numpy() if logdet is None else logdet  # (the same bits in every chunk)
    if single:
        return SampleScores(maha[0], dens[0], logdet[0])
    return SampleScores(maha, dens, logdet)


# ============================================================================================ after the path
METRIC_KEYS = ("FDR", "TPR", "FPR", "SHD", "nnzTrue", "nnzPred", "precision", "recall", "Fbeta", "aupr", "auc")


# Smallest D > max_eig_dim whose metrics report goes to uglad_support_metrics_wide; below it (and above max_eig_dim) the host formulation
# would run.  0: the whole range goes to the device.  scripts/metrics_wide_probe.py times both sides; a range where the host wins end to
# end belongs here.
WIDE_METRICS_MIN_DIM = 0


def device_report_metrics(true_theta, pred_theta, beta: int = 1):
    """`report_metrics_all` (ref utils/metrics.py:25-108) for K (true, predicted) precision matrices at once, counted on the
    device: list of K dicts with the reference's keys, rounded to 3 decimals as the reference does.  D <= max_eig_dim:
    uglad_support_metrics (one workgroup per pair); beyond, up to max_dim: uglad_support_metrics_wide (the edges sorted by score, many
    workgroups per pair)."""
    lib = _lib.get_lib()
    dev = _lib.device()
    T = torch.as_tensor(np.asarray(true_theta.detach().cpu() if torch.is_tensor(true_theta) else true_theta).real,
                        dtype=torch.float32) if not (torch.is_tensor(true_theta) and true_theta.device == dev) else true_theta
    G = pred_theta if torch.is_tensor(pred_theta) else torch.as_tensor(np.asarray(pred_theta).real, dtype=torch.float32)
    T = T.detach().to(device=dev, dtype=torch.float32)
    G = G.detach().to(device=dev, dtype=torch.float32)
    if T.dim() == 2:
        T, G = T[None], G[None]
    D = T.shape[-1]
    if D > lib.max_dim or lib.max_eig_dim < D < WIDE_METRICS_MIN_DIM:
        # beyond what the device covers: the report is evaluated where the reference evaluates it -- on the host, from the same definitions
        # (utils/metrics.py = ref utils/metrics.py:25-108).  After the path, once per fit; round 3 raised UgladError here AFTER all epochs
        # of a fit(X, true_theta=...) at D > 256 had run.
        Tn, Gn = T.cpu().numpy(), G.cpu().numpy()
        return [report_metrics_all(Tn[k], Gn[k], beta=beta) for k in range(Tn.shape[0])]
    metrics = lib.support_metrics if D <= lib.max_eig_dim else lib.support_metrics_wide
    out = metrics(T.contiguous(), G.contiguous(), beta=beta).cpu().numpy()
    return [{k: round(float(v), 3) for k, v in zip(METRIC_KEYS, row)} for row in out]


def get_partial_correlations(precision):
    """rho_ij = -p_ij / sqrt(p_ii p_jj), ones on the diagonal (ref main.py:796-821: its double loop fills the upper triangle
    with that formula and mirrors it).  (D,D) or (K,D,D).
    A host array (what the reference takes: `precision_` is numpy) is evaluated on the host in float64 like the reference -- an O(D^2)
    formula needs no GPU and loses nothing to fp32; a tensor already on the device goes through uglad_partial_correlations (fp32, K
    matrices per launch) and comes back as a device tensor."""
    if torch.is_tensor(precision) and precision.is_cuda:
        P = precision.detach().to(dtype=torch.float32)
        single = P.dim() == 2
        rho = _lib.get_lib().partial_correlations((P[None] if single else P).contiguous())
        return rho[0] if single else rho
    P = np.asarray(precision.detach().cpu() if torch.is_tensor(precision) else precision, dtype=np.float64)
    d = np.sqrt(np.diagonal(P, axis1=-2, axis2=-1))
    up = np.triu(-P / (d[..., :, None] * d[..., None, :]), k=1)  # the reference reads the upper triangle and mirrors it
    rho = up + np.swapaxes(up, -1, -2)
    idx = np.arange(P.shape[-1])
    rho[..., idx, idx] = 1.0
    return rho


# -------------------------------------------------------------------------------------------- the recovered graph
GRAPH_STAT_KEYS = ("num_nodes", "num_edges", "avg_degree", "density", "avg_clustering", "transitivity", "diameter", "avg_shortest_path")


class RecoveredGraph(object):
    """One recovered graph: `edges` (m, 2) int32 with i < j in row-major order, `weights` (m,) -- the partial correlation of every edge
    (float32 from the device, float64 from the host formulation) -- `threshold`, `degree` (D,), `triangles` (D,) (None without stats) and
    `stats`, a dict with the keys of the reference's compute_graph_statistics (diameter and avg_shortest_path None: networkx's to give)."""

    __slots__ = ("edges", "weights", "threshold", "degree", "triangles", "stats")

    def __init__(self, edges, weights, threshold, degree, triangles, stats):
        self.edges, self.weights, self.threshold, self.degree, self.triangles, self.stats = edges, weights, threshold, degree, triangles, stats

    @property
    def positive(self) -> np.ndarray:
        """(m,) bool: the edge's sign ("+", the reference's green: rho > th)."""
        return self.weights > self.threshold


def _stats_dict(six) -> dict:
    d = {"num_nodes": int(six[0]), "num_edges": int(six[1])}
    d.update({key: float(x) for key, x in zip(GRAPH_STAT_KEYS[2:6], six[2:6])})
    d["diameter"] = d["avg_shortest_path"] = None
    return d


def _n_keep(sparsity, D: int) -> int:
    E = D * (D - 1) // 2
    n = int(sparsity * E)  # (ref main.py:865)
    if not 0 <= n <= E:
        raise ValueError(f"sparsity {sparsity} keeps {n} of {E} edges")
    return n


def _recovered_graph_host(values, from_precision: bool, n_keep, threshold, stats: bool) -> RecoveredGraph:
    """uglad_graph_wide's definitions for ONE (D, D) matrix on the host in float64, vectorised (sort, compare, (A A) o A): for a host array
    whose values float32 cannot hold -- rounding could merge a value with the threshold -- and for sizes the device does not cover."""
    V = np.asarray(values, dtype=np.float64)
    D = V.shape[-1]
    i, j = np.triu_indices(D, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = -V[i, j] / np.sqrt(V[i, i] * V[j, j]) if from_precision else V[i, j]
    if n_keep is None:
        th = np.float64(threshold)
    else:
        s = np.sort(np.abs(rho))
        th = s[len(s) - n_keep] if n_keep > 0 else s[0]  # (the reference's rho_upper[-0])
    keep = (rho > th) | (rho < -th)
    ei, ej = i[keep], j[keep]
    A = np.zeros((D, D))
    A[ei, ej] = A[ej, ei] = 1.0
    degree = A.sum(axis=1).astype(np.int64)
    triangles = st = None
    if stats:
        t2 = ((A @ A) * A).sum(axis=1).astype(np.int64)  # (exact: integers below 2^53)
        triangles = t2 // 2
        st = _stats_dict(_six_statistics(D, int(keep.sum()), degree, t2))
    return RecoveredGraph(np.stack([ei, ej], axis=1).astype(np.int32), rho[keep], th, degree, triangles, st)


def _six_statistics(D: int, m: int, degree, t2):
    """The operations networkx performs (density, average_clustering, transitivity), in its order, on Python integers."""
    d = [int(x) for x in degree]
    t = [int(x) for x in t2]
    c = [0 if ti == 0 else ti / (di * (di - 1)) for di, ti in zip(d, t)]
    return (D, m, sum(d) / D, m / (D * (D - 1)) * 2, sum(c) / D, 0 if sum(t) == 0 else sum(t) / sum(di * (di - 1) for di in d))


def _fits_float32(a: np.ndarray) -> bool:
    if a.dtype == np.float32:
        return True
    with np.errstate(over="ignore", invalid="ignore"):
        back = a.astype(np.float32).astype(a.dtype)
    return bool(np.all((back == a) | (a != a)))


def _recovered_graphs(values, from_precision: bool, n_keep, threshold, stats: bool):
    """K graphs of a (K, D, D) device tensor or host array: on the device wherever float32 holds the values (uglad_graph_wide), else by
    the host formulation."""
    lib = _lib.get_lib()
    on_device = torch.is_tensor(values) and values.device.type != "cpu"
    host = None if on_device else np.asarray(values.detach() if torch.is_tensor(values) else values)
    K, D = int(values.shape[0]), int(values.shape[-1])
    if D < 2 or D > lib.max_dim or not (on_device or _fits_float32(host)):
        host = values.detach().cpu().numpy() if on_device else host
        return [_recovered_graph_host(host[k], from_precision, n_keep, threshold, stats) for k in range(K)]
    V = values.detach() if on_device else torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32))
    V = V.to(device=_lib.device(), dtype=torch.float32).contiguous()
    g = lib.graph_wide(V, n_keep=n_keep, threshold=None if n_keep is not None else threshold, from_precision=from_precision, want_stats=stats)
    count = g.edge_count.cpu().numpy()
    th, degree = g.threshold.cpu().numpy(), g.degree.cpu().numpy()
    t2, six = (g.triangles2.cpu().numpy(), g.stats.cpu().numpy()) if stats else (None, None)
    out = []
    for k in range(K):
        m = int(count[k])
        out.append(RecoveredGraph(g.edge_ij[k, :m].cpu().numpy(), g.edge_w[k, :m].cpu().numpy(), th[k], degree[k],
                                  t2[k] // 2 if stats else None, _stats_dict(six[k]) if stats else None))
    return out


def recovered_graph(precision, sparsity: float = 0.1, threshold=None, stats: bool = True):
    """The graph a precision matrix stands for (ref main.py:985-1005: partial correlations, then the `sparsity` fraction of the edges
    with the largest |rho|; or every edge beyond a given `threshold`), with degrees, triangle counts and the statistics of the reference's
    compute_graph_statistics, all computed on the device (uglad_graph_wide).  (D, D) or (K, D, D), a numpy array or a device tensor ->
    a RecoveredGraph or a list of K.  No networkx: graph_from_partial_correlations builds its nx.Graph from the same edge list."""
    single = len(precision.shape) == 2
    P = precision[None] if single else precision
    n_keep = None if threshold is not None else _n_keep(sparsity, int(P.shape[-1]))
    out = _recovered_graphs(P, True, n_keep, threshold, stats)
    return out[0] if single else out


def graph_from_partial_correlations(rho, names, sparsity=1, title="", fig_size=12, PLOT=True, save_file=None, roundOFF=5):
    """The reference's graph_from_partial_correlations (main.py:825-946), same arguments and return values: (nx.Graph with every node
    of `names` and the kept edges -- attributes color, weight rounded to `roundOFF` decimals, label -- , the PNG bytes of its drawing or
    None without PLOT, the edge list as strings).  The threshold, the membership test and the edge order come from uglad_graph_wide instead
    of a Python loop over D^2 entries: a device tensor stays on the device, a host array goes there when float32 holds its values
    exactly, and is otherwise evaluated on the host in float64 (rounding could merge values with the threshold)."""
    import networkx as nx

    names = list(names)
    D = int(rho.shape[-1])
    g = _recovered_graphs(rho[None], False, _n_keep(sparsity, D), None, False)[0]
    G = nx.Graph()
    G.add_nodes_from(names)
    edge_strings = []
    for (i, j), w, plus in zip(g.edges.tolist(), g.weights, g.positive):
        colour, w = ("green", "+") if plus else ("red", "-"), round(np.float64(w), roundOFF)
        G.add_edge(names[i], names[j], color=colour[0], weight=w, label=colour[1])
        edge_strings.append(f"({names[i]}, {names[j]}, {w}, {colour[0]})")
    return G, _draw_graph(G, title, fig_size, save_file) if PLOT else None, edge_strings


def _draw_graph(G, title, fig_size, save_file):
    """PNG bytes of a spring layout of G: grey nodes with their names just above them, edges in their colour, as wide as |weight| relative
    to the largest."""
    import io

    import matplotlib.pyplot as plt
    import networkx as nx

    colours = [c for _, _, c in G.edges(data="color")]
    widths = np.abs(np.array([w for _, _, w in G.edges(data="weight")], dtype=np.float64))
    if widths.size:
        widths = widths / widths.max()
    fig = plt.figure(figsize=(fig_size, fig_size))
    try:
        ax = fig.gca()
        where = nx.spring_layout(G, scale=0.2, k=1.0 / np.sqrt(G.number_of_edges() + 10))
        nx.draw_networkx_nodes(G, where, node_color="grey", node_size=100, ax=ax)
        nx.draw_networkx_edges(G, where, edge_color=colours, width=widths, ax=ax)
        nx.draw_networkx_labels(G, {node: (x, y + 0.008) for node, (x, y) in where.items()}, ax=ax)
        ax.set_title(str(title), fontsize=20)
        ax.margins(0.15)
        fig.tight_layout()
        if save_file:
            fig.savefig(save_file, bbox_inches="tight")
        png = io.BytesIO()
        fig.savefig(png)
        return png.getvalue()
    finally:
        plt.close(fig)


def compute_graph_statistics(G):
    """The reference's compute_graph_statistics (main.py:1263-1300): a one-row DataFrame with num_nodes, num_edges, avg_degree, density,
    avg_clustering, transitivity, diameter, avg_shortest_path.  The first six are counted on the device from G's adjacency matrix
    (uglad_graph_wide with the threshold 0.5: degrees, the triangle product); the last two are all-pairs searches and stay networkx's,
    for a connected graph only.  A graph the device does not cover (fewer than 2 or more than max_dim nodes, self-loops, directed or
    parallel edges) is networkx's as a whole."""
    import networkx as nx
    import pandas as pd

    D = G.number_of_nodes()
    if D < 2 or D > _lib.get_lib().max_dim or G.is_directed() or G.is_multigraph() or nx.number_of_selfloops(G):
        row = {"num_nodes": D, "num_edges": G.number_of_edges(), "avg_degree": sum(dict(G.degree()).values()) / D if D > 0 else 0,
               "density": nx.density(G), "avg_clustering": nx.average_clustering(G), "transitivity": nx.transitivity(G)}
    else:
        A = nx.to_numpy_array(G, dtype=np.float32, weight=None)
        row = _recovered_graphs(A[None], False, None, 0.5, True)[0].stats
    connected = nx.is_connected(G)
    row["diameter"] = nx.diameter(G) if connected else None
    row["avg_shortest_path"] = nx.average_shortest_path_length(G) if connected else None
    return pd.DataFrame([{key: row[key] for key in GRAPH_STAT_KEYS}])


# Smallest D > max_eig_dim that goes to uglad_conditional_mean_wide; below it (and above max_eig_dim) the host formulation would run.  0: the
# whole range goes to the device.  scripts/after_wide_probe.py times both sides; a range where the host wins end to end belongs here.
WIDE_CONDITIONAL_MIN_DIM = 0


def conditional_gaussian_batch(precision, mean, observed_mask, observed_values, clip01: bool = False, want_cov: bool = True):
    """K conditional-Gaussian problems on the device: precision (K,D,D), mean (K,D), observed_mask (K,D) bool, observed_values (K,D)
    (read where observed) -> full_mean (K,D), cond_cov (K,D,D) (L_uu^-1 on the unobserved block, identity elsewhere), log_pdf (K) --
    fp32 torch tensors on the device.  D <= max_eig_dim: uglad_conditional_mean (the path's eigensolver, fp32); beyond, up to max_dim:
    uglad_conditional_mean_wide (fp64 Cholesky, many workgroups per problem; `want_cov=False` skips the inverse and returns None for it)."""
    full, cov, logp = _conditional_gaussian_device(precision, mean, observed_mask, observed_values, clip01, want_cov)
    return full.to(torch.float32), cov, logp.to(torch.float32)


def _conditional_gaussian_device(precision, mean, observed_mask, observed_values, clip01, want_cov):
    """conditional_gaussian_batch in the precision the entry point computes in: full_mean and log_pdf are fp64 beyond max_eig_dim."""
    dev = _lib.device()
    lib = _lib.get_lib()

    def to(a, dtype):
        # a host array is converted on the host and uploaded once; a device tensor is converted on the device
        if torch.is_tensor(a):
            return a.detach().to(device=dev, dtype=dtype).contiguous()
        return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev).contiguous()

    D = np.shape(precision)[-1]
    if D <= lib.max_eig_dim:
        f = lambda a: to(a, torch.float32)  # noqa: E731
        return lib.conditional_mean(f(precision), f(mean), f(observed_mask), f(observed_values), clip01=clip01)
    if D > lib.max_dim or D < WIDE_CONDITIONAL_MIN_DIM:
        return _conditional_gaussian_host(precision, mean, observed_mask, observed_values, clip01, dev)
    f = lambda a: to(a, torch.float64)  # noqa: E731
    return lib.conditional_mean_wide(f(precision), f(mean), to(observed_mask, torch.float32), f(observed_values), clip01=clip01,
                                     want_cov=want_cov)


def _conditional_gaussian_host(precision, mean, observed_mask, observed_values, clip01, dev):
    """D beyond what the device covers (uglad_conditional_mean_wide, D <= max_dim = 2048): the reference's own formulation on the host in
    float64 (ref main.py:1176-1227: mean_u - L_uu^-1 L_uo (x_o - mean_o), conditional covariance L_uu^-1, the density at the MAP point), returned
    in the layout of the device entry point (full mean; L_uu^-1 on the unobserved block, identity elsewhere; log density)."""
    to64 = lambda a: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np.float64)  # noqa: E731
    P, mu, mask, vals = to64(precision), to64(mean), to64(observed_mask) != 0, to64(observed_values)
    K, D = mu.shape
    full, cov, logp = np.empty((K, D)), np.empty((K, D, D)), np.empty(K)
    for k in range(K):
        o, u = np.where(mask[k])[0], np.where(~mask[k])[0]
        Luu_inv = np.linalg.inv(P[k][np.ix_(u, u)]) if u.size else np.zeros((0, 0))
        m = mu[k].copy()
        m[o] = vals[k][o]
        if u.size:
            m[u] = mu[k][u] - Luu_inv @ (P[k][np.ix_(u, o)] @ (vals[k][o] - mu[k][o]))
        if clip01:
            m = np.clip(m, 0.0, 1.0)
        full[k] = m
        cov[k] = np.eye(D)
        cov[k][np.ix_(u, u)] = Luu_inv
        # density of the conditional Gaussian at its own mean: (2 pi)^(-n_u / 2) det(L_uu)^(1/2)
        sign, ld = np.linalg.slogdet(P[k][np.ix_(u, u)]) if u.size else (1.0, 0.0)
        logp[k] = -0.5 * u.size * np.log(2.0 * np.pi) + 0.5 * ld if sign > 0 else np.nan
    t = lambda a: torch.as_tensor(a, dtype=torch.float32).to(dev)  # noqa: E731
    return t(full), t(cov), t(logp)


def conditional_gaussian_with_probabilities(precision, mean, observed_idx, observed_values):
    """Conditional mean, conditional covariance and density at the MAP point of a Gaussian given observed coordinates
    (ref main.py:1176-1227, same arguments and return values): (full_mean (n,), conditional_cov (n_u, n_u), pdf).
    The reference solves with scipy on the host; here the path's eigensolver does it on the device (fp32), and beyond its size the fp64
    Cholesky of uglad_conditional_mean_wide: the density is the exponential of its fp64 logarithm."""
    precision = np.asarray(precision)
    mean = np.asarray(mean, dtype=np.float64)
    n = len(mean)
    observed_idx = [int(i) for i in observed_idx]
    mask = np.zeros(n, dtype=np.float32)
    mask[observed_idx] = 1.0
    vals = np.zeros(n, dtype=np.float64)
    vals[observed_idx] = np.asarray(observed_values, dtype=np.float64)
    full, cov, logp = _conditional_gaussian_device(precision[None], mean[None], mask[None], vals[None], False, True)
    unobs = [i for i in range(n) if mask[i] == 0.0]
    cov = cov[0].cpu().numpy().astype(np.float64)
    return full[0].cpu().numpy().astype(np.float64), cov[np.ix_(unobs, unobs)], float(np.exp(np.float64(logp[0].item())))


def compute_map_estimate(observed_nodes: dict, model_uGLAD) -> np.ndarray:
    """MAP estimate of all nodes given some observed ones, clamped to [0, 1] (ref main.py:1229-1260): uses the estimator's
    precision_, location_ and node_names_."""
    names = list(model_uGLAD.node_names_)
    idx = [names.index(k) for k in observed_nodes.keys()]
    n = len(names)
    mask = np.zeros(n, dtype=np.float32)
    mask[idx] = 1.0
    vals = np.zeros(n, dtype=np.float64)
    vals[idx] = list(observed_nodes.values())
    full, _, _ = conditional_gaussian_batch(np.asarray(model_uGLAD.precision_)[None], np.asarray(model_uGLAD.location_)[None],
                                            mask[None], vals[None], clip01=True, want_cov=False)
    return full[0].cpu().numpy().astype(np.float64)


def save_uGLAD_model(obj, filepath: str) -> None:
    """Pickle the estimator's attributes to `filepath` and the 42 parameters (state_dict) to `filepath + "_model.pt"` -- the
    file layout of the reference (main.py:1132-1149)."""
    import pickle

    d = obj.__dict__.copy()
    has_model = d.get("model_glad") is not None
    if has_model:
        torch.save({k: v.detach().cpu() for k, v in obj.model_glad.state_dict().items()}, filepath + "_model.pt")
    d["model_glad"] = None
    d["_has_model"] = has_model  # (the reference tests the pickled None here and therefore never restores its model)
    with open(filepath, "wb") as f:
        pickle.dump(d, f)


def load_uGLAD_model(filepath: str):
    """Inverse of save_uGLAD_model (ref main.py:1152-1173, with its restore actually taking place): the estimator comes back
    with a GladParams on the current device, ready for predict()."""
    import pickle

    with open(filepath, "rb") as f:
        d = pickle.load(f)
    has_model = d.pop("_has_model", False)
    obj = uGLAD_multitask() if isinstance(d.get("covariance_"), list) or np.ndim(d.get("precision_")) == 3 else uGLAD_GL()
    obj.__dict__.update(d)
    if has_model:
        model = GladParams(1.0, device=_lib.device())
        model.load_state_dict(torch.load(filepath + "_model.pt", map_location="cpu"))
        obj.model_glad = model
    return obj
