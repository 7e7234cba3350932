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

How a table becomes the input matrix lives in `inputs.py`, everything after the path (the reference's main.py:796-1300) in `after.py`;
their public names are imported here, so `uglad_amd.main.X` resolves as it does in the reference.
"""
from __future__ import annotations

import copy
from time import time
from typing import Optional

import numpy as np
import torch

from . import _lib
from .after import (  # noqa: F401  (everything after the path: uglad_amd/after.py)
    GRAPH_STAT_KEYS, METRIC_KEYS, RecoveredGraph, SampleScores, _to_model_coordinates, compute_graph_statistics, compute_map_estimate,
    conditional_gaussian_batch, conditional_gaussian_with_probabilities, device_report_metrics, edge_frequency, get_partial_correlations,
    graph_from_partial_correlations, recovered_graph, sample_scores)
from .dist import Collective, get_collective
from .glad import glad
from .glad.glad_params import GladParams
from .inputs import (  # noqa: F401  (how a table becomes the input matrix: uglad_amd/inputs.py)
    _covariance, _rank_tables, _stacked_tables, _to_dev, device_covariance, mixed_association, pairwise_covariance, pairwise_flag_message,
    rank_correlation, weight_flag_message, weighted_covariance)
from .utils import prepare_data
from .utils.metrics import report_metrics_all  # noqa: F401  (host-side API parity; the drivers count on the device)


# ============================================================================================ loss
def _loss_forward(theta: torch.Tensor, S: torch.Tensor, struct: Optional[torch.Tensor]):
    """uglad_loss_fwd on contiguous theta (M, D, D): (the M terms -logdet Theta_b + tr(S_b Theta_b) [+ penalty], Theta^-1)."""
    lib = _lib.get_lib()
    M, D, _ = theta.shape
    partial = torch.empty(M, dtype=torch.float32, device=theta.device)
    theta_inv = torch.empty_like(theta)
    wsp = lib.workspace(M, D, theta)
    lib.loss_fwd(theta, S, struct, partial, theta_inv, wsp)
    return partial, theta_inv


class _GlassoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, theta, S, struct, divisor):
        f32 = dict(dtype=torch.float32, device=theta.device)
        theta = theta.contiguous()
        partial, theta_inv = _loss_forward(theta, S, struct)
        total = torch.empty(1, **f32)
        _lib.get_lib().sum_partials(partial, total)
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
    theta = theta.detach().contiguous()
    return _loss_forward(theta, S.detach().to(device=theta.device, dtype=torch.float32).contiguous(), None)[0]


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


def _print_every(EPOCHS: int) -> int:
    return max(1, int(EPOCHS / 10))


def _allreduce_grads(model, loss, coll: Collective):
    """Exchange (ii): SUM of the 42 gradients and of the loss over ranks, in one 43-float message."""
    if coll.world_size == 1:
        return loss.detach()
    flat = torch.cat([p.grad.reshape(-1) for p in model.parameters()] + [loss.detach().reshape(1)])
    coll.all_reduce_sum(flat)
    model.load_packed_(flat, grads=True)
    return flat[-1]


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
    pending = None  # (epoch, event, pinned flag, predTheta of that epoch, snapshot taken before that epoch's step)

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
            # (the snapshot is one launch: the 42 parameters packed; the optimiser is not returned, its state needs no rescue)
            pending = (e, ev, flag, predTheta_e, model_glad.packed().detach())
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
        model_glad.load_packed_(stopped[4])
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
    best_loss = torch.full((), float("inf"), dtype=torch.float32, device=Sb_train.device)
    best_state = model_glad.packed().detach()  # the 42 parameters, packed
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
            best_state = torch.where(improved, model_glad.packed(), best_state)
        if not e % PRINT_EVERY and VERBOSE:
            print(f"Fold {_k}: epoch:{e}/{EPOCHS} test-loss:{float(loss_test.item())}")
    best = float(best_loss.item())
    best_model = None
    if best < np.inf:
        best_model = copy.deepcopy(model_glad)
        best_model.load_packed_(best_state)
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
            model.load_packed_(best_P[i])
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


def _check_shardable(K: int, coll: Collective, what: str) -> None:
    """Every rank must own at least one matrix: an empty shard would fail locally while the other ranks wait in the first
    collective.  K and world_size are known everywhere, so every rank raises the same error before any exchange."""
    if K < coll.world_size:
        raise ValueError(f"{K} {what} cannot be sharded over {coll.world_size} ranks (need at least one per rank)")


def _broadcast_model(model, coll: Collective):
    """Replicate rank 0's freshly initialised 42 parameters (each rank draws its own otherwise)."""
    if coll.world_size == 1:
        return
    flat = model.packed().detach()
    if coll.rank != 0:
        flat.zero_()
    coll.all_reduce_sum(flat)
    model.load_packed_(flat)


def _train_sharded(Sb, coll: Collective, global_batch: int, EPOCHS, lr, INIT_DIAG, L, VERBOSE, sqrt_mode, loss_Sb=None):
    """The epoch loop of the missing-data and multi-task modes (ref main.py:600-630, 755-778): ONE model, rank 0's draw, trained on this
    rank's shard Sb of a batch of `global_batch` matrices; per epoch the pass, the backward, exchange (ii) and the step.  The loss is
    taken on Sb, or against `loss_Sb`.  Returns (predTheta of the last epoch, model)."""
    model_glad, optimizer_glad = init_uGLAD(lr=lr, theta_init_offset=1.0, nF=3, H=3)
    _broadcast_model(model_glad, coll)
    PRINT_EVERY = _print_every(EPOCHS)
    predTheta = None
    for e in range(EPOCHS):
        optimizer_glad.zero_grad()
        predTheta, loss = forward_uGLAD(Sb, model_glad, L=L, INIT_DIAG=INIT_DIAG, loss_Sb=loss_Sb, sqrt_mode=sqrt_mode,
                                        collective=coll, global_batch=global_batch)
        loss.backward()
        total = _allreduce_grads(model_glad, loss, coll)
        optimizer_glad.step()
        if not e % PRINT_EVERY and VERBOSE:
            print(f"epoch:{e}/{EPOCHS} loss:{float(total)}")
    return predTheta, model_glad


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
    predTheta, model_glad = _train_sharded(S_K, coll, K_batch, EPOCHS, lr, INIT_DIAG, L, VERBOSE, sqrt_mode, loss_Sb=Sb)
    predTheta = get_final_precision_from_batch(predTheta, type="min", collective=coll)
    compare_theta = None
    if trueTheta is not None:
        compare_theta = device_report_metrics(trueTheta[:1], predTheta[:1])[0]
        if VERBOSE:
            print(f"Comparison - {compare_theta}")
    return predTheta, compare_theta, model_glad


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
    predTheta, model_glad = _train_sharded(Sb, coll, K, EPOCHS, lr, INIT_DIAG, L, VERBOSE, sqrt_mode)
    predTheta = coll.all_gather_cat(predTheta.detach())
    compare_theta = []
    if trueTheta is not None:
        compare_theta = device_report_metrics(np.asarray(trueTheta), predTheta)  # all K graphs in one launch
        if VERBOSE:
            for b, rM in enumerate(compare_theta):
                print(f"Metrics for graph {b}: {rM}\n")
    return predTheta, compare_theta, model_glad


# ============================================================================================ public classes
class _Estimator(object):
    """What the two estimators share: their attributes, the end of a fit, the no_grad pass behind predict(), recovered_graph()."""

    def __init__(self, device_covariance: bool = False):
        """device_covariance (additive): form the input covariances + eigenvalue repair on the GPU."""
        super().__init__()
        self.device_covariance = bool(device_covariance)
        self.covariance_: Optional[np.ndarray] = None
        self.precision_: Optional[np.ndarray] = None
        self.location_: Optional[np.ndarray] = None    # (uGLAD_multitask: (K, D), the tasks' means)
        self.data_min_: Optional[np.ndarray] = None    # (additive) column minima and ranges of the table(s) fit() normalised: what
        self.data_range_: Optional[np.ndarray] = None  # places a new row in the model's coordinates (mahalanobis, score_samples, score)
        self.model_glad: Optional[GladParams] = None
        self._fit_cfg = None

    def _finish_fit(self, start, verbose, precision, model_glad, cond_max, compare_theta, **cfg):
        """The end of every fit: precision_ (a device tensor or None), model_glad, what predict() needs of the fit's arguments (`cfg`),
        cond_max_ -- the regime diagnostic (additive): the largest cond(b^T b + 4/lambda I) any pass of this fit saw, from
        warn_if_outside, which the caller runs so that the warning points at the caller's caller -- and the runtime line."""
        if precision is not None:
            self.precision_ = precision.detach().cpu().numpy()
        if model_glad is not None:
            self.model_glad = model_glad
        self._fit_cfg = cfg
        self.cond_max_ = cond_max
        if verbose:
            print(f"Total runtime: {time() - start} secs\n")
        return compare_theta

    def _forward(self, tables, S):
        """The no_grad pass behind predict(): the trained model over the covariances S ((D, D) or (K, D, D)), or over those of the
        `tables`, processed like fit() processes its own -> (Theta (K, D, D) as a numpy array, the pass's regime monitor)."""
        if self.model_glad is None:
            raise ValueError("call fit() first")
        cfg = self._fit_cfg
        if S is None:
            tables = [np.array(prepare_data.process_table(X, NORM="min_max", VERBOSE=False)) for X in tables]
            S = prepare_data.get_covariance(tables, offset=cfg["eval_offset"])
        S = np.asarray(S, dtype=np.float64)
        with torch.no_grad(), glad.regime_monitor() as regime:
            theta = glad.glad(_to_dev(S[None] if S.ndim == 2 else S), self.model_glad, L=cfg["L"], INIT_DIAG=cfg["INIT_DIAG"],
                              sqrt_mode=cfg["sqrt_mode"], collective=Collective())
        return theta.cpu().numpy(), regime

    def recovered_graph(self, sparsity: float = 0.1):
        """The graph(s) of the fitted precision_ (recovered_graph): the `sparsity` fraction of the edges with the largest |rho|."""
        if self.precision_ is None:
            raise ValueError("call fit() first")
        return recovered_graph(self.precision_, sparsity=sparsity)


class uGLAD_GL(_Estimator):
    """Drop-in for the reference's `uGLAD_GL` (main.py:34-151): `fit` sets covariance_ (float64), precision_ (float32),
    location_, node_names_, model_glad and returns the metrics dict (or None) -- not self, like the reference."""

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
        cond_max = regime.warn_if_outside("uGLAD_GL.fit", get_collective() if mode == "missing" else None)  # (the sharded mode)
        return self._finish_fit(start, verbose, None if pred_theta is None else pred_theta[0], model_glad, cond_max, compare_theta,
                                L=L, INIT_DIAG=INIT_DIAG, eval_offset=eval_offset, sqrt_mode=sqrt_mode)

    @staticmethod
    def _train_direct_on(A, true_theta, eval_offset, epochs, lr, INIT_DIAG, L, verbose, sqrt_mode):
        """Direct-mode training on the (1, D, D) device matrix A that takes the covariance's place (fit_mixed, fit_copula):
        run_uGLAD_direct's three results and the regime monitor of its passes."""
        D = A.shape[-1]
        true_theta_b = None if true_theta is None else np.asarray(true_theta).reshape(1, D, D)
        with glad.regime_monitor() as regime:
            pred_theta, compare_theta, model_glad = run_uGLAD_direct(None, trueTheta=true_theta_b, eval_offset=eval_offset, EPOCHS=epochs,
                                                                     lr=lr, INIT_DIAG=INIT_DIAG, L=L, VERBOSE=verbose,
                                                                     sqrt_mode=sqrt_mode, Sb=A)
        return pred_theta, compare_theta, model_glad, regime

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
        A, mn, A64 = _lib.get_lib().association(torch.from_numpy(table[None]).to(_lib.device()), maps, eval_offset=eval_offset,
                                                repair=True, want_f64=True)
        pred_theta, compare_theta, model_glad, regime = self._train_direct_on(A, true_theta, eval_offset, epochs, lr, INIT_DIAG, L,
                                                                              verbose, sqrt_mode)
        self.covariance_ = A64[0].cpu().numpy()
        self.association_min_eig_ = float(mn[0])
        self.location_ = np.where(maps.kinds == "r", table.mean(axis=0), np.nan)
        self.data_min_ = self.data_range_ = None  # (a mixed table is not normalised, and its rows cannot be scored)
        self.node_names_ = [str(n) for n in maps.names]
        cond_max = regime.warn_if_outside("uGLAD_GL.fit_mixed", None)
        return self._finish_fit(start, verbose, None if pred_theta is None else pred_theta[0], model_glad, cond_max, compare_theta,
                                L=L, INIT_DIAG=INIT_DIAG, eval_offset=eval_offset, sqrt_mode=sqrt_mode)

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
        pred_theta, compare_theta, model_glad, regime = self._train_direct_on(out.A, true_theta, eval_offset, epochs, lr, INIT_DIAG, L,
                                                                              verbose, sqrt_mode)
        self.covariance_ = out.A64[0].cpu().numpy()
        self.copula_min_eig_ = float(out.min_eig[0])
        self.location_ = tables[0].mean(axis=0)
        self.data_min_ = self.data_range_ = None  # (rows of a copula fit are not scored)
        self.node_names_ = names
        cond_max = regime.warn_if_outside("uGLAD_GL.fit_copula", None)
        return self._finish_fit(start, verbose, None if pred_theta is None else pred_theta[0], model_glad, cond_max, compare_theta,
                                L=L, INIT_DIAG=INIT_DIAG, eval_offset=eval_offset, sqrt_mode=sqrt_mode)

    def fit_pairwise(self, X, true_theta=None, eval_offset=0.1, epochs=250, lr=0.002, INIT_DIAG=0, L=15, verbose=True, sqrt_mode=None,
                     min_pairs=2, k_fold=0):
        """`fit` for a table with missing entries (NaN) without imputing them (additive; `fit` fills every NaN with the column mean, as
        the reference does, which shrinks every covariance): the table is min-max normalised over its observed entries and its
        available-case (pairwise-complete) covariance -- entry (i, j) over the rows where both columns are observed -- is formed and
        repaired on the device (uglad_pairwise_covariance, pairwise_covariance); training runs on that matrix.  X is an (N, D) array or
        DataFrame; no row or column is dropped.  k_fold = 0: direct mode.  k_fold >= 2: the reference's missing-mode ensemble
        (run_uGLAD_missing) on pairwise matrices -- the k_fold row folds of the table with its NaN kept, one matrix each (one device call
        per group of folds of one shape), one shared model trained on that batch with the loss against the full table's matrix, the
        consensus get_final_precision_from_batch(type="min") at the end; on one device only.  A column that is never observed, constant,
        infinite, or observed together with another in fewer than `min_pairs` rows -- in the table or in a fold -- raises ValueError.
        Sets covariance_ (the UNREPAIRED matrix, float64), precision_, location_ (the observed means in the model's coordinates),
        data_min_ / data_range_ (of the observed entries: mahalanobis / score_samples work afterwards, NaN for a row that holds a NaN),
        node_names_, model_glad, cond_max_, pairwise_min_eig_ and pairwise_counts_ ((D, D) int: the rows behind every entry);
        predict(S=...), recovered_graph() and save / load work afterwards."""
        start = time()
        if verbose:
            print("Running uGLAD on a pairwise-complete covariance")
        tables, single, names = _stacked_tables(X, "fit_pairwise")
        if not single:
            raise ValueError("fit_pairwise takes one (N, D) table")
        if k_fold != 0 and get_collective().world_size > 1:
            raise ValueError("fit_pairwise(k_fold=...) is not sharded over ranks: run it in one process")
        table = tables[0]
        N, D = table.shape
        names = names if names is not None else [f"node_{i}" for i in range(D)]
        lib = _lib.get_lib()

        def matrices(group, what):
            out = lib.pairwise_covariance(torch.from_numpy(np.ascontiguousarray(group)).to(_lib.device()), normalize=True,
                                          min_pairs=min_pairs, eval_offset=eval_offset, repair=True, want_f64=True, want_counts=True)
            for k, info in enumerate(out.info.cpu().numpy()):
                if info.any():
                    raise ValueError(f"fit_pairwise: {what(k)} has no pairwise-complete covariance: {pairwise_flag_message(info, names)}")
            return out

        full = matrices(tables, lambda k: "the table")
        if k_fold == 0:
            pred_theta, compare_theta, model_glad, regime = self._train_direct_on(full.S, true_theta, eval_offset, epochs, lr, INIT_DIAG, L,
                                                                                  verbose, sqrt_mode)
        else:
            folds = [table[train] for train, _ in _kfold_indices(N, k_fold)]
            groups = {}
            for i, fold in enumerate(folds):
                groups.setdefault(fold.shape, []).append(i)
            S_K = torch.empty(k_fold, D, D, dtype=torch.float32, device=_lib.device())
            for idx in groups.values():
                S_K[idx] = matrices(np.stack([folds[i] for i in idx]), lambda k: f"fold {idx[k]}").S
            one = Collective()
            with glad.regime_monitor() as regime:
                pred_theta, model_glad = _train_sharded(S_K, one, k_fold, epochs, lr, INIT_DIAG, L, verbose, sqrt_mode, loss_Sb=full.S)
                pred_theta = get_final_precision_from_batch(pred_theta, type="min", collective=one)
            compare_theta = None
            if true_theta is not None:
                compare_theta = device_report_metrics(_to_dev(np.asarray(true_theta).reshape(1, D, D)), pred_theta[:1])[0]
                if verbose:
                    print(f"Comparison - {compare_theta}")
        mn, scale = prepare_data.observed_min_scale(table)
        self.covariance_ = full.S64[0].cpu().numpy()
        self.pairwise_min_eig_ = float(full.min_eig[0])
        self.pairwise_counts_ = full.counts[0].cpu().numpy()
        self.location_ = np.nanmean((table - mn) * scale, axis=0)
        self.data_min_, self.data_range_ = mn, np.nanmax(table, axis=0) - mn
        self.node_names_ = names
        cond_max = regime.warn_if_outside("uGLAD_GL.fit_pairwise", None)
        return self._finish_fit(start, verbose, None if pred_theta is None else pred_theta[0], model_glad, cond_max, compare_theta,
                                L=L, INIT_DIAG=INIT_DIAG, eval_offset=eval_offset, sqrt_mode=sqrt_mode)

    def fit_stability(self, X, n_resamples=50, scheme="subsample", fraction=0.5, sparsity=0.1, seed=0, true_theta=None, eval_offset=0.1,
                      epochs=250, lr=0.002, INIT_DIAG=0, L=15, verbose=True, node_names=None, sqrt_mode=None):
        """`fit` with a measure of how far to trust every edge (additive; the reference ends in one graph: the selection frequencies of
        stability selection and the instability of StARS, as R's huge offers them): the table is processed and normalised as `fit` does,
        `n_resamples` weightings of its rows are drawn (prepare_data.resample_weights: `scheme` "subsample" with `fraction` of the rows,
        or "bootstrap"; seeded by `seed`), the all-ones weighting is placed in front, and ONE device call forms and repairs the R + 1
        covariances from one upload of the table (uglad_weighted_covariance).  One shared model is trained on that batch, every matrix
        with the loss against itself as in multitask mode; on one device only.  Sets precision_ (the all-ones member: the full table's),
        precision_resamples_ (R, D, D), edge_frequency_ / edge_sign_frequency_ ((D, D) float64: the fraction of the resamples whose
        graph at `sparsity` holds the edge, and holds it with a positive partial correlation; uglad_edge_frequency), instability_
        (StARS: the mean over the edges of 2 f (1 - f)), resample_weights_ (R, N), resample_min_eig_ (R,), and covariance_, location_,
        data_min_ / data_range_, node_names_, model_glad and cond_max_ as `fit` does; stable_edges(), predict, recovered_graph(),
        scoring and save / load work afterwards."""
        start = time()
        if verbose:
            print("Running uGLAD on resamples of the table")
        if get_collective().world_size > 1:
            raise ValueError("fit_stability is not sharded over ranks: run it in one process")
        processed = prepare_data.process_table(X, NORM="min_max", VERBOSE=verbose)
        data_min, data_range = prepare_data.kept_min_range(X, processed)
        X = np.array(processed, dtype=np.float64)
        N, D = X.shape
        if not np.isfinite(X).all():
            raise ValueError("fit_stability: the processed table holds NaN or infinity")
        R = int(n_resamples)
        weights = prepare_data.resample_weights(N, R, scheme=scheme, fraction=fraction, rng=seed)
        out = _lib.get_lib().weighted_covariance(_to_dev(X, torch.float64), _to_dev(np.vstack([np.ones((1, N)), weights]), torch.float64),
                                                 eval_offset=eval_offset, repair=True)
        for r, flag in enumerate(out.info.cpu().numpy()):
            if flag:
                raise ValueError(f"fit_stability: weighting {r} has no covariance: {weight_flag_message(flag)}")
        one = Collective()
        with glad.regime_monitor() as regime:
            pred_theta, model_glad = _train_sharded(out.S, one, R + 1, epochs, lr, INIT_DIAG, L, verbose, sqrt_mode)
        pred_theta = pred_theta.detach()
        compare_theta = None
        if true_theta is not None:
            compare_theta = device_report_metrics(_to_dev(np.asarray(true_theta).reshape(1, D, D)), pred_theta[:1])[0]
            if verbose:
                print(f"Comparison - {compare_theta}")
        self.edge_frequency_, self.edge_sign_frequency_, self.instability_ = edge_frequency(pred_theta[1:].contiguous(), sparsity=sparsity)
        self.precision_resamples_ = pred_theta[1:].cpu().numpy()
        self.resample_weights_ = weights
        self.resample_min_eig_ = out.min_eig[1:].cpu().numpy()
        self.covariance_ = prepare_data.empirical_covariance(X)
        self.location_ = X.mean(axis=0)
        self.data_min_, self.data_range_ = data_min, data_range
        self.node_names_ = list(node_names) if node_names is not None else [f"node_{i}" for i in range(D)]
        cond_max = regime.warn_if_outside("uGLAD_GL.fit_stability", None)
        return self._finish_fit(start, verbose, pred_theta[0], model_glad, cond_max, compare_theta,
                                L=L, INIT_DIAG=INIT_DIAG, eval_offset=eval_offset, sqrt_mode=sqrt_mode)

    def stable_edges(self, threshold: float = 0.8):
        """The edges fit_stability saw in at least `threshold` of its resamples (and in one at least): a list of (i, j, frequency), i < j,
        by frequency descending and then by index."""
        if getattr(self, "edge_frequency_", None) is None:
            raise ValueError("call fit_stability() first")
        f = self.edge_frequency_
        i, j = np.triu_indices(f.shape[0], 1)
        keep = (f[i, j] >= threshold) & (f[i, j] > 0)
        rows = sorted(zip((-f[i, j][keep]).tolist(), i[keep].tolist(), j[keep].tolist()))
        return [(a, b, -nf) for nf, a, b in rows]

    def predict(self, X=None, S=None) -> np.ndarray:
        """Inference-only pass: the trained 42 parameters applied to new data (no_grad forward, the reference's
        main.py:539-540 pattern).  Give a samples table X (processed like `fit` does) or covariance(s) S.
        Warns (UgladRegimeWarning) when the pass leaves the validated regime -- e.g. an un-normalised covariance given as S."""
        out, regime = self._forward([X], S)
        self.predict_cond_max_ = regime.warn_if_outside("uGLAD_GL.predict")
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


class uGLAD_multitask(_Estimator):
    """Drop-in for the reference's `uGLAD_multitask` (main.py:155-226): K tables, one shared model, batched attributes."""

    def __init__(self, device_covariance: bool = False):
        super().__init__(device_covariance)
        self.covariance_ = []  # (load_uGLAD_model tells the two classes apart by this)

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
        self.location_ = np.array([X.mean(axis=0) for X in Xb])
        self.data_min_, self.data_range_ = np.array([m for m, _ in min_range]), np.array([r for _, r in min_range])
        cond_max = regime.warn_if_outside("uGLAD_multitask.fit", get_collective())
        return self._finish_fit(start, verbose, pred_theta, model_glad, cond_max, compare_theta,
                                L=L, INIT_DIAG=INIT_DIAG, eval_offset=eval_offset, sqrt_mode=sqrt_mode)

    def predict(self, Xb=None, S=None) -> np.ndarray:
        """no_grad forward of the trained model on new tables (list) or covariances (K, D, D)."""
        out, regime = self._forward(Xb, S)
        self.predict_cond_max_ = regime.warn_if_outside("uGLAD_multitask.predict")
        return out


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
