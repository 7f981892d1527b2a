"""
Optimal-permutation (Hungarian) training on MI355X: Dovrat, Nachmani and Wolf, "Many-Speakers Single Channel Speech Separation with Optimal
Permutation Training", 2021.  The reference's src/criterion/hungarian.py is a stub whose HungarianLoss.forward raises NotImplementedError; the API
here mirrors `pit` / `PIT` of criterion/pit.py: `criterion(input, target, batch_mean) -> (loss, pattern)` with `pattern` (B, n) int64 such that
`criterion(input, target[:, pattern])` is the optimum -- the minimum of the criterion, or its maximum if `criterion.maximize`.

PIT walks a table of all n! permutations: 3.6 M rows at n = 10, impossible at n = 20.  For a criterion that is additive over the sources the
best permutation is a linear assignment problem on the n x n matrix of pair values, solved exactly in O(n^3) by shortest augmenting paths
(sep_assign).  Among several optimal permutations any one may be returned -- the same one for the same input every time; it is not PIT's "first
in itertools order".

With SI-SDR, SDR or the thresholded SNR (criterion.sdr) on fp32 (B, n, T) estimates and n <= 64 everything runs on three kernels: sep_pair_gram
makes one pass over the 2 n waveforms into the inner products behind every pair measure, sep_pair_assign forms the measures and solves the
assignment, sep_pair_bwd applies the analytic gradient of the chosen pairs.  Every other case -- other additive criteria, the clipped
subclasses, 4-D inputs, CPU tensors beside the HIP library, n > 64 -- takes the composed route: the pair matrix from the criterion itself on
single-source rows (no tape, a bounded block at a time), the assignment on it, the criterion once more with the tape on the chosen permutation.
"""
import numpy as np
import torch
import torch.nn as nn

import sepkernels
from criterion.sdr import SISDR, NegSISDR, SDR, NegSDR, ThresholdedSNR, NegThresholdedSNR

_KINDS = {SISDR: (0, 1.0), NegSISDR: (0, -1.0), SDR: (1, 1.0), NegSDR: (1, -1.0), ThresholdedSNR: (2, 1.0), NegThresholdedSNR: (2, -1.0)}
_MAX_ROWS = 65535          # the kernels put the batch on a 16-bit grid dimension: larger batches go through in slices
_BLOCK_ELEMS = 1 << 25     # composed route: elements of the single-source rows formed at a time


def _kernel_route(criterion, input, target):
    if type(criterion) not in _KINDS or criterion.reduction not in ("mean", "sum"):
        return False
    if input.dim() != 3 or target.dim() != 3 or input.dtype != torch.float32:
        return False
    if sepkernels.backend().name == "hip" and not input.is_cuda:
        return False
    return 1 <= input.shape[1] <= sepkernels.ASSIGN_MAX_N


class _HungarianFn(torch.autograd.Function):
    """est, tgt (B, n, T) -> (best (B,), perm (B, n) int64, per_src (B, n)): the best reduced measure (in dB, not negated), the target of every
    estimate and the measure of every estimate against it"""

    @staticmethod
    def forward(ctx, est, tgt, kind, maximize, use_mean, eps, tau):
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("gradient w.r.t. the target of the Hungarian loss is not implemented")
        K = sepkernels.backend()
        est, tgt = est.contiguous(), tgt.contiguous()
        B, n, T = est.shape
        dev = est.device
        dots = torch.empty(B, n, n, device=dev, dtype=torch.float64)
        tt = torch.empty(B, n, device=dev, dtype=torch.float64)
        xx = torch.empty(B, n, device=dev, dtype=torch.float64)
        best = torch.empty(B, device=dev, dtype=torch.float32)
        perm = torch.empty(B, n, device=dev, dtype=torch.int64)
        per_src = torch.empty(B, n, device=dev, dtype=torch.float32)
        scratch = torch.empty(max(1, K.pair_gram_scratch_bytes(min(B, _MAX_ROWS), n, T) // 8), device=dev, dtype=torch.float64)
        for b0 in range(0, B, _MAX_ROWS):
            b1 = min(B, b0 + _MAX_ROWS)
            K.pair_gram(est[b0:b1], tgt[b0:b1], dots[b0:b1], tt[b0:b1], xx[b0:b1], scratch, b1 - b0, n, T)
            K.pair_assign(dots[b0:b1], tt[b0:b1], xx[b0:b1], b1 - b0, n, kind, maximize, use_mean, eps, tau, best[b0:b1], perm[b0:b1], per_src[b0:b1], None)
        ctx.save_for_backward(est, tgt, dots, tt, xx, perm)
        ctx.meta = (kind, use_mean, eps, tau)
        ctx.mark_non_differentiable(perm, per_src)
        return best, perm, per_src

    @staticmethod
    def backward(ctx, gbest, _gperm, _gper):
        K = sepkernels.backend()
        est, tgt, dots, tt, xx, perm = ctx.saved_tensors
        kind, use_mean, eps, tau = ctx.meta
        B, n, T = est.shape
        gw = (gbest / n if use_mean else gbest).to(torch.float32).contiguous()      # what arrives at every per-source measure
        d_est = torch.empty_like(est)
        for b0 in range(0, B, _MAX_ROWS):
            b1 = min(B, b0 + _MAX_ROWS)
            K.pair_bwd(est[b0:b1], tgt[b0:b1], dots[b0:b1], tt[b0:b1], xx[b0:b1], perm[b0:b1], gw[b0:b1], d_est[b0:b1], b1 - b0, n, T, kind, eps, tau)
        return d_est, None, None, None, None, None, None


def _fused_hungarian(criterion, input, target, batch_mean):
    kind, sign = _KINDS[type(criterion)]
    # the kernels score the measure itself: minimising its negative and maximising it pick the same permutation
    maximize = bool(criterion.maximize) == (sign > 0)
    tau = float(criterion.tau) if kind == 2 else 0.0
    best, perm, _ = _HungarianFn.apply(input, target.to(input.dtype), kind, maximize, criterion.reduction == "mean", float(criterion.eps), tau)
    loss = best if sign > 0 else -best
    if batch_mean:
        loss = loss.mean(dim=0)
    return loss, perm


def _solve_host(cost):
    """(B, n, n) fp64 on the host -> (B, n) int64: the minimum-cost perfect matching of every item by shortest augmenting paths with potentials
    (Jonker-Volgenant), the algorithm of sep_assign with the column scan as one numpy expression.  Bounded loops only: a cost that does not
    compare (NaN) is offered as +inf and the lowest unused column is taken when nothing compares, so any input ends with a permutation."""
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    B, n, _ = cost.shape
    out = np.empty((B, n), dtype=np.int64)
    for b in range(B):
        C = cost[b]
        u, v = np.zeros(n), np.zeros(n)
        p = np.full(n, -1, dtype=np.int64)                 # the row matched to every column
        with np.errstate(invalid="ignore"):
            for i in range(n):
                minv = np.full(n, np.inf)
                way = np.full(n, -1, dtype=np.int64)
                used = np.zeros(n, dtype=bool)
                in_tree = np.zeros(n, dtype=bool)
                i0, j0 = i, -1
                for _ in range(n + 1):
                    in_tree[i0] = True
                    cur = C[i0] - u[i0] - v
                    better = ~used & (cur < minv)
                    minv[better] = cur[better]
                    way[better] = j0
                    open_cols = np.flatnonzero(~used)                     # never empty: only matched columns are marked, fewer than n are matched
                    offer = np.where(np.isnan(minv[open_cols]), np.inf, minv[open_cols])
                    j1 = int(open_cols[np.argmin(offer)])                 # the first minimum: the lowest unused column among equals
                    delta = offer.min()
                    u[in_tree] += delta
                    v[used] -= delta
                    minv[~used] -= delta
                    j0 = j1
                    used[j0] = True
                    i0 = int(p[j0])
                    if i0 < 0:
                        break
                for _ in range(n):
                    j1 = int(way[j0])
                    p[j0] = i if j1 < 0 else p[j1]
                    j0 = j1
                    if j0 < 0:
                        break
        out[b, p] = np.arange(n)
    return out


def _assign(cost, maximize):
    """(B, n, n) fp64 pair values -> (B, n) int64 optimal permutation: sep_assign where the backend takes the matrix, the host solver otherwise
    (CPU tensors beside the HIP library, n beyond the kernel's limit)"""
    K = sepkernels.backend()
    B, n, _ = cost.shape
    if n > sepkernels.ASSIGN_MAX_N or (K.name == "hip" and not cost.is_cuda):
        signed = -cost if maximize else cost
        return torch.from_numpy(_solve_host(signed.detach().cpu().numpy())).to(cost.device)
    cost = cost.contiguous()
    perm = torch.empty(B, n, device=cost.device, dtype=torch.int64)
    total = torch.empty(B, device=cost.device, dtype=torch.float64)
    duals = torch.empty(B, 2 * n, device=cost.device, dtype=torch.float64)
    K.assign(cost, B, n, maximize, perm, total, duals)
    return perm


def _composed_hungarian(criterion, input, target, batch_mean):
    """any criterion that is additive over the sources: the value of every (estimate, target) pair from the criterion itself on single-source
    rows, without a tape and a bounded block of rows at a time; the assignment on that matrix; then the criterion once more, with the tape, on
    the targets in the chosen order"""
    B, n = input.shape[:2]
    target = target.to(input.dtype)
    maximize = bool(getattr(criterion, "maximize", False))
    rows = B * n * n
    per_row = max(1, input[0, 0].numel())
    block = max(1, min(rows, _BLOCK_ELEMS // per_row))
    values = []
    with torch.no_grad():
        index = torch.arange(rows, device=input.device)
        b, i, j = index // (n * n), (index // n) % n, index % n
        for r0 in range(0, rows, block):
            sl = slice(r0, min(rows, r0 + block))
            scores = criterion(input[b[sl], i[sl]].unsqueeze(1), target[b[sl], j[sl]].unsqueeze(1), batch_mean=False)
            if scores.dim() != 1:
                raise ValueError("the Hungarian loss needs a criterion that returns one value per item (a reduction over the sources)")
            values.append(scores.double())
    pattern = _assign(torch.cat(values).view(B, n, n), maximize)
    loss = criterion(input, target[torch.arange(B, device=input.device).unsqueeze(1), pattern], batch_mean=False)
    if batch_mean:
        loss = loss.mean(dim=0)
    return loss, pattern


def hungarian(criterion, input, target, batch_mean=True):
    """
    Args:
        criterion <callable>: criterion(input, target, batch_mean=False) -> (batch_size,), additive over the sources (a sum or mean of per-source values)
        input, target (batch_size, n_sources, *)
    Returns:
        loss: () or (batch_size,) best loss per item (min, or max if criterion.maximize)
        pattern (batch_size, n_sources) int64: the target every estimate is matched to: criterion(input, target[:, pattern]) is the optimum
    """
    if input.dim() != target.dim() or input.dim() < 3:
        raise ValueError("the Hungarian loss takes (batch_size, n_sources, *) estimates and targets, given {} and {}".format(tuple(input.shape), tuple(target.shape)))
    if input.shape != target.shape:
        raise ValueError("estimates {} and targets {} differ in batch size, number of sources or length".format(tuple(input.shape), tuple(target.shape)))
    if target.requires_grad:
        raise NotImplementedError("gradient w.r.t. the target of the Hungarian loss is not implemented")
    if _kernel_route(criterion, input, target):
        return _fused_hungarian(criterion, input, target, batch_mean)
    return _composed_hungarian(criterion, input, target, batch_mean)


class HungarianLoss(nn.Module):
    def __init__(self, criterion=None):
        super().__init__()
        self.criterion = NegSISDR() if criterion is None else criterion

    def forward(self, input, target, batch_mean=True):
        return hungarian(self.criterion, input, target, batch_mean=batch_mean)
