"""
Mixture invariant training (MixIT) on MI355X: Wisdom et al., "Unsupervised Sound Separation Using Mixture Invariant Training", 2020.
The reference's src/criterion/mixit.py is a stub that raises NotImplementedError; the API here mirrors `pit` / `PIT` of criterion/pit.py:
`criterion(input, target, batch_mean) -> (loss, assignment)`.

The model hears the sum of N reference mixtures `target` (B, N, T) and emits M estimates `input` (B, M, T).  An assignment hands every
estimate to exactly one mixture; mixture n is scored against the sum of its estimates (the remix, zero for an empty set -- the criterion's own
eps decides that value) and the loss is the best of the N^M assignments: the minimum of the criterion, or its maximum if `criterion.maximize`.
Assignments are enumerated in itertools.product(range(N), repeat=M) order, estimate 0 most significant, and the first extremum wins
(torch.min / torch.max, as in sep_pit_search).  `assignment` is (B, M) int64: the mixture index of every estimate.

With SI-SDR, SDR or the thresholded SNR (criterion.sdr) on fp32 (B, M, T) estimates the value of a remix is a function of three inner
products that are sums of entries of ONE Gram matrix of the M + N rows: sep_mixit_gram makes one pass over the waveforms,
sep_mixit_search scores all N^M assignments on the small matrix, sep_mixit_bwd applies the analytic gradient of the chosen one.  Nothing
of size N^M x T is ever formed.  Every other case -- other criteria, the clipped subclasses, 4-D inputs, CPU tensors beside the HIP library,
searches beyond the kernels' limits -- takes the composed route: remixes for a block of assignments at a time, the criterion itself on them.
"""
import torch
import torch.nn as nn

import sepkernels
from criterion.sdr import SISDR, NegSISDR, SDR, NegSDR, ThresholdedSNR, NegThresholdedSNR

_KINDS = {SISDR: (0, 1.0), NegSISDR: (0, -1.0), SDR: (1, 1.0), NegSDR: (1, -1.0), ThresholdedSNR: (2, 1.0), NegThresholdedSNR: (2, -1.0)}
_MAX_ROWS = 65535          # the kernels put the batch on a 16-bit grid dimension: larger batches go through in slices
_BLOCK_ELEMS = 1 << 25     # composed route: elements of the remixes formed at a time


def _kernel_route(criterion, input, target):
    if type(criterion) not in _KINDS or criterion.reduction not in ("mean", "sum"):
        return False
    if input.dim() != 3 or target.dim() != 3 or input.dtype != torch.float32:
        return False
    if sepkernels.backend().name == "hip" and not input.is_cuda:
        return False
    M, N = input.shape[1], target.shape[1]
    return 1 <= M <= sepkernels.MIXIT_MAX_EST and 1 <= N <= sepkernels.MIXIT_MAX_MIX and N ** M <= sepkernels.MIXIT_MAX_CODES


class _MixITFn(torch.autograd.Function):
    """est (B, M, T), tgt (B, N, T) -> (best (B,), code (B,) int64, per_mix (B, N)): the best reduced measure (in dB, not negated), the code of
    its assignment and the measure of every mixture under it"""

    @staticmethod
    def forward(ctx, est, tgt, kind, maximize, use_mean, eps, tau):
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("gradient w.r.t. the MixIT target (the reference mixtures) is not implemented")
        K = sepkernels.backend()
        est, tgt = est.contiguous(), tgt.contiguous()
        B, M, T = est.shape
        N = tgt.shape[1]
        R, dev = M + N, est.device
        gram = torch.empty(B, R, R, device=dev, dtype=torch.float64)
        best = torch.empty(B, device=dev, dtype=torch.float32)
        code = torch.empty(B, device=dev, dtype=torch.int64)
        per_mix = torch.empty(B, N, device=dev, dtype=torch.float32)
        scratch = torch.empty(max(1, K.mixit_scratch_bytes(min(B, _MAX_ROWS), M, N, T) // 8), device=dev, dtype=torch.float64)
        for b0 in range(0, B, _MAX_ROWS):
            b1 = min(B, b0 + _MAX_ROWS)
            K.mixit_gram(est[b0:b1], tgt[b0:b1], gram[b0:b1], scratch, b1 - b0, M, N, T)
            K.mixit_search(gram[b0:b1], b1 - b0, M, N, kind, maximize, use_mean, eps, tau, best[b0:b1], code[b0:b1], per_mix[b0:b1])
        ctx.save_for_backward(est, tgt, gram, code)
        ctx.meta = (kind, use_mean, eps, tau)
        ctx.mark_non_differentiable(code, per_mix)
        return best, code, per_mix

    @staticmethod
    def backward(ctx, gbest, _gcode, _gper):
        K = sepkernels.backend()
        est, tgt, gram, code = ctx.saved_tensors
        kind, use_mean, eps, tau = ctx.meta
        B, M, T = est.shape
        N = tgt.shape[1]
        gw = (gbest / N if use_mean else gbest).to(torch.float32).contiguous()      # what arrives at every per-mixture measure
        d_est = torch.empty_like(est)
        for b0 in range(0, B, _MAX_ROWS):
            b1 = min(B, b0 + _MAX_ROWS)
            K.mixit_bwd(est[b0:b1], tgt[b0:b1], gram[b0:b1], code[b0:b1], gw[b0:b1], d_est[b0:b1], b1 - b0, M, N, T, kind, eps, tau)
        return d_est, None, None, None, None, None, None


def _digits(code, M, N):
    """(B,) codes -> (B, M) mixture index of every estimate (estimate 0 most significant)"""
    weights = torch.tensor([N ** (M - 1 - m) for m in range(M)], device=code.device, dtype=torch.int64)
    return (code.unsqueeze(1) // weights) % N


def _fused_mixit(criterion, input, target, batch_mean):
    kind, sign = _KINDS[type(criterion)]
    M, N = input.shape[1], target.shape[1]
    # the kernels score the measure itself: minimising its negative and maximising it pick the same assignment
    maximize = bool(criterion.maximize) == (sign > 0)
    tau = float(criterion.tau) if kind == 2 else 0.0
    best, code, _ = _MixITFn.apply(input, target.to(input.dtype), kind, maximize, criterion.reduction == "mean", float(criterion.eps), tau)
    loss = best if sign > 0 else -best
    if batch_mean:
        loss = loss.mean(dim=0)
    return loss, _digits(code, M, N)


def _remix_matrix(codes, M, N, dtype):
    """(K,) codes -> (K, N, M) 0/1: [k][n][m] = 1 where code k hands estimate m to mixture n"""
    return torch.nn.functional.one_hot(_digits(codes, M, N), N).transpose(1, 2).to(dtype)


def _composed_mixit(criterion, input, target, batch_mean):
    """any criterion: the extremum is searched without a tape on remixes of a block of assignments at a time, then the criterion is evaluated
    once more, with the tape, on the remix of the chosen assignment"""
    B, M = input.shape[:2]
    N = target.shape[1]
    target = target.to(input.dtype)
    maximize = bool(getattr(criterion, "maximize", False))
    total = N ** M
    block = max(1, min(total, _BLOCK_ELEMS // max(1, target.numel())))      # the remixes of one assignment are as large as the target
    best = code = None
    with torch.no_grad():
        for c0 in range(0, total, block):
            codes = torch.arange(c0, min(total, c0 + block), device=input.device, dtype=torch.int64)
            k = codes.numel()
            remix = torch.einsum("knm,bm...->bkn...", _remix_matrix(codes, M, N, input.dtype), input)
            tgt = target.unsqueeze(1).expand(B, k, *target.shape[1:])
            scores = criterion(remix.reshape(B * k, *remix.shape[2:]), tgt.reshape(B * k, *target.shape[1:]), batch_mean=False)
            if scores.dim() != 1:
                raise ValueError("MixIT needs a criterion that returns one value per item (a reduction over the mixtures)")
            val, idx = scores.view(B, k).max(dim=1) if maximize else scores.view(B, k).min(dim=1)
            idx = idx + c0
            if best is None:
                best, code = val, idx
            else:
                better = val > best if maximize else val < best          # strict: an earlier block keeps a tie
                best, code = torch.where(better, val, best), torch.where(better, idx, code)
    remix = torch.einsum("bnm,bm...->bn...", _remix_matrix(code, M, N, input.dtype), input)
    loss = criterion(remix, target, batch_mean=False)
    if batch_mean:
        loss = loss.mean(dim=0)
    return loss, _digits(code, M, N)


def mixit(criterion, input, target, batch_mean=True):
    """
    Args:
        criterion <callable>: criterion(input, target, batch_mean=False) -> (batch_size,), scoring (batch_size, N, *) remixes against target
        input (batch_size, M, *): the estimates
        target (batch_size, N, *): the reference mixtures (the model was fed target.sum(1, keepdim=True))
    Returns:
        loss: () or (batch_size,) best loss per item (min, or max if criterion.maximize)
        assignment (batch_size, M) int64: the mixture every estimate is handed to
    """
    if input.dim() != target.dim() or input.dim() < 3:
        raise ValueError("MixIT takes (batch_size, M, *) estimates and (batch_size, N, *) mixtures, given {} and {}".format(tuple(input.shape), tuple(target.shape)))
    if input.shape[0] != target.shape[0] or input.shape[2:] != target.shape[2:]:
        raise ValueError("estimates {} and mixtures {} differ in batch size or length".format(tuple(input.shape), tuple(target.shape)))
    if target.requires_grad:
        raise NotImplementedError("gradient w.r.t. the MixIT target (the reference mixtures) is not implemented")
    if _kernel_route(criterion, input, target):
        return _fused_mixit(criterion, input, target, batch_mean)
    return _composed_mixit(criterion, input, target, batch_mean)


class MixIT(nn.Module):
    def __init__(self, criterion):
        super().__init__()
        self.criterion = criterion

    def forward(self, input, target, batch_mean=True):
        return mixit(self.criterion, input, target, batch_mean=batch_mean)
