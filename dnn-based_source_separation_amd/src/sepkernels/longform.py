"""
Long recordings through a non-causal separator, window by window (continuous speech separation; Chen et al., "Continuous speech separation:
dataset and analysis", ICASSP 2020).  The models here are trained on segments of a few seconds; `model(mixture)` on a meeting costs memory
that grows with T, takes gLN statistics over minutes the model never saw and drives the dual-path models' chunk count out of the trained
range.  separate_long cuts the recording into overlapping windows of the trained length, separates every window on its own, undoes the
arbitrary output order of each window by matching its estimates to its neighbour's on the samples they share, and cross-fades the aligned
windows into n continuous tracks.  The reference has nothing of the kind.

stitch() is the part after the model.  For estimates (B, W, n, win) of W windows at stride hop, O = win - hop:
    cost[b][w][i][j]   = sum_{t < O} (est[b][w][i][hop + t] - est[b][w + 1][j][t])^2                          (fp64)
    perm_local[b][w]   = the minimum-cost perfect matching of cost[b][w] (row i of window w continues in row perm_local[b][w][i] of w + 1)
    perm_abs[b][0][s]  = s,   perm_abs[b][w + 1][s] = perm_local[b][w][perm_abs[b][w][s]]
    out[b][s][t]       = a + g (c - a) inside the overlap with the window before, c elsewhere; w = min(t // hop, W - 1), k = t - w hop,
                         c = est[b][w][perm_abs[b][w][s]][k], a = est[b][w - 1][perm_abs[b][w - 1][s]][hop + k], g = (k + 0.5) / O
win / 2 <= hop < win: a sample lies in at most two windows and the cross-fade weights add to one.  On contiguous fp32 device tensors with
n <= 64 this is four launches without a host synchronisation in between (sep_stitch_cost, sep_assign, sep_stitch_chain, sep_stitch_ola:
csrc/stitch.hip, csrc/assign.hip); everything else -- CPU tensors beside the HIP library, fp64, n > 64, a strided view -- is the same
definitions composed in torch, with criterion.hungarian._assign for the matching.  Inference only: nothing here carries a gradient.
"""
import torch
import torch.nn.functional as F

import sepkernels

_BLOCK_ELEMS = 1 << 24     # composed route: elements of the pair differences formed at a time


def _on_kernels(t):
    """contiguous fp32 where the backend's kernels can take it: the device beside the HIP library, any tensor beside another backend"""
    return t.dtype == torch.float32 and t.is_contiguous() and (t.is_cuda or sepkernels.backend().name != "hip")


def _stitch_kernels(est, hop, length):
    K = sepkernels.backend()
    B, W, n, win = est.shape
    dev = est.device
    out = torch.empty(B, n, length, device=dev, dtype=torch.float32)
    perm_abs = torch.empty(B, W, n, device=dev, dtype=torch.int64)
    total = torch.empty(B, W - 1, device=dev, dtype=torch.float64)
    cost = perm_local = None
    if W > 1:
        cost = torch.empty(B, W - 1, n, n, device=dev, dtype=torch.float64)
        perm_local = torch.empty(B, W - 1, n, device=dev, dtype=torch.int64)
        duals = torch.empty(B, W - 1, 2 * n, device=dev, dtype=torch.float64)
        K.stitch_cost(est, cost, B, W, n, win, hop)
        K.assign(cost, B * (W - 1), n, 0, perm_local, total, duals)
    K.stitch_chain(perm_local, perm_abs, B, W, n)
    K.stitch_ola(est, perm_abs, out, B, W, n, win, hop, length)
    return out, perm_abs, total


def _stitch_composed(est, hop, length):
    from criterion.hungarian import _assign
    B, W, n, win = est.shape
    dev, O = est.device, win - hop
    rows = torch.arange(B, device=dev).view(B, 1, 1)
    perm_abs = torch.arange(n, device=dev).repeat(B, W, 1)
    total = torch.empty(B, W - 1, device=dev, dtype=torch.float64)
    if W > 1:
        cost = torch.empty(B, W - 1, n, n, device=dev, dtype=torch.float64)
        step = max(1, _BLOCK_ELEMS // max(1, B * n * n * O))
        for w0 in range(0, W - 1, step):                       # a bounded block of boundaries at a time
            w1 = min(W - 1, w0 + step)
            a, c = est[:, w0:w1, :, hop:].double(), est[:, w0 + 1:w1 + 1, :, :O].double()
            cost[:, w0:w1] = (a.unsqueeze(3) - c.unsqueeze(2)).square().sum(-1)
        perm_local = _assign(cost.view(B * (W - 1), n, n), False).view(B, W - 1, n)
        total = cost.gather(3, perm_local.unsqueeze(3)).squeeze(3).sum(-1)
        for w in range(W - 1):
            perm_abs[:, w + 1] = perm_local[:, w].gather(1, perm_abs[:, w])
    t = torch.arange(length, device=dev)
    w = torch.clamp(t // hop, max=W - 1)
    k = t - w * hop
    fade = (w >= 1) & (k < O)
    c = est[rows, w.view(1, 1, -1), perm_abs[:, w].transpose(1, 2), k.view(1, 1, -1)]
    wa, ka = torch.clamp(w - 1, min=0), torch.where(fade, k + hop, k)
    a = est[rows, wa.view(1, 1, -1), perm_abs[:, wa].transpose(1, 2), ka.view(1, 1, -1)]
    g = ((k.to(est.dtype) + 0.5) / O).view(1, 1, -1)
    return torch.where(fade.view(1, 1, -1), a + g * (c - a), c), perm_abs, total


def stitch(estimates, hop, length):
    """
    Args:
        estimates (batch_size, n_windows, n_sources, window): the separated windows of every recording, window w over samples [w hop, w hop + window)
        hop <int>: window / 2 <= hop < window
        length <int>: samples of the recording, 1 <= length <= (n_windows - 1) hop + window
    Returns:
        output (batch_size, n_sources, length): the windows in the order of the first one, cross-faded over the overlaps
        perm_abs (batch_size, n_windows, n_sources) int64: the row of window w that continues track s
        boundary_cost (batch_size, n_windows - 1) float64: the squared distance between the matched rows on every overlap -- how well
            the neighbours agreed
    """
    if estimates.dim() != 4:
        raise ValueError("stitch takes (batch_size, n_windows, n_sources, window) estimates, given {}".format(tuple(estimates.shape)))
    B, W, n, win = estimates.shape
    hop, length = int(hop), int(length)
    if min(B, W, n) < 1 or win < 2:
        raise ValueError("stitch needs at least one recording, window and source and a window of two samples, given {}".format(tuple(estimates.shape)))
    if not (win <= 2 * hop and hop < win):
        raise ValueError("hop must lie in [window / 2, window) so that a sample lies in at most two windows: window {}, hop {}".format(win, hop))
    if not 1 <= length <= (W - 1) * hop + win:
        raise ValueError("{} windows of {} at hop {} cover {} samples, not {}".format(W, win, hop, (W - 1) * hop + win, length))
    if not estimates.is_floating_point():
        raise ValueError("stitch takes floating-point estimates, given {}".format(estimates.dtype))
    with torch.no_grad():
        if n <= sepkernels.ASSIGN_MAX_N and _on_kernels(estimates):
            return _stitch_kernels(estimates, hop, length)
        return _stitch_composed(estimates, hop, length)


def _windows(x, W, window, hop):
    """(B, T) -> (B, W, window): window w holds samples [w hop, w hop + window), zeros beyond T"""
    B, T = x.shape
    if _on_kernels(x):
        out = torch.empty(B, W, window, device=x.device, dtype=x.dtype)
        sepkernels.backend().segment(x, out, B, T, T, W, window, hop, 0)
        return out
    return F.pad(x, (0, (W - 1) * hop + window - T)).unfold(1, window, hop)


def separate_long(model, mixture, window, hop=None, batch_windows=16):
    """
    Args:
        model: (batch_size, 1, T) -> (batch_size, n_sources, T); the caller chooses model.eval()
        mixture (T,), (1, T) or (batch_size, 1, T)
        window <int>: samples per window -- the length the model was trained on
        hop <int>: window / 2 <= hop < window, default window // 2
        batch_windows <int>: windows per forward of the model
    Returns:
        output (batch_size, n_sources, T), or (n_sources, T) for an unbatched mixture: for T <= window model(mixture) itself, else the
        windows' estimates stitched (stitch above).  NOT model(mixture) of the whole recording: every window is normalised and masked by
        what the model sees in that window alone.
    """
    window, batch_windows = int(window), int(batch_windows)
    hop = window // 2 if hop is None else int(hop)
    if mixture.dim() not in (1, 2, 3) or (mixture.dim() > 1 and mixture.shape[-2] != 1):
        raise ValueError("separate_long takes a (T,), (1, T) or (batch_size, 1, T) mixture, given {}".format(tuple(mixture.shape)))
    if window < 2 or not (window <= 2 * hop and hop < window):
        raise ValueError("hop must lie in [window / 2, window) so that a sample lies in at most two windows: window {}, hop {}".format(window, hop))
    if batch_windows < 1:
        raise ValueError("batch_windows must be positive, given {}".format(batch_windows))
    batched = mixture.dim() == 3
    x = mixture.reshape(-1, 1, mixture.shape[-1])
    B, _, T = x.shape
    with torch.no_grad():
        if T <= window:
            out = model(x)
            return out if batched else out[0]
        W = -(-(T - window) // hop) + 1                    # the smallest count with (W - 1) hop + window >= T
        wins = _windows(x.reshape(B, T).contiguous(), W, window, hop).reshape(B * W, 1, window)
        est = None
        for r0 in range(0, B * W, batch_windows):
            y = model(wins[r0:r0 + batch_windows].contiguous())
            if y.dim() != 3 or y.shape[0] != min(batch_windows, B * W - r0) or y.shape[2] != window:
                raise ValueError("the model returned {} for windows {}".format(tuple(y.shape), tuple(wins[r0:r0 + batch_windows].shape)))
            if est is None:
                est = torch.empty(B * W, y.shape[1], window, device=y.device, dtype=y.dtype)
            est[r0:r0 + y.shape[0]] = y
        out, _, _ = stitch(est.view(B, W, est.shape[1], window), hop, T)
    return out if batched else out[0]
