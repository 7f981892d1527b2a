"""
BSS-eval v3 ("sources"): SDR, SIR and SAR of separated signals (Vincent, Gribonval, Fevotte 2006), the metric behind every published
Conv-TasNet figure.  API of reference src/utils/bss.py:4-30 (`bss_eval_sources`, a wrapper of mir_eval.separation.bss_eval_sources) plus a
batched form.

The native route evaluates the published definition with the two kernels of libsepkernels that carry its O(T flen) work --
sep_bss_xcorr (the lagged correlations that fill the normal equations) and sep_bss_energies (the FIR pass with the solved filters and the
five energies of every pair), fp64 arithmetic on fp32 audio -- and torch.linalg in fp64 for the (n flen)^2 solve between them.  The projected
signals are never stored.  Definition, for references r_i and estimates e_j of T samples, all extended by flen - 1 zeros:
    P_i(e_j)   least-squares projection of e_j on { r_i delayed by tau, tau = 0 .. flen - 1 },  P_all(e_j) the same over every reference;
    s_filt = P_i(e_j),  e_interf = P_all(e_j) - P_i(e_j),  e_artif = e_j - P_all(e_j);
    SDR = 10 log10(|s_filt|^2 / |e_interf + e_artif|^2),  SIR = 10 log10(|s_filt|^2 / |e_interf|^2),
    SAR = 10 log10(|s_filt + e_interf|^2 / |e_artif|^2);  a zero denominator gives +inf.

SEPK_BSS_EVAL = auto (default) | native | mir_eval selects the route of `bss_eval_sources`: `auto` hands the call to mir_eval exactly as the
reference's wrapper does when that package can be imported (a machine that has it keeps the reference's numbers) and runs the native route
otherwise; `mir_eval` insists on the package.  An all-zero reference or estimate is a ValueError on either route.

BSS-eval v4 ("images"), the framewise SDR, ISR, SIR and SAR that music separation is published with (museval 0.4's metrics.bss_eval as
eval_mus_track calls it: window = hop = 1 s, 512 taps, filters from the whole recording, no permutation search), is `bss_eval_images_batch`,
`bss_eval_images` and `eval_track` below; its definition stands in include/sepkernels.h at sep_bss_image_energies and in DESIGN.md 4.14.  The
filters come from the same two sep_bss_xcorr calls on (B, n C, T) views and the same dense solve; sep_bss_image_energies applies them frame by
frame.  These functions run the native route only, whatever SEPK_BSS_EVAL says: museval's own entry point takes a musdb track object and estimates
of another layout, so handing a call over is not a few obvious lines, and the package is on none of the project's machines to check against.
"""
import itertools
import os
import warnings

import torch

import sepkernels

FILTER_LENGTH = 512            # mir_eval's fixed filter length
_ROUTES = ("auto", "native", "mir_eval")
_solve_route = None            # "device" | "host": where the last dense solve ran
_device_solver = None          # whether this torch build solves dense fp64 systems on the GPU: decided by the first attempt, kept for the process


def solve_route():
    """where the last native evaluation solved its normal equations: "device", "host", or None before the first one"""
    return _solve_route


class _HostComposition:
    """The two kernel calls as fp64 torch arithmetic on CPU tensors: what the native route runs when the HIP library is the backend and no
    GPU is present (`--use_cuda 0` evaluation).  Row by row on the row's own samples, so a row's result does not depend on the batch."""

    name = "host"

    def bss_scratch_bytes(self, B, n, m, T, flen):
        return 8

    def bss_xcorr(self, a, c, lengths, out, scratch, B, n, m, T, lag_lo, nlag):
        for b in range(B):
            Tb = T if lengths is None else int(lengths[b])
            x, y = a[b, :, :Tb].double(), c[b, :, :Tb].double()
            for l in range(nlag):
                lag = lag_lo + l
                lo, hi = max(0, -lag), min(Tb, Tb - lag)
                out[b, :, :, l] = x[:, lo:hi] @ y[:, lo + lag:hi + lag].t() if hi > lo else 0.0

    def bss_energies(self, ref, est, filt_all, filt_one, lengths, out, scratch, B, n, m, T, flen):
        conv = torch.nn.functional.conv1d
        for b in range(B):
            Tb = T if lengths is None else int(lengths[b])
            r = torch.nn.functional.pad(ref[b, :, :Tb].double(), (flen - 1, flen - 1))[None]           # (1, n, Tb + 2 (flen - 1))
            e = torch.nn.functional.pad(est[b, :, :Tb].double(), (0, flen - 1))                         # (m, Tx)
            p_all = conv(r, filt_all[b].flip(-1))[0]                                                     # (m, Tx)
            s = conv(r, filt_one[b].permute(1, 0, 2).reshape(n * m, 1, flen).flip(-1), groups=n)[0]     # row i m + j: P_i(e_j)
            s = s.reshape(n, m, -1).permute(1, 0, 2)                                                     # (m, n, Tx)
            interf, artif = p_all[:, None] - s, (e - p_all)[:, None]
            for q, v in enumerate((s, interf, artif, interf + artif, s + interf)):
                out[b, :, :, q] = v.square().sum(-1)

    def bss_image_scratch_bytes(self, B, n, C, flen, window, nwin):
        return 8

    def bss_image_energies(self, ref, est, filt_all, filt_one, lengths, out, scratch, B, n, C, T, flen, window, hop, nwin):
        conv = torch.nn.functional.conv1d
        out.zero_()
        for b in range(B):
            Tb = T if lengths is None else int(lengths[b])
            fa = filt_all[b].reshape(n * C, n * C, flen).flip(-1)                                        # [(j, c)][(k, c2)]
            fo = filt_one[b].reshape(n * C, C, flen).flip(-1)                                            # [(j, c)][c2], group j
            for w in range(min(nwin, _num_frames(Tb, window, hop))):
                seg = slice(w * hop, w * hop + window)
                s = torch.nn.functional.pad(ref[b, :, :, seg].double(), (0, flen - 1))                   # (n, C, W + flen - 1)
                e = torch.nn.functional.pad(est[b, :, :, seg].double(), (0, flen - 1))
                rp = torch.nn.functional.pad(s.reshape(1, n * C, -1), (flen - 1, 0))
                p_all, p_j = conv(rp, fa)[0].reshape(n, C, -1), conv(rp, fo, groups=n)[0].reshape(n, C, -1)
                for q, v in enumerate((s, e - s, p_j - s, p_j, p_all - p_j, p_all, e - p_all)):
                    out[b, :, w, q] = v.square().sum((-2, -1))
                out[b, :, w, 7] = (s[..., :window].sum(1) != 0).sum(-1).double()
                out[b, :, w, 8] = (e[..., :window].sum(1) != 0).sum(-1).double()


def _kernels(t):
    """(object with bss_scratch_bytes / bss_xcorr / bss_energies, device the evaluation runs on)"""
    K = sepkernels.backend()
    if K.name != "hip":
        return K, t.device                          # (the tests' emulator of the C ABI)
    if t.is_cuda:
        return K, t.device
    if torch.cuda.is_available():
        return K, torch.device("cuda", torch.cuda.current_device())
    return _HostComposition(), t.device


def _lstsq(G, D):
    return torch.linalg.lstsq(G.cpu(), D.cpu(), driver="gelsd").solution.to(G.device)


def _no_device_solver(error):
    """whether a RuntimeError of torch.linalg.solve on a GPU tensor says that the build lacks the routine (torch words these as
    '... requires compiling PyTorch with MAGMA', '... library not found in compilation', 'not implemented for ...') and nothing else"""
    if isinstance(error, NotImplementedError):
        return True
    text = str(error).lower()
    return any(w in text for w in ("magma", "lapack", "not implemented", "not compiled", "not found in compilation"))


def _solve(G, D):
    """G (..., N, N), D (..., N, m), fp64 -> G^-1 D.  On the GPU when this torch build has a dense solver there; if it refuses, on the
    host from then on (once per process).  A solve that raises for the matrix (singular) falls back to least squares, as mir_eval does."""
    global _solve_route, _device_solver
    if G.is_cuda and _device_solver is not False:
        try:
            x = torch.linalg.solve(G, D)
            _device_solver, _solve_route = True, "device"
            return x
        except torch.linalg.LinAlgError:
            _solve_route = "device"
            return _lstsq(G, D)
        except RuntimeError as e:
            if not _no_device_solver(e):
                raise                               # out of memory, a fault of earlier work, ...: not a reason to carry on elsewhere
            _device_solver = False
            warnings.warn("utils.bss: this torch build has no dense fp64 solver on the GPU ({}); the BSS-eval solves run on the host "
                          "for the rest of the process".format(str(e).splitlines()[0]))
    _solve_route = "host"
    try:
        return torch.linalg.solve(G.cpu(), D.cpu()).to(G.device)
    except torch.linalg.LinAlgError:
        return _lstsq(G, D)


def _db(num, den):
    return torch.where(den == 0, torch.full_like(num, float("inf")), 10 * torch.log10(num / den))


def bss_energies_batch(reference, estimated, lengths=None, filter_length=FILTER_LENGTH):
    """reference, estimated (B, n, T) -> (B, n, n, 5) fp64 on the CPU: for estimate j (axis 1) and reference i (axis 2) the energies
    |s_filt|^2, |e_interf|^2, |e_artif|^2, |e_interf + e_artif|^2, |s_filt + e_interf|^2.  One pass of the two kernels for the batch."""
    if reference.dim() != 3 or reference.shape != estimated.shape:
        raise ValueError("reference and estimated sources must both be (B, n, T); got {} and {}".format(tuple(reference.shape), tuple(estimated.shape)))
    B, n, T = reference.shape
    flen = int(filter_length)
    if flen < 1 or B < 1 or n < 1 or T < 1:
        raise ValueError("empty input or filter_length < 1")
    K, dev = _kernels(reference)
    ref = reference.detach().to(dev, torch.float32).contiguous()
    est = estimated.detach().to(dev, torch.float32).contiguous()
    if lengths is not None:
        host = torch.as_tensor(lengths).to("cpu", torch.int64).reshape(-1)
        if host.numel() != B or int(host.min()) < 1 or int(host.max()) > T:
            raise ValueError("lengths must hold one value in [1, T] per row")
        lengths = host.to(torch.int32).to(dev)
        valid = torch.arange(T, device=dev)[None, None, :] < lengths[:, None, None]
        audible = ((ref != 0) & valid).any(-1)
    else:
        audible = (ref != 0).any(-1)
    heard = (est != 0) if lengths is None else ((est != 0) & valid)
    silent_ref, silent_est = (not bool(audible.all())), (not bool(heard.any(-1).all()))
    if silent_ref:
        raise ValueError("a reference source is all zeros: the projection on it is undefined")
    if silent_est:                                   # as mir_eval: the ratios of an all-zero estimate are 0 / 0
        raise ValueError("an estimated source is all zeros: its SDR, SIR and SAR are undefined")
    scratch = torch.empty(max(1, K.bss_scratch_bytes(B, n, n, T, flen) // 8), device=dev, dtype=torch.float64)
    xrr, xre = _correlations(K, ref, est, lengths, flen, scratch)
    filt_all, filt_one = _filters(xrr, xre, flen)
    return _energies(K, ref, est, filt_all, filt_one, lengths, flen, scratch).cpu()


def _correlations(K, ref, est, lengths, flen, scratch):
    """-> xrr (B, n, n, 2 flen - 1): references x references at lags -(flen - 1) .. flen - 1; xre (B, n, n, flen): references x estimates at 0 .. flen - 1"""
    B, n, T = ref.shape
    xrr = torch.empty(B, n, n, 2 * flen - 1, device=ref.device, dtype=torch.float64)
    xre = torch.empty(B, n, n, flen, device=ref.device, dtype=torch.float64)
    K.bss_xcorr(ref, ref, lengths, xrr, scratch, B, n, n, T, -(flen - 1), 2 * flen - 1)
    K.bss_xcorr(ref, est, lengths, xre, scratch, B, n, n, T, 0, flen)
    return xrr, xre


def _filters(xrr, xre, flen):
    """the normal equations G C = D of every row, solved: G[(i, p), (k, q)] = <r_i delayed p, r_k delayed q> = xrr[i][k][p - q] (block Toeplitz),
    D[(i, p), j] = <r_i delayed p, e_j> = xre[i][j][p] -> filt_all (B, n, n, flen): [b][j][k] the filter on r_k in P_all(e_j); filt_one: [b][j][i]
    the filter of P_i(e_j), from the diagonal block G[i, i] and D[i] alone"""
    B, n = xrr.shape[:2]
    dev = xrr.device
    tau = torch.arange(flen, device=dev)
    toeplitz = tau[:, None] - tau[None, :] + (flen - 1)
    idx = torch.arange(n, device=dev)
    filt_all = torch.empty(B, n, n, flen, device=dev, dtype=torch.float64)
    filt_one = torch.empty(B, n, n, flen, device=dev, dtype=torch.float64)
    for b in range(B):                              # one solve per row: a row's filters do not depend on the batch around it
        blocks = xrr[b][:, :, toeplitz]             # (n, n, flen, flen): [i][k][p][q]
        D = xre[b].permute(0, 2, 1)                 # (n, flen, n): [i][p][j]
        C = _solve(blocks.permute(0, 2, 1, 3).reshape(n * flen, n * flen), D.reshape(n * flen, n))
        filt_all[b] = C.reshape(n, flen, n).permute(2, 0, 1)
        filt_one[b] = _solve(blocks[idx, idx], D).permute(2, 0, 1)
    return filt_all, filt_one


def _energies(K, ref, est, filt_all, filt_one, lengths, flen, scratch):
    B, n, T = ref.shape
    out = torch.empty(B, n, n, 5, device=ref.device, dtype=torch.float64)
    K.bss_energies(ref, est, filt_all, filt_one, lengths, out, scratch, B, n, n, T, flen)
    return out


def bss_eval_sources_batch(reference, estimated, lengths=None, filter_length=FILTER_LENGTH, compute_permutation=True):
    """reference, estimated (B, n, T) on any device, rows of their own `lengths` (B values in [1, T]) if given ->
    sdr, sir, sar (B, n) fp64 and perm (B, n) long, on the CPU, ordered by true source: entry [b, i] scores estimate perm[b, i] against
    reference i.  With compute_permutation the permutation maximising the mean SIR is chosen (the first in itertools order among equals),
    otherwise estimate i is scored against reference i."""
    en = bss_energies_batch(reference, estimated, lengths, filter_length)
    B, n = en.shape[:2]
    sdr, sir, sar = _db(en[..., 0], en[..., 3]), _db(en[..., 0], en[..., 1]), _db(en[..., 4], en[..., 2])      # [b][estimate][reference]
    true = torch.arange(n)
    perm = true.repeat(B, 1)
    if compute_permutation:
        for b in range(B):
            best = None
            for p in itertools.permutations(range(n)):
                score = sir[b, list(p), true].mean().item()
                if best is None or score > best:
                    best, perm[b] = score, torch.tensor(p)
    pick = lambda v: torch.gather(v, 1, perm[:, None, :])[:, 0]
    return pick(sdr), pick(sir), pick(sar), perm


def _route():
    route = os.environ.get("SEPK_BSS_EVAL", "auto")
    if route not in _ROUTES:
        raise ValueError("SEPK_BSS_EVAL must be one of {} (got '{}')".format(_ROUTES, route))
    return route


def bss_eval_sources(reference_sources, estimated_sources, compute_permutation=True, **kwargs):
    """
    Args:
        reference_sources <torch.Tensor>: (n_sources, T), on any device
        estimated_sources <torch.Tensor>: (n_sources, T)
    Returns:
        sdr, sir, sar <torch.DoubleTensor>: (n_sources,)
        perm <torch.LongTensor>: (n_sources,)
    """
    route = _route()
    if route != "native":
        try:
            from mir_eval.separation import bss_eval_sources as bss_eval_sources_np
        except ImportError:
            if route == "mir_eval":
                raise
            bss_eval_sources_np = None
        if bss_eval_sources_np is not None:
            if not compute_permutation:
                kwargs = dict(kwargs, compute_permutation=False)
            result = bss_eval_sources_np(reference_sources=reference_sources.detach().cpu().numpy(),
                                         estimated_sources=estimated_sources.detach().cpu().numpy(), **kwargs)
            sdr, sir, sar, perm = [torch.as_tensor(r) for r in result]
            return sdr, sir, sar, perm
    if kwargs:
        raise TypeError("the native BSS-eval takes no further arguments (got {})".format(sorted(kwargs)))
    if reference_sources.dim() != 2:
        raise ValueError("reference_sources must be (n_sources, T)")
    sdr, sir, sar, perm = bss_eval_sources_batch(reference_sources[None], estimated_sources[None], compute_permutation=compute_permutation)
    return sdr[0], sir[0], sar[0], perm[0]


# ---- BSS-eval v4 ("images"): framewise SDR, ISR, SIR, SAR as museval scores a MUSDB18 track ----------------------------------------------------
IMAGE_METRICS = ("SDR", "ISR", "SIR", "SAR")


def _num_frames(T, window, hop):
    """full frames of `window` samples every `hop` in T samples: a trailing partial window is dropped"""
    return max(0, (T - window + hop) // hop) if T >= window else 0


def _image_kernels(t):
    K, dev = _kernels(t)
    if not hasattr(K, "bss_image_energies"):        # a backend object from before the images call: the composition on whatever device holds the data
        K = _HostComposition()
    return K, dev


def _image_filters(xrr, xre, n, C, flen):
    """xrr (B, n C, n C, 2 flen - 1), xre (B, n C, n C, flen) of the reference and estimate CHANNELS -> filt_all (B, n, C, n C, flen): [b][j][c][(k, c2)]
    the filter on r[k][c2] in the projection of e[j][c] on every reference channel, from G (n C flen)^2 and D as in `_filters`; filt_one
    (B, n, C, C, flen): [b][j][c][c2] the filter on r[j][c2] in its projection on the channels of reference j alone, from the diagonal
    (C flen)^2 block of source j and the rows and columns of D that belong to it"""
    B, nc = xrr.shape[:2]
    dev = xrr.device
    tau = torch.arange(flen, device=dev)
    toeplitz = tau[:, None] - tau[None, :] + (flen - 1)
    filt_all = torch.empty(B, n, C, nc, flen, device=dev, dtype=torch.float64)
    filt_one = torch.empty(B, n, C, C, flen, device=dev, dtype=torch.float64)
    for b in range(B):                              # one solve per row: a row's filters do not depend on the batch around it
        G = xrr[b][:, :, toeplitz].permute(0, 2, 1, 3).reshape(nc * flen, nc * flen)
        D = xre[b].permute(0, 2, 1).reshape(nc * flen, nc)             # [(k, c2, p)][(j, c)]
        filt_all[b] = _solve(G, D).reshape(nc, flen, n, C).permute(2, 3, 0, 1)
        own = [slice(j * C * flen, (j + 1) * C * flen) for j in range(n)]
        Gj = torch.stack([G[own[j], own[j]] for j in range(n)])
        Dj = torch.stack([D[own[j], j * C:(j + 1) * C] for j in range(n)])
        filt_one[b] = _solve(Gj, Dj).reshape(n, C, flen, C).permute(0, 3, 1, 2)
    return filt_all, filt_one


def bss_image_energies_batch(reference, estimated, lengths=None, window=44100, hop=44100, filter_length=FILTER_LENGTH):
    """reference, estimated (B, n, C, T) -> (B, n, nwin, 9) fp64 on the CPU, the sums of sep_bss_image_energies (include/sepkernels.h) of every
    source and frame, and num_frames (B,) long; nwin is the largest frame count of the batch, rows with fewer frames hold zeros beyond theirs"""
    if reference.dim() != 4 or reference.shape != estimated.shape:
        raise ValueError("reference and estimated images must both be (B, n, C, T); got {} and {}".format(tuple(reference.shape), tuple(estimated.shape)))
    B, n, C, T = reference.shape
    flen, window, hop = int(filter_length), int(window), int(hop)
    if flen < 1 or window < 1 or hop < 1 or B < 1 or n < 1 or C < 1 or T < 1:
        raise ValueError("empty input, or filter_length, window or hop < 1")
    K, dev = _image_kernels(reference)
    ref = reference.detach().to(dev, torch.float32).contiguous()
    est = estimated.detach().to(dev, torch.float32).contiguous()
    if lengths is not None:
        host = torch.as_tensor(lengths).to("cpu", torch.int64).reshape(-1)
        if host.numel() != B or int(host.min()) < 1 or int(host.max()) > T:
            raise ValueError("lengths must hold one value in [1, T] per row")
        lengths = host.to(torch.int32).to(dev)
        audible = ((ref != 0) & (torch.arange(T, device=dev) < lengths[:, None, None, None])).any(-1)
    else:
        host = torch.full((B,), T, dtype=torch.int64)
        audible = (ref != 0).any(-1)
    if not bool(audible.all()):
        raise ValueError("a reference channel is all zeros: the projection on it is undefined")
    num_frames = torch.tensor([_num_frames(int(t), window, hop) for t in host], dtype=torch.int64)
    nwin = int(num_frames.max())
    if nwin == 0:
        return torch.zeros(B, n, 0, 9, dtype=torch.float64), num_frames
    nc = n * C
    nbytes = max(K.bss_scratch_bytes(B, nc, nc, T, flen), K.bss_image_scratch_bytes(B, n, C, flen, window, nwin))
    scratch = torch.empty(max(1, nbytes // 8), device=dev, dtype=torch.float64)
    xrr, xre = _correlations(K, ref.reshape(B, nc, T), est.reshape(B, nc, T), lengths, flen, scratch)
    filt_all, filt_one = _image_filters(xrr, xre, n, C, flen)
    del xrr, xre
    out = torch.empty(B, n, nwin, 9, device=dev, dtype=torch.float64)
    K.bss_image_energies(ref, est, filt_all, filt_one, lengths, out, scratch, B, n, C, T, flen, window, hop, nwin)
    return out.cpu(), num_frames


def bss_eval_images_batch(reference, estimated, lengths=None, window=44100, hop=44100, filter_length=FILTER_LENGTH):
    """reference, estimated (B, n, C, T) or (B, n, T) on any device, rows of their own `lengths` (B values in [1, T]) if given; window and hop in
    samples -> sdr, isr, sir, sar (B, n, nwin) fp64 on the CPU and num_frames (B,) long.  Estimate i is scored against reference i.  Row b has
    num_frames[b] = max(0, (T_b - window + hop) // hop) frames (window > T_b: none, not an error), nwin is the largest of them, frames beyond a
    row's own count are NaN; so is, for every source, a frame in which some reference or some estimate is silent (channel sum zero at every
    sample).  A zero denominator gives +inf."""
    if reference.dim() == 3 and estimated.dim() == 3:
        reference, estimated = reference[:, :, None], estimated[:, :, None]
    en, num_frames = bss_image_energies_batch(reference, estimated, lengths, window, hop, filter_length)
    sdr, isr, sir, sar = _db(en[..., 0], en[..., 1]), _db(en[..., 0], en[..., 2]), _db(en[..., 3], en[..., 4]), _db(en[..., 5], en[..., 6])
    silent = ((en[..., 7] == 0) | (en[..., 8] == 0)).any(1, keepdim=True)                # (B, 1, nwin): any source silent blanks the frame
    beyond = torch.arange(en.shape[2])[None, None, :] >= num_frames[:, None, None]
    nan = torch.full_like(sdr, float("nan"))
    return tuple(torch.where(silent | beyond, nan, v) for v in (sdr, isr, sir, sar)) + (num_frames,)


def bss_eval_images(reference, estimated, window=44100, hop=44100, filter_length=FILTER_LENGTH):
    """one recording: reference, estimated (n, C, T) or (n, T) -> sdr, isr, sir, sar (n, nwin) fp64"""
    if reference.dim() not in (2, 3):
        raise ValueError("reference must be (n_sources, C, T) or (n_sources, T)")
    return tuple(v[0] for v in bss_eval_images_batch(reference[None], estimated[None], None, window, hop, filter_length)[:4])


def nanmedian(values):
    """median of the values that are not NaN, the mean of the two middle ones for an even count (numpy.nanmedian); NaN if there are none"""
    v = torch.as_tensor(values, dtype=torch.float64).reshape(-1)
    v = v[~torch.isnan(v)].sort().values
    k = v.numel()
    if k == 0:
        return float("nan")
    lo, hi = v[(k - 1) // 2].item(), v[k // 2].item()
    return lo if lo == hi else 0.5 * (lo + hi)       # (inf with inf stays inf instead of inf - inf games)


def eval_track(references, estimates, rate, window_s=1.0, hop_s=1.0, filter_length=FILTER_LENGTH):
    """references, estimates: dicts name -> (C, T) or (T,) tensor with the same names; rate in Hz.  museval.eval_mus_track's rule: the named stems
    are scored jointly in one evaluation; when `vocals` is among them (with at least one more stem) a second evaluation of two sources,
    `vocals` and `accompaniment` = the sum of the side's other stems, supplies the `accompaniment` rows and only those.
    -> {target: {"frames": {"SDR": [...], "ISR": [...], "SIR": [...], "SAR": [...]}, "SDR": median, ...}}, frames as floats with NaN for silent
    frames, medians over the frames that are not NaN."""
    names = list(references)
    if not names or set(names) != set(estimates):
        raise ValueError("references and estimates must name the same, at least one, targets")
    if "accompaniment" in names:
        raise ValueError("`accompaniment` is formed here as the sum of the stems other than `vocals`; do not pass it")
    image = lambda x: x[None] if x.dim() == 1 else x                   # noqa: E731
    ref = torch.stack([image(references[k]) for k in names])
    est = torch.stack([image(estimates[k]) for k in names]).to(ref.device)
    window, hop = int(round(window_s * rate)), int(round(hop_s * rate))
    scores = {}

    def take(values, rows):
        for name, i in rows:
            frames = {m: values[q][i].tolist() for q, m in enumerate(IMAGE_METRICS)}
            scores[name] = dict({"frames": frames}, **{m: nanmedian(frames[m]) for m in IMAGE_METRICS})
    take(bss_eval_images(ref, est, window, hop, filter_length), [(k, i) for i, k in enumerate(names)])
    if "vocals" in names and len(names) > 1:
        v = names.index("vocals")
        rest = [i for i in range(len(names)) if i != v]
        pair = lambda x: torch.stack([x[v].double(), x[rest].double().sum(0)])      # noqa: E731  (summed in fp64, rounded to fp32 audio once)
        take(bss_eval_images(pair(ref), pair(est), window, hop, filter_length), [("accompaniment", 1)])
    return scores
