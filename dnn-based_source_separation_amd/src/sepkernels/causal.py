"""
Explicit forward / backward of the staged (causal) Conv-TasNet on the sepkernels C ABI: what sepkernels/net.py is for the fused family.

ConvTasNet._run_staged (models/conv_tasnet.py) runs the causal family layer by layer through torch.autograd.Functions
(sepkernels/functional.py); every launch then costs the interpreter's autograd bookkeeping, and the glue between launches (the mask's
sigmoid, sums of gradients, zero fills, the PReLU slopes' reductions) is torch kernels.  Here the same operations -- the plain functions
those Functions are made of -- are called in order, forward and then backward, with backend calls only: no autograd, no torch kernel
between the first and the last launch, every gradient written straight into the caller's views G[name].  That makes the causal training
step recordable (sepkernels.train.FusedTrainStep.record -> one sep_run_sequence call per step).

Against _run_staged + autograd's backward of it, launch for launch, the differences are the glue:
    sum of the two gradients at a layer input     sep_axpby behind the conv1^T product (the same kernel and the same single rounding as the eager step's)
    sum of the two gradients at the encoder out   sep_axpby (through the first norm + through mask * w), ReLU mask by sep_relu_drop_bwd
    PReLU slopes: pa.sum(dtype=float64)           sep_sum_f64 (fp64 accumulation in a fixed order)
    depthwise d weight / d bias slices            two sep_repack copies of the summed (C, Kw + 1) rows
    torch.zeros                                   K.zeros / sep_memset
A model with separable=False (full P-tap convolutions output_conv1d / skip_conv1d, reference tdcn.py:100-104, 133-147) takes the second branch of
the layer loops: conv1 -> PReLU + cLN -> sep_unfold_dilated -> the heads' products over the unfolded rows (K = H P, the (M, H, P) weights as they
lie), and backward the [Wo; Ws]^T product, sep_fold_dilated and the one norm's backward -- the same entry points, so the step records alike.
reference: src/models/conv_tasnet.py:121-171, tdcn.py:107-147 / 177-196, modules/norm.py:58-101.
"""
import torch

import sepkernels

from . import STATS_SLOTS, backend
from . import functional as _fn
from . import net as _net


def _flat(t):
    return t.reshape(-1)          # (1, C, 1) gain / shift of a cLN -> (C), a view


def _add(K, x, y):
    """x += y by sep_axpby: the sum autograd forms where two gradients reach one tensor (one rounding of x + y, as torch's add)"""
    if hasattr(K, "axpby"):
        K.axpby(x, 1.0, y, 1.0, x, x.numel())
    else:                                        # (the CPU emulator of the tests has no such call)
        x.add_(y)


def forward(cfg, P, mixture, want_latent=False, save=True):
    """See _forward; sets the per-pass weight bound of SEP_ARITH_F16X3 around it."""
    prev = sepkernels.set_weights_amax(_net._weights_amax(P))
    try:
        return _forward(cfg, P, mixture, want_latent, save)
    finally:
        sepkernels.set_weights_amax(prev)


def _forward(cfg, P, mixture, want_latent, save):
    """cfg: model config dict of a `staged` ConvTasNet; P: dict name -> parameter tensor; mixture (B, Cin, T) contiguous.
    Returns (est (B, n_src, Cin, T), latent (B, n_src, N, ldt) or None, Saved or None)."""
    K = backend()
    dev = mixture.device
    B, Cin, T_in = mixture.shape
    N, L, S = cfg["n_basis"], cfg["kernel_size"], cfg["stride"]
    Pk = cfg["sep_kernel_size"]
    eps = float(cfg.get("eps", 1e-12))
    teps = float(cfg.get("tcn_eps", 1e-12))      # the TCN norms keep tdcn.EPS (the reference never forwards eps to them)
    relu = cfg.get("enc_nonlinear") == "relu"
    geo = _net.Geometry(T_in, L, S)
    F, ldt = geo.F, geo.ldt
    f32 = dict(device=dev, dtype=mixture.dtype)

    # head: encoder -> cLN -> 1x1 bottleneck
    w = torch.empty(B, N, ldt, **f32)
    stats = _net._zeros(K, B, STATS_SLOTS, 2, device=dev, dtype=torch.float64)        # the encoder kernel's by-product, unused here
    K.encoder_fwd(mixture, P["encoder.conv1d.weight"], w, stats, B, Cin, T_in, N, L, S, F, ldt, geo.pad_left, relu)
    xn, mean0, rstd0 = _fn.cln_forward(w, F, None, _flat(P["separator.norm1d.gamma"]), _flat(P["separator.norm1d.beta"]), eps)
    x = _fn.pointwise_forward(xn, F, P["separator.bottleneck_conv1d.weight"], P["separator.bottleneck_conv1d.bias"], None)

    total = None
    acts = []
    dense = not cfg.get("separable", True)
    for pre, dil, dual in _net.layer_names(cfg):
        sp = pre + "separable_conv1d."
        a = _fn.pointwise_forward(x, F, P[pre + "bottleneck_conv1d.weight"], P[pre + "bottleneck_conv1d.bias"], None)
        if dense:
            v, mean1, rstd1 = _fn.cln_forward(a, F, P[pre + "nonlinear1d.weight"], _flat(P[pre + "norm1d.gamma"]), _flat(P[pre + "norm1d.beta"]), teps)
            cols = _fn.unfold_forward(v, F, Pk, dil, (Pk - 1) * dil)
            xo, total = _fn.heads_forward(cols, F, P[pre + "output_conv1d.weight"] if dual else None, P[pre + "output_conv1d.bias"] if dual else None,
                                          P[pre + "skip_conv1d.weight"], P[pre + "skip_conv1d.bias"], x, total)
            if save:
                acts.append((x, a, mean1, rstd1, cols))
            x = xo
            continue
        z, sv1 = _fn.cln_depthwise_forward(a, F, P[pre + "nonlinear1d.weight"], _flat(P[pre + "norm1d.gamma"]), _flat(P[pre + "norm1d.beta"]), teps,
                                           P[sp + "depthwise_conv1d.weight"], P[sp + "depthwise_conv1d.bias"], dil, (Pk - 1) * dil)
        v2, mean2, rstd2 = _fn.cln_forward(z, F, P[sp + "nonlinear1d.weight"], _flat(P[sp + "norm1d.gamma"]), _flat(P[sp + "norm1d.beta"]), teps)
        xo, total = _fn.heads_forward(v2, F, P[sp + "output_pointwise_conv1d.weight"] if dual else None,
                                      P[sp + "output_pointwise_conv1d.bias"] if dual else None,
                                      P[sp + "skip_pointwise_conv1d.weight"], P[sp + "skip_pointwise_conv1d.bias"], x, total)
        if save:
            acts.append((x, a, sv1, z, mean2, rstd2, v2))
        x = xo

    est, latent, m = _net.tail_forward(cfg, P, geo, w, total, mixture.shape, want_latent)
    sv = None
    if save:
        sv = _net.Saved()
        sv.geo, sv.w, sv.xn, sv.mean0, sv.rstd0, sv.acts, sv.total, sv.m, sv.mixture = geo, w, xn, mean0, rstd0, acts, total, m, mixture
    return est, latent, sv


def backward(cfg, P, sv, d_est, G, on_ready=None):
    """See _backward; sets the per-pass weight bound of SEP_ARITH_F16X3 around it."""
    prev = sepkernels.set_weights_amax(_net._weights_amax(P))
    try:
        return _backward(cfg, P, sv, d_est, G, on_ready)
    finally:
        sepkernels.set_weights_amax(prev)


def _backward(cfg, P, sv, d_est, G, on_ready=None):
    """Writes the gradient of every parameter into G[name] (overwrites; the views have the parameters' shapes).  d_est (B, n_src, Cin, T).
    on_ready(r): called when every gradient of TCN block r is final -- first the last block (with the whole tail: mask PReLU, mask
    convolution, decoder), then once per earlier block down to block 1; block 0 and the head are final when this function returns
    (as net._backward)."""
    K = backend()
    mixture = sv.mixture
    B, Cin, T_in = mixture.shape
    N, L, S = cfg["n_basis"], cfg["kernel_size"], cfg["stride"]
    Pk = cfg["sep_kernel_size"]
    eps = float(cfg.get("eps", 1e-12))
    teps = float(cfg.get("tcn_eps", 1e-12))
    relu = cfg.get("enc_nonlinear") == "relu"
    geo, w = sv.geo, sv.w
    F, ldt = geo.F, geo.ldt
    f32 = dict(device=mixture.device, dtype=mixture.dtype)
    layers = _net.layer_names(cfg)
    X_layers = cfg["sep_num_layers"]
    dense = not cfg.get("separable", True)

    # tail: decoder, mask * w, mask nonlinearity, mask convolution behind its PReLU
    dal = _net._zeros(K, 1, device=mixture.device, dtype=torch.float64)
    dS, dwm = _net.tail_backward(cfg, P, geo, w, sv.total, sv.m, mixture.shape, d_est, G, dal)
    K.f64_to_f32(dal, G["separator.prelu.weight"], 1, 0)

    # TCN layers, reversed.  Every layer's skip head reads the same dS; d_out is the gradient at the layer's output (None for the last layer,
    # which has no output head) and reaches the layer's input twice: through the residual and through conv1.
    d_out = None
    for li in range(len(layers) - 1, -1, -1):
        pre, dil, dual = layers[li]
        sp = pre + "separable_conv1d."
        if dense:
            x, a, mean1, rstd1, cols = sv.acts[li]
            dcols = _fn.heads_backward(cols, P[pre + "output_conv1d.weight"] if dual else None, P[pre + "skip_conv1d.weight"], None, F,
                                       d_out if dual else None, dS,
                                       dWo=G[pre + "output_conv1d.weight"] if dual else None, dbo=G[pre + "output_conv1d.bias"] if dual else None,
                                       dWs=G[pre + "skip_conv1d.weight"], dbs=G[pre + "skip_conv1d.bias"])[0]
            dv = _fn.unfold_backward(dcols, F, Pk, dil, (Pk - 1) * dil)
            da = _fn.cln_backward(dv, a, _flat(P[pre + "norm1d.gamma"]), mean1, rstd1, P[pre + "nonlinear1d.weight"], F, teps,
                                  dgamma=_flat(G[pre + "norm1d.gamma"]), dbeta=_flat(G[pre + "norm1d.beta"]), dalpha=G[pre + "nonlinear1d.weight"])[0]
        else:
            x, a, sv1, z, mean2, rstd2, v2 = sv.acts[li]
            dv2 = _fn.heads_backward(v2, P[sp + "output_pointwise_conv1d.weight"] if dual else None, P[sp + "skip_pointwise_conv1d.weight"], None, F,
                                     d_out if dual else None, dS,
                                     dWo=G[sp + "output_pointwise_conv1d.weight"] if dual else None, dbo=G[sp + "output_pointwise_conv1d.bias"] if dual else None,
                                     dWs=G[sp + "skip_pointwise_conv1d.weight"], dbs=G[sp + "skip_pointwise_conv1d.bias"])[0]
            dz = _fn.cln_backward(dv2, z, _flat(P[sp + "norm1d.gamma"]), mean2, rstd2, P[sp + "nonlinear1d.weight"], F, teps,
                                  dgamma=_flat(G[sp + "norm1d.gamma"]), dbeta=_flat(G[sp + "norm1d.beta"]), dalpha=G[sp + "nonlinear1d.weight"])[0]
            da = _fn.cln_depthwise_backward(dz, a, sv1, P[pre + "nonlinear1d.weight"], _flat(P[pre + "norm1d.gamma"]), _flat(P[pre + "norm1d.beta"]), teps, F,
                                            P[sp + "depthwise_conv1d.weight"], dil, (Pk - 1) * dil, True,
                                            dweight=G[sp + "depthwise_conv1d.weight"], dbias=G[sp + "depthwise_conv1d.bias"],
                                            dgamma=_flat(G[pre + "norm1d.gamma"]), dbeta=_flat(G[pre + "norm1d.beta"]), dalpha=G[pre + "nonlinear1d.weight"])[0]
        dx = _fn.pointwise_backward(x, P[pre + "bottleneck_conv1d.weight"], None, None, F, True, da,
                                    dW=G[pre + "bottleneck_conv1d.weight"], db=G[pre + "bottleneck_conv1d.bias"])[0]
        if dual:
            _add(K, dx, d_out)                   # through conv1 + through the residual: autograd's sum of the two, in the same arithmetic
        d_out = dx
        if on_ready is not None and li % X_layers == 0 and li > 0:
            on_ready(li // X_layers)

    # head: bottleneck, first cLN, encoder.  The encoder output collects two gradients: through the norm and through mask * w.
    dxn = _fn.pointwise_backward(sv.xn, P["separator.bottleneck_conv1d.weight"], None, None, F, True, d_out,
                                 dW=G["separator.bottleneck_conv1d.weight"], db=G["separator.bottleneck_conv1d.bias"])[0]
    dw = _fn.cln_backward(dxn, w, _flat(P["separator.norm1d.gamma"]), sv.mean0, sv.rstd0, None, F, eps,
                          dgamma=_flat(G["separator.norm1d.gamma"]), dbeta=_flat(G["separator.norm1d.beta"]))[0]
    n = dw.numel()
    _add(K, dw, dwm)
    if relu:
        dpre = torch.empty_like(dw)
        K.relu_drop_bwd(dw, w, dpre, n, 0.0)     # w = ReLU(pre): no gradient where the encoder output is zero
        dw = dpre
    Fx = torch.empty(B, Cin * L, ldt, **f32)
    K.unfold(mixture, Fx, B, Cin, T_in, L, S, F, ldt, geo.pad_left)
    part, _, ns = _net._wgrad(K, B, F, ldt, 0.0, f32, N, Cin * L, dw, Fx, False)
    K.reduce_slabs([(part, 0, G["encoder.conv1d.weight"], N * Cin * L, ns, N * Cin * L, 0, 1.0)])
    return None
