"""Hybrid -- the "HYBRID ATTACKS" block of the reference's video model (models/IRNcrop_model.py:347-373): every child attack runs on every
frame, alpha = softmax(randn(N, K), dim=1) is drawn per frame, and the output is the per-frame mix sum_k alpha[n, k] * child_k(image)[n],
optionally followed by clamp_with_grad + Quantization (:372-373).  The reference's loop body (:369) adds the bare weights and never multiplies
them into attacked_image_k; the mix above is what it means to compute.

The children run through their own fwd / bwd pairs; the mix (and the clamp + quantisation) is one fused launch forwards and one backwards
(csrc/hybrid.hip: wm_mix_fwd / wm_mix_bwd).  The weights are drawn with torch per call, so a step through this layer is not capturable."""
import torch
import torch.nn as nn

from .. import ops
from ._device_rng import call_fwd, need_cuda
from .crop import Crop
from .resize import Resize


class _HybridFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, cover, weights, layer):
        y, ctx.c = layer.fwd(image.float().contiguous(), cover, weights)
        ctx.layer = layer
        return y

    @staticmethod
    def backward(ctx, g):
        return ctx.layer.bwd(ctx.c, g.float().contiguous()), None, None, None


class Hybrid(nn.Module):
    capturable = False   # the weights are drawn with torch on every call

    def __init__(self, layers, quantize=False):
        super(Hybrid, self).__init__()
        layers = list(layers)
        if not 1 <= len(layers) <= ops.MIX_MAX_K:
            raise ValueError(f"Hybrid mixes 1..{ops.MIX_MAX_K} layers, got {len(layers)}")
        for layer in layers:
            if isinstance(layer, Crop):
                raise ValueError("Hybrid cannot mix a Crop: the per-frame mix needs aligned frames")
        self.layers = nn.ModuleList(layers)
        self.quantize = bool(quantize)
        self.name = "Hybrid"
        self.needs_cover = any(getattr(layer, "needs_cover", False) for layer in layers)
        self.last_weights = None

    def forward(self, image, cover=None, weights=None):
        need_cuda(self.name, image, cover, weights)
        return _HybridFn.apply(image, cover, weights, self)

    # explicit (autograd-free) interface used by the training step
    def fwd(self, image, cover=None, weights=None):
        need_cuda(self.name, image, cover, weights)
        N, K = image.shape[0], len(self.layers)
        if weights is None:
            weights = torch.softmax(torch.randn(N, K, device=image.device), dim=1)
        elif tuple(weights.shape) != (N, K):
            raise ValueError(f"Hybrid: weights must be [{N}, {K}], got {tuple(weights.shape)}")
        weights = weights.detach().float().contiguous()
        ys, ctxs = [], []
        for layer in self.layers:
            if isinstance(layer, Resize):
                y, c = layer.fwd(image, resize_ratio=0.7)   # (the fixed arguments of the attack cycle)
            else:
                y, c = call_fwd(layer, image, cover)
            ys.append(y)
            ctxs.append(c)
        self.last_weights = weights
        return ops.mix_fwd(ys, weights, quant=self.quantize), (ctxs, weights)

    def bwd(self, ctx, g):
        """sum_k child_k.bwd(ctx_k, w[:, k] * g); a child whose backward is identically zero (Jpeg: torch.round) is left out of both
        the mix's backward (its w * g is not stored) and the sum"""
        ctxs, weights = ctx
        needs = [not (hasattr(layer, "bwd_is_zero") and layer.bwd_is_zero(c)) for layer, c in zip(self.layers, ctxs)]
        gs = ops.mix_bwd(g, weights, len(self.layers), needs=needs)
        total = None
        for layer, c, gk in zip(self.layers, ctxs, gs):
            if gk is None:
                continue
            gi = layer.bwd(c, gk)
            total = gi if total is None else ops.add_scaled(total, gi)
        return total if total is not None else torch.zeros_like(g)
