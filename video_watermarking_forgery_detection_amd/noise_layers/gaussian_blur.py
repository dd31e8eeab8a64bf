"""GaussianBlur -- mirror of the reference's noise_layers/gaussian_blur.py:7-56: depthwise k x k,
sigma=2, zero padding (k-1)/2, normalised weights (rebuilt per call in the reference; here they are
kernel arguments).  kernel_size 3, the size the reference's trainers build, is the 3 x 3 stencil with
its nine weights (symmetric, so its backward is the same launch).  Every other odd size up to 15 runs
the separable kernel (csrc/gauss_sep.hip) with the 1-D taps t = g / sum(g), g_i = exp(-(i - (k-1)/2)^2
/ (2 sigma^2)): the reference's 2-D weights, normalised by their 2-D sum, are outer(t, t) in exact
arithmetic (the 1/(2 pi sigma^2) factor cancels)."""
import math

import numpy as np

import torch
import torch.nn as nn

from .. import ops


def _gaussian_weights(kernel_size=3, sigma=2.0):
    """gaussian_blur.py:17-38 evaluated with the same fp32 torch expressions."""
    x_coord = torch.arange(kernel_size)
    x_grid = x_coord.repeat(kernel_size).view(kernel_size, kernel_size)
    y_grid = x_grid.t()
    xy_grid = torch.stack([x_grid, y_grid], dim=-1).float()
    mean = (kernel_size - 1) / 2.
    variance = sigma ** 2.
    k = (1. / (2. * math.pi * variance)) * torch.exp(-torch.sum((xy_grid - mean) ** 2., dim=-1) / (2 * variance))
    return k / torch.sum(k)


MIN_K, MAX_K = 3, ops.GAUSS_SEP_MAX_K


def gaussian_taps(kernel_size, sigma=2.0):
    """the 1-D taps of the k x k blur: formed in float64, rounded once to float32 (a list of k Python floats)"""
    d = np.arange(kernel_size, dtype=np.float64) - (kernel_size - 1) / 2.
    g = np.exp(-d * d / (2. * float(sigma) ** 2))
    return [float(v) for v in (g / g.sum()).astype(np.float32)]


class _SepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, taps, border):
        ctx.taps, ctx.border = taps, border
        return ops.gauss_sep(x.float(), taps, border)

    @staticmethod
    def backward(ctx, g):
        return ops.gauss_sep_bwd(g.float(), ctx.taps, ctx.border), None, None


class _StencilFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w9):
        ctx.w9 = w9
        return ops.stencil3(x.float(), w9)

    @staticmethod
    def backward(ctx, g):
        return ops.stencil3(g.float(), ctx.w9[::-1]), None  # transpose of a correlation = flipped taps


class GaussianBlur(nn.Module):
    capturable = True    # deterministic launches: Hidden.enable_graph may capture a step through this layer

    def __init__(self, kernel_size=3, channels=3):
        super(GaussianBlur, self).__init__()
        if kernel_size != int(kernel_size) or kernel_size % 2 == 0 or not MIN_K <= kernel_size <= MAX_K:
            raise NotImplementedError(f"GaussianBlur: kernel_size must be odd and in {MIN_K}..{MAX_K} (got {kernel_size})")
        kernel_size = int(kernel_size)
        self.kernel_size = kernel_size
        self.channels = channels
        self.name = "G_Blur"
        # 3: the stencil's nine weights, as before; larger: the separable kernel's taps
        self._w9 = _gaussian_weights(kernel_size).flatten().tolist() if kernel_size == 3 else None
        self._taps = gaussian_taps(kernel_size) if kernel_size != 3 else None

    def get_gaussian_kernel(self, kernel_size=3, sigma=2, channels=3):
        return _gaussian_weights(self.kernel_size, sigma)

    def forward(self, tensor, cover_image=None):
        self.name = "GaussianBlur"
        if not tensor.is_cuda:
            raise RuntimeError("GaussianBlur runs on the HIP path only: move the input to cuda")
        if self._taps is not None:
            return _SepFn.apply(tensor, self._taps, ops.BORDER_ZERO)
        return _StencilFn.apply(tensor, self._w9)

    def fwd(self, image):
        self.name = "GaussianBlur"
        if self._taps is not None:
            return ops.gauss_sep(image, self._taps, ops.BORDER_ZERO), None
        return ops.stencil3(image, self._w9), None

    def bwd(self, ctx, g):
        if self._taps is not None:
            return ops.gauss_sep_bwd(g, self._taps, ops.BORDER_ZERO)
        return ops.stencil3(g, self._w9[::-1])
