"""GF -- mirror of the reference's noise_layers/gaussian_filter.py:5-13: kornia's GaussianBlur2d((k, k), (sigma, sigma)) of the image.

kornia is not a dependency of this package, so its semantics are RESTATED here, not imported: the 1-D taps are exp(-x^2 / (2 sigma^2)) on
x = arange(k) - k // 2, normalised by their sum (kornia.filters.get_gaussian_kernel1d), the 2-D kernel is their outer product, and the border
is reflected (GaussianBlur2d's default border_type='reflect', F.pad(mode='reflect')).  The taps are formed in float64 and rounded once to
float32.  The blur is the separable HIP kernel (csrc/gauss_sep.hip) with the reflected border; its backward folds the gradient of the
reflected halo back onto the interior pixels.  Like torch's reflect padding, the image must be larger than k // 2 in both directions.

Importable from this submodule only (noise_layers.gaussian_filter.GF), as noise_layers.gaussian.Gaussian is."""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ._device_rng import need_cuda

MIN_K, MAX_K = 3, ops.GAUSS_SEP_MAX_K


def kornia_taps(kernel, sigma):
    """kornia's get_gaussian_kernel1d for an odd kernel size, in float64, rounded once to float32 (a list of k Python floats)"""
    x = np.arange(kernel, dtype=np.float64) - kernel // 2
    g = np.exp(-x * x / (2. * float(sigma) ** 2))
    return [float(v) for v in (g / g.sum()).astype(np.float32)]


class _GFFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, taps):
        ctx.taps = taps
        return ops.gauss_sep(x.float(), taps, ops.BORDER_REFLECT)

    @staticmethod
    def backward(ctx, g):
        return ops.gauss_sep_bwd(g.float(), ctx.taps, ops.BORDER_REFLECT), None


class GF(nn.Module):
    capturable = True    # deterministic launches: Hidden.enable_graph may capture a step through this layer

    def __init__(self, sigma, kernel=7):
        super(GF, self).__init__()
        if kernel != int(kernel) or kernel % 2 == 0 or not MIN_K <= kernel <= MAX_K:
            raise NotImplementedError(f"GF: kernel must be odd and in {MIN_K}..{MAX_K} (got {kernel})")
        if not sigma > 0:
            raise ValueError(f"GF: sigma must be positive (got {sigma})")
        self.sigma = float(sigma)
        self.kernel = int(kernel)
        self.name = "GF"
        self._taps = kornia_taps(self.kernel, self.sigma)

    def forward(self, image_and_cover):
        image, cover_image = image_and_cover
        need_cuda(self.name, image)
        return _GFFn.apply(image, self._taps)

    def apply_attack(self, image, cover=None):
        return self.forward([image, cover])

    # explicit (autograd-free) interface used by the training step and Hybrid
    def fwd(self, image):
        return ops.gauss_sep(image, self._taps, ops.BORDER_REFLECT), None

    def bwd(self, ctx, g):
        return ops.gauss_sep_bwd(g, self._taps, ops.BORDER_REFLECT)
