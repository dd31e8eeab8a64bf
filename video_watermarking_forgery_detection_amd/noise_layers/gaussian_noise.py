"""GN -- mirror of the reference's noise_layers/gaussian_noise.py:6-20: x + N(mean, sqrt(var)), no clamp; forward([image, cover]).
The noise comes from the layer's device generator (csrc/noise.hip) inside the one launch; the gradient is the identity."""
import math

import torch
import torch.nn as nn

from .. import ops
from ._device_rng import DeviceRng, need_cuda


class _GNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, layer):
        return ops.noise_fwd(ops.NOISE_GN, x, layer.mean, layer._sd, layer._rng.state_on(x.device))[0]

    @staticmethod
    def backward(ctx, g):
        return g, None


class GN(nn.Module):
    capturable = True    # the draws come from device state: a step through this layer may be captured, and every replay draws fresh noise

    def __init__(self, var, mean=0):
        super(GN, self).__init__()
        self.var = var
        self.mean = mean
        self._sd = math.sqrt(var)    # var ** 0.5 (gaussian_noise.py:13)
        self.name = "GN"
        self._rng = DeviceRng()

    def forward(self, image_and_cover):
        image, cover_image = image_and_cover
        need_cuda(self.name, image)
        return _GNFn.apply(image, self)

    def apply_attack(self, image, cover=None):
        return self.forward([image, cover])

    def fwd(self, image, cover=None):
        return ops.noise_fwd(ops.NOISE_GN, image, self.mean, self._sd, self._rng.state_on(image.device))[0], None

    def bwd(self, ctx, g):
        return g
