"""Gaussian -- mirror of the reference's noise_layers/gaussian.py:4-17: clamp(x + N(mean, stddev), 0, 1), mean / stddev as forward
arguments (0 / 0.05).  The noise comes from the layer's device generator (csrc/noise.hip), generated inside the one launch; the backward
regenerates it and passes the gradient where 0 <= x + n <= 1 (torch.clamp's rule)."""
import torch
import torch.nn as nn

from .. import ops
from ._device_rng import DeviceRng, need_cuda


class _GaussianFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, layer, mean, stddev):
        x = x.float().contiguous()
        y, rec = ops.noise_fwd(ops.NOISE_GAUSS, x, mean, stddev, layer._rng.state_on(x.device))
        ctx.rec, ctx.ms = rec, (mean, stddev)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.noise_bwd(ops.NOISE_GAUSS, g, ctx.ms[0], ctx.ms[1], ctx.rec, x=x)[0], None, None, None


class Gaussian(nn.Module):
    '''Adds random noise to a tensor.'''
    capturable = True    # the draws come from device state: a step through this layer may be captured, and every replay draws fresh noise

    def __init__(self):
        super(Gaussian, self).__init__()
        self.name = "Gaussian"
        self._rng = DeviceRng()

    def forward(self, tensor, cover_image=None, mean=0, stddev=0.05):
        self.name = "Gaussian"
        need_cuda(self.name, tensor)
        return _GaussianFn.apply(tensor, self, float(mean), float(stddev))

    def apply_attack(self, image, cover=None):
        return self.forward(image, cover)

    # explicit (autograd-free) interface used by the training step: the reference's defaults
    def fwd(self, image, cover=None, mean=0, stddev=0.05):
        self.name = "Gaussian"
        ms = (float(mean), float(stddev))
        y, rec = ops.noise_fwd(ops.NOISE_GAUSS, image, ms[0], ms[1], self._rng.state_on(image.device))
        return y, (image, rec, ms)

    def bwd(self, ctx, g):
        x, rec, ms = ctx
        return ops.noise_bwd(ops.NOISE_GAUSS, g, ms[0], ms[1], rec, x=x)[0]
