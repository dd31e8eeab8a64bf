"""SaltPepper -- mirror of the reference's noise_layers/salt_pepper_noise.py:5-23: u ~ U[0,1) per element; u > 1 - prob/2 -> 0, then
u < prob/2 -> 1 (in that order); the gradient passes where neither replaced the pixel.  u comes from the layer's device generator
(csrc/noise.hip) inside the one launch; the thresholds are the f32 values torch compares an f32 tensor with."""
import torch
import torch.nn as nn

from .. import ops
from ._device_rng import DeviceRng, need_cuda


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


class _SaltPepperFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, layer):
        y, rec = ops.noise_fwd(ops.NOISE_SP, x, layer._lo, layer._hi, layer._rng.state_on(x.device))
        ctx.layer, ctx.rec = layer, rec
        return y

    @staticmethod
    def backward(ctx, g):
        return ops.noise_bwd(ops.NOISE_SP, g, ctx.layer._lo, ctx.layer._hi, ctx.rec)[0], None


class SaltPepper(nn.Module):
    capturable = True    # the draws come from device state: a step through this layer may be captured, and every replay draws fresh noise

    def __init__(self, prob):
        super(SaltPepper, self).__init__()
        self.prob = prob
        prob_zero = prob / 2
        prob_one = 1 - prob_zero
        self._lo, self._hi = _f32(prob_zero), _f32(prob_one)
        self.name = "SaltPepper"
        self._rng = DeviceRng()

    def forward(self, image):
        need_cuda(self.name, image)
        return _SaltPepperFn.apply(image, self)

    def apply_attack(self, image, cover=None):
        return self.forward(image)

    def fwd(self, image):
        y, rec = ops.noise_fwd(ops.NOISE_SP, image, self._lo, self._hi, self._rng.state_on(image.device))
        return y, rec

    def bwd(self, ctx, g):
        return ops.noise_bwd(ops.NOISE_SP, g, self._lo, self._hi, ctx)[0]
