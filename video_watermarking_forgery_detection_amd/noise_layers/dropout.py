"""Dropout -- mirror of the reference's noise_layers/dropout.py:4-27 (the class the trainers construct: `Dropout()`): keep ratio
r ~ U(keep_min, keep_max) per call, one H x W keep mask (P(keep) = r) shared over batch and channels, noised*m + cover*(1-m).  Ratio and mask
come from the layer's device generator (csrc/noise.hip, wm_dropout_fwd), not numpy: one launch per direction, no mask tensor."""
import torch
import torch.nn as nn

from .. import ops
from ._device_rng import DeviceRng, need_cuda


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, noised, cover, layer):
        y, rec = ops.dropout_fwd(noised, cover, layer.keep_min, layer._span, layer._rng.state_on(noised.device))
        ctx.layer, ctx.rec = layer, rec
        return y

    @staticmethod
    def backward(ctx, g):
        gx, gc = ops.dropout_bwd(g, ctx.layer.keep_min, ctx.layer._span, ctx.rec, want_cover=ctx.needs_input_grad[1])
        return gx, gc, None


class Dropout(nn.Module):
    """Drops random pixels from the noised image and substitutes them with the pixels of the cover image"""
    capturable = True    # the draws come from device state: a step through this layer may be captured, and every replay draws fresh noise
    needs_cover = True

    def __init__(self, keep_ratio_range=(0.5, 1)):
        super(Dropout, self).__init__()
        self.keep_min = keep_ratio_range[0]
        self.keep_max = keep_ratio_range[1]
        self._span = float(torch.tensor(float(self.keep_max) - float(self.keep_min), dtype=torch.float32))
        self.name = "Dropout"
        self._rng = DeviceRng()

    def forward(self, noised_image, cover_image):
        self.name = "Dropout"
        need_cuda(self.name, noised_image, cover_image)
        return _DropoutFn.apply(noised_image, cover_image, self)

    def apply_attack(self, image, cover=None):
        return self.forward(image, cover)

    # explicit (autograd-free) interface used by the training step
    def fwd(self, image, cover=None):
        if cover is None:
            raise ValueError("Dropout mixes in the cover image: fwd(image, cover=...)")
        y, rec = ops.dropout_fwd(image, cover, self.keep_min, self._span, self._rng.state_on(image.device))
        return y, rec

    def bwd(self, ctx, g):
        return ops.dropout_bwd(g, self.keep_min, self._span, ctx)[0]
