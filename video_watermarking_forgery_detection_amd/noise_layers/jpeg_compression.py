"""JpegCompression -- mirror of the reference's noise_layers/jpeg_compression.py:65-159, HiDDeN's "JPEG-Drop" attack: zero pad to a
multiple of 8, analog rgb2yuv, unnormalised 8x8 DCT-II, zig-zag keep mask of yuv_keep_weights coefficients per channel, IDCT, yuv2rgb, un-pad.
One launch forward (csrc/jpeg_drop.hip), one backward: the exact transpose of the linear map.  Deterministic."""
import torch
import torch.nn as nn

from .. import ops
from ._device_rng import need_cuda


class _JpegDropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, keep):
        ctx.keep = keep
        return ops.jpeg_drop_fwd(x, keep)

    @staticmethod
    def backward(ctx, g):
        return ops.jpeg_drop_bwd(g, ctx.keep), None


class JpegCompression(nn.Module):
    capturable = True    # the same launch with the same arguments every call: a step through this layer may be captured

    def __init__(self, device=None, yuv_keep_weights=(25, 9, 9)):
        super(JpegCompression, self).__init__()
        self.device = device
        self.yuv_keep_weighs = tuple(int(v) for v in yuv_keep_weights)   # (sic: the reference's attribute name)
        if len(self.yuv_keep_weighs) != 3 or not all(0 <= v <= 64 for v in self.yuv_keep_weighs):
            raise ValueError("yuv_keep_weights: three coefficient counts in [0, 64]")
        self.name = "JpegCompression"

    def forward(self, noised_image):
        need_cuda(self.name, noised_image)
        return _JpegDropFn.apply(noised_image, self.yuv_keep_weighs)

    def apply_attack(self, image, cover=None):
        return self.forward(image)

    def fwd(self, image):
        return ops.jpeg_drop_fwd(image, self.yuv_keep_weighs), None

    def bwd(self, ctx, g):
        return ops.jpeg_drop_bwd(g, self.yuv_keep_weighs)
