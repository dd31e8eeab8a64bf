"""Crop -- mirror of the reference's noise_layers/crop.py:8-55 (`forward`): random (numpy RNG) or
`apex`-given rectangle, bilinear resize back to the full frame; returns (image, apex).  The slice and
the interpolation are one gather kernel (the rectangle is an offset into the source planes).

Dropout -- mirror of crop.py:136-147 (the Dropout the reference's noise_layers package exports):
per-element u ~ U[0,1), where(u > prob, cover, image), from the layer's device generator (csrc/noise.hip).

Cropout -- mirror of crop.py:121-134: the image inside a random rectangle of (height_ratio, width_ratio) of the frame, the cover elsewhere
(csrc/gauss_sep.hip: wm_cropout_fwd / wm_cropout_bwd, one selection launch each way).  Two things differ from the reference, on purpose:
its forward calls self.get_random_rectangle_inside, which the class never defines (crop.py:131) -- Crop's method (crop.py:13-30, numpy RNG)
is used; and it writes the rectangle into cover_image in place and returns that tensor -- here the result is a fresh tensor with the same
values and the cover is left untouched.  Importable from this submodule only (noise_layers.crop.Cropout)."""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ._device_rng import DeviceRng, need_cuda


class _CropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rect):
        x = x.float()
        ctx.rect, ctx.hw = rect, (x.shape[2], x.shape[3])
        return ops.resample_fwd(x, rect, (x.shape[2], x.shape[3]), ops.BILINEAR)

    @staticmethod
    def backward(ctx, g):
        return ops.resample_bwd(g.float(), None, ctx.hw, ctx.rect, ops.BILINEAR), None


class Crop(nn.Module):
    def __init__(self):
        super(Crop, self).__init__()
        self.name = "Crop"

    def get_random_rectangle_inside(self, image_shape, height_ratio, width_ratio):
        """crop.py:13-30"""
        image_height, image_width = image_shape[2], image_shape[3]
        remaining_height = int(height_ratio * image_height)
        remaining_width = int(width_ratio * image_width)
        height_start = 0 if remaining_height == image_height else np.random.randint(0, image_height - remaining_height)
        width_start = 0 if remaining_width == image_width else np.random.randint(0, image_width - remaining_width)
        return height_start, height_start + remaining_height, width_start, width_start + remaining_width

    def _apex(self, image, apex, min_rate, max_rate):
        # the ratio draws happen even when apex is given (crop.py:33-40): the RNG stream must advance the same way
        if min_rate:
            self.height_ratio = min_rate + (max_rate - min_rate) * np.random.rand()
            self.width_ratio = min_rate + (max_rate - min_rate) * np.random.rand()
        else:
            self.height_ratio = 0.3 + 0.7 * np.random.rand()
            self.width_ratio = 0.3 + 0.7 * np.random.rand()
        self.height_ratio = min(self.height_ratio, self.width_ratio + 0.2)
        self.width_ratio = min(self.width_ratio, self.height_ratio + 0.2)
        if apex is not None:
            return tuple(int(v) for v in apex)
        return self.get_random_rectangle_inside(image.shape, self.height_ratio, self.width_ratio)

    def forward(self, image, apex=None, min_rate=0.5, max_rate=1.0):
        if not image.is_cuda:
            raise RuntimeError("Crop runs on the HIP path only: move the input to cuda")
        h_start, h_end, w_start, w_end = self._apex(image, apex, min_rate, max_rate)
        rect = (h_start, h_end - h_start, w_start, w_end - w_start)
        return _CropFn.apply(image, rect), (h_start, h_end, w_start, w_end)

    def fwd(self, image, apex=None, min_rate=0.5, max_rate=1.0):
        h_start, h_end, w_start, w_end = self._apex(image, apex, min_rate, max_rate)
        rect = (h_start, h_end - h_start, w_start, w_end - w_start)
        y = ops.resample_fwd(image, rect, (image.shape[2], image.shape[3]), ops.BILINEAR)
        self.last_apex = (h_start, h_end, w_start, w_end)
        return y, (rect, (image.shape[2], image.shape[3]))

    def bwd(self, ctx, g):
        rect, hw = ctx
        return ops.resample_bwd(g, None, hw, rect, ops.BILINEAR)


class _DropFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, cover, layer):
        y, rec = ops.noise_fwd(ops.NOISE_DROP, image, layer._prob, 0.0, layer._rng.state_on(image.device), cover=cover)
        ctx.layer, ctx.rec = layer, rec
        return y

    @staticmethod
    def backward(ctx, g):
        gx, gc = ops.noise_bwd(ops.NOISE_DROP, g, ctx.layer._prob, 0.0, ctx.rec, want_cover=ctx.needs_input_grad[1])
        return gx, gc, None


class Dropout(nn.Module):
    capturable = True    # the draws come from device state: a step through this layer may be captured, and every replay draws fresh noise
    needs_cover = True

    def __init__(self, prob=0.5):
        super(Dropout, self).__init__()
        self.prob = prob
        self._prob = float(torch.tensor(self.prob * 1., dtype=torch.float32))   # rdn > self.prob * 1. compares in f32
        self.name = "Dropout"
        self._rng = DeviceRng()

    def forward(self, image_and_cover):
        image, cover_image = image_and_cover
        need_cuda(self.name, image, cover_image)
        return _DropFn.apply(image, cover_image, self)

    def apply_attack(self, image, cover=None):
        return self.forward([image, cover])

    def fwd(self, image, cover=None):
        if cover is None:
            raise ValueError("Dropout mixes in the cover image: fwd(image, cover=...)")
        return ops.noise_fwd(ops.NOISE_DROP, image, self._prob, 0.0, self._rng.state_on(image.device), cover=cover)

    def bwd(self, ctx, g):
        return ops.noise_bwd(ops.NOISE_DROP, g, self._prob, 0.0, ctx)[0]


class _CropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, cover, rect):
        ctx.rect = rect
        return ops.cropout_fwd(image.float(), cover.float(), rect)

    @staticmethod
    def backward(ctx, g):
        gx, gc = ops.cropout_bwd(g.float(), ctx.rect, want_cover=ctx.needs_input_grad[1])
        return gx, gc, None


class Cropout(nn.Module):
    capturable = False   # the rectangle is drawn on the host (numpy RNG) on every call
    needs_cover = True

    def __init__(self, height_ratio, width_ratio):
        super(Cropout, self).__init__()
        self.height_ratio = height_ratio
        self.width_ratio = width_ratio
        self.name = "Cropout"
        self.last_rect = None

    get_random_rectangle_inside = Crop.get_random_rectangle_inside   # (the reference's Cropout calls this method without defining it)

    def _rect(self, image):
        rect = self.get_random_rectangle_inside(image.shape, self.height_ratio, self.width_ratio)
        if rect[0] >= rect[1] or rect[2] >= rect[3]:
            raise ValueError(f"Cropout: ratios ({self.height_ratio}, {self.width_ratio}) leave an empty rectangle of a "
                             f"{image.shape[2]} x {image.shape[3]} image")
        self.last_rect = rect
        return rect

    def forward(self, image_and_cover):
        image, cover_image = image_and_cover
        if cover_image is None:
            raise ValueError("Cropout mixes in the cover image: forward([image, cover]) / apply_attack(image, cover)")
        need_cuda(self.name, image, cover_image)
        return _CropoutFn.apply(image, cover_image, self._rect(image))

    def apply_attack(self, image, cover=None):
        return self.forward([image, cover])

    def fwd(self, image, cover=None):
        if cover is None:
            raise ValueError("Cropout mixes in the cover image: fwd(image, cover=...)")
        rect = self._rect(image)
        return ops.cropout_fwd(image, cover, rect), rect

    def bwd(self, ctx, g):
        return ops.cropout_bwd(g, ctx)[0]
