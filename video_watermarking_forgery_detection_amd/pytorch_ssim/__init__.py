"""pytorch_ssim -- the reference's structural-similarity module (pytorch_ssim/__init__.py:42-73) on the fused HIP kernels of csrc/ssim.hip:
`SSIM(window_size=11, size_average=True)` and `ssim(img1, img2, window_size=11, size_average=True)`, differentiable under torch autograd
for either argument.  11 x 11 Gaussian window (sigma 1.5), zero padding, float32 NCHW images on the GPU; no CPU path, no host sync."""
import torch

from .. import ops
from ..noise_layers._device_rng import need_cuda


class _SSIMFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, size_average):
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        a, b = img1.detach().contiguous(), img2.detach().contiguous()
        if need1:
            val, planes = ops.ssim(a, b, size_average, want_grad=True)
        else:
            val, planes = ops.ssim(a, b, size_average), None
        ctx.size_average = size_average
        ctx.save_for_backward(a, b, planes)
        return val.clone()

    @staticmethod
    def backward(ctx, gout):
        a, b, planes = ctx.saved_tensors
        per_image = not ctx.size_average
        gout = gout.detach().to(torch.float32).contiguous().reshape(-1)
        g1 = g2 = None
        if ctx.needs_input_grad[0]:
            g1 = ops.ssim_bwd(planes, a, b, gout=gout, per_image=per_image)
        if ctx.needs_input_grad[1]:   # S(x, y) = S(y, x): the second image's gradient is the first's of the swapped call
            _, swapped = ops.ssim(b, a, ctx.size_average, want_grad=True)
            g2 = ops.ssim_bwd(swapped, b, a, gout=gout, per_image=per_image)
        return g1, g2, None


def _check(img1, img2, window_size):
    if window_size != 11:
        raise NotImplementedError("SSIM: only the 11 x 11 window the reference's trainers use is implemented (window_size=%r)" % (window_size,))
    need_cuda("SSIM", img1, img2)
    if img1.dtype != torch.float32 or img2.dtype != torch.float32:
        raise TypeError("SSIM: float32 images expected")


def ssim(img1, img2, window_size=11, size_average=True):
    """mean SSIM of the batch (a 0-dim tensor) or, size_average=False, of each image ([B])"""
    _check(img1, img2, window_size)
    return _SSIMFunction.apply(img1, img2, bool(size_average))


class SSIM(torch.nn.Module):
    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        if window_size != 11:
            raise NotImplementedError("SSIM: only the 11 x 11 window the reference's trainers use is implemented (window_size=%r)" % (window_size,))
        self.window_size = window_size
        self.size_average = size_average

    def forward(self, img1, img2):
        return ssim(img1, img2, self.window_size, self.size_average)
