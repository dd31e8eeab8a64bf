"""loss -- the reference's `ExclusionLoss(level=3)` and `GradientLoss()` (loss.py:309-360, 413-423) on the fused HIP kernels of
csrc/imgloss.hip, differentiable under torch autograd for every input.  float32 [B,C,H,W] tensors on the GPU; no CPU path, no host sync,
bit-reproducible (no atomics).

    GradientLoss()(a)                = mean |a[..., :-1] - a[..., 1:]| + mean |a[..., :-1, :] - a[..., 1:, :]|
    ExclusionLoss(level)(img1, img2) = (sum gradx terms + sum grady terms) / (level * 9) / 2, a term per level (the images 2 x 2
        average-pooled between levels), direction and channel pair: mean(s1^2 s2^2) ** 0.25 with s = 2 sigmoid(difference) - 1.
        The divisor is 9 whatever C1 * C2 is, as in the reference.  1 <= level <= 3, 1 <= C1, C2 <= 4, H and W >= 2 << (level - 1).

The reference forms the loss from 54 mean reductions over tensors it materialises (several hundred launches under autograd); here the
forward is one fused launch and a finalise, the backward one launch.  ExclusionLoss's helper methods compute_gradient, _all_comb and
get_gradients are NOT carried over: they exist to build those intermediate tensors, which the kernel never writes.
Two deliberate differences: (1) a term whose mean is exactly 0 (a constant image) contributes a zero gradient where the reference's autograd
returns NaN (0 * inf); its forward value is 0 either way.  (2) channel counts may differ (the reference's pair loop then indexes the wrong
image and raises): term i2 * C1 + i1 pairs img1's channel i1 with img2's i2, the reference's order when the counts agree.
Not carried over from that file: StdLoss, ExtendedL1Loss, NonBlurryLoss and the gray losses."""
import torch

from . import ops
from .noise_layers._device_rng import need_cuda


def _check(name, *ts):
    need_cuda(name, *ts)
    for t in ts:
        if t.dtype != torch.float32:
            raise TypeError(name + ": float32 tensors expected")
        if t.dim() != 4:
            raise ValueError(name + ": [B,C,H,W] tensors expected")


class _ExclusionFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, level):
        a, b = img1.detach().contiguous(), img2.detach().contiguous()
        loss, _, coef = ops.exclusion_fwd(a, b, level)
        ctx.level = level
        ctx.save_for_backward(a, b, coef)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        a, b, coef = ctx.saved_tensors
        gout = gout.detach().to(torch.float32).contiguous().reshape(-1)
        g1, g2 = ops.exclusion_bwd(a, b, coef, ctx.level, want=ctx.needs_input_grad[:2], gout=gout)
        return g1, g2, None


class _GradientFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a):
        x = a.detach().contiguous()
        ctx.save_for_backward(x)
        return ops.gradient_loss(x).reshape(())

    @staticmethod
    def backward(ctx, gout):
        (x,) = ctx.saved_tensors
        return ops.gradient_loss_bwd(x, gout=gout.detach().to(torch.float32).contiguous().reshape(-1))


class ExclusionLoss(torch.nn.Module):
    def __init__(self, level=3):
        """Loss on the gradient, based on Zhang et al., Single Image Reflection Separation with Perceptual Losses, CVPR 2018"""
        super().__init__()
        self.level = level

    def forward(self, img1, img2):
        _check("ExclusionLoss", img1, img2)
        return _ExclusionFunction.apply(img1, img2, int(self.level))


class GradientLoss(torch.nn.Module):
    """L1 loss on the gradient of the picture"""
    def forward(self, a):
        _check("GradientLoss", a)
        return _GradientFunction.apply(a)
