"""loss -- the reference's `ExclusionLoss(level=3)` and `GradientLoss()` (loss.py:309-360, 413-423) on the fused HIP kernels of
csrc/imgloss.hip, and its `AdversarialLoss(type='nsgan')` (loss.py:41-88) on those of csrc/advloss.hip, differentiable under torch autograd
for every input.  float32 tensors on the GPU; no CPU path, no host sync, bit-reproducible (no atomics).

    AdversarialLoss(type)(outputs, is_real, is_disc=None, mask=None), the reference's branches:
        hinge:  is_disc -> mean relu(1 - outputs) (is_real) or mean relu(1 + outputs);  otherwise (-outputs).mean(), whatever is_real says
        nsgan:  nn.BCELoss()(outputs, labels) on probabilities;  lsgan: nn.MSELoss()(outputs, labels)
                labels = real_label (is_real), fake_label (not is_real, no mask), or with a mask real_label * (1 - mask_down), mask_down the
                mask resized to the outputs' H x W bilinearly (F.upsample: align_corners=False, no antialiasing).  The mask is read only when
                not is_real, it is sampled inside the loss kernel (mask_down is never written), and NO gradient flows to it: the reference's
                own mask is a data tensor.  is_disc is ignored outside hinge, as in the reference.

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

    SSIM_Loss()(x, y)               = clamp((1 - SSIM_n / SSIM_d) / 2, 0, 1), a [B,C,H,W] MAP (loss.py:9-39): both images reflect-padded by 1,
        3 x 3 box means mu, E[x^2], E[y^2], E[xy], C1 = 0.01^2, C2 = 0.03^2.  H, W >= 2.  One launch forwards, one backwards (csrc/ssim3.hip);
        the clamp passes the gradient on its bounds, as torch.clamp.  x is y gives exactly 0.
    ExtendedL1Loss()(a, b, mask)    = mean |mask*a - mask*b| / mean |mask| (loss.py:363-376).  Gradients wrt a and b (sign(0) = 0, as torch's
        L1Loss), none wrt the mask.  A zero mask gives NaN as the reference does: it is not guarded.  The mask broadcasts to a's shape.
    NonBlurryLoss()(x)              = 1 - mean (x - 1/2)^2 (loss.py:379-388)
    GrayLoss()(x)                   = 1 / mean |x - 1/2| (loss.py:403-410)
Not carried over from that file: StdLoss and GrayscaleLoss -- both raise NameError in the reference as written, its `from layers import ...
GrayscaleLayer` being commented out."""
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


class _AdvFunction(torch.autograd.Function):
    """ops.adv_loss under autograd: the forward is the loss alone, the backward ONE launch of the same kernel with the gradient asked for"""
    @staticmethod
    def forward(ctx, x, objective, label, mask, real_label):
        a = x.detach().contiguous()
        ctx.args = (objective, label, mask, real_label)
        ctx.save_for_backward(a)
        return ops.adv_loss(a, objective, label, mask, real_label).reshape(())

    @staticmethod
    def backward(ctx, gout):
        (a,) = ctx.saved_tensors
        objective, label, mask, real_label = ctx.args
        gout = gout.detach().to(torch.float32).contiguous().reshape(-1)
        _, g = ops.adv_loss(a, objective, label, mask, real_label, want_grad=True, gout=gout)
        return g, None, None, None, None


def adv_objective(x, objective, label=None, mask=None, real_label=1.0):
    """ops.adv_loss(x, objective, ...) as a differentiable scalar (the building block of AdversarialLoss and models.modules.loss.GANLoss)"""
    need_cuda("adv_objective", x)
    if x.dtype != torch.float32:
        raise TypeError("adv_objective: float32 tensors expected")
    if mask is not None:
        need_cuda("adv_objective", mask)
        mask = mask.detach().to(torch.float32).contiguous()
    return _AdvFunction.apply(x, objective, label, mask, real_label)


class AdversarialLoss(torch.nn.Module):
    r"""
    Adversarial loss
    https://arxiv.org/abs/1711.10337
    """

    def __init__(self, type='nsgan', target_real_label=1.0, target_fake_label=0.0):
        r"""
        type = nsgan | lsgan | hinge
        """
        super().__init__()
        if type not in ('nsgan', 'lsgan', 'hinge'):
            # (the reference constructs such an object and fails at the first call, with no `criterion`)
            raise ValueError("AdversarialLoss: type must be nsgan, lsgan or hinge, got %r" % (type,))
        self.type = type
        self.register_buffer('real_label', torch.tensor(target_real_label))
        self.register_buffer('fake_label', torch.tensor(target_fake_label))
        # the labels as host numbers: reading the buffers at call time would synchronise.  load_state_dict refreshes them
        self._labels = (float(target_real_label), float(target_fake_label))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._labels = (float(self.real_label), float(self.fake_label))

    def __call__(self, outputs, is_real, is_disc=None, mask=None):
        if self.type == 'hinge':
            if is_disc:
                return adv_objective(outputs, "hinge_disc", -1.0 if is_real else 1.0)
            return adv_objective(outputs, "neg_mean")
        objective = "bce_prob" if self.type == 'nsgan' else "mse"
        real, fake = self._labels
        if is_real:
            return adv_objective(outputs, objective, real)
        if mask is None:
            return adv_objective(outputs, objective, fake)
        return adv_objective(outputs, objective, None, mask, real)


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


class _SSIM3Function(torch.autograd.Function):
    """ops.ssim3_map_fwd under autograd: the backward is ONE launch for the gradients the graph asks for"""
    @staticmethod
    def forward(ctx, x, y):
        a, b = x.detach().contiguous(), y.detach().contiguous()
        ctx.save_for_backward(a, b)
        return ops.ssim3_map_fwd(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return ops.ssim3_map_bwd(a, b, g.detach().to(torch.float32).contiguous(), want=ctx.needs_input_grad[:2])


class SSIM_Loss(torch.nn.Module):
    """Layer to compute the SSIM loss between a pair of images
    """
    def __init__(self):
        super().__init__()
        self.C1 = 0.01 ** 2
        self.C2 = 0.03 ** 2

    def forward(self, x, y):
        _check("SSIM_Loss", x, y)
        if x.shape != y.shape:
            raise ValueError("SSIM_Loss: x and y must have one shape")
        if x.shape[2] < 2 or x.shape[3] < 2:
            raise ValueError("SSIM_Loss: H and W must be at least 2 (ReflectionPad2d(1) needs two pixels)")
        return _SSIM3Function.apply(x, y)


class _PixLossFunction(torch.autograd.Function):
    """the three reductions of csrc/ssim3.hip under autograd: sums + finalise forwards, one launch backwards"""
    @staticmethod
    def forward(ctx, kind, a, b, mask):
        ts = [t.detach().contiguous() for t in (a, b, mask) if t is not None]
        loss, coef = {"masked_l1": ops.extended_l1_fwd, "non_blurry": ops.non_blurry_fwd, "gray": ops.gray_loss_fwd}[kind](*ts)
        ctx.kind = kind
        ctx.save_for_backward(coef, *ts)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        coef, *ts = ctx.saved_tensors
        gout = gout.detach().to(torch.float32).contiguous().reshape(-1)
        if ctx.kind == "masked_l1":
            ga, gb = ops.extended_l1_bwd(*ts, coef, want=ctx.needs_input_grad[1:3], gout=gout)
            return None, ga, gb, None
        bwd = ops.non_blurry_bwd if ctx.kind == "non_blurry" else ops.gray_loss_bwd
        return None, bwd(ts[0], coef, gout=gout), None, None


def _check_any(name, *ts):
    need_cuda(name, *ts)
    for t in ts:
        if t.dtype != torch.float32:
            raise TypeError(name + ": float32 tensors expected")
        if t.numel() == 0:
            raise ValueError(name + ": non-empty tensors expected")


class ExtendedL1Loss(torch.nn.Module):
    """
    also pays attention to the mask, to be relative to its size
    """
    def forward(self, a, b, mask):
        _check_any("ExtendedL1Loss", a, b, mask)
        if a.shape != b.shape:
            raise ValueError("ExtendedL1Loss: a and b must have one shape")
        if mask.shape != a.shape:
            mask = mask.expand_as(a)      # (mean |mask| over the expanded mask is the mean over the mask)
        return _PixLossFunction.apply("masked_l1", a, b, mask.detach())


class NonBlurryLoss(torch.nn.Module):
    def __init__(self):
        """
        Loss on the distance to 0.5
        """
        super().__init__()

    def forward(self, x):
        _check_any("NonBlurryLoss", x)
        return _PixLossFunction.apply("non_blurry", x, None, None)


class GrayLoss(torch.nn.Module):
    def forward(self, x):
        _check_any("GrayLoss", x)
        return _PixLossFunction.apply("gray", x, None, None)
