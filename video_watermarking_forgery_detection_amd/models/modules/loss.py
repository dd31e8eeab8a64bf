"""models.modules.loss -- the reference's `ReconstructionLoss(losstype='l_char', eps=1e-6)` (models/modules/loss.py:5-22) on the fused HIP
kernels of csrc/imgloss.hip, and its `CWLoss()` and `GANLoss(gan_type)` (:24-42, 77-109) on those of csrc/advloss.hip, differentiable under
torch autograd.  float32 tensors on the GPU; no CPU path, no host sync, bit-reproducible (no atomics).

    forward(x, target, losstype='l_char') = mean over the batch of the per-sample SUM over (C, H, W) of
        l2:      (x - target)^2
        l_char:  sqrt((x - target)^2 + eps)
        l1:      x - target            -- the reference's SIGNED sum: it takes no abs, and neither does this

It is a sum per sample, not a mean: at 3 x 256 x 256 the l2 form is 196,608 x an MSE.  Two quirks of the reference are kept: the call-time
`losstype` decides and the constructor's is only stored; an unknown type prints "reconstruction loss type error!" and returns 0.

    CWLoss()(logits, target, is_targeted, num_classes=1000, kappa=0) = sum_b max(other_b - real_b, kappa) when targeted, otherwise
        sum_b max(real_b - other_b, kappa);  real = logits[b, target_b], other = the row's largest value with the target's slot set to
        -10000 (not -inf).  A SUM over rows.  Gradient: +-1 at the target column and at the column torch.max(x, 1) returns (the lowest
        among equals), 1/2 each where the margin equals kappa exactly, 0 where kappa wins.  A target outside [0, K) is checked on the
        device: it is never used as an index and makes the loss (and that gradient row) NaN -- the reference raises IndexError on the
        host, which here would cost a synchronisation per call (ops.cw_margin(check_target=True) does that check).
    GANLoss(gan_type)(input, target_is_real): gan / ragan = BCE-with-logits against real_label_val / fake_label_val, lsgan = MSE against
        them, wgan-gp = -mean(input) (real) or mean(input).
    SSIM_Loss()(x, y) (:44-74, the same text as loss.py:9-39): the [B,C,H,W] map clamp((1 - SSIM_n / SSIM_d) / 2, 0, 1) of reflect-padded 3 x 3
        box statistics on the kernels of csrc/ssim3.hip -- the one class of the package's loss module, re-exported here.
Not carried over from that file: GradientPenaltyLoss, which needs a second-order backward through the convolutions."""
import torch

from ... import ops
from ...loss import SSIM_Loss, adv_objective  # noqa: F401  (SSIM_Loss: this module exports it too, as the reference's does)
from ...noise_layers._device_rng import need_cuda


class _ReconFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, kind, eps):
        a, b = x.detach().contiguous(), target.detach().contiguous()
        ctx.kind, ctx.eps = kind, eps
        ctx.save_for_backward(a, b)
        return ops.recon_loss_fwd(a, b, kind, eps).reshape(())

    @staticmethod
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        gout = gout.detach().to(torch.float32).contiguous().reshape(-1)
        gx = ops.recon_loss_bwd(a, b, ctx.kind, ctx.eps, gout=gout) if ctx.needs_input_grad[0] else None
        gt = ops.recon_loss_bwd(a, b, ctx.kind, ctx.eps, gout=gout, gscale=-1.0) if ctx.needs_input_grad[1] else None
        return gx, gt, None, None


class ReconstructionLoss(torch.nn.Module):
    def __init__(self, losstype='l_char', eps=1e-6):
        super().__init__()
        self.losstype = losstype     # stored and, as in the reference, never read: forward's own argument decides
        self.eps = eps

    def forward(self, x, target, losstype='l_char'):
        if losstype not in ops.RECON_KINDS:
            print("reconstruction loss type error!")
            return 0
        need_cuda("ReconstructionLoss", x, target)
        if x.dtype != torch.float32 or target.dtype != torch.float32:
            raise TypeError("ReconstructionLoss: float32 tensors expected")
        if x.shape != target.shape:
            raise ValueError("ReconstructionLoss: x and target must have one shape")
        return _ReconFunction.apply(x, target, losstype, float(self.eps))


class _CWFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, is_targeted, kappa):
        a = logits.detach().contiguous()
        ctx.args = (bool(is_targeted), float(kappa))
        ctx.save_for_backward(a, target)
        return ops.cw_margin(a, target, *ctx.args).reshape(())

    @staticmethod
    def backward(ctx, gout):
        a, target = ctx.saved_tensors
        gout = gout.detach().to(torch.float32).contiguous().reshape(-1)
        _, g = ops.cw_margin(a, target, *ctx.args, want_grad=True, gout=gout)
        return g, None, None, None


class CWLoss(torch.nn.Module):
    def __init__(self):
        super().__init__()

    def forward(self, logits, target, is_targeted, num_classes=1000, kappa=0):
        # inputs to the softmax function are called logits.
        # https://arxiv.org/pdf/1608.04644.pdf
        need_cuda("CWLoss", logits, target)
        if logits.dtype != torch.float32 or logits.dim() != 2:
            raise TypeError("CWLoss: float32 logits [B, num_classes] expected")
        if num_classes != logits.shape[1]:
            # (where the reference fails to broadcast target_one_hot [B, num_classes] against logits)
            raise ValueError("CWLoss: num_classes = %d, but logits has %d columns" % (num_classes, logits.shape[1]))
        if target.dim() != 1 or target.shape[0] != logits.shape[0]:
            raise ValueError("CWLoss: target [B] expected, one class index per row of logits")
        return _CWFunction.apply(logits, target.detach().long().contiguous(), is_targeted, kappa)


# Define GAN loss: [vanilla | lsgan | wgan-gp]
class GANLoss(torch.nn.Module):
    def __init__(self, gan_type, real_label_val=1.0, fake_label_val=0.0):
        super().__init__()
        self.gan_type = gan_type.lower()
        self.real_label_val = real_label_val
        self.fake_label_val = fake_label_val
        if self.gan_type == 'gan' or self.gan_type == 'ragan':
            self._objective = "bce_logits"
        elif self.gan_type == 'lsgan':
            self._objective = "mse"
        elif self.gan_type == 'wgan-gp':
            self._objective = None
        else:
            raise NotImplementedError('GAN type [{:s}] is not found'.format(self.gan_type))

    def get_target_label(self, input, target_is_real):
        """the reference's: the boolean itself for wgan-gp, otherwise a tensor like input filled with the label value.  forward does not call
        it: the kernels take the label as a scalar and never read a label tensor"""
        if self.gan_type == 'wgan-gp':
            return target_is_real
        if target_is_real:
            return torch.empty_like(input).fill_(self.real_label_val)
        else:
            return torch.empty_like(input).fill_(self.fake_label_val)

    def forward(self, input, target_is_real):
        if self._objective is None:
            return adv_objective(input, "neg_mean" if target_is_real else "pos_mean")
        return adv_objective(input, self._objective, float(self.real_label_val if target_is_real else self.fake_label_val))
