"""models.modules.loss -- the reference's `ReconstructionLoss(losstype='l_char', eps=1e-6)` (models/modules/loss.py:5-22) on the fused HIP
kernels of csrc/imgloss.hip, differentiable under torch autograd for both arguments.  float32 tensors on the GPU; no CPU path, no host
sync, bit-reproducible (no atomics).

    forward(x, target, losstype='l_char') = mean over the batch of the per-sample SUM over (C, H, W) of
        l2:      (x - target)^2
        l_char:  sqrt((x - target)^2 + eps)
        l1:      x - target            -- the reference's SIGNED sum: it takes no abs, and neither does this

It is a sum per sample, not a mean: at 3 x 256 x 256 the l2 form is 196,608 x an MSE.  Two quirks of the reference are kept: the call-time
`losstype` decides and the constructor's is only stored; an unknown type prints "reconstruction loss type error!" and returns 0.
Not carried over from that file: CWLoss (needs a target classifier this project does not have) and the other classes."""
import torch

from ... import ops
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
