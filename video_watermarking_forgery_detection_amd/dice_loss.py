"""dice_loss -- the reference's Dice losses (dice_loss.py:7-96) on the fused HIP kernels of csrc/dice.hip: `make_one_hot(input, num_classes)`,
`BinaryDiceLoss(smooth=1, p=2, reduction='mean')` and `DiceLoss(weight=None, ignore_index=None, **kwargs)`, differentiable under torch
autograd for the prediction.  float32 tensors on the GPU; no CPU path, no host sync, bit-reproducible (no atomics).

    loss_b = 1 - (sum p*t + smooth) / (sum p^p + sum t^p + smooth)        over the flattened sample b, then reduced by `reduction`

Same constructor arguments, assertion messages and `Exception('Unexpected reduction ...')` as the reference.  One deliberate difference:
the reference's weighted DiceLoss cannot run -- its forward reads `self.weights`, an attribute it never sets, and raises AttributeError --
so here `weight[i]` multiplies class i's loss, as its docstring intends.  The multi-class form supports up to 32 classes."""
import torch

from . import ops
from .noise_layers._device_rng import need_cuda


def make_one_hot(input, num_classes):
    """class indices [N, 1, *] (int64) -> one-hot float tensor [N, num_classes, *], built on the CPU like the reference's"""
    shape = list(input.shape)
    shape[1] = num_classes
    return torch.zeros(shape).scatter_(1, input.cpu(), 1)


class _BinaryDiceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, predict, target, smooth, p, reduction):
        a, b = predict.detach().contiguous(), target.detach().contiguous()
        loss, coef = ops.dice_binary_fwd(a, b, smooth, p, reduction)
        ctx.p, ctx.reduction = p, reduction
        ctx.save_for_backward(a, b, coef)
        return loss if reduction == 'none' else loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("BinaryDiceLoss: the gradient wrt the target is not implemented")
        a, b, coef = ctx.saved_tensors
        gout = gout.detach().to(torch.float32).contiguous().reshape(-1)
        g = ops.dice_binary_bwd(a, b, coef, ctx.p, ctx.reduction, gout=gout) if ctx.needs_input_grad[0] else None
        return g, None, None, None, None


class _SoftmaxDiceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, predict, target, weight, ignore_index, smooth, p, reduction):
        a, b = predict.detach().contiguous(), target.detach().contiguous()
        loss, coef = ops.dice_softmax_fwd(a, b, smooth, p, reduction, ignore_index, weight)
        ctx.p, ctx.reduction, ctx.ignore_index = p, reduction, ignore_index
        ctx.save_for_backward(a, b, coef, weight)
        return loss if reduction == 'none' else loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            raise NotImplementedError("DiceLoss: only the gradient wrt the prediction is implemented")
        a, b, coef, weight = ctx.saved_tensors
        gout = gout.detach().to(torch.float32).contiguous().reshape(-1)
        g = None
        if ctx.needs_input_grad[0]:
            g = ops.dice_softmax_bwd(a, b, coef, ctx.p, ctx.reduction, ctx.ignore_index, weight, gout=gout)
        return g, None, None, None, None, None, None


def _check(name, predict, target, reduction):
    if reduction not in ops.DICE_REDUCTIONS:
        raise Exception('Unexpected reduction {}'.format(reduction))
    need_cuda(name, predict, target)
    if predict.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(name + ": float32 tensors expected")


class BinaryDiceLoss(torch.nn.Module):
    """Dice loss of one class.  predict, target: float32 [N, *] of one size; smooth avoids 0/0 (an empty target gives 1 - smooth/den);
    p is the exponent of the denominator's sums; reduction 'mean' / 'sum' (0-dim) or 'none' ([N])"""
    def __init__(self, smooth=1, p=2, reduction='mean'):
        super().__init__()
        self.smooth = smooth
        self.p = p
        self.reduction = reduction

    def forward(self, predict, target):
        assert predict.shape[0] == target.shape[0], "predict & target batch size don't match"
        _check("BinaryDiceLoss", predict, target, self.reduction)
        if predict.numel() != target.numel():
            raise ValueError("BinaryDiceLoss: predict and target must hold the same number of elements")
        return _BinaryDiceFunction.apply(predict, target, float(self.smooth), float(self.p), self.reduction)


class DiceLoss(torch.nn.Module):
    """Multi-class Dice loss: predict float32 logits [N, C, *] (softmax over C is taken inside the kernel), target one-hot of the same shape.
    weight: [C] array / tensor multiplying each class's loss; ignore_index: a class left out of the sum (the sum is still divided by C, as in
    the reference); other keyword arguments go to BinaryDiceLoss (smooth, p, reduction)"""
    def __init__(self, weight=None, ignore_index=None, **kwargs):
        super().__init__()
        self.kwargs = kwargs
        self.weight = weight
        self.ignore_index = ignore_index
        self._binary = BinaryDiceLoss(**kwargs)   # validates the keyword names as the reference's per-call construction does

    def forward(self, predict, target):
        assert predict.shape == target.shape, 'predict & target shape do not match'
        if self.weight is not None:
            assert self.weight.shape[0] == target.shape[1], \
                'Expect weight shape [{}], get[{}]'.format(target.shape[1], self.weight.shape[0])
        b = self._binary
        _check("DiceLoss", predict, target, b.reduction)
        weight = None if self.weight is None else torch.as_tensor(self.weight, dtype=torch.float32).to(predict.device)
        return _SoftmaxDiceFunction.apply(predict, target, weight, self.ignore_index, float(b.smooth), float(b.p), b.reduction)
