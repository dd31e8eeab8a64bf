"""Torch-CPU restatement of the Dice losses the kernels of csrc/dice.hip compute (the reference's dice_loss.py BinaryDiceLoss / DiceLoss).
Dtype-generic: run at float32 it applies the reference's ops in the reference's order (the CPU tests compare it with the recorded outputs in
tests/golden/dice.npz), run at float64 it is the yardstick of the GPU tests.  The weighted multi-class path, which the reference cannot
run (it reads an attribute it never sets), is stated as its docstring intends: weight[i] multiplies class i's loss.
Also here: the seeded generators of the fixture's inputs and of the 16 x 1 x 256 x 256 case no file stores.  torch and numpy only."""
import numpy as np
import torch

BINARY_SHAPES = ((2, 1, 32, 32), (3, 1, 30, 43))
MULTI_SHAPES = ((2, 4, 32, 32), (4, 3, 64, 64))
BIG_SHAPE = (16, 1, 256, 256)           # C5's mask and prediction
POWERS = (1, 2, 3)
REDUCTIONS = ("mean", "sum", "none")


def binary_dice(predict, target, smooth=1, p=2, reduction="mean"):
    n = predict.shape[0]
    x, y = predict.reshape(n, -1), target.reshape(n, -1)
    num = (x * y).sum(dim=1) + smooth
    den = (x.pow(p) + y.pow(p)).sum(dim=1) + smooth
    loss = 1 - num / den
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    if reduction == "none":
        return loss
    raise Exception("Unexpected reduction {}".format(reduction))


def dice(logits, target, weight=None, ignore_index=None, smooth=1, p=2, reduction="mean"):
    s = torch.softmax(logits, dim=1)
    C = target.shape[1]
    total = 0
    for c in range(C):
        if c == ignore_index:
            continue
        term = binary_dice(s[:, c], target[:, c], smooth, p, reduction)
        if weight is not None:
            term = term * weight[c]
        total = total + term
    return total / C


def grad_of(fn, x, gout=None):
    """d sum(gout * fn(x)) / dx through autograd; gout defaults to ones"""
    x = x.detach().clone().requires_grad_(True)
    v = fn(x)
    g = torch.ones_like(v) if gout is None else torch.as_tensor(gout, dtype=v.dtype).reshape(v.shape)
    (gr,) = torch.autograd.grad(v, x, g)
    return gr


def chain_sigmoid(g, p):
    """the gradient wrt z of a loss whose gradient wrt p = sigmoid(z) is g"""
    return g * p * (1 - p)


def gen_binary(shape, seed, empty=None):
    """pred = sigmoid(2 randn), target = rand < 0.15 (float32); sample `empty` has an all-zero target"""
    g = torch.Generator().manual_seed(seed)
    pred = torch.sigmoid(2 * torch.randn(shape, generator=g))
    target = (torch.rand(shape, generator=g) < 0.15).float()
    if empty is not None:
        target[empty] = 0
    return pred, target


def gen_multi(shape, seed):
    """logits = 2 randn, labels uniform over the classes -> (logits, one-hot float32 target)"""
    g = torch.Generator().manual_seed(seed)
    logits = 2 * torch.randn(shape, generator=g)
    B, C = shape[0], shape[1]
    labels = torch.randint(0, C, (B, 1) + tuple(shape[2:]), generator=g)
    return logits, torch.zeros(shape).scatter_(1, labels, 1)


def big_case():
    return gen_binary(BIG_SHAPE, 4242, empty=5)


def fixture_case(g, name):
    """inputs of a stored case: binary b0, b1 -> (pred, target); multi-class m0, m1 -> (logits, one-hot target)"""
    x = torch.from_numpy(g[name + "_x"])
    if name.startswith("b"):
        return x, torch.from_numpy(g[name + "_t"].astype(np.float32))
    labels = torch.from_numpy(g[name + "_labels"].astype(np.int64))
    return x, torch.zeros(x.shape).scatter_(1, labels, 1)
