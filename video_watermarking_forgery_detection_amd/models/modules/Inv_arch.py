"""models/modules/Inv_arch.py of the reference: the invertible rescaling generator every IRN trainer gets from `define_G` --
`InvRescaleNet` (:240-313), a stack of `HaarDownsampling` (:134-174) and `InvBlockExp` couplings (:55-88) -- and `AttackNet` (:176-238), on
the HIP layer toolkit (glayers.py; csrc/invblock.hip, csrc/inn.hip, csrc/gconv.hip).  Same constructors, the same forward contract on
NCHW f32 tensors, the same state_dict keys (`operations.0.haar_weights`, `operations.1.F.conv1.weight`, `operations_inverse...`).
Between the layers an activation is an NHWC tensor of the toolkit; the modules below take and return those."""
import math

import torch
import torch.nn as nn

from ... import glayers as G
from .Subnet_constructor import DenseBlock


def _need_gpu(x):
    if not x.is_cuda:
        raise RuntimeError("the HIP layer toolkit runs on the GPU only; there is no CPU fallback")


def _haar_weights(channels):
    # :139-152, unscaled (+-1): kept as a frozen parameter so checkpoints round-trip; the kernel (csrc/inn.hip) has these signs built in
    w = torch.ones(4, 1, 2, 2)
    w[1, 0, 0, 1] = -1
    w[1, 0, 1, 1] = -1
    w[2, 0, 1, 0] = -1
    w[2, 0, 1, 1] = -1
    w[3, 0, 1, 0] = -1
    w[3, 0, 0, 1] = -1
    return torch.cat([w] * channels, 0)


class HaarDownsampling(nn.Module):
    """:134-174.  forward(x [B,H,W,cpad(C)]) -> [B,H/2,W/2,cpad(4C)]: the +-1 filters / 4, wavelet k of channel c at channel k*C + c (the
    reference's reshape / transpose); rev: [B,H,W,cpad(4C)] -> [B,2H,2W,cpad(C)] with the unscaled filters.  `last_jac` is the reference's
    host number: elements / 4 * log(1/16) forwards, elements / 4 * log(16) in reverse, elements = C*H*W of the call's input."""

    def __init__(self, channel_in):
        super().__init__()
        self.channel_in = channel_in
        self.haar_weights = nn.Parameter(_haar_weights(channel_in), requires_grad=False)

    def forward(self, x, rev=False, cal_jacobian=False):
        _need_gpu(x)
        C = self.channel_in
        if x.dim() != 4 or x.shape[3] != G.cpad(4 * C if rev else C) or (not rev and (x.shape[1] % 2 or x.shape[2] % 2)):
            raise ValueError(f"HaarDownsampling({C}): rev={rev} got an activation {tuple(x.shape)}")
        if not rev:
            self.elements = C * x.shape[1] * x.shape[2]
            self.last_jac = self.elements / 4 * math.log(1 / 16.)
            return G.haar_down(x, C, 0.25, by_wavelet=True)
        self.elements = 4 * C * x.shape[1] * x.shape[2]
        self.last_jac = self.elements / 4 * math.log(16.)
        return G.haar_up(x, C, 1.0, by_wavelet=True)

    def jacobian(self, x, rev=False):
        return self.last_jac


class InvBlockExp(nn.Module):
    """:55-88 on x [B,H,W,cpad(channel_num)], x1 = the first channel_split_num channels, x2 = the rest:
        rev False: y1 = x1 + F(x2);  s = clamp * (2 sigmoid(H(y1)) - 1);  y2 = x2 * exp(s) + G(y1)
        rev True:  s = clamp * (2 sigmoid(H(x1)) - 1);  y2 = (x2 - G(x1)) / exp(s);  y1 = x1 - F(y2)
    -> cat(y1, y2).  fused=True (the product path): one chan_slice for the first subnet's input and two launches of csrc/invblock.hip, which
    read x in place and write y1 / the block output whole.  fused=False composes the same block from chan_slice / add / coupling(eps=0) /
    chan_cat: the A/B path (tools/bench_invblock.py) and the tests' cross-check.

    jacobian(x, rev) = +-sum(s) / B of the LAST forward, a detached 0-dim f32 device tensor.  sum(s) comes from the affine kernel, which
    forms it only when that forward was called with cal_jacobian=True (InvRescaleNet passes its own flag down); otherwise jacobian()
    raises.  It is NOT differentiable: the reference never back-propagates through it (its trainers only log it)."""

    def __init__(self, subnet_constructor, channel_num, channel_split_num, clamp=1., fused=True):
        super().__init__()
        self.split_len1 = channel_split_num
        self.split_len2 = channel_num - channel_split_num
        self.clamp = clamp
        self.fused = bool(fused)
        self.F = subnet_constructor(self.split_len2, self.split_len1)
        self.G = subnet_constructor(self.split_len1, self.split_len2)
        self.H = subnet_constructor(self.split_len1, self.split_len2)
        self._jac = None

    def forward(self, x, rev=False, cal_jacobian=False):
        _need_gpu(x)
        n1, n2 = self.split_len1, self.split_len2
        if x.dim() != 4 or x.shape[3] != G.cpad(n1 + n2):
            raise ValueError(f"InvBlockExp expects an NHWC activation of {n1 + n2} channels (stride {G.cpad(n1 + n2)}), got {tuple(x.shape)}")
        self._jac = None
        if self.fused:
            if not rev:
                y1 = G.invblock_shift(x, self.F(G.chan_slice(x, n1, n2)), n1, n2, 1.0)
                out, jac = G.invblock_affine(x, self.H(y1), self.G(y1), n1, n2, self.clamp, False, other=y1, want_jac=cal_jacobian)
            else:
                x1 = G.chan_slice(x, 0, n1)
                y2, jac = G.invblock_affine(x, self.H(x1), self.G(x1), n1, n2, self.clamp, True, want_jac=cal_jacobian)
                out = G.invblock_shift(x, self.F(y2), n1, n2, -1.0, other=y2)
            self._jac = jac
            return out
        if cal_jacobian:
            raise NotImplementedError("InvBlockExp(fused=False) has no kernel for sum(s): the Jacobian term comes from the fused path")
        x1, x2 = G.chan_slice(x, 0, n1), G.chan_slice(x, n1, n2)
        if not rev:
            y1 = G.add(x1, self.F(x2))
            y2 = G.coupling(x2, self.H(y1), self.G(y1), self.clamp, 0.0, False)
        else:
            y2 = G.coupling(x2, self.H(x1), self.G(x1), self.clamp, 0.0, True)
            y1 = G.sub(x1, self.F(y2))
        return G.chan_cat(y1, n1, y2, n2)

    def jacobian(self, x, rev=False):
        if self._jac is None:
            raise RuntimeError("InvBlockExp.jacobian: the last forward was not called with cal_jacobian=True")
        total = self._jac.sum() / x.shape[0]
        return -total if rev else total


def _frame(channel_in, down_num, blocks):
    """the reference's layer list: down_num x (HaarDownsampling, then blocks(i, channels))"""
    ops_, c = [], channel_in
    for i in range(down_num):
        ops_.append(HaarDownsampling(c))
        c *= 4
        ops_.extend(blocks(i, c))
    return ops_, c


def _check_image(x, channel_in, down_num):
    _need_gpu(x)
    m = 1 << down_num
    if x.dim() != 4 or x.shape[1] != channel_in or x.shape[2] % m or x.shape[3] % m:
        raise ValueError(f"expected [B,{channel_in},H,W] with H, W multiples of {m}, got {tuple(x.shape)}")


class InvRescaleNet(nn.Module):
    """:240-313: `operations` = down_num x (HaarDownsampling, block_num[i] InvBlockExp(channels, channel_out)), and the reference's
    `with_reverse` second half `operations_inverse`, the same list again, run backwards in the opposite direction.
    forward(x [B,C,H,W] f32) -> [B,C,H,W] f32: operations forwards, then operations_inverse reversed with rev=True;
    forward(y, rev=True): operations_inverse with rev=False, then operations reversed with rev=True -- the exact inverse.
    cal_jacobian=True returns (out, jacobian): the sum of every layer's term, a 0-dim f32 device tensor (not differentiable).
    `dtype`: the compute dtype of the activations between the layers (float32 = the parity path)."""

    def __init__(self, channel_in=3, channel_out=3, subnet_constructor=None, block_num=[8, 8, 8, 8], down_num=2, dtype=torch.float32):
        super().__init__()
        self.dtype = dtype
        self.channel_in, self.down_num = channel_in, down_num
        self.with_reverse = True

        def blocks(i, c):
            return [InvBlockExp(subnet_constructor, c, channel_out) for _ in range(block_num[i])]

        self.operations = nn.ModuleList(_frame(channel_in, down_num, blocks)[0])
        self.operations_inverse = nn.ModuleList(_frame(channel_in, down_num, blocks)[0])

    def forward(self, x, rev=False, cal_jacobian=False):
        _check_image(x, self.channel_in, self.down_num)
        out = G.to_nhwc(x, self.dtype)
        jacobian = 0
        if not rev:
            plan = [(op, False) for op in self.operations] + [(op, True) for op in reversed(self.operations_inverse)]
        else:
            plan = [(op, False) for op in self.operations_inverse] + [(op, True) for op in reversed(self.operations)]
        for op, r in plan:
            out = op(out, r, cal_jacobian)
            if cal_jacobian:
                jacobian = jacobian + op.jacobian(out, r)
        out = G.to_nchw(out, self.channel_in)
        return (out, jacobian) if cal_jacobian else out


class AttackNet(nn.Module):
    """:176-238: InvRescaleNet's frame (down_num = 2, both halves) over four bare DenseBlock(c, c) per level instead of couplings; same
    state_dict keys.  The reference's forward calls every layer without a direction, so its second half would run HaarDownsampling(3) on
    48 channels and cannot execute; here the second half's Haar stages run as synthesis, as InvRescaleNet's do, and the dense blocks are the
    same either way: forward(x [B,C,H,W] f32, rev) -> [B,C,H,W] f32."""

    def __init__(self, channel_in=3, channel_out=3, dtype=torch.float32):
        super().__init__()
        self.dtype = dtype
        self.channel_in, self.down_num = channel_in, 2
        self.with_reverse = True

        def blocks(i, c):
            return [DenseBlock(c, c) for _ in range(4)]

        self.operations = nn.ModuleList(_frame(channel_in, 2, blocks)[0])
        self.operations_inverse = nn.ModuleList(_frame(channel_in, 2, blocks)[0])

    def forward(self, x, rev=False):
        _check_image(x, self.channel_in, self.down_num)
        out = G.to_nhwc(x, self.dtype)
        first, second = (self.operations, self.operations_inverse) if not rev else (self.operations_inverse, self.operations)
        for op in first:
            out = op(out)
        for op in reversed(second):
            out = op(out, True) if isinstance(op, HaarDownsampling) else op(out)
        return G.to_nchw(out, self.channel_in)
