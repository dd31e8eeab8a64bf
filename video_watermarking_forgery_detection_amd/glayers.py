"""General HIP layer toolkit for the networks either side of the HiDDeN path: nn.Conv2d / nn.ConvTranspose2d /
nn.Linear / the activations / residual and QF-attention combines / global average pooling / symmetric, replication and reflection
padding / spectral norm (of a convolution and of a transposed one), each an autograd Function over the C ABI's wm_gconv_* / wm_unary_* / ... entry points (include/wm_hip.h, "general
layer family").  Parameters keep torch's layouts and names, so a reference state_dict loads unchanged
(models/networks.py:631-749, models/conditional_jpeg_generator.py:40-374,697-826).

Between layers an activation is a contiguous NHWC tensor [B,H,W,Cp] (Cp = channels rounded up to 16, padding channels zero or
ignored) of the network's compute dtype (float32 = the parity path, bfloat16 / float16); images enter and leave as NCHW float32
through `to_nhwc` / `to_nchw`.  There is no CPU or PyTorch fallback: every Function launches HIP kernels.
"""
import math

import torch
import torch.nn as nn
from torch.autograd import Function

from . import ops
from .optim import CapturedStep, FlatAdam, FlatParameters, _flat_grad   # noqa: F401 -- (G.CapturedStep, G.FlatParameters: re-exported)

cpad = ops.cpad


def _pad_bias(bias, n):
    if bias is None:
        return None
    if bias.numel() == n and bias.dtype == torch.float32 and bias.is_contiguous():
        return bias.detach()            # (no padding channels: two launches fewer per call -- the embedder makes ~1,600 such calls a step)
    out = torch.zeros(n, device=bias.device, dtype=torch.float32)
    out[: bias.numel()] = bias.detach()
    return out


_PLAN = None


def set_pack_plan(plan):
    """Route the packed 3x3 weights of plain Conv2d layers through `plan` (ops.PackPlan; None switches it off): a layer's packed
    weight -- forward and transposed orientation -- is then a persistent tensor that ONE launch refreshes for every layer after an
    optimiser step (FlatAdamW.step does it; with another optimiser call plan.refresh() yourself) instead of one small launch per
    layer, call and orientation (2,800 a step in the invertible embedder).  In-place torch writes to a weight (load_state_dict, init)
    are noticed through its autograd version and fall back to a one-off pack until the next refresh."""
    global _PLAN
    _PLAN = plan


def _pack3(weight, rows, cols, dtype, transpose, plan_ok):
    w = weight.detach()
    if _PLAN is not None and plan_ok:
        return _PLAN.get(w, rows, cols, dtype, transpose=transpose)
    return ops.pack_w3x3(w, rows, cols, dtype, transpose=transpose)


def _fast3x3(weight, stride, pad, dtype, out_stride, dil=1):
    """3x3 stride-1 pad-1 undilated convolutions on 16-bit activations whose output stride is a multiple of 32 run on the hot path's
    wave-specialised / streamed-filter kernels (csrc/conv3x3*.hip, wgrad_ws.hip) instead of the general direct kernel"""
    return (dil == 1 and dtype in (torch.bfloat16, torch.float16) and tuple(weight.shape[2:]) == (3, 3) and stride == 1 and pad == 1 and out_stride % 32 == 0)


def _conv_forward(ctx, x, weight, bias, stride, pad, dil=1):
    """the convolution itself + what both autograd nodes below keep for their backward (everything but the saved tensors)"""
    Cout, Cin, KH, KW = weight.shape
    B, IH, IW, KC = x.shape
    if KC != cpad(Cin):
        raise ValueError(f"conv expects {Cin} input channels (stride {cpad(Cin)}), the activation has stride {KC}")
    NC = cpad(Cout)
    OH, OW = (IH + 2 * pad - dil * (KH - 1) - 1) // stride + 1, (IW + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    ctx.geo = (stride, pad, bias is not None)
    ctx.dil = dil
    ctx.plan_ok = isinstance(weight, nn.Parameter)       # (a computed weight -- spectral norm -- is a new tensor every call: never planned)
    ctx.bias_ptr = bias.data_ptr() if bias is not None else 0
    if _fast3x3(weight, stride, pad, x.dtype, NC, dil):
        wp = _pack3(weight, NC, KC, x.dtype, False, ctx.plan_ok)
        out, _ = ops.conv3x3_fwd(x, wp, _pad_bias(bias, NC), None, None, want_stats=False)
        return out
    wp = ops.gconv_pack(weight.detach(), NC, KC, False, x.dtype)
    return ops.gconv_fwd(x, wp, _pad_bias(bias, NC), (OH, OW), KH, KW, stride, pad, dilation=dil)


class _ConvFn(Function):
    """nn.Conv2d on NHWC: weight [Cout,Cin,KH,KW] f32"""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, dil, bias_f64):
        out = _conv_forward(ctx, x, weight, bias, stride, pad, dil)
        ctx.save_for_backward(x, weight)
        ctx.bias_f64 = bias_f64
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        stride, pad, has_bias = ctx.geo
        gx, gw, gb = _conv_backward(x, weight, g.contiguous(), stride, pad, ctx.needs_input_grad[0],
                                    ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]), has_bias, ctx.plan_ok, ctx.bias_ptr, ctx.dil, ctx.bias_f64)
        return gx, gw, gb, None, None, None, None


def _conv_backward(x, weight, g, stride, pad, need_gx, need_gw, want_bias, plan_ok=False, bias_ptr=0, dil=1, bias_f64=False):
    """(gx, gw, gb) of nn.Conv2d for the output gradient g (NHWC, contiguous); gb only if want_bias.  A parameter whose .grad is a view
    of a FlatAdamW buffer gets its gradient ADDED there by the kernel and None returned for it (autograd would otherwise launch one
    add per parameter and contribution: 3,200 a step in the invertible embedder, whose weights all serve twice)."""
    Cout, Cin, KH, KW = weight.shape
    gx = gw = gb = None
    if need_gx:
        if _fast3x3(weight, stride, pad, g.dtype, x.shape[3], dil):
            wt = _pack3(weight, g.shape[3], x.shape[3], g.dtype, True, plan_ok)
            gx, _ = ops.conv3x3_fwd(g, wt, None, None, None, want_stats=False)
        else:
            wt = ops.gconv_pack(weight.detach(), x.shape[3], g.shape[3], True, g.dtype)
            gx = ops.gconv_fwd(g, wt, None, (x.shape[1], x.shape[2]), KH, KW, stride, pad, dgrad=True, dilation=dil)
    if need_gw:
        wacc = _flat_grad(weight.data_ptr(), weight.numel())
        bacc = _flat_grad(bias_ptr, Cout) if want_bias else None
        if wacc is None or (want_bias and bacc is None):
            wacc = bacc = None
        if _fast3x3(weight, stride, pad, g.dtype, 32, dil):      # (the weight-gradient kernels take any 8-multiple of channels)
            gw = wacc.view(Cout, Cin, 3, 3) if wacc is not None else torch.empty(Cout, Cin, 3, 3, device=g.device, dtype=torch.float32)
            ops.conv3x3_wgrad(x, x.shape[3], None, None, g, gw, wacc is not None)
            gb = ops.gcolsum(g, Cout, out_acc=bacc, f64=bias_f64) if want_bias else None
        elif want_bias and bias_f64:     # (the bias gradient summed in double: Conv2d(bias_grad_f64=True))
            gw, _ = ops.gconv_wgrad(g, x, Cout, Cin, KH, KW, stride, pad, want_bias=False, dw_acc=wacc, dilation=dil)
            gb = ops.gcolsum(g, Cout, out_acc=bacc, f64=True)
        else:
            gw, gb = ops.gconv_wgrad(g, x, Cout, Cin, KH, KW, stride, pad, want_bias=want_bias, dw_acc=wacc, db_acc=bacc, dilation=dil)
        if wacc is not None:
            gw = gb = None
    return gx, gw, gb


FUSE_ELU = True   # (tests switch it off to compare with the separate launches)


def _elu_fused(kind, weight, stride, pad, x, dil=1):
    return (FUSE_ELU and dil == 1 and kind == "elu" and tuple(weight.shape[2:]) == (3, 3) and stride == 1 and pad == 1 and weight.shape[0] == 64
            and x.shape[3] == cpad(weight.shape[1]) and ops.conv3x3_fwd_elu_supported(x.shape[3], 64, x.dtype))


class _ConvEluFn(Function):
    """elu(nn.Conv2d(x)) for the 3x3 layers the persistent kernel takes (16-bit activations, 64 output channels, 16 / 32 / 64 input
    channels: the coupling subnets' conv1..conv4, models/invertible_net.py:326-366) in ONE launch forwards -- only the output is kept --
    and TWO + the slab reduction backwards: the input-gradient kernel forms gz = g * elu'(.) from (g, out) while it stages its tiles,
    writes gz for the weight gradient and leaves the bias gradient's partial sums, which the weight gradient's reduction launch folds
    (before: conv, ELU | ELU' + column sums, their reduce, input gradient, weight gradient, its reduce)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        Cout, Cin = weight.shape[0], weight.shape[1]
        ctx.plan_ok = isinstance(weight, nn.Parameter)
        ctx.bias_ptr = bias.data_ptr() if bias is not None else 0
        ctx.has_bias = bias is not None
        wp = _pack3(weight, 64, x.shape[3], x.dtype, False, ctx.plan_ok)
        out = ops.conv3x3_fwd_elu(x, wp, _pad_bias(bias, 64))
        ctx.save_for_backward(x, weight, out)
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, out = ctx.saved_tensors
        Cout, Cin = weight.shape[0], weight.shape[1]
        need_gx, need_gw, need_gb = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        g = g.contiguous()
        if x.shape[3] in (64, 32, 16) and ops.conv3x3_dgrad_elufused_supported(x.shape[3], g.dtype):
            # (16-channel inputs: the filter packed to 32 rows -- the upper 16 zero -- for the 32-channel consumers, which store 16)
            wt = _pack3(weight, 64, max(x.shape[3], 32), g.dtype, True, ctx.plan_ok)
            gx, gz, part = ops.conv3x3_dgrad_elufused(g, out, wt, want_gz=need_gw, dx_stride=x.shape[3])
            gb = None
        else:   # (the 16-channel first layers: their input gradient runs on the general kernel)
            bacc = _flat_grad(ctx.bias_ptr, Cout) if need_gb else None
            gz, gb = ops.unary_bwd_colsum(out, g, "elu_out", Cout, db_acc=bacc)
            gx, gw, _ = _conv_backward(x, weight, gz, 1, 1, need_gx, need_gw, False, ctx.plan_ok)
            return (gx if need_gx else None), gw, (gb if need_gb and bacc is None else None)
        gw = None
        if need_gw or need_gb:
            wacc = _flat_grad(weight.data_ptr(), weight.numel())
            bacc = _flat_grad(ctx.bias_ptr, Cout) if need_gb else None
            if wacc is None or (need_gb and bacc is None):
                wacc = bacc = None
            gw = wacc.view(Cout, Cin, 3, 3) if wacc is not None else torch.empty(Cout, Cin, 3, 3, device=g.device, dtype=torch.float32)
            gb = bacc if bacc is not None else torch.empty(Cout, device=g.device, dtype=torch.float32)
            ops.conv3x3_wgrad_bias(x, gz, gw, wacc is not None, part, gb, bacc is not None)
            if wacc is not None:
                gw = gb = None
            elif not need_gb:
                gb = None
        return (gx if need_gx else None), gw, gb


class _ConvActFn(Function):
    """act(nn.Conv2d(x)) as ONE autograd node: the backward forms gz = g * act'(z) and the bias gradient (its column sums) in one pass
    over the data (ops.unary_bwd_colsum: two launches instead of three, gz not read back), then the convolution's two gradients from gz"""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, dil, kind):
        z = _conv_forward(ctx, x, weight, bias, stride, pad, dil)
        ctx.save_for_backward(x, weight, z)
        ctx.kind = kind
        return ops.unary_fwd(z, kind)

    @staticmethod
    def backward(ctx, g):
        x, weight, z = ctx.saved_tensors
        stride, pad, has_bias = ctx.geo
        bacc = _flat_grad(ctx.bias_ptr, weight.shape[0]) if (has_bias and ctx.needs_input_grad[2]) else None
        gz, gb = ops.unary_bwd_colsum(z, g, ctx.kind, weight.shape[0], db_acc=bacc)
        gx, gw, _ = _conv_backward(x, weight, gz, stride, pad, ctx.needs_input_grad[0], ctx.needs_input_grad[1], False, ctx.plan_ok, dil=ctx.dil)
        return gx, gw, (gb if has_bias and ctx.needs_input_grad[2] and bacc is None else None), None, None, None, None


class _Head2Fn(Function):
    """act(nn.Conv2d(na + nb, Cout, 1)(torch.cat((a[..., :na], b[..., :nb]), channels))) -> NCHW f32 [B,Cout,H,W] as ONE node and one launch
    each way (+ the partial sums' finalise backwards): both NHWC sources are read in place (ops.head2_fwd / head2_bwd), act 0 none, 1 sigmoid;
    weight [Cout, na+nb, 1, 1] f32, Cout <= 4.  The parameter gradients are summed in double and rounded once (Conv2d(bias_grad_f64=True)'s
    convention) and, like _conv_backward's, ADDED into a live FlatAdamW's buffer when both parameters are registered there."""

    @staticmethod
    def forward(ctx, a, na, b, nb, weight, bias, act):
        out = ops.head2_fwd(a, na, b, nb, weight.detach(), bias.detach() if bias is not None else None, act)
        ctx.save_for_backward(a, b, weight, out)
        ctx.meta = (na, nb, act, bias is not None, bias.data_ptr() if bias is not None else 0)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, weight, out = ctx.saved_tensors
        na, nb, act, has_bias, bias_ptr = ctx.meta
        wacc = _flat_grad(weight.data_ptr(), weight.numel()) if ctx.needs_input_grad[4] else None
        bacc = _flat_grad(bias_ptr, weight.shape[0]) if (has_bias and ctx.needs_input_grad[5]) else None
        if wacc is None or bacc is None:
            wacc = bacc = None
        ga, gb, gw, gbias = ops.head2_bwd(a, na, b, nb, weight.detach(), g.contiguous(), out if act == 1 else None, wacc, bacc)
        if wacc is not None:
            gw = gbias = None
        else:
            gw = gw.view_as(weight) if ctx.needs_input_grad[4] else None
            gbias = gbias if (has_bias and ctx.needs_input_grad[5]) else None
        return (ga if ctx.needs_input_grad[0] else None), None, (gb if ctx.needs_input_grad[2] else None), None, gw, gbias, None


class _ConvTFn(Function):
    """nn.ConvTranspose2d on NHWC: weight [Cin,Cout,KH,KW] f32 -- the input gradient of the conv Cout -> Cin with the same filter"""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad):
        Cin, Cout, KH, KW = weight.shape
        B, IH, IW, KC = x.shape
        if KC != cpad(Cin):
            raise ValueError(f"transposed conv expects {Cin} input channels, the activation has stride {KC}")
        NC = cpad(Cout)
        OH, OW = (IH - 1) * stride - 2 * pad + KH, (IW - 1) * stride - 2 * pad + KW
        wt = ops.gconv_pack(weight.detach(), NC, KC, True, x.dtype)
        out = ops.gconv_fwd(x, wt, _pad_bias(bias, NC), (OH, OW), KH, KW, stride, pad, dgrad=True)
        ctx.save_for_backward(x, weight)
        ctx.geo = (stride, pad, bias is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        stride, pad, has_bias = ctx.geo
        Cin, Cout, KH, KW = weight.shape
        g = g.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            wp = ops.gconv_pack(weight.detach(), x.shape[3], g.shape[3], False, g.dtype)
            gx = ops.gconv_fwd(g, wp, None, (x.shape[1], x.shape[2]), KH, KW, stride, pad)
        if ctx.needs_input_grad[1]:
            gw, _ = ops.gconv_wgrad(x, g, Cin, Cout, KH, KW, stride, pad, want_bias=False)
        if has_bias and ctx.needs_input_grad[2]:
            gb = ops.gcolsum(g, Cout)
        return gx, gw, gb, None, None


class _ActFn(Function):
    @staticmethod
    def forward(ctx, x, kind):
        ctx.save_for_backward(x)
        ctx.kind = kind
        return ops.unary_fwd(x, kind)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.unary_bwd(x, g, ctx.kind), None


class _AddFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        return ops.add_scaled(a, b, 1.0)

    @staticmethod
    def backward(ctx, g):
        return g, g


class _SubFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        return ops.add_scaled(a, b, -1.0)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        return g, ops.add_scaled(g, g, -2.0)        # g - 2 g = -g, exactly


class _QFAttFn(Function):
    """x + gamma * res + beta, gamma / beta f32 [B, Cp] (conditional_jpeg_generator.py:196-200)"""

    @staticmethod
    def forward(ctx, x, res, gamma, beta):
        ctx.save_for_backward(res, gamma)
        return ops.qfatt_fwd(x, res, gamma, beta)

    @staticmethod
    def backward(ctx, g):
        res, gamma = ctx.saved_tensors
        gres, gg, gb = ops.qfatt_bwd(g, res, gamma)
        return g, gres, gg, gb


class _PoolFn(Function):
    """AdaptiveAvgPool2d((1,1)) + Flatten: NHWC [B,H,W,Cp] -> f32 [B,1,1,Cp]"""

    @staticmethod
    def forward(ctx, x):
        ctx.meta = (tuple(x.shape), x.dtype)
        return ops.gpool_fwd(x).view(x.shape[0], 1, 1, x.shape[3])

    @staticmethod
    def backward(ctx, g):
        shape, dtype = ctx.meta
        return ops.gpool_bwd(g.reshape(shape[0], shape[3]), shape, dtype)


class _ToNHWC(Function):
    @staticmethod
    def forward(ctx, img, pads, mode, dtype):
        ctx.meta = (tuple(img.shape), pads, mode)
        return ops.pad_nchw_to_nhwc(img, pads, mode, dtype)

    @staticmethod
    def backward(ctx, g):
        shape, pads, mode = ctx.meta
        return ops.pad_nchw_to_nhwc_bwd(g, shape, pads, mode), None, None, None


class _ToNCHW(Function):
    @staticmethod
    def forward(ctx, x, C, H, W):
        ctx.meta = (tuple(x.shape), x.dtype)
        return ops.gunpack_nchw(x, C, H, W)

    @staticmethod
    def backward(ctx, g):
        shape, dtype = ctx.meta
        return ops.gunpack_nchw_bwd(g, shape, dtype), None, None, None


class _SpectralNormFn(Function):
    @staticmethod
    def forward(ctx, weight_orig, u, v, do_iter):
        wsn, sigma = ops.spectral_norm_fwd(weight_orig.detach(), u, v, do_iter)
        ctx.save_for_backward(wsn, u.clone(), v.clone(), sigma)
        return wsn

    @staticmethod
    def backward(ctx, g):
        wsn, u, v, sigma = ctx.saved_tensors
        return ops.spectral_norm_bwd(g, wsn, u, v, sigma), None, None, None


class _ReflectPadFn(Function):
    """nn.ReflectionPad2d(p) on NHWC; the backward gathers the <= 9 padded positions of every pixel (ops.reflect_pad_bwd)"""

    @staticmethod
    def forward(ctx, x, pad):
        ctx.pad = pad
        return ops.reflect_pad_fwd(x, pad)

    @staticmethod
    def backward(ctx, g):
        return ops.reflect_pad_bwd(g.contiguous(), ctx.pad), None


def to_nhwc(img, dtype, pads=(0, 0, 0, 0), mode=ops.PAD_SYMMETRIC):
    """NCHW f32 image -> NHWC activation, optionally padded (left, right, top, bottom) symmetrically or by replication"""
    if not img.is_cuda:
        raise RuntimeError("the HIP layer toolkit runs on the GPU only; there is no CPU fallback")
    return _ToNHWC.apply(img, tuple(int(p) for p in pads), mode, dtype)


def to_nchw(x, C, H=None, W=None):
    """NHWC activation -> NCHW f32 [B,C,H,W] (the top-left window when H / W are smaller than the activation's)"""
    return _ToNCHW.apply(x, C, x.shape[1] if H is None else H, x.shape[2] if W is None else W)


def add(a, b):
    return _AddFn.apply(a, b)


def sub(a, b):
    return _SubFn.apply(a, b)


def qf_attention(x, res, gamma, beta):
    B, Cp = x.shape[0], x.shape[3]
    return _QFAttFn.apply(x, res, gamma.reshape(B, -1).float(), beta.reshape(B, -1).float())


def global_avg_pool(x):
    return _PoolFn.apply(x)


def _kaiming_uniform_(w, fan_in):
    # torch's default reset_parameters of Conv2d / Linear: kaiming_uniform_(a=sqrt(5)) = U(-1/sqrt(fan_in), 1/sqrt(fan_in))
    bound = 1.0 / math.sqrt(fan_in) if fan_in > 0 else 0.0
    with torch.no_grad():
        w.uniform_(-bound, bound)


class Conv2d(nn.Module):
    """nn.Conv2d(in, out, k, stride, padding, dilation=dilation, bias=bias) on NHWC activations; parameters `weight` [out,in,k,k],
    `bias` [out].  dilation > 1 needs stride 1.  bias_grad_f64: the bias gradient (a sum over every pixel of the output gradient) is
    accumulated in double and rounded once -- for a network's output layer, whose few channels receive the loss gradient itself"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, dilation=1, bias_grad_f64=False):
        super().__init__()
        self.bias_grad_f64 = bool(bias_grad_f64)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = int(kernel_size), int(stride), int(padding), int(dilation)
        if self.dilation < 1 or (self.dilation > 1 and self.stride != 1):
            raise ValueError(f"Conv2d: dilation {dilation} with stride {stride} is not supported (dilation >= 1, and stride 1 when it is > 1)")
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, self.kernel_size, self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        fan_in = in_channels * self.kernel_size ** 2
        _kaiming_uniform_(self.weight, fan_in)
        if bias:
            _kaiming_uniform_(self.bias, fan_in)

    def effective_weight(self):
        return self.weight

    def forward(self, x):
        return _ConvFn.apply(x, self.effective_weight(), self.bias, self.stride, self.padding, self.dilation, self.bias_grad_f64)


class SpectralNormConv2d(Conv2d):
    """nn.utils.spectral_norm(nn.Conv2d(..)) (networks.py:1381-1385): parameters `weight_orig`, buffers `weight_u`, `weight_v`,
    one power iteration per training forward, none in eval."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, dilation=1):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias, dilation)
        w = self.weight
        del self._parameters["weight"]
        self.weight_orig = nn.Parameter(w.data)
        n = in_channels * self.kernel_size ** 2
        self.register_buffer("weight_u", nn.functional.normalize(torch.randn(out_channels), dim=0, eps=1e-12))
        self.register_buffer("weight_v", nn.functional.normalize(torch.randn(n), dim=0, eps=1e-12))

    def effective_weight(self):
        return _SpectralNormFn.apply(self.weight_orig, self.weight_u, self.weight_v, self.training)


class ConvAct(nn.Module):
    """nn.Sequential(conv, activation) with the state_dict keys of that Sequential (`0.weight`, `0.bias`) and one autograd node for the
    pair (_ConvActFn); `conv` is a Conv2d / SpectralNormConv2d of this module"""

    def __init__(self, conv, kind):
        super().__init__()
        if kind not in ops.ACT_KINDS:
            raise ValueError(f"unknown activation {kind}")
        self.add_module("0", conv)
        self.kind = kind

    def __getitem__(self, i):
        if i != 0:
            raise IndexError(i)
        return self._modules["0"]

    def forward(self, x):
        c = self._modules["0"]
        w = c.effective_weight()
        if _elu_fused(self.kind, w, c.stride, c.padding, x, c.dilation):
            return _ConvEluFn.apply(x, w, c.bias)
        return _ConvActFn.apply(x, w, c.bias, c.stride, c.padding, c.dilation, self.kind)

    def extra_repr(self):
        return self.kind


class FusedSequential(nn.Sequential):
    """nn.Sequential with the same children and state_dict keys whose forward runs every (Conv2d, Act) neighbour pair as one autograd
    node (_ConvActFn): the activation's backward and the convolution's bias gradient become one pass over the data.  Any other child
    (a ReflectionPad2d between two pairs, a transposed convolution, a convolution with no activation behind it) runs as itself"""

    def forward(self, x):
        mods = list(self._modules.values())
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, Conv2d) and i + 1 < len(mods) and isinstance(mods[i + 1], Act):
                w = m.effective_weight()
                if _elu_fused(mods[i + 1].kind, w, m.stride, m.padding, x, m.dilation):
                    x = _ConvEluFn.apply(x, w, m.bias)
                else:
                    x = _ConvActFn.apply(x, w, m.bias, m.stride, m.padding, m.dilation, mods[i + 1].kind)
                i += 2
            else:
                x = m(x)
                i += 1
        return x


class ConvTranspose2d(nn.Module):
    """nn.ConvTranspose2d(in, out, k, stride, padding, bias); `weight` [in,out,k,k]"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = int(kernel_size), int(stride), int(padding)
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels, self.kernel_size, self.kernel_size))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        fan_in = out_channels * self.kernel_size ** 2      # torch computes fan_in from dim 1 of the weight
        _kaiming_uniform_(self.weight, fan_in)
        if bias:
            _kaiming_uniform_(self.bias, fan_in)

    def effective_weight(self):
        return self.weight

    def forward(self, x):
        return _ConvTFn.apply(x, self.effective_weight(), self.bias, self.stride, self.padding)


class SpectralNormConvTranspose2d(ConvTranspose2d):
    """nn.utils.spectral_norm(nn.ConvTranspose2d(..)) (networks.py:991,1000).  torch normalises a transposed convolution over dim 1: the
    matrix is weight_orig.permute(1,0,2,3).reshape(out, -1), so `weight_u` has `out` elements and `weight_v` in * k * k; parameter
    `weight_orig` [in,out,k,k]; one power iteration per training forward, none in eval (the kernels of SpectralNormConv2d on that view)"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias)
        w = self.weight
        del self._parameters["weight"]
        self.weight_orig = nn.Parameter(w.data)
        n = in_channels * self.kernel_size ** 2
        self.register_buffer("weight_u", nn.functional.normalize(torch.randn(out_channels), dim=0, eps=1e-12))
        self.register_buffer("weight_v", nn.functional.normalize(torch.randn(n), dim=0, eps=1e-12))

    def effective_weight(self):
        mat = self.weight_orig.permute(1, 0, 2, 3).contiguous()          # [out, in, k, k]: rows = dim 1 of the parameter
        return _SpectralNormFn.apply(mat, self.weight_u, self.weight_v, self.training).permute(1, 0, 2, 3)


class ReflectionPad2d(nn.Module):
    """nn.ReflectionPad2d(p) on NHWC activations (the same p on all four sides, p <= min(H, W) - 1)"""

    def __init__(self, padding):
        super().__init__()
        self.padding = int(padding)
        if self.padding < 0:
            raise ValueError(f"ReflectionPad2d: negative padding {padding}")

    def forward(self, x):
        return _ReflectPadFn.apply(x, self.padding)

    def extra_repr(self):
        return str(self.padding)


class Linear(nn.Module):
    """nn.Linear on [B,1,1,Cp] activations or on every token of a [B,H,W,Cp] grid (a 1x1 convolution either way); `weight` [out,in],
    `bias` [out]"""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        _kaiming_uniform_(self.weight, in_features)
        if bias:
            _kaiming_uniform_(self.bias, in_features)

    def forward(self, x):
        return _ConvFn.apply(x, self.weight.view(self.out_features, self.in_features, 1, 1), self.bias, 1, 0, 1, False)


class Act(nn.Module):
    """ReLU / LeakyReLU(0.2) / GELU / ELU / Sigmoid / Tanh"""

    def __init__(self, kind):
        super().__init__()
        if kind not in ops.ACT_KINDS:
            raise ValueError(f"unknown activation {kind}")
        self.kind = kind

    def forward(self, x):
        return _ActFn.apply(x, self.kind)

    def extra_repr(self):
        return self.kind


class _InstanceNormFn(Function):
    """act(nn.InstanceNorm2d(x)) as one node: the forward keeps x and the f32 statistics [B,Cp] (not xhat, not the output); the backward
    recomputes xhat and the ReLU mask from them (ops.instnorm_bwd)"""

    @staticmethod
    def forward(ctx, x, weight, bias, C, eps, act):
        gamma = weight.detach().contiguous() if weight is not None else None
        beta = bias.detach().contiguous() if bias is not None else None
        y, mean, rstd = ops.instnorm_fwd(x, C, eps, gamma, beta, act)
        ctx.save_for_backward(x, mean, rstd, gamma, beta)
        ctx.meta = (C, act)
        return y

    @staticmethod
    def backward(ctx, g):
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        C, act = ctx.meta
        dx, dgamma, dbeta = ops.instnorm_bwd(x, g, C, mean, rstd, gamma, beta, act, want_params=ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        return (dx if ctx.needs_input_grad[0] else None), (dgamma if ctx.needs_input_grad[1] else None), \
            (dbeta if ctx.needs_input_grad[2] else None), None, None, None


class InstanceNorm2d(nn.Module):
    """nn.InstanceNorm2d(num_features, eps, momentum, affine, track_running_stats=False) on NHWC activations, optionally with the ReLU
    the reference puts behind it (act="relu": one launch fewer each way, and no second activation kept for the backward).  Every
    (sample, channel) plane is normalised with its own biased statistics, in training and in eval alike -- torch's behaviour without
    running statistics, which this layer does not have (track_running_stats=True raises; the reference never sets it; `momentum` is
    accepted and unused).  state_dict: `weight`, `bias` [num_features] when affine (ones / zeros at first), nothing otherwise."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=False, track_running_stats=False, act=None):
        super().__init__()
        if track_running_stats:
            raise NotImplementedError("InstanceNorm2d: track_running_stats=True (running statistics) is not implemented")
        if act not in ops.INSTNORM_ACTS:
            raise ValueError(f"InstanceNorm2d: act {act!r} (None or 'relu')")
        self.num_features, self.eps, self.momentum = int(num_features), float(eps), momentum
        self.affine, self.track_running_stats, self.act = bool(affine), False, act
        self.weight = nn.Parameter(torch.ones(self.num_features)) if self.affine else None
        self.bias = nn.Parameter(torch.zeros(self.num_features)) if self.affine else None

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("the HIP layer toolkit runs on the GPU only; there is no CPU fallback")
        if x.dim() != 4 or x.shape[3] != cpad(self.num_features):
            raise ValueError(f"InstanceNorm2d expects an NHWC activation of {self.num_features} channels (stride {cpad(self.num_features)}), got {tuple(x.shape)}")
        B, H, W, _ = x.shape
        if H * W == 1:      # (torch's _verify_spatial_size; it checks whenever the input's own statistics are used: always, here)
            raise ValueError(f"Expected more than 1 spatial element when training, got input size {torch.Size([B, self.num_features, H, W])}")
        return _InstanceNormFn.apply(x, self.weight, self.bias, self.num_features, self.eps, self.act)

    def extra_repr(self):
        return f"{self.num_features}, eps={self.eps}, affine={self.affine}" + (f", act={self.act}" if self.act else "")


class _LayerNormFn(Function):
    """nn.LayerNorm over the channels of every token: the forward keeps x and the f32 statistics per token; the backward recomputes xhat"""

    @staticmethod
    def forward(ctx, x, weight, bias, C, eps):
        gamma, beta = weight.detach().contiguous(), bias.detach().contiguous()
        y, mean, rstd = ops.layernorm_fwd(x, C, gamma, beta, eps)
        ctx.save_for_backward(x, mean, rstd, gamma)
        ctx.C = C
        return y

    @staticmethod
    def backward(ctx, g):
        x, mean, rstd, gamma = ctx.saved_tensors
        dx, dgamma, dbeta = ops.layernorm_bwd(x, g, ctx.C, gamma, mean, rstd, want_params=ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        return (dx if ctx.needs_input_grad[0] else None), (dgamma if ctx.needs_input_grad[1] else None), \
            (dbeta if ctx.needs_input_grad[2] else None), None, None


class LayerNorm(nn.Module):
    """nn.LayerNorm(C, eps) (affine) over the channels of every token of a [B,H,W,Cp] grid; parameters `weight`, `bias` [C]"""

    def __init__(self, normalized_shape, eps=1e-5):
        super().__init__()
        if not isinstance(normalized_shape, int):
            (normalized_shape,) = normalized_shape
        self.normalized_shape, self.eps = (int(normalized_shape),), float(eps)
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("the HIP layer toolkit runs on the GPU only; there is no CPU fallback")
        C = self.normalized_shape[0]
        if x.dim() != 4 or x.shape[3] != cpad(C):
            raise ValueError(f"LayerNorm expects a token grid [B,H,W,{cpad(C)}] of {C} channels, got {tuple(x.shape)}")
        return _LayerNormFn.apply(x, self.weight, self.bias, C, self.eps)

    def extra_repr(self):
        return f"{self.normalized_shape}, eps={self.eps}"


class _WindowAttentionFn(Function):
    """the Swin attention core as one node over two launches; keeps qkv, the table and the row log-sum-exp"""

    @staticmethod
    def forward(ctx, qkv, table, C, num_heads, ws, shift, scale):
        tbl = table.detach().contiguous()
        out, lse = ops.winattn_fwd(qkv, tbl, C, num_heads, ws, shift, scale)
        ctx.save_for_backward(qkv, tbl, lse)
        ctx.meta = (C, num_heads, ws, shift, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        qkv, tbl, lse = ctx.saved_tensors
        g_qkv, g_table = ops.winattn_bwd(g, qkv, tbl, lse, *ctx.meta)
        return (g_qkv if ctx.needs_input_grad[0] else None), (g_table if ctx.needs_input_grad[1] else None), None, None, None, None, None


def window_attention(qkv, table, num_heads, ws, shift, scale, H, W, dim=None):
    """softmax(scale q k^T + table[relative index] + shifted-window mask) v per (ws x ws window of the grid rolled by -shift, head), written
    back at the tokens' own grid positions.  qkv [B,H,W,cpad(3C)]: the qkv Linear's output on the un-partitioned grid, channels in the
    reference's reshape(B_, N, 3, nH, hd) order; table f32 [(2ws-1)^2, nH] -> [B,H,W,cpad(C)].  dim = C; it may be left out only when the
    stride says it (3C a multiple of 16)"""
    if not qkv.is_cuda:
        raise RuntimeError("the HIP layer toolkit runs on the GPU only; there is no CPU fallback")
    if qkv.dim() != 4 or tuple(qkv.shape[1:3]) != (H, W):
        raise ValueError(f"window_attention expects a [B,{H},{W},Cp] grid, got {tuple(qkv.shape)}")
    if dim is None:
        if qkv.shape[3] % 3:
            raise ValueError(f"window_attention: a qkv stride of {qkv.shape[3]} does not say how many channels it holds; pass dim")
        dim = qkv.shape[3] // 3
    return _WindowAttentionFn.apply(qkv, table, int(dim), int(num_heads), int(ws), int(shift), float(scale))


class GlobalAvgPool(nn.Module):
    """torch.nn.AdaptiveAvgPool2d((1,1)); the result is f32 [B,1,1,Cp] and stays f32 through the Linear layers after it"""

    def forward(self, x):
        return global_avg_pool(x)


class Flatten(nn.Module):
    """torch.nn.Flatten after the pool: nothing to do on [B,1,1,Cp]; keeps the reference's Sequential indices"""

    def forward(self, x):
        return x


def vector_in(v, dtype=torch.float32):
    """[B,F] f32 -> [B,1,1,cpad(F)] activation (the input of a Linear stack)"""
    if not v.is_cuda:
        raise RuntimeError("the HIP layer toolkit runs on the GPU only; there is no CPU fallback")
    B, F = v.shape
    return to_nhwc(v.reshape(B, F, 1, 1).float(), dtype)


def vector_out(x, F):
    """[B,1,1,Cp] -> [B,F] f32"""
    return to_nchw(x, F, 1, 1).reshape(x.shape[0], F)


# ----------------------------------------------------------------------------- invertible-embedder pieces (models/invertible_net.py)
class _HaarFn(Function):
    @staticmethod
    def forward(ctx, x, C, fac, up, by_wavelet=False):
        ctx.meta = (C, fac, up, by_wavelet)
        return ops.haar(x, C, fac, up, by_wavelet)

    @staticmethod
    def backward(ctx, g):
        C, fac, up, by_wavelet = ctx.meta
        return ops.haar(g.contiguous(), C, fac, not up, by_wavelet), None, None, None, None


class _ChanSliceFn(Function):
    """x[..., off:off+n] as its own NHWC tensor (stride cpad(n), padding zero); one launch each way (ops.chan_place)"""

    @staticmethod
    def forward(ctx, x, off, n):
        ctx.meta = (x.shape[3], off, n)
        return ops.chan_place(cpad(n), x, off, 0, n)

    @staticmethod
    def backward(ctx, g):
        stride, off, n = ctx.meta
        return ops.chan_place(stride, g.contiguous(), 0, off, n), None, None


class _ChanCatFn(Function):
    """torch.cat((a[..., :na], b[..., :nb]), channel dim)"""

    @staticmethod
    def forward(ctx, a, na, b, nb):
        ctx.meta = (na, nb)
        return ops.chan_place(cpad(na + nb), a, 0, 0, na, b, 0, na, nb)

    @staticmethod
    def backward(ctx, g):
        na, nb = ctx.meta
        g = g.contiguous()
        return ops.chan_place(cpad(na), g, 0, 0, na), None, ops.chan_place(cpad(nb), g, na, 0, nb), None


class _CouplingFn(Function):
    """rev False: e(s) * x + t; rev True: (x - t) / e(s)   (invertible_net.py:140-141,153-173)"""

    @staticmethod
    def forward(ctx, x, s, t, clamp, eps, rev):
        y = ops.coupling_fwd(x, s, t, clamp, eps, rev)
        ctx.save_for_backward(y if rev else x, s)
        ctx.meta = (clamp, eps, rev)
        return y

    @staticmethod
    def backward(ctx, g):
        v, s = ctx.saved_tensors
        clamp, eps, rev = ctx.meta
        gx, gs, gt = ops.coupling_bwd(g, v, s, clamp, eps, rev)
        return gx, gs, gt, None, None, None


def haar_down(x, C, fac, by_wavelet=False):
    return _HaarFn.apply(x, C, float(fac), False, bool(by_wavelet))


def haar_up(x, C, fac, by_wavelet=False):
    return _HaarFn.apply(x, C, float(fac), True, bool(by_wavelet))


def chan_slice(x, off, n):
    return _ChanSliceFn.apply(x, off, n)


def chan_cat(a, na, b, nb):
    return _ChanCatFn.apply(a, na, b, nb)


def coupling(x, s, t, clamp, eps, rev):
    return _CouplingFn.apply(x, s, t, float(clamp), float(eps), bool(rev))


# ----------------------------------------------------------------------------- InvBlockExp couplings (models/modules/Inv_arch.py)
class _InvShiftFn(Function):
    """x[..., :n1] + sign * f, alone or as cat(that, other[..., :n2]); x is the block's whole input, read in place (ops.invblock_shift_fwd).
    The backward is one launch: gx at x's width (zero outside the first n1 channels), gf, gother"""

    @staticmethod
    def forward(ctx, x, f, other, n1, n2, sign):
        ctx.meta = (n1, n2, sign, other is not None, x.shape[3])
        return ops.invblock_shift_fwd(x, f, n1, n2, sign, other)

    @staticmethod
    def backward(ctx, g):
        n1, n2, sign, whole, xstride = ctx.meta
        gx, gf, gother = ops.invblock_shift_bwd(g.contiguous(), n1, n2, sign, whole, xstride)
        return gx, gf, gother, None, None, None


class _InvAffineFn(Function):
    """rev False: x[..., n1:n1+n2] * exp(s) + g, rev True: (.. - g) / exp(s), s = clamp * (2 sigmoid(h) - 1), alone or as
    cat(other[..., :n1], that) (ops.invblock_affine_fwd) -> (out, jac); jac = sum of s per sample, f32 [B] (None unless want_jac), is not
    differentiable.  Saved for the backward, as _CouplingFn does: x for rev False, the output for rev True; and h"""

    @staticmethod
    def forward(ctx, x, h, g, other, n1, n2, clamp, rev, want_jac):
        out, jac = ops.invblock_affine_fwd(x, h, g, n1, n2, clamp, rev, other, want_jac)
        whole = other is not None
        ctx.save_for_backward(out if rev else x, h)
        ctx.meta = (n1, n2, clamp, rev, whole, x.shape[3])
        if jac is not None:
            ctx.mark_non_differentiable(jac)
        return out, jac

    @staticmethod
    def backward(ctx, gout, _gjac):
        v, h = ctx.saved_tensors
        n1, n2, clamp, rev, whole, xstride = ctx.meta
        voff = n1 if (not rev or whole) else 0
        gx, gh, gg, gother = ops.invblock_affine_bwd(gout.contiguous(), v, voff, h, n1, n2, clamp, rev, whole, xstride)
        return gx, gh, gg, gother, None, None, None, None, None


def invblock_shift(x, f, n1, n2, sign=1.0, other=None):
    """InvBlockExp's additive half on the block's whole input x [B,H,W,cpad(n1+n2)]: x1 + sign * f [.., cpad(n1)], or with `other`
    [.., cpad(n2)] the whole block output cat(x1 + sign * f, other)"""
    return _InvShiftFn.apply(x, f, other, int(n1), int(n2), float(sign))


def invblock_affine(x, h, g, n1, n2, clamp, rev, other=None, want_jac=False):
    """InvBlockExp's affine half on the block's whole input x: (out, jac).  out = x2 * exp(s) + g (rev: (x2 - g) / exp(s)) [.., cpad(n2)], or
    with `other` [.., cpad(n1)] the whole block output cat(other, that); jac (want_jac) = sum of s per sample, f32 [B], detached"""
    return _InvAffineFn.apply(x, h, g, other, int(n1), int(n2), float(clamp), bool(rev), bool(want_jac))


# ----------------------------------------------------------------------------- losses, clamp and the optimiser of the literal IRNrhi step
def _scaled(grad, g):
    """grad * g for the 1-element upstream gradient g of a scalar loss (device scalar: no host sync)"""
    return ops.scale_dev_(grad.clone(), g.reshape(1).float().contiguous())


class _SmoothL1Fn(Function):
    @staticmethod
    def forward(ctx, a, b, beta):
        loss, grad = ops.smooth_l1(a, b, beta, want_grad=True)
        ctx.save_for_backward(grad)
        ctx.shape = a.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return _scaled(grad, g).reshape(ctx.shape), None, None


class _BCEProbFn(Function):
    @staticmethod
    def forward(ctx, p, target):
        loss, grad = ops.bce_prob(p, target, want_grad=True)
        ctx.save_for_backward(grad)
        ctx.shape = p.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return _scaled(grad, g).reshape(ctx.shape), None


class _CrossEntropyFn(Function):
    @staticmethod
    def forward(ctx, logits, labels):
        loss, grad = ops.cross_entropy(logits, labels, want_grad=True)
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return _scaled(grad, g), None


class _Clamp01Fn(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.clamp01_fwd(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.clamp01_bwd(x, g)


def smooth_l1_loss(a, b, beta=1.0):
    """nn.SmoothL1Loss()(a, b); b carries no gradient (a target)"""
    return _SmoothL1Fn.apply(a, b.detach(), float(beta))


def bce_loss(p, target):
    """nn.BCELoss()(p, torch.full_like(p, target)) for the constant targets 1.0 / 0.0 of the GAN terms"""
    return _BCEProbFn.apply(p, float(target))


def cross_entropy_loss(logits, labels):
    return _CrossEntropyFn.apply(logits, labels)


def clamp01(x):
    """torch.clamp(x, 0, 1) (gradient where 0 <= x <= 1)"""
    return _Clamp01Fn.apply(x)


class FlatAdamW(FlatAdam):
    """torch.optim.AdamW over ONE flat f32 buffer holding every trainable parameter of `module` (optim.FlatAdam, decoupled, over one
    FlatParameters: each nn.Parameter becomes a view of the buffer, each .grad a view of a flat gradient buffer autograd accumulates into):
    zero_grad = one memset, clip_grad_norm_ = one norm, step = one launch of the library's Adam kernel.  While the optimiser lives, the
    convolution backward kernels ADD a registered parameter's gradient straight into the flat buffer and hand autograd None for it
    (_conv_backward): use loss.backward(); torch.autograd.grad(loss, parameters) would see None for those and still change the buffer."""

    def __init__(self, module, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01):
        super().__init__([FlatParameters(module, "FlatAdamW")], lr, betas, eps, weight_decay, decoupled=True)
        self._ensure()   # the moments now: this optimiser steps OUTSIDE a CapturedStep, and its first step may follow the capture

    flat = property(lambda self: self.modules[0].flat_params)
    grad = property(lambda self: self.modules[0].flat_grads)

    def state_dict(self):
        """the training state BaseModel.save_training_state stores: step count, the param group, the two flat moment buffers (on the CPU).
        FlatAdam.load_state_dict reads it back"""
        return {"step": self._steps(), "param_groups": [dict(self.param_groups[0])], "exp_avg": self._m[0].detach().cpu().clone(),
                "exp_avg_sq": self._v[0].detach().cpu().clone()}

    def zero_grad(self):
        g = self.grad
        g.zero_()
        for p in self.modules[0].params:           # autograd may have replaced a view (first accumulation into a None grad)
            if p.grad is None or p.grad.data_ptr() < g.data_ptr() or p.grad.data_ptr() >= g.data_ptr() + 4 * g.numel():
                raise RuntimeError("FlatAdamW: a parameter's .grad no longer views the flat gradient buffer (do not set grads to None)")

    def clip_grad_norm_(self, max_norm):
        """nn.utils.clip_grad_norm_(module.parameters(), max_norm); returns the [2] device tensor (coefficient, total norm)"""
        return ops.clip_grad_norm_([self.grad], float(max_norm))

    def step(self):
        super().step()
        if _PLAN is not None:
            _PLAN.refresh()        # every registered packed weight from the new values, one launch
