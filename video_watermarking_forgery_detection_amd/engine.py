"""Explicit forward / backward of the ConvBNRelu stacks on the HIP kernels.

This is the host side of the hot path: it sequences the C-ABI kernels (ops.py)
for HiDDeN's encoder / decoder / discriminator (hidden_models/*.py of the
reference) without autograd -- the backward order is written out, so the step
can be captured, overlapped with RCCL and profiled kernel by kernel.

Data layout in HBM
  * activations: NHWC, bf16 (production) or f32 (parity), one tensor per conv
    output holding the RAW convolution result y; the BatchNorm+ReLU that follows
    is never materialised -- an `Act` carries (y, scale, shift) and every consumer
    kernel applies relu(scale*y+shift) while it stages its input;
  * image inputs: 3 channels zero-padded to 16 (one 32-byte bf16 pixel);
  * parameters / gradients / Adam moments: f32, one flat buffer per network.
"""
import collections
import contextlib
import threading
import types

import torch

from . import ops
from .optim import flatten_parameters


class Act:
    """NHWC activation: logical value = t (if scale is None) or relu(scale*t+shift)."""
    __slots__ = ("t", "C", "scale", "shift", "bwd", "rev", "src")

    def __init__(self, t, C, scale=None, shift=None, rev=None, src=None):
        self.t, self.C, self.scale, self.shift = t, C, scale, shift
        self.bwd = None   # backward: the BnSums the consumer's dgrad left when it reduced this layer's BatchNorm sums (leave_bn_sums / take_bn_sums)
        self.src = src    # (bn module, stats [4,CP]) of the ConvBNRelu that produced t (lets the consumer's backward finish this layer's statistics).
                          # NOT the layer's ctx: ctx.out -> Act -> src -> ctx would be a reference cycle, and a cycle keeps a step's 134 MB
                          # tensors alive until Python's cyclic collector runs -- the caching allocator then falls back to hipMalloc mid-step
                          # (measured: 40-60 ms host stalls)
        self.rev = rev    # sweep direction of the conv that just wrote t (False forward, True backward, None: not fresh)


def _opposite(rev):
    """sweep direction for a kernel whose main input was written in direction `rev`: start where the producer stopped (its
    last tiles are the part of the tensor still in the Infinity Cache).  None (not fresh) -> forward."""
    return rev is False


def round_up(n, m):
    return (n + m - 1) // m * m


_tls = threading.local()   # per host thread: .image_acts = id(image) -> (image, version, dtype, NHWC16 tensor) while a share_image_acts()
                            # block is open; .bumps = module -> pending count while a defer_bn_counters() block is open


@contextlib.contextmanager
def share_image_acts(dtype=None):
    """inside the block, image_to_act converts an image tensor once: a training step feeds `images` to the discriminator and the
    encoder and `encoded` to two discriminator passes (the images are not modified in between -- checked through their
    version counters).  dtype: the networks' activation dtype, for producers that can write the NHWC16 form themselves
    (wanted_image_act_dtype)"""
    if getattr(_tls, "image_acts", None) is not None:
        yield
        return
    _tls.image_acts = {}
    _tls.image_act_dtype = dtype
    try:
        yield
    finally:
        _tls.image_acts = None
        _tls.image_act_dtype = None


def image_to_act(img, dtype):
    """[B,3,H,W] f32 (NCHW) -> Act over a [B,H,W,16] zero-padded NHWC tensor."""
    B, C, H, W = img.shape
    assert C == 3
    cache = getattr(_tls, "image_acts", None)
    if cache is not None:
        hit = cache.get(id(img))
        if hit is not None and hit[0] is img and hit[1] == img._version and hit[2] == dtype:
            return Act(hit[3], 3)
    t = torch.empty(B, H, W, 16, device=img.device, dtype=dtype)
    ops.nchw_to_nhwc(img, t, 0, 13)
    if cache is not None:
        cache[id(img)] = (img, img._version, dtype, t)
    return Act(t, 3)


def register_image_act(img, t):
    """inside a share_image_acts() block: `t` [B,H,W,16] IS image_to_act(img, t.dtype) already (written by the kernel that produced img:
    the encoder's head, the block-JPEG attack), so the first layer that reads img launches no conversion"""
    cache = getattr(_tls, "image_acts", None)
    if cache is not None and t is not None:
        cache[id(img)] = (img, img._version, t.dtype, t)


def sharing_image_acts():
    return getattr(_tls, "image_acts", None) is not None


def wanted_image_act_dtype():
    """inside a training step (share_image_acts(dtype)): the activation dtype of the networks that will read an image this step produces --
    a kernel that writes such an image may write its NHWC16 form beside it (register_image_act); None outside a step"""
    return getattr(_tls, "image_act_dtype", None) if sharing_image_acts() else None


class CBRCtx:
    __slots__ = ("x", "y", "stats", "perm", "training", "out")


def _packed(conv, CoutP, CinP, dtype, perm, transpose):
    """packed weights of `conv`: from the owning network's PackPlan (one launch per optimiser step, see
    FlatModule.refresh_packs) when there is one, else packed on the spot."""
    plan = getattr(conv, "_wm_plan", None)
    if plan is None:
        return ops.pack_w3x3(conv.weight.data, CoutP, CinP, dtype, perm=perm, transpose=transpose)
    # (the Parameter itself, not a `.data` alias: its version counter is the one torch bumps for `with no_grad(): w.add_(..)` etc.)
    return plan.get(conv.weight.detach(), CoutP, CinP, dtype, perm=perm, transpose=transpose)


def cbr_forward(conv, bn, x, dtype, perm=None, training=True, momentum=0.1):
    """ConvBNRelu forward (conv_bn_relu.py:11-15).  conv.weight [Cout,Cin,3,3], conv.bias or None,
    bn: BatchNorm2d parameters/buffers.  x: Act whose physical channel count (x.t.shape[-1]) is the
    K extent.  Returns (Act(y, scale, shift), ctx)."""
    Cout = conv.weight.shape[0]
    CoutP = round_up(Cout, 32)
    CinX = x.t.shape[-1]
    wp = _packed(conv, CoutP, CinX, dtype, perm, False)
    bias = conv.bias.data if conv.bias is not None else None
    d = _opposite(x.rev)
    y, st = ops.conv3x3_fwd(x.t, wp, bias, x.scale, x.shift, want_stats=training, reverse=d)
    return cbr_finish(conv, bn, x, y, st, d, perm, training, momentum)


def cbr_finish(conv, bn, x, y, st, d, perm=None, training=True, momentum=0.1):
    """second half of a ConvBNRelu forward: the raw conv output y (+ its statistics partials st) -> (Act(y, scale, shift), ctx)"""
    Cout = conv.weight.shape[0]
    CoutP = y.shape[-1]
    B, H, W, _ = y.shape
    if training:
        stats = ops.bn_finalize(st, Cout, CoutP, B * H * W, bn.weight.data, bn.bias.data, bn.running_mean,
                                bn.running_var, momentum if bn.momentum is None else bn.momentum, bn.eps)
    else:
        invstd = torch.rsqrt(bn.running_var + bn.eps)
        scale = bn.weight.data * invstd
        stats = torch.zeros(4, CoutP, device=y.device, dtype=torch.float32)
        stats[0, :Cout] = scale
        stats[1, :Cout] = bn.bias.data - bn.running_mean * scale
        stats[2, :Cout] = bn.running_mean
        stats[3, :Cout] = invstd
    ctx = CBRCtx()
    ctx.x, ctx.y, ctx.stats, ctx.perm, ctx.training = x, y, stats, perm, training
    ctx.out = Act(y, Cout, stats[0], stats[1], rev=d, src=(bn, stats))
    return ctx.out, ctx


def fin_rider(x, part, grads, accumulate):
    """the BatchNorm-backward finalisation of the layer that produced Act `x`, to ride on a weight-gradient slab reduction"""
    if x.src is None or not ops.fin_rider_enabled():
        return None
    pbn, pstats = x.src
    return dict(partials=part, y_shape=tuple(x.t.shape), stats=pstats, C=x.C, gamma=pbn.weight.data, dgamma=grads[pbn.weight],
                dbeta=grads[pbn.bias], accumulate=accumulate)


# A layer's BatchNorm-backward sums, reduced ahead of its backward by the kernel that produced `g`, the gradient wrt its output (the consumer's
# input-gradient kernel, a 1x1 head's backward): valid for exactly that tensor at that version.  partials [n,2,CP] = sum(gz), sum(gz*y);
# coef [3,CP]: finished already by a rider on the consumer's weight-gradient reduction (dgamma / dbeta written there), or None
BnSums = collections.namedtuple("BnSums", "g partials coef version")


def leave_bn_sums(act, g, partials, coef=None):
    act.bwd = BnSums(g, partials, coef, g._version)


def take_bn_sums(act, g):
    """the sums left on `act` for the gradient g now handed to its layer, or None; nothing stays behind.  A different or edited g would use
    stale sums or count dgamma / dbeta twice: refused, even where the coefficients come from elsewhere (coef_pre, pool_stats)"""
    sums, act.bwd = act.bwd, None
    if sums is not None and (sums.g is not g or g._version != sums.version):
        raise RuntimeError("cbr_backward: the gradient handed to this layer is not the tensor its consumer's input-gradient "
                           "kernel produced (or it was modified in place since); its pre-reduced BatchNorm sums are stale")
    return sums


# Two facts travel on a gradient tensor itself, since g crosses module boundaries bare: the sweep of the kernel that wrote it (its reader starts
# where it stopped; forward when there is no tensor) and "already multiplied by its layer's ReLU mask" (written by ops._premasked)
def sweep_after(g):
    return g is not None and _opposite(getattr(g, "_wm_rev", None))


def mark_sweep(gx, d):
    gx._wm_rev = d
    return gx


def is_premasked(g):
    return getattr(g, "_wm_masked", False)


def select_bwd_route(f):
    """name of the route cbr_backward takes for a layer with the facts f (bwd_facts: plain values, no tensors).  First match wins"""
    plain = not f.permuted and f.stats_contig
    if f.weight_grads and not f.need_input_grad and f.has_g and not f.fed_by_cbr and plain and f.wgrad_bnfused_ok:
        return "first_layer_weights_only"   # conv1 of the encoder, the UNet, the discriminator in its own update, the decoder behind a zero gradient
    if not f.weight_grads:                  # the discriminator under the generator's loss: nobody reads its weight gradients
        if not f.need_input_grad:
            return "bn_only"                # (no layer of a training step: dgamma / dbeta alone)
        if f.has_gvec and plain and f.CoutY == 64 and f.feed_stats and f.gvfused_ok:
            return "dx_only_pooled"         # its pooled last layer
        if f.g_dense and plain and f.CoutY == 64 and f.rows in (64, 32) and f.applyfused_ok:
            return "dx_only"                # its body layers (which feed sums) and its conv1 (32 rows)
        return "dx_only_unfused"            # the same in f32 / shapes without a fused input-gradient kernel
    if f.has_gvec and f.need_input_grad and f.fed_by_cbr and plain and f.rows == 64 and f.CinX == 64 and f.gvfused_ok:
        if f.feed_stats and f.CoutY == 64 and f.bwd_fused_ok and f.gvec_cols == 64 and f.B <= f.gvec_max_batch:
            return "pooled_onepass"         # the discriminator's last layer (64 -> 64) in its own update
        return "pooled_feed" if f.feed_stats else "pooled"   # the decoder's last layer (64 -> 30), a batch above the one-pass limit / a sliced input
    if f.g_dense and f.need_input_grad and not f.fed_by_cbr and plain and f.CoutY == 64 and f.bwd_fused16_ok:
        return "first_layer_onepass"        # conv1 of the decoder and the discriminator when the image gets a gradient (whole 8x16 tiles)
    if f.g_dense and f.need_input_grad and plain and f.rows in (64, 32) and f.CoutY == 64 and f.applyfused_ok:
        if f.feed_stats and f.bwd_fused_ok and not f.keep_dy:
            return "body_onepass"           # the 64 -> 64 body layers of every network, the UNet's 64-channel level
        return "body_two_kernels"           # those beyond the one-pass kernel's 32-bit offsets or behind a pool; conv1 on partial tiles; keep_dy
    return "generic"                        # f32 (parity), the unsplit after-concat layer (permuted), the UNet's other widths


def bwd_facts(conv, ctx, g, gvec, need_input_grad, dgrad_channels, perm_dev, weight_grads, keep_dy=False):
    """what select_bwd_route decides on, each computed once: plain values, no tensors.  keep_dy: the caller reads dy again afterwards"""
    x, y = ctx.x, ctx.y
    CinX, CoutY, dtype = x.t.shape[-1], y.shape[-1], y.dtype
    rows = dgrad_channels or round_up(CinX, 32)                     # width of the input gradient
    fed_by_cbr = x.scale is not None                                # the input is itself a ConvBNRelu output
    permuted = ctx.perm is not None or perm_dev is not None         # the input is the encoder's permuted concat
    g_dense = g is not None and g.shape == y.shape and g.is_contiguous()
    # this layer's input-gradient kernel can reduce the FEEDING layer's BatchNorm-backward sums on the way
    feed_stats = (need_input_grad and fed_by_cbr and not permuted and rows == 64 and CinX == 64 and x.t.is_contiguous()
                  and ops.conv3x3_dgrad_bwdstats_supported(CoutY, rows, dtype))
    # the library's answers, each asked only where select_bwd_route gets to it
    bwd_fused_ok = feed_stats and CoutY == 64 and ops.conv3x3_bwd_fused_supported(dtype, y.shape)
    bwd_fused16_ok = (g_dense and weight_grads and need_input_grad and not fed_by_cbr and CinX == 16 and dgrad_channels is None
                      and conv.weight.shape[1] <= 16 and ops.conv3x3_bwd_fused16_supported(y.shape, dtype))    # an image filter, 16 channels back
    return types.SimpleNamespace(
        has_g=g is not None, has_gvec=gvec is not None, need_input_grad=need_input_grad, weight_grads=weight_grads, keep_dy=keep_dy,
        fed_by_cbr=fed_by_cbr, permuted=permuted, rows=rows, CinX=CinX, CoutY=CoutY, dtype=dtype, B=y.shape[0], g_dense=g_dense,
        gvec_cols=gvec.shape[-1] if gvec is not None else 0, feed_stats=feed_stats, stats_contig=ctx.stats.is_contiguous(),
        wgrad_bnfused_ok=(weight_grads and not need_input_grad and g is not None and not fed_by_cbr and g.shape[-1] == CoutY
                          and ops.conv3x3_wgrad_bnfused_supported(CinX, CoutY, dtype)),
        gvfused_ok=gvec is not None and need_input_grad and ops.conv3x3_gvfused_supported(64, CoutY, dtype),
        applyfused_ok=g_dense and need_input_grad and not bwd_fused16_ok and ops.conv3x3_dgrad_applyfused_supported(64, rows, dtype),
        bwd_fused_ok=bwd_fused_ok, bwd_fused16_ok=bwd_fused16_ok,
        gvec_max_batch=ops.conv3x3_bwd_fused_gvec_max_batch() if gvec is not None and bwd_fused_ok else 0)


def cbr_backward(conv, bn, ctx, grads, g=None, gvec=None, need_input_grad=True, accumulate=False,
                 dgrad_channels=None, perm_dev=None, pool_stats=None, weight_grads=True, coef_pre=None, slice_perms=None):
    """Backward of ConvBNRelu.  g: NHWC gradient wrt the ReLU output ([B,H,W,>=CoutP]) or gvec [B,CoutP]
    (global-average-pool gradient, already / (H*W)).  grads: dict param -> f32 grad view.
    Returns the NHWC gradient wrt the (activated) input, `dgrad_channels` wide (default: the input's
    physical channels rounded up to 32), or None.
    weight_grads=False: the input gradient alone -- conv.weight's gradient is neither computed nor touched (the BatchNorm affine
    gradients, a by-product of the backward coefficients, still are): the discriminator under the generator's loss, whose parameter
    gradients nobody reads (hidden.py:67 zeroes them first thing in the next step).
    slice_perms: the encoder's split after-concat layer, an unpermuted 64 -> 64 layer whose filter is a channel slice of a wider one:
    (that selection for the filter pack, the same for the weight gradient).  dy then stays in memory and (input gradient, dy) is returned."""
    if not ctx.training:
        raise RuntimeError("backward through eval-mode BatchNorm is not supported by the HIP path")
    f = bwd_facts(conv, ctx, g, gvec, need_input_grad, dgrad_channels, perm_dev, weight_grads, keep_dy=slice_perms is not None)
    route = select_bwd_route(f)
    x, y, stats = ctx.x, ctx.y, ctx.stats
    xin = (x.t, x.scale, x.shift)
    feed = xin if f.feed_stats else ()
    bn_args = (y, stats, conv.weight.shape[0], bn.weight.data, grads[bn.weight], grads[bn.bias], accumulate)
    dw = grads[conv.weight] if weight_grads else None
    wperm, wgrad_perm = (ctx.perm, perm_dev) if slice_perms is None else slice_perms    # channel order of the filter pack / the weight gradient
    sums = take_bn_sums(ctx.out, g)
    d = sweep_after(g)                                  # this layer's input-gradient sweep
    # the premasked tag (the staging then skips the mask arithmetic) is trusted only for the tensor a kernel returned, unmodified: the one with sums
    premasked = sums is not None and is_premasked(g)

    def coef_of():
        """coefficients [3,CP] of the BatchNorm-backward apply pass; dgamma / dbeta are written on the way, or were by whoever finished them"""
        if gvec is not None and coef_pre is not None:       # the fused pooled head (ops.pooled_head)
            return coef_pre
        if gvec is not None and pool_stats is not None:     # (N+, S+) from the forward pool: no pass over y
            return ops.bn_bwd_coef_pooled(gvec, pool_stats, *bn_args)
        if sums is None:
            return ops.bn_bwd_coef(g, gvec, *bn_args)
        if sums.coef is not None:                           # finished by a rider on the consumer's weight-gradient reduction
            return sums.coef
        return ops.bn_bwd_coef_raw(sums.partials, *bn_args)

    def wpt(cols=f.rows):
        return _packed(conv, f.CoutY, cols, f.dtype, wperm, True)
    def rider(part):    # the feeding layer's BatchNorm-backward finalisation, to ride on this layer's weight-gradient reduction
        return None if part is None else fin_rider(x, part, grads, accumulate)

    def leave(gx, part=None, pcoef=None, direction=d):      # gx is the result: mark its sweep, leave the feeding layer's sums for who gets it
        if part is not None:
            leave_bn_sums(x, gx, part, pcoef)
        return mark_sweep(gx, direction)

    gx = dy = None
    if route == "first_layer_weights_only":     # dy has ONE consumer, the weight gradient: its kernel forms dy from (g, y) while staging
        ops.conv3x3_wgrad_bnfused(x.t, g, y, stats, coef_of(), dw, accumulate)
    elif route == "bn_only":
        coef_of()
    elif route == "dx_only_pooled":
        gx = leave(*ops.conv3x3_dgrad_bwdstats(y, wpt(), *xin, gvec, stats, coef_of()))
    elif route == "dx_only":
        packed = wpt()
        _, gx, part = ops.conv3x3_dgrad_applyfused(g, y, stats, coef_of(), packed, *feed, reverse=d, want_dy=False)
        gx = leave(gx, part)
    elif route in ("pooled_onepass", "body_onepass"):
        # one kernel (csrc/bwd_ws.hip): dy is formed in the LDS from (g or gvec, y) and feeds BOTH gradients; its input's raw tensor is read once
        gx = leave(*ops.conv3x3_bwd_fused(g, y, stats, coef_of(), wpt(), *xin, dw, accumulate, reverse=d, fin=rider, premasked=premasked, gvec=gvec))
    elif route == "pooled_feed":
        # no apply pass: both kernels form dy from (gvec, y).  Input gradient first: a rider on the weight-gradient reduction finishes its sums
        coef, packed = coef_of(), wpt()
        gx, part = ops.conv3x3_dgrad_bwdstats(y, packed, *xin, gvec, stats, coef)
        gx = leave(gx, part, ops.conv3x3_wgrad_gvfused(*xin, gvec, y, stats, coef, dw, accumulate, fin=rider(part)))
    elif route == "pooled":
        coef, packed = coef_of(), wpt()
        ops.conv3x3_wgrad_gvfused(*xin, gvec, y, stats, coef, dw, accumulate)
        gx = leave(ops.conv3x3_dgrad_gvfused(y, packed, gvec, stats, coef))
    elif route == "first_layer_onepass":        # one kernel (csrc/bwd_ws16.hip) forms dy once for both gradients (the input's: 16 channels, 3 real)
        gx = leave(ops.conv3x3_bwd_fused16(g, y, stats, coef_of(), wpt(16), x.t, dw, accumulate, reverse=d, premasked=premasked))
    elif route == "body_two_kernels":
        # the input-gradient kernel reads g and y, forms dy while staging and leaves it in memory for the weight gradient: no apply pass
        coef, packed = coef_of(), wpt()
        dy, gx, part = ops.conv3x3_dgrad_applyfused(g, y, stats, coef, packed, *feed, reverse=d)
        pcoef = ops.conv3x3_wgrad(x.t, f.CinX, x.scale, x.shift, dy, dw, accumulate, perm_dev=wgrad_perm, reverse=not d, fin=rider(part))
        gx = leave(gx, part, pcoef)
    else:   # "dx_only_unfused", "generic": the stand-alone apply pass, then the plain kernels.  The gradient of a conv bias in front of a
        # training-mode BatchNorm is identically zero (the batch mean removes the bias): its view is zero-initialised and never written
        dy = ops.bn_bwd(g, gvec, *bn_args, None, coef=coef_of())
        if weight_grads:
            ops.conv3x3_wgrad(x.t, f.CinX, x.scale, x.shift, dy, dw, accumulate, perm_dev=wgrad_perm, reverse=True)   # the apply pass swept forwards
        if need_input_grad and f.feed_stats and weight_grads:
            gx = leave(*ops.conv3x3_dgrad_bwdstats(dy, wpt(), *xin), direction=False)
        elif need_input_grad:
            gx = leave(ops.conv3x3_fwd(dy, wpt(), None, None, None, want_stats=False)[0], direction=False)
    return gx if slice_perms is None else (gx, dy)


def grad_dict(module, flat_grad=None):
    """param -> gradient view.  With flat_grad None, uses/creates p.grad."""
    out = {}
    off = 0
    for p in module.parameters():
        if flat_grad is None:
            if p.grad is None:
                p.grad = torch.zeros_like(p.data)
            out[p] = p.grad
        else:
            n = p.numel()
            out[p] = flat_grad[off:off + n].view_as(p)
            off += n
    return out


class FlatModule:
    """Mixin: keeps all parameters of an nn.Module in one flat f32 buffer (and the gradients in
    another) so the optimiser step is one kernel and the gradient all-reduce one RCCL bucket."""

    def flatten_parameters_(self):
        params = list(self.parameters())
        if not params:
            return
        dev = params[0].device
        n = sum(p.numel() for p in params)
        flat = getattr(self, "_flat", None)
        ok = flat is not None and flat.device == dev and flat.numel() == n
        if ok:
            off = 0
            for p in params:
                if p.data_ptr() != flat.data_ptr() + 4 * off:
                    ok = False
                    break
                off += p.numel()
        if ok:
            return
        flat, gflat = flatten_parameters(params)
        object.__setattr__(self, "_flat", flat)
        object.__setattr__(self, "_gflat", gflat)
        if not getattr(self, "_wm_load_hook", False):
            # a state_dict load writes the parameters behind every version check (copy_ into `.data` aliases): drop the packs
            self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate_packs())
            object.__setattr__(self, "_wm_load_hook", True)
        # BatchNorm step counters: views of one int64 tensor, so a forward bumps them with one launch
        bns = [m for m in self.modules() if isinstance(m, torch.nn.BatchNorm2d) and m.num_batches_tracked is not None]
        if bns:
            nbt = torch.stack([m.num_batches_tracked.to(dev) for m in bns])
            for i, m in enumerate(bns):
                m._buffers["num_batches_tracked"] = nbt[i]
            object.__setattr__(self, "_nbt", nbt)

    # ---- packed conv weights: one launch per optimiser step instead of one per conv call
    def pack_plan(self):
        """the network's ops.PackPlan (created on first use; every 3x3 conv of the module points at it)."""
        plan = getattr(self, "_pack_plan", None)
        flat = getattr(self, "_flat", None)
        if plan is None or getattr(self, "_pack_plan_flat", None) is not flat:
            plan = ops.PackPlan()
            object.__setattr__(self, "_pack_plan", plan)
            object.__setattr__(self, "_pack_plan_flat", flat)   # a re-flatten moves the parameters: start over
            for m in self.modules():
                if isinstance(m, torch.nn.Conv2d) and tuple(m.kernel_size) == (3, 3):
                    object.__setattr__(m, "_wm_plan", plan)
        return plan

    def refresh_packs(self):
        """(re)pack every conv weight the network has used so far from the CURRENT parameters, in one launch; the packs
        stay valid until invalidate_packs().  Callers own the validity window (Hidden.train_on_batch)."""
        self.flatten_parameters_()
        self.pack_plan().refresh()

    def invalidate_packs(self):
        plan = getattr(self, "_pack_plan", None)
        if plan is not None:
            plan.invalidate()

    @property
    def flat_params(self):
        self.flatten_parameters_()
        return self._flat

    @property
    def flat_grads(self):
        self.flatten_parameters_()
        return self._gflat


def set_compute_dtype(module, dtype):
    """torch.bfloat16 (production), torch.float16 (the reference's autocast dtype; needs loss scaling, see models/IRNrhi_model.py)
    or torch.float32 (parity path) for every HIP-backed submodule."""
    if dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError("compute dtype must be torch.float32, torch.bfloat16 or torch.float16")
    for m in module.modules():
        if hasattr(m, "compute_dtype"):
            m.compute_dtype = dtype
    return module


@contextlib.contextmanager
def defer_bn_counters():
    """inside the block, bump_bn_counters only counts; one multi-tensor add applies everything at exit (a training step
    runs five network forwards: one launch instead of five)"""
    if getattr(_tls, "bumps", None) is not None:   # nested: the outer block flushes
        yield
        return
    _tls.bumps = {}
    try:
        yield
    finally:
        pend, _tls.bumps = _tls.bumps, None
        if pend:
            torch._foreach_add_([m._nbt for m in pend], [pend[m] for m in pend])


def bump_bn_counters(module):
    """num_batches_tracked += 1 for every BatchNorm2d of `module` (one launch when the counters are flat)."""
    nbt = getattr(module, "_nbt", None)
    if nbt is not None and all(m.num_batches_tracked.data_ptr() == nbt[i].data_ptr() for i, m in enumerate(
            mm for mm in module.modules() if isinstance(mm, torch.nn.BatchNorm2d) and mm.num_batches_tracked is not None)):
        pend = getattr(_tls, "bumps", None)
        if pend is not None:
            pend[module] = pend.get(module, 0) + 1
            return
        nbt += 1
        return
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm2d) and m.num_batches_tracked is not None:
            m.num_batches_tracked += 1
