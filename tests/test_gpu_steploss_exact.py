"""GPU: the scalar-loss and step-glue kernels per element against float64 (tests/steploss_exact.py): csrc/losses.hip (wm_smooth_l1,
wm_bce_prob, wm_cross_entropy, wm_clamp01_fwd, wm_clamp01_bwd, wm_psnr255_partials), csrc/localise.hip (wm_splice_fwd with
wm_splice_nparts, wm_psnr_gate, wm_mse_fwd_bwd_gated, wm_bce_logits_target, wm_masked_axpy, wm_mask_threshold, wm_scale_dev) and the loss
half of csrc/optim.hip (wm_mse_fwd_bwd, wm_image_grad_mse, wm_bce_logits, wm_message_loss, wm_hidden_metrics, wm_sumsq, wm_axpy,
wm_nonfinite), at the smallest sizes that take each path: one element, the wave and workgroup edges, the first size with two workgroups
and a ragged stride, three elements above every grid cap, more rows than threads, ld > K, a different mask per batch item, and the
hand-placed values at which a comparison, a clamp, a truncation or a rounding tie decides.

The ops.* wrappers run every case; where a wrapper hides nparts or ld the typed entry of _lib.lib() is called as well.  Every test prints
one line per comparison and the largest observed multiple of the bound per kernel before it asserts (run with -s).
tests/test_cpu_steploss_exact.py shows that these comparisons fail on the defects they are there to catch."""
import time

import numpy as np
import pytest
import torch

import steploss_exact as SX

pytestmark = pytest.mark.gpu


def dev(a, dt="f32"):
    return None if a is None else (a if torch.is_tensor(a) else SX.store(a, dt)).cuda()


def filled(n, dtype=torch.float32):
    return torch.full((n,), SX.SENTINEL, dtype=dtype, device="cuda")


def scalar(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device="cuda")


def report(kernel, cmps, worst):
    for c in cmps:
        print("  ", c.line())
    worst[kernel] = max(worst.get(kernel, 0.0), SX.worst(cmps))
    return cmps


class Run:
    """prints the wall time and the worst multiple of the bound per kernel, then asserts every comparison collected"""

    def __enter__(self):
        print()
        torch.cuda.synchronize()
        self.t, self.worst, self.cmps = time.perf_counter(), {}, []
        return self

    def add(self, kernel, cmps):
        self.cmps += report(kernel, cmps, self.worst)

    def __exit__(self, et, ev, tb):
        torch.cuda.synchronize()
        print("   wall time %.2f s" % (time.perf_counter() - self.t))
        for k, v in sorted(self.worst.items()):
            print("   worst multiple of the bound  %-22s %.3f" % (k, v))
        if et is None:
            for c in self.cmps:
                c.assert_ok()


def _mods():
    from video_watermarking_forgery_detection_amd import _lib, ops
    return _lib, ops, _lib.lib(), torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def guarded(n, pad=8):
    """a float32 destination of n elements inside a SENTINEL buffer: (whole buffer, the view a kernel writes)"""
    buf = filled(n + 2 * pad)
    return buf, buf[pad:pad + n]


def around_ok(kernel, buf, n, pad=8):
    b = SX.f64(buf)
    rest = np.concatenate([b[:pad], b[pad + n:]])
    return [SX.ECmp(kernel + " around the destination", rest, np.full(rest.shape, SX.SENTINEL))]


def nparts_of(n):
    return list(SX.FREE_NPARTS) if n == 4097 else []


# ----------------------------------------------------------------------------------------------------------------- losses.hip
def test_smooth_l1():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for key in SX.SMOOTH_L1_KEYS:
            c = SX.smooth_l1_case(*key)
            a, b = dev(c.a), dev(c.b)
            r.add("smooth_l1", c.check(*ops.smooth_l1(a, b, c.beta)))
            for npt in nparts_of(c.n) if not key[2] else [1]:
                part, loss = filled(npt), filled(1)
                gbuf, grad = guarded(c.n)
                _lib.check(L.wm_smooth_l1(p(a), p(b), c.n, c.beta, p(part), npt, p(loss), p(grad), stream), c.label)
                r.add("smooth_l1", c.check(loss, grad, nparts=npt) + around_ok(c.label, gbuf, c.n))


def test_bce_prob():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for key in SX.BCE_PROB_KEYS:
            c = SX.bce_prob_case(*key)
            x = dev(c.p)
            r.add("bce_prob", c.check(*ops.bce_prob(x, c.target)))
            for npt in nparts_of(c.n):
                part, loss = filled(npt), filled(1)
                gbuf, grad = guarded(c.n)
                _lib.check(L.wm_bce_prob(p(x), c.target, c.n, p(part), npt, p(loss), p(grad), stream), c.label)
                r.add("bce_prob", c.check(loss, grad, nparts=npt) + around_ok(c.label, gbuf, c.n))


def test_cross_entropy():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for B, K in SX.CE_KEYS:
            c = SX.cross_entropy_case(B, K)
            y = torch.from_numpy(c.y).cuda()
            r.add("cross_entropy", c.check(*ops.cross_entropy(dev(c.z), y)))
            c = SX.cross_entropy_case(B, K, K + SX.CE_PAD)                 # wm_cross_entropy with ld = K + 3: the padding stays
            z, loss = c.logits().cuda(), filled(1)
            gbuf, grad = guarded(B * c.ld)
            _lib.check(L.wm_cross_entropy(p(z), p(y), B, K, c.ld, p(loss), p(grad), stream), c.label)
            r.add("cross_entropy", c.check(loss, grad) + around_ok(c.label, gbuf, B * c.ld))


def test_clamp01():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for key in SX.CLAMP_KEYS:
            c = SX.clamp01_case(*key)
            x, g = dev(c.x), dev(c.g)
            r.add("clamp01", c.check_fwd(ops.clamp01_fwd(x)) + c.check_bwd(ops.clamp01_bwd(x, g)))
            if c.n <= 4097:
                ybuf, y = guarded(c.n)
                gbuf, gx = guarded(c.n)
                _lib.check(L.wm_clamp01_fwd(p(x), p(y), c.n, stream), c.label)
                _lib.check(L.wm_clamp01_bwd(p(x), p(g), p(gx), c.n, stream), c.label)
                r.add("clamp01", c.check_fwd(y) + c.check_bwd(gx) + around_ok(c.label + " fwd", ybuf, c.n) + around_ok(c.label + " bwd", gbuf, c.n))


@pytest.mark.parametrize("view", ["channel slice", "permuted", "float64"])
def test_clamp01_autograd_on_views(view):
    """glayers.clamp01 forward and backward on an input that is not a contiguous float32 tensor, against torch.clamp's autograd in float64:
    the backward must gate element i of g by element i of x, not by element i of x's storage"""
    from video_watermarking_forgery_detection_amd import glayers as G
    base = SX.data32((2, 5, 4, 6), 11000)
    g = SX.data32((2, 3, 4, 6) if view == "channel slice" else ((2, 4, 6, 5) if view == "permuted" else (2, 5, 4, 6)), 11001)

    def pick(t):
        return t[:, 1:4] if view == "channel slice" else (t.permute(0, 2, 3, 1) if view == "permuted" else t)
    xr = torch.from_numpy(base).requires_grad_(True)
    yr = torch.clamp(pick(xr), 0, 1)
    (yr * torch.from_numpy(g)).sum().backward()
    xd = (torch.from_numpy(base) if view == "float64" else SX.store(base, "f32")).cuda().requires_grad_(True)
    xin = pick(xd)
    assert view == "float64" or not xin.is_contiguous()
    yd = G.clamp01(xin)
    (yd * SX.store(g, "f32").cuda()).sum().backward()
    with Run() as r:
        r.add("clamp01", [SX.ECmp("clamp01 autograd %s fwd" % view, yd, yr.detach().numpy()),
                          SX.ECmp("clamp01 autograd %s bwd" % view, xd.grad, xr.grad.numpy())])


def test_clamp01_bwd_and_glue_wrappers_refuse_mismatched_operands():
    _lib, ops, L, stream = _mods()
    x = torch.zeros(2, 3, 4, 4, device="cuda")
    with pytest.raises(ValueError):
        ops.clamp01_bwd(x, x[:, :2])
    with pytest.raises(ValueError):
        ops.mse_fwd_bwd_gated(x, x[:, :2], 1.0, scalar(1.0))
    with pytest.raises(ValueError):
        ops.mse_fwd_bwd_gated(x, x.double(), 1.0, scalar(1.0))
    with pytest.raises(ValueError):
        ops.masked_axpy_(x, x.clone(), torch.zeros(2, 3, 4, 4, device="cuda"))
    with pytest.raises(ValueError):
        ops.masked_axpy_(x, x.clone(), torch.zeros(2, 1, 4, 4, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.masked_axpy_(x, x.half(), torch.zeros(2, 1, 4, 4, device="cuda"))


def test_psnr255():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for n in SX.FLAT_N:
            c = SX.psnr255_case(n)
            a, b = dev(c.a), dev(c.b)
            r.add("psnr255", SX.check_psnr(c.label, ops.psnr255(a, b), c.total, n))
            for npt in [SX.wrapper_nparts(n)] + nparts_of(n):
                pbuf = torch.full((npt + 4,), SX.SENTINEL, dtype=torch.float64, device="cuda")
                _lib.check(L.wm_psnr255_partials(p(a), p(b), n, p(pbuf[2:]), npt, stream), c.label)
                rest = torch.cat([pbuf[:2], pbuf[2 + npt:]])
                r.add("psnr255", c.check(pbuf[2:2 + npt]) + [SX.ECmp(c.label + " around the partials", rest, np.full(4, SX.SENTINEL))])


def test_psnr_gate():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for npt in SX.GATE_NPARTS:
            for zero in (False, True):
                c = SX.PsnrGateCase(npt, zero)
                part = torch.from_numpy(c.partials).cuda()
                out = ops.psnr_gate(part, c.n, 33.0, *SX.GATE_W)
                r.add("psnr_gate", c.check(out, 33.0))
                for thr in SX.around(float(out[0].item())):      # wm_psnr_gate: the strict `<` against the value it returned itself
                    r.add("psnr_gate", c.check(ops.psnr_gate(part, c.n, thr, *SX.GATE_W), thr))


# ----------------------------------------------------------------------------------------------------------------- localise.hip
def _run_splice(c, mode, ops):
    B, C, HW = c.B, c.C, c.HW
    shape = (B, C, 1, HW)
    enc = dev(c.enc).reshape(shape)
    real = dev(c.real).reshape(shape) if mode in ("real", "all") else None
    prev = dev(c.prev).reshape(shape) if mode in ("tampered", "all") else None
    mask = dev(c.mask).reshape(B, 1, 1, HW) if prev is not None else None
    fwd, tam, part = ops.splice_fwd(enc, real=real, prev=prev, mask=mask, want_fwd=mode in ("fwd_q", "all"))
    assert (fwd is None) == (mode not in ("fwd_q", "all")) and (tam is None) == (prev is None) and (part is None) == (real is None)
    return c.check(mode, fwd, tam, part)


def test_splice_fwd():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for key in SX.PLANE_KEYS:
            c = SX.splice_case(*key)
            assert L.wm_splice_nparts(c.enc.size) == min(max(-(-c.enc.size // 256), 1), 1024)
            for mode in SX.SPLICE_MODES:
                r.add("splice_fwd", _run_splice(c, mode, ops))
        c = SX.splice_case(*SX.SPLICE_CAP_KEY)
        r.add("splice_fwd", _run_splice(c, "all", ops))
        # the typed entry, every output inside SENTINEL
        c = SX.splice_case(3, 3, 771)
        n = c.enc.size
        fb, fq = guarded(n)
        tb, tam = guarded(n)
        npt = L.wm_splice_nparts(n)
        part = torch.zeros(npt, dtype=torch.float64, device="cuda")
        enc, real, prev, mask = dev(c.enc), dev(c.real), dev(c.prev), dev(c.mask)
        _lib.check(L.wm_splice_fwd(p(enc), p(real), p(prev), p(mask), p(fq), p(tam), p(part), 3, 3, 771, stream), c.label)
        r.add("splice_fwd", c.check("all", fq, tam, part) + around_ok(c.label + " fwd_q", fb, n) + around_ok(c.label + " tampered", tb, n))


def test_masked_axpy():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for key in SX.PLANE_KEYS + ((1, 1, SX.CAP_ELEM + 3, "pattern"),):
            c = SX.MaskedAxpyCase(*key)
            a = dev(c.a).reshape(c.B, c.C, 1, c.HW)
            ops.masked_axpy_(a, dev(c.g).reshape(a.shape), dev(c.mask).reshape(c.B, 1, 1, c.HW))
            r.add("masked_axpy", c.check(a))
        c = SX.MaskedAxpyCase(3, 3, 771)
        n = c.a.size
        buf, a = guarded(n)
        a.copy_(dev(c.a))
        g, mask = dev(c.g), dev(c.mask)
        _lib.check(L.wm_masked_axpy(p(a), p(g), p(mask), 3, 3, 771, stream), c.label)
        r.add("masked_axpy", c.check(a) + around_ok(c.label, buf, n))


def test_axpy_scale_dev_mask_threshold():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for n, data in SX.ELEM_KEYS:
            c = SX.AxpyCase(n, data)
            buf, a = guarded(n)
            a.copy_(dev(c.a))
            b = dev(c.b)
            if n < SX.CAP_ELEM:
                _lib.check(L.wm_axpy(p(a), p(b), c.s, n, stream), c.label)
            else:
                ops.axpy_(a, b, c.s)
            r.add("axpy", c.check(a) + around_ok(c.label, buf, n))
            for s in (1.0, 0.3):
                c = SX.ScaleDevCase(n, data, s)
                buf, x = guarded(n)
                x.copy_(dev(c.x))
                sd = scalar(c.s)
                if n < SX.CAP_ELEM:
                    _lib.check(L.wm_scale_dev(p(x), n, p(sd), stream), c.label)
                else:
                    ops.scale_dev_(x, sd)
                r.add("scale_dev", c.check(x) + around_ok(c.label, buf, n))
            for thr in (0.5, 0.3):
                c = SX.MaskThresholdCase(n, data, thr)
                pr = dev(c.p)
                r.add("mask_threshold", c.check(ops.mask_threshold(pr, c.thr)))
                if n < SX.CAP_ELEM:
                    obuf = torch.full((n + 16,), 7, dtype=torch.uint8, device="cuda")
                    _lib.check(L.wm_mask_threshold(p(pr), c.thr, p(obuf[8:]), n, stream), c.label)
                    rest = torch.cat([obuf[:8], obuf[8 + n:]])
                    r.add("mask_threshold", c.check(obuf[8:8 + n]) + [SX.ECmp(c.label + " around the destination", rest, np.full(16, 7.0))])


def _run_mse(c, ops, L, _lib, stream, npt=None):
    a, b = dev(c.a), dev(c.b)
    gate, gd = scalar(c.gate), scalar(c.gdev)
    if npt is None:
        if c.gate is not None:
            return c.check(*ops.mse_fwd_bwd_gated(a, b, c.gscale, gate, gscale_dev=gd))
        return c.check(*ops.mse_fwd_bwd(a, b, c.gscale, gscale_dev=gd))
    part = filled(npt)
    gbuf, grad = guarded(c.n)
    if c.gate is not None:
        rc = L.wm_mse_fwd_bwd_gated(p(a), p(b), p(grad), c.gscale, p(gate), p(gd), p(part), npt, c.n, stream)
    else:
        rc = L.wm_mse_fwd_bwd(p(a), p(b), p(grad), c.gscale, p(gd), p(part), npt, c.n, stream)
    _lib.check(rc, c.label)
    return c.check(part, grad, nparts=npt) + around_ok(c.label, gbuf, c.n)


def test_mse_fwd_bwd_and_gated():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for n in SX.FLAT_N:
            for gate, gdev in ((None, None), (None, 1.5), (0.8, None), (0.8, 1.5)):
                c = SX.mse_case(n, 0.7, gdev, gate)
                kernel = "mse_fwd_bwd_gated" if gate is not None else "mse_fwd_bwd"
                r.add(kernel, _run_mse(c, ops, L, _lib, stream))
                for npt in nparts_of(n):
                    r.add(kernel, _run_mse(c, ops, L, _lib, stream, npt))


def test_mse_fwd_bwd_above_the_partial_cap():
    """n = 4096 * 1024 + 4097: the wrapper's 1024 partials, every thread 17 trips; index-pattern data, the loss half only (no gradient
    buffer: two 17 MB operands move)"""
    _lib, ops, L, stream = _mods()
    with Run() as r:
        c = SX.mse_case(SX.MSE_LARGE, 0.7, None, None, "pattern")
        part, grad = ops.mse_fwd_bwd(dev(c.a), dev(c.b), c.gscale, want_grad=False)
        assert grad is None and part.numel() == 1024
        r.add("mse_fwd_bwd", c.check(part, None))


def test_sumsq_and_nonfinite():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for n in SX.FLAT_N:
            c = SX.SumsqCase(n)
            x = dev(c.x)
            r.add("sumsq", c.check(ops.sumsq(x)))
            for npt in nparts_of(n):
                part = filled(npt)
                _lib.check(L.wm_sumsq(p(x), n, p(part), npt, stream), c.label)
                r.add("sumsq", c.check(part))
        for key in SX.NONFINITE_KEYS:
            c = SX.NonfiniteCase(*key)
            x = dev(c.x)
            r.add("nonfinite", c.check(ops.nonfinite(x)))
            for npt in nparts_of(c.n):
                part = filled(npt)
                _lib.check(L.wm_nonfinite(p(x), c.n, p(part), npt, stream), c.label)
                r.add("nonfinite", c.check(part))


def test_image_grad_mse():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for key in SX.image_grad_keys():
            c = SX.ImageGradMseCase(*key)
            g = c.g().cuda().reshape(c.B, 1, c.HW, c.ld)
            a, b = dev(c.a).reshape(c.B, c.C, 1, c.HW), dev(c.b).reshape(c.B, c.C, 1, c.HW)
            out, part = ops.image_grad_mse(g, a, b, c.gscale, C=c.C, C_off=c.c0)
            r.add("image_grad_mse", c.check(out, part))
        c = SX.ImageGradMseCase(3, 3, 771, "bf16", 32, 5, gdev=1.5)
        g, a, b, gd = c.g().cuda(), dev(c.a), dev(c.b), scalar(c.gdev)
        n = c.a.size
        for npt in (SX.wrapper_nparts(n),) + SX.FREE_NPARTS:
            part = filled(npt)
            obuf, out = guarded(n)
            rc = L.wm_image_grad_mse(p(g), c.ld, c.c0, p(a), p(b), p(out), c.gscale, p(gd), p(part), npt, 3, 3, 1, 771, ops.dt_id(torch.bfloat16), stream)
            _lib.check(rc, c.label)
            r.add("image_grad_mse", c.check(out, part) + around_ok(c.label, obuf, n))


# ----------------------------------------------------------------------------------------------------------------- BCE with logits
def test_bce_logits():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for key in SX.BCE_LOGITS_KEYS:
            c = SX.bce_logits_case(*key)
            r.add("bce_logits", c.check(*ops.bce_logits(dev(c.x), float(c.t[0]), c.gscale, gscale_dev=scalar(c.gdev))))
        c = SX.bce_logits_case(257, False, 1.0, 1.5, False, True)
        gbuf, grad = guarded(c.n)
        loss = filled(1)
        x, gd = dev(c.x), scalar(c.gdev)
        _lib.check(L.wm_bce_logits(p(x), 1.0, c.n, c.gscale, p(gd), p(loss), p(grad), stream), c.label)
        r.add("bce_logits", c.check(loss, grad) + around_ok(c.label, gbuf, c.n))


def test_bce_logits_target():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for key in SX.BCE_TARGET_KEYS:
            c = SX.bce_logits_case(*key)
            x, t, gd = dev(c.x), dev(c.t), scalar(c.gdev)
            loss, grad = ops.bce_logits_target(x, t, c.gscale, chain_sigmoid=c.chain, gscale_dev=gd)
            r.add("bce_logits_target", c.check(loss, grad, nparts=SX.wrapper_nparts(c.n)))
            for npt in nparts_of(c.n):
                part, loss = filled(npt), filled(1)
                gbuf, grad = guarded(c.n)
                rc = L.wm_bce_logits_target(p(x), p(t), c.n, c.gscale, p(gd), p(part), npt, p(loss), p(grad), 1 if c.chain else 0, stream)
                _lib.check(rc, c.label)
                r.add("bce_logits_target", c.check(loss, grad, nparts=npt) + around_ok(c.label, gbuf, c.n))


# ----------------------------------------------------------------------------------------------------------------- message loss, metrics
def test_message_loss():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for key in SX.MESSAGE_KEYS:
            c = SX.message_loss_case(*key)
            r.add("message_loss", c.check(*ops.message_loss(dev(c.d), dev(c.m), c.gscale, gscale_dev=scalar(c.gdev))))
        c = SX.message_loss_case(257, 1.5, True)
        gbuf, grad = guarded(c.n)
        out = filled(4)
        d, m, gd = dev(c.d), dev(c.m), scalar(c.gdev)
        _lib.check(L.wm_message_loss(p(d), p(m), c.n, c.gscale, p(gd), p(out), p(grad), stream), c.label)
        r.add("message_loss", c.check(out[:2], grad) + around_ok(c.label, gbuf, c.n) +
              [SX.ECmp(c.label + " after out[1]", out[2:], np.full(2, SX.SENTINEL))])


def test_hidden_metrics():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for npt in SX.GATE_NPARTS:
            c = SX.HiddenMetricsCase(npt)
            out = ops.hidden_metrics(dev(c.partials), c.n_img, dev(c.msg2), dev(c.adv), dev(c.d_cover), dev(c.d_enc), *c.w)
            r.add("hidden_metrics", c.check(out))
        obuf = filled(9)
        ts = [dev(v) for v in (c.partials, c.msg2, c.adv, c.d_cover, c.d_enc)]
        rc = L.wm_hidden_metrics(p(ts[0]), c.nparts, c.n_img, p(ts[1]), p(ts[2]), p(ts[3]), p(ts[4]), *c.w, p(obuf[1:]), stream)
        _lib.check(rc, c.label)
        r.add("hidden_metrics", c.check(obuf[1:8]) + [SX.ECmp(c.label + " around out7", obuf[[0, 8]], np.full(2, SX.SENTINEL))])
