"""GPU: the BatchNorm, pooling, head, up-convolution and layout kernels (csrc/bn.hip, csrc/heads.hip, csrc/unet.hip, csrc/upconv_mfma.hip,
csrc/layout.hip) per element against float64 (tests/layers_exact.py), at the smallest shapes that take each path: the in-place row fold above 256 partial
rows in its vector and its scalar form, count == 1 and a negative raw variance, the 1024- and 256-thread backward passes with one, two
and 64 vectors per pixel, a per-sample gradient whose block straddles samples, the 256-row and 64-slice grid caps, strided operands
with sentinel-filled gaps, ragged up-conv tiles, the f16 twin of the MFMA up-conv, the 1x1 head's four-pixel trip, its act16 copy and its BatchNorm rows, and
every stage of the pooled head.

Every bound follows from the number formats and the operation counts (derived in tests/layers_exact.py); counts, pooling, copies, zero
padding and the bytes around strided destinations are exact.  Every test prints one line per comparison (run with -s).
tests/test_cpu_layers_exact.py shows that these comparisons fail on the defects they are there to catch.  Where ops.* hides an argument
a case needs (a stride, the count, dbias_partials) the call goes to _lib.lib() directly."""
import numpy as np
import pytest
import torch

import layers_exact as LX

pytestmark = pytest.mark.gpu


def dev(a, dt="f32"):
    return None if a is None else (a if torch.is_tensor(a) else LX.store(a, dt)).cuda()


def report(cmps):
    for c in cmps:
        print("  ", c.line())
    for c in cmps:
        c.assert_ok()


def _mods():
    from video_watermarking_forgery_detection_amd import _lib, ops
    return _lib, ops, ops._p, torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------------------------------------------------------------------- finalisations
@pytest.mark.parametrize("running", [True, False], ids=["running", "no_running"])
def test_bn_finalize(running):
    _lib, ops, _p, _ = _mods()
    print()
    for key in LX.BN_FINALIZE_CASES:
        c = LX.bn_finalize_case(*key)
        rows = dev(c.rows)                                  # a fresh copy: the call folds the rows in place
        rm, rv = (dev(c.rmean), dev(c.rvar)) if running else (None, None)
        st = ops.bn_finalize(rows, c.C, c.CP, c.count, dev(c.gamma), dev(c.beta), rm, rv, LX.MOMENTUM, LX.BN_EPS)
        out = {"scale": st[0], "shift": st[1], "mean": st[2], "invstd": st[3], "running_mean": rm, "running_var": rv}
        report(c.check(out, running))


@pytest.mark.parametrize("kind", LX.BWD_FIN_KINDS)
def test_bn_bwd_finalize(kind):
    _lib, ops, _p, stream = _mods()
    L = _lib.lib()
    print()
    for key in LX.BN_BWD_FINALIZE_CASES:
        if key[0] != kind:
            continue
        c = LX.bn_bwd_finalize_case(*key)
        gamma, mean, invstd = dev(c.gamma), dev(c.mean), dev(c.invstd)
        dgamma, dbeta = dev(c.dgamma0), dev(c.dbeta0)
        coef = torch.full((3, c.CP), LX.SENTINEL, device="cuda", dtype=torch.float32)
        if kind == "pooled":
            gvec, npos, ysum = dev(c.gvec), dev(c.npos), dev(c.ysum)
            rc = L.wm_bn_bwd_finalize_pooled(_p(gvec), _p(npos), _p(ysum), c.n, c.C, c.CP, c.count, _p(gamma), _p(mean), _p(invstd), _p(dgamma),
                                             _p(dbeta), c.accumulate, _p(coef), stream)
            _lib.check(rc, "wm_bn_bwd_finalize_pooled")
            report(c.check_rows(ops.pooled_bwd_rows(gvec, (npos, ysum))))
        elif kind == "raw":
            rows = dev(c.rows)
            rc = L.wm_bn_bwd_finalize_raw(_p(rows), c.n, c.C, c.CP, c.count, _p(gamma), _p(mean), _p(invstd), _p(dgamma), _p(dbeta), c.accumulate,
                                          _p(coef), stream)
            _lib.check(rc, "wm_bn_bwd_finalize_raw")
        else:
            rows = dev(c.rows)
            rc = L.wm_bn_bwd_finalize(_p(rows), c.n, c.C, c.CP, c.count, _p(gamma), _p(invstd), _p(dgamma), _p(dbeta), c.accumulate, _p(coef), stream)
            _lib.check(rc, "wm_bn_bwd_finalize")
        report(c.check({"dgamma": dgamma, "dbeta": dbeta, "coef": coef}))


def test_colsum_finalize():
    _lib, ops, _p, _ = _mods()
    print()
    for key in LX.COLSUM_CASES:
        c = LX.colsum_case(*key)
        out = dev(c.out0)
        ops.colsum(dev(c.rows), c.C, c.ldp, out, bool(c.accumulate))
        report(c.check(out))


# ----------------------------------------------------------------------------------------------------------------- BN backward passes
def _run_bn_bwd(c):
    _lib, ops, _p, stream = _mods()
    L = _lib.lib()
    dtid = ops.dt_id(LX.TORCH[c.dt])
    g, gvec, y = (dev(t) for t in c.operands())
    sc, sh, mu, isd, coef = dev(c.sc), dev(c.sh), dev(c.mu), dev(c.isd), dev(c.coef)
    nparts = L.wm_bn_bwd_nparts(c.npix)
    assert nparts == LX.bn_bwd_nparts(c.npix)
    ldg = 0 if g is None else c.ld
    rows = torch.full((nparts, 2, c.CP), LX.SENTINEL, device="cuda", dtype=torch.float32)
    rc = L.wm_bn_bwd_reduce(_p(g), ldg, _p(gvec), _p(y), c.ld, _p(sc), _p(sh), _p(mu), _p(isd), _p(rows), c.B, c.hw, c.CP, dtid, stream)
    _lib.check(rc, "wm_bn_bwd_reduce")
    cm = c.check_reduce(rows)
    for form in ("1024 threads, dbias rows", "256 threads"):
        dy = LX.sentinel_dest(c.npix, c.ld, c.dt).cuda()
        bias = torch.full((nparts, c.CP), LX.SENTINEL, device="cuda", dtype=torch.float32) if form.startswith("1024") else None
        rc = L.wm_bn_bwd_apply(_p(g), ldg, _p(gvec), _p(y), c.ld, _p(sc), _p(sh), _p(mu), _p(isd), _p(coef), _p(dy), c.ld, _p(bias), c.B, c.hw,
                               c.CP, dtid, stream)
        _lib.check(rc, "wm_bn_bwd_apply")
        cm += c.check_apply(dy, bias, form)
    return cm


@pytest.mark.parametrize("dt", LX.DTYPES)
def test_bn_bwd_reduce_and_apply(dt):
    print()
    for row in LX.bn_bwd_cases(dt):
        report(_run_bn_bwd(LX.bn_bwd_case(dt, *row)))


@pytest.mark.parametrize("gform", ["g", "gvec"])
def test_bn_bwd_above_the_grid_cap(gform):
    """2 x 147456 pixels at CP = 32, bf16: 288 blocks' worth of pixels on 256 workgroups, several trips in both sweep directions"""
    dt, CP, B, hw = LX.BWD_LARGE
    print()
    report(_run_bn_bwd(LX.BnBwdCase(dt, CP, B, hw, gform, 0)))


# ----------------------------------------------------------------------------------------------------------------- average pool, copy
@pytest.mark.parametrize("dt", LX.DTYPES)
def test_bnrelu_avgpool(dt):
    _lib, ops, _p, stream = _mods()
    L = _lib.lib()
    dtid = ops.dt_id(LX.TORCH[dt])
    print()
    for row in LX.avgpool_cases(dt):
        c = LX.avgpool_case(dt, *row)
        y, sc, sh = dev(c.operand()), dev(c.sc), dev(c.sh)
        S = L.wm_avgpool_slices(c.hw)
        assert S == LX.avgpool_slices(c.hw)
        ws = torch.empty(c.B * S * 3 * c.CP, device="cuda", dtype=torch.float32)
        out = torch.full((c.B, c.CP), LX.SENTINEL, device="cuda", dtype=torch.float32)
        rc = L.wm_bnrelu_avgpool(_p(y), c.ld, _p(sc), _p(sh), _p(out), _p(ws), c.B, c.hw, c.CP, dtid, stream)
        _lib.check(rc, "wm_bnrelu_avgpool")
        out3 = torch.full((3, c.B, c.CP), LX.SENTINEL, device="cuda", dtype=torch.float32)
        rc = L.wm_bnrelu_avgpool_stats(_p(y), c.ld, _p(sc), _p(sh), _p(out3), _p(ws), c.B, c.hw, c.CP, dtid, stream)
        _lib.check(rc, "wm_bnrelu_avgpool_stats")
        report(c.check(out) + c.check(out3[0], out3[1], out3[2], form="stats"))


@pytest.mark.parametrize("dt", LX.DTYPES)
def test_bnrelu_copy(dt):
    _lib, ops, _p, _ = _mods()
    print()
    for C, c0, s in LX.copy_cases(dt):
        c = LX.CopyCase(dt, C, c0, s)
        x = dev(c.operand()).view(1, 1, c.npix, c.ldx)
        out = dev(c.dest()).view(1, 1, c.npix, c.ldy)
        ops.bnrelu_copy(x, dev(c.sc) if s else None, dev(c.sh) if s else None, out, c0, C)
        report(c.check(out.view(c.npix, c.ldy)))


# ----------------------------------------------------------------------------------------------------------------- max pool
@pytest.mark.parametrize("dt", LX.DTYPES)
def test_maxpool(dt):
    _lib, ops, _p, _ = _mods()
    print()
    for B, H, W in LX.POOL2_SHAPES:
        for C in LX.POOL2_C[dt]:
            c = LX.maxpool_case(dt, B, H, W, C)
            sc, sh = dev(c.sc), dev(c.sh)
            gp = dev(c.gp, dt)
            for c0a in (0, C):                              # c0a = C also runs y and g_skip strided, g_skip from channel C
                ldy = C + (LX.GAP if c0a else 0)
                y = dev(LX.strided(c.y.reshape(-1, C), ldy, dt)).view(B, H, W, ldy)
                act = dev(LX.sentinel_dest(B * H * W, c0a + C + LX.GAP, dt)).view(B, H, W, -1)
                pooled = ops.bnrelu_maxpool2(y, sc, sh, C, act, c0a)
                cm = c.check_fwd(pooled, act, c0a)
                cm += c.check_fwd(ops.bnrelu_maxpool2(y, sc, sh, C), None, 0)
                gs = dev(LX.strided(c.gs.reshape(-1, C), c0a + C + LX.GAP, dt, c0a)).view(B, H, W, -1)
                cm += c.check_bwd(ops.maxpool2_bwd(y, sc, sh, gp, gs, c0a, C), True)
                cm += c.check_bwd(ops.maxpool2_bwd(y, sc, sh, gp, None, 0, C), False)
                report(cm)


# ----------------------------------------------------------------------------------------------------------------- up-convolution
def _run_upconv(dt, mfma):
    _lib, ops, _p, _ = _mods()
    tdt = LX.TORCH[dt]
    for i, row in enumerate(LX.upconv_cases(mfma)):
        c = LX.upconv_case(dt, *row, w16=mfma)
        assert ops.upconv2x2_mfma_supported(c.Cin, c.Cout, tdt) == mfma, c.label
        xs, gys = c.operands()
        x, gy = dev(xs).view(c.B, c.H, c.W, c.ldx), dev(gys).view(c.B, 2 * c.H, 2 * c.W, c.ldy)
        sc, sh = (dev(c.sc), dev(c.sh)) if c.with_scale else (None, None)
        w, bias = dev(c.w), dev(c.bias)
        if c.ldx > c.Cin:                                   # ops takes Cin from w and the stride from x
            assert x.shape[-1] == c.ldx and w.shape[0] == c.Cin
        out = dev(c.dest()).view(c.B, 2 * c.H, 2 * c.W, c.ldy)
        ops.upconv2x2_fwd(x, sc, sh, w, bias, out, c.c0)
        cm = c.check_fwd(out)
        acc = bool(i % 2)
        dw, db = dev(c.dw0), dev(c.db0)
        gx = ops.upconv2x2_bwd(x, sc, sh, w, gy, c.c0, dw, db, acc)
        cm += c.check_bwd(gx, dw, db, acc)
        if mfma:
            cm += c.check_pack(*ops.upconv2x2_pack(w, tdt))
        else:
            assert (_lib.lib().wm_upconv2x2_dw_chunks(c.B, c.H, c.W) > 1) == (c.npix > 1024)
        report(cm)


@pytest.mark.parametrize("dt", LX.DTYPES)
def test_upconv_scalar(dt):
    print()
    assert any(B * H * W > 1024 for _, _, B, H, W, _, _, _ in LX.upconv_cases())
    _run_upconv(dt, False)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_upconv_mfma(dt):
    print()
    _run_upconv(dt, True)


# ----------------------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("dt", LX.DTYPES)
def test_layout(dt):
    _lib, ops, _p, _ = _mods()
    ve = LX.VE[dt]
    print()
    for B, H, W in LX.LAYOUT_SHAPES:
        c = LX.layout_case(dt, B, H, W)
        npix = B * H * W
        cm = []
        for planes, c0, tail, ld, what in ((c.img, 0, 13, 16, "image"), (c.planes, 8, 3, 8 + 5 + 3 + 16, "general")):
            buf = dev(LX.sentinel_dest(npix, ld, dt)).view(B, H, W, ld)
            ops.nchw_to_nhwc(dev(planes), buf, c0, tail)
            cm += c.check_nchw_to_nhwc(buf, planes, c0, tail, what)
            Cp = planes.shape[1]
            cm += c.check_nhwc_to_nchw(ops.nhwc_to_nchw(buf, Cp, c0), c.to_nhwc(planes), what)
        c0, tail = 2 * ve, 40
        ld = c0 + tail + 16
        buf = dev(LX.sentinel_dest(npix, ld, dt)).view(B, H, W, ld)
        msg, img = dev(c.msg), dev(c.img)                   # (named: a temporary's memory may be reused before the launch)
        rc = _lib.lib().wm_concat_tail(_p(msg), _p(img), _p(buf), B, 30, H, W, ld, c0, tail, ops.dt_id(LX.TORCH[dt]),
                                       torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "wm_concat_tail")
        cm += c.check_concat_tail(buf, c0, tail)
        buf = dev(LX.sentinel_dest(npix, c0 + 31, dt)).view(B, H, W, c0 + 31)
        ops.broadcast_to_nhwc(dev(c.msg), buf, c0)
        cm += c.check_broadcast(buf, c0)
        ldx = c.C + LX.GAP
        x = dev(LX.strided(c.x, ldx, dt)).view(B, H, W, ldx)
        full = dev(LX.sentinel_dest(npix, c.C + 40, dt)).view(B, H, W, c.C + 40)
        ops.concat_full(x, dev(c.sc), dev(c.sh), dev(c.msg), dev(c.img), full, c.C)
        cm += c.check_concat_full(full)
        report(cm)


# ----------------------------------------------------------------------------------------------------------------- 1x1 heads
@pytest.mark.parametrize("dt", LX.DTYPES)
def test_conv1x1_head_fwd(dt):
    _lib, ops, _p, stream = _mods()
    L = _lib.lib()
    dtid = ops.dt_id(LX.TORCH[dt])
    print()
    for row in LX.head_fwd_cases(dt):
        c = LX.HeadCase(dt, *row)
        y, w, bias = dev(c.operand()), dev(c.w), dev(c.bias)
        sc, sh = (dev(c.sc), dev(c.sh)) if c.with_scale else (None, None)
        cm = []
        for act in (0, 1):
            out = torch.full((c.B, c.Cout, c.hw), LX.SENTINEL, device="cuda", dtype=torch.float32)
            rc = L.wm_conv1x1_head_fwd(_p(y), c.ld, _p(sc), _p(sh), _p(w), _p(bias), _p(out), c.B, c.hw, c.Cin, c.Cout, act, dtid, stream)
            _lib.check(rc, "wm_conv1x1_head_fwd")
            cm += c.check_fwd(out, act)
        out = torch.full((c.B, c.Cout, c.hw), LX.SENTINEL, device="cuda", dtype=torch.float32)
        a16 = LX.sentinel_dest(c.npix, 16, dt).cuda()
        rc = L.wm_conv1x1_head_fwd_act(_p(y), c.ld, _p(sc), _p(sh), _p(w), _p(bias), _p(out), _p(a16), c.B, c.hw, c.Cin, c.Cout, 0, dtid, stream)
        _lib.check(rc, "wm_conv1x1_head_fwd_act")
        cm += c.check_fwd(out, 0, a16)
        report(cm)


@pytest.mark.parametrize("dt", LX.DTYPES)
def test_conv1x1_head_bwd(dt):
    _lib, ops, _p, stream = _mods()
    L = _lib.lib()
    dtid = ops.dt_id(LX.TORCH[dt])
    print()
    for i, row in enumerate(LX.head_bwd_cases(dt)):
        c = LX.HeadCase(dt, *row)
        acc = bool(i % 2)
        y, w, gout = dev(c.operand()), dev(c.w), dev(c.gout)
        sc, sh = (dev(c.sc), dev(c.sh)) if c.with_scale else (None, None)
        nparts = L.wm_conv1x1_head_nparts(c.npix)
        assert nparts == LX.head_nparts(c.npix)
        ldp = c.Cout * (c.Cin + 1)
        for with_bn in ((False, True) if c.with_scale else (False,)):
            part = torch.full((nparts, ldp), LX.SENTINEL, device="cuda", dtype=torch.float32)
            bnp = torch.full((nparts, 2, c.Cin), LX.SENTINEL, device="cuda", dtype=torch.float32) if with_bn else None
            g = LX.sentinel_dest(c.npix, c.ld, dt).cuda()
            rc = L.wm_conv1x1_head_bwd(_p(y), c.ld, _p(sc), _p(sh), _p(w), _p(gout), _p(g), c.ld, _p(part), _p(bnp), c.B, c.hw, c.Cin, c.Cout,
                                       dtid, stream)
            _lib.check(rc, "wm_conv1x1_head_bwd")
            dw, db = dev(c.dw0), dev(c.db0)
            ops.colsum(part, c.Cout * c.Cin, ldp, dw, acc)                # folds the rows in place above 256: the scalar fold at this pitch
            ops.colsum(part[:(nparts if nparts <= 256 else 64), c.Cout * c.Cin:], c.Cout, ldp, db, acc)
            report(c.check_bwd(g, dw, db, acc, bnp))


# ----------------------------------------------------------------------------------------------------------------- linear / pooled heads
def test_linear_head():
    _lib, ops, _p, _ = _mods()
    print()
    for key in LX.LINEAR_CASES:
        c = LX.linear_case(*key)
        pooled, w, bias = dev(c.pooled), dev(c.w), dev(c.bias)
        assert pooled.shape[1] == c.ldp > c.I
        cm = c.check_fwd(ops.linear_head_fwd(pooled, w, bias, c.I))
        dw, db = dev(c.dw0), dev(c.db0)
        gvec = ops.linear_head_bwd(pooled, w, dev(c.gout), dw, db, bool(c.accumulate), c.CP, LX.INV_HW)
        report(cm + c.check_bwd(dw, db, gvec))


@pytest.mark.parametrize("kind", [0, 1])
def test_pooled_head(kind):
    _lib, ops, _p, _ = _mods()
    print()
    for key in LX.LINEAR_CASES:
        c = LX.linear_case(*key)
        assert ops.pooled_head_supported(c.B, c.CP, c.I, c.O)
        out3, w, bias = dev(c.out3), dev(c.w), dev(c.bias)
        dw, db, dgamma, dbeta = dev(c.dw0), dev(c.db0), dev(c.dgamma0), dev(c.dbeta0)
        stats = torch.zeros(4, c.CP, device="cuda", dtype=torch.float32)
        stats[2, :c.C], stats[3, :c.C] = dev(c.mean), dev(c.invstd)
        logits, loss, gvec, coef = ops.pooled_head(out3, c.I, w, bias, kind, c.target, dev(c.msg) if kind == 1 else None, c.gscale, None, dw, db,
                                                   bool(c.accumulate), LX.INV_HW, c.C, c.count, dev(c.gamma), stats, dgamma, dbeta)
        report(c.check_pooled_head(kind, logits, loss, dw, db, gvec, dgamma, dbeta, coef))
