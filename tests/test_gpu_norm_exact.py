"""GPU: the instance-norm, Dice and two-source mask-head kernels per element against float64 (tests/norm_exact.py): csrc/instnorm.hip
(wm_instnorm_stats, _apply, _bwd_sums, _bwd_apply, _splits, _scratch_doubles), csrc/dice.hip (wm_dice_sums, _softmax_sums, _finalize, _bwd,
_softmax_bwd, _nparts) and csrc/mask_head.hip (wm_head2_fwd, _bwd, _finalize, _nparts), each entry point on its own through the typed
handle _lib.lib() -- apply and bwd_apply on float32 statistics no stats call would give -- and through the ops wrappers / glayers where
those pick a path.  Shapes: channel strides 16, 48 (idle threads) and the one-slot strides 1024 / 2048 with C < CP and NaN / +inf in the
padding channels; planes of 1 .. 513 pixels, 64 splits and the first size whose chunk grows; per-sample sizes around the 16-byte split
and past the 64-partial cap at three alignments; every class count and plane size of the softmax form, VEC and strided; every Cout and
lane-group width of the head, and one pixel past the forward's capped grid.

Every test prints one line per comparison and the largest observed multiple of the bound per kernel and dtype, with the element, before it
asserts (run with -s).  tests/test_cpu_norm_exact.py shows that these comparisons fail on the defects they are there to catch.

Measured on an MI355X against the float64 restatement (largest share of its bound; 0.5 is a correctly rounded float32 against the
1-ulp rule, and a 16-bit store lands next to its half ulp somewhere in every large tensor):
instnorm float32 stats 0.500 (mean, CP=1024 hw=2), apply 0.250 (CP=48 hw=513 B=3), bwd_sums 0.500 (mg), bwd_apply 0.220 (CP=16 hw=16384);
bfloat16 stats 0.500, apply 0.995, bwd_sums 0.500, bwd_apply 0.996; float16 stats 0.500, apply 0.998, bwd_sums 0.500, bwd_apply 0.999;
the layer float32 0.495 (dbeta, constant planes), bfloat16 0.995 (dx, cancellation plane), float16 0.984 (y).
dice_sums 0.168 (per=1 pw=2), dice_finalize 0.498 (loss), dice_bwd 0.249 (per=262149 pw=2, accumulate), dice_softmax_sums 0.087 (C=5 HW=1
pw=3), dice_softmax_bwd 0.494 (C=5 HW=1028 pw=1.5, dominated logits, per-sample upstream).
head2 float32 fwd 0.099, bwd 0.167 (ga), finalize 0.399 (dw, accumulate), second trip of the forward 0.006; bfloat16 fwd 0.099, bwd 0.994
(ga), finalize 0.466; float16 fwd 0.095, bwd 1.000 to three places and within it (ga: a 16-bit store next to its half ulp), finalize 0.457.  No kernel missed a bound."""
import time

import numpy as np
import pytest
import torch

import norm_exact as NX

pytestmark = pytest.mark.gpu
PAD = 8                                                    # guard elements on either side of a destination: 16 bytes at 16 bits, 32 in float32


def _mods():
    from video_watermarking_forgery_detection_amd import _lib, ops
    return _lib, ops, _lib.lib(), torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def dev(t):
    return None if t is None else t.cuda()


def f32dev(a):
    return None if a is None else NX.store(np.asarray(a, dtype=np.float64), "f32").cuda()


def guarded(shape, dt="f32", off=0, init=None):
    """a destination of `shape` inside a SENTINEL buffer, `off` elements past a 16-byte boundary: (whole buffer, the view a kernel writes)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD + off,), NX.SENTINEL, dtype=NX.TORCH[dt], device="cuda")
    view = buf[PAD + off:PAD + off + n].view(shape)
    if init is not None:
        view.copy_(init)
    assert (view.data_ptr() % 16) == (off * buf.element_size()) % 16
    return buf, view


def around(what, buf, view, off=0):
    b, n = NX.f64(buf), view.numel()
    rest = np.concatenate([b[:PAD + off], b[PAD + off + n:]])
    return [NX.ECmp(what + " around the destination", rest, np.full(rest.shape, NX.SENTINEL))]


def placed(a, off):
    """a float32 device copy of `a` whose first element lies `off` elements past a 16-byte boundary"""
    t = NX.store(np.asarray(a, dtype=np.float64), "f32")
    buf = torch.empty(t.numel() + off + 4, dtype=torch.float32, device="cuda")
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * off
    return view


def same_bits(what, a, b):
    return [NX.ECmp(what + " two runs, same bits", NX.f64(a), NX.f64(b))] + ([] if torch.equal(a, b) else [NX.ECmp(what + " torch.equal", [1.0], [0.0])])


class Run:
    """prints the wall time and, per kernel, the worst multiple of the bound with the comparison it occurred in, then asserts everything"""

    def __enter__(self):
        print()
        torch.cuda.synchronize()
        self.t, self.worst, self.cmps = time.perf_counter(), {}, []
        return self

    def add(self, kernel, cmps):
        for c in cmps:
            print("  ", c.line())
            if not c.exact and c.worst >= self.worst.get(kernel, (-1.0, ""))[0]:
                self.worst[kernel] = (c.worst, c.what)
        self.cmps += cmps

    def __exit__(self, et, ev, tb):
        torch.cuda.synchronize()
        print("   wall time %.2f s" % (time.perf_counter() - self.t))
        for k, (v, what) in sorted(self.worst.items()):
            print("   worst multiple of the bound  %-28s %.3f  in %s" % (k, v, what))
        if et is None:
            for c in self.cmps:
                c.assert_ok()
                assert c.skipped == 0


# ----------------------------------------------------------------------------------------------------------------- instance normalisation
def in_run(r, c, again=False):
    _lib, ops, L, stream = _mods()
    dt, B, hw, C, CP, did = c.dt, c.B, c.hw, c.C, c.CP, NX.WM_DT[c.dt]
    x, dy = c.t_x().cuda(), c.t_dy().cuda()
    gamma, beta = dev(c.t_gamma()), dev(c.t_beta())
    S = L.wm_instnorm_splits(hw)
    assert S == NX.in_splits(hw) and L.wm_instnorm_scratch_doubles(B, hw, CP) == NX.in_scratch_doubles(B, hw, CP)
    part = torch.full((NX.in_scratch_doubles(B, hw, CP),), NX.SENTINEL, dtype=torch.float64, device="cuda")
    k = "instnorm %s " % dt
    # stats
    mb, mean = guarded((B, CP))
    rb, rstd = guarded((B, CP))
    _lib.check(L.wm_instnorm_stats(p(x), p(part), p(mean), p(rstd), B, hw, C, CP, c.eps, did, stream), c.label)
    r.add(k + "stats", c.check_stats(mean, rstd) + around(c.label + " mean", mb, mean) + around(c.label + " rstd", rb, rstd))
    # apply, on statistics of its own
    sm, sr, smg, smgx = (c.t_rows(n).cuda() for n in ("smean", "srstd", "smg", "smgx"))
    yb, y = guarded((B, hw, CP), dt)
    _lib.check(L.wm_instnorm_apply(p(x), p(sm), p(sr), p(gamma), p(beta), p(y), B, hw, C, CP, c.act, did, stream), c.label)
    r.add(k + "apply", c.check_apply(y) + around(c.label + " y", yb, y))
    # bwd_sums: the finalise launch (dgamma given) and, at one split, the direct store (dgamma NULL)
    got = {}
    for params in ((True, False) if c.affine else (False,)):
        gb_, mg = guarded((B, CP))
        xb_, mgx = guarded((B, CP))
        dgamma = torch.full((C,), NX.SENTINEL, device="cuda") if params else None
        dbeta = torch.full((C,), NX.SENTINEL, device="cuda") if params else None
        _lib.check(L.wm_instnorm_bwd_sums(p(x), p(dy), p(sm), p(sr), p(gamma), p(beta), p(part), p(mg), p(mgx), p(dgamma), p(dbeta), B, hw, C, CP, c.act,
                                          did, stream), c.label)
        r.add(k + "bwd_sums", c.check_sums(mg, mgx, dgamma, dbeta) + around(c.label + " mg", gb_, mg) + around(c.label + " mgx", xb_, mgx))
        got[params] = (mg, mgx)
    if len(got) == 2:
        r.add(k + "bwd_sums", same_bits(c.label + " mg with and without dgamma (%d split)" % S, got[True][0], got[False][0])
              + same_bits(c.label + " mgx with and without dgamma", got[True][1], got[False][1]))
    # bwd_apply, on means of its own
    db_, dx = guarded((B, hw, CP), dt)
    _lib.check(L.wm_instnorm_bwd_apply(p(x), p(dy), p(sm), p(sr), p(gamma), p(beta), p(smg), p(smgx), p(dx), B, hw, C, CP, c.act, did, stream), c.label)
    r.add(k + "bwd_apply", c.check_bwd_apply(dx) + around(c.label + " dx", db_, dx))
    if again:
        y2, dx2 = torch.empty_like(y), torch.empty_like(dx)
        _lib.check(L.wm_instnorm_apply(p(x), p(sm), p(sr), p(gamma), p(beta), p(y2), B, hw, C, CP, c.act, did, stream), c.label)
        _lib.check(L.wm_instnorm_bwd_apply(p(x), p(dy), p(sm), p(sr), p(gamma), p(beta), p(smg), p(smgx), p(dx2), B, hw, C, CP, c.act, did, stream), c.label)
        r.add(k + "apply", same_bits(c.label + " y", y, y2))
        r.add(k + "bwd_apply", same_bits(c.label + " dx", dx, dx2))


@pytest.mark.parametrize("dt", NX.DTYPES)
def test_instnorm_entry_points(dt):
    with Run() as r:
        for key in NX.in_keys(dt):
            c = NX.in_case(*key)
            assert c.ambiguous == 0
            in_run(r, c, again=c.hw in (257, 16385))


@pytest.mark.parametrize("dt", NX.DTYPES)
def test_instnorm_chained_through_the_layer(dt):
    """glayers.InstanceNorm2d (+ ReLU, affine) on the case with the two constant planes -- y exactly beta as stored, dx exactly 0 behind the
    ReLU that masks them -- and on the cancellation plane 1000 + N(0, 1)"""
    from video_watermarking_forgery_detection_amd import glayers as G
    with Run() as r:
        for kind, hw, B, act in (("const", 257, 3, 1), ("cancel", 513, 1, 0)):
            c = NX.in_case(dt, 16, 13, hw, B, 1, act, NX.IN_EPS[0], kind)
            m = G.InstanceNorm2d(c.C, eps=c.eps, affine=True, act="relu" if act else None).cuda()
            with torch.no_grad():
                m.weight.copy_(c.t_gamma()), m.bias.copy_(c.t_beta())
            x = c.t_x().cuda().view(c.B, c.hw, 1, c.CP).requires_grad_(True)
            y = m(x)
            y.backward(c.t_dy().cuda().view(y.shape))
            r.add("instnorm %s layer" % dt, c.check_chain(y.detach().view(c.B, c.hw, c.CP), x.grad.view(c.B, c.hw, c.CP), m.weight.grad, m.bias.grad))


def test_instnorm_refusals_and_split_rule():
    _lib, ops, L, stream = _mods()
    for hw in NX.IN_SPLIT_SIZES:
        assert L.wm_instnorm_splits(hw) == NX.in_splits(hw) == ops.instnorm_splits(hw), hw
        assert L.wm_instnorm_scratch_doubles(3, hw, 48) == NX.in_scratch_doubles(3, hw, 48), hw
    for dt in NX.DTYPES:
        did, CP = NX.WM_DT[dt], NX.IN_REFUSED_CP[dt]
        x = torch.zeros(2 * CP + 16, dtype=NX.TORCH[dt], device="cuda")
        y, d = torch.zeros_like(x), torch.zeros_like(x)
        v = [torch.zeros(CP, device="cuda") for _ in range(8)]
        part = torch.zeros(4 * CP, dtype=torch.float64, device="cuda")
        m, rs, ga, be, mg, mgx, dga, dbe = v

        def calls(xp, CPc, gam=ga, bet=be, dg=dga, dbt=dbe):
            return (L.wm_instnorm_stats(xp, p(part), p(m), p(rs), 1, 2, 13, CPc, 1e-5, did, stream),
                    L.wm_instnorm_apply(xp, p(m), p(rs), p(gam), p(bet), p(y), 1, 2, 13, CPc, 1, did, stream),
                    L.wm_instnorm_bwd_sums(xp, p(d), p(m), p(rs), p(gam), p(bet), p(part), p(mg), p(mgx), p(dg), p(dbt), 1, 2, 13, CPc, 1, did, stream),
                    L.wm_instnorm_bwd_apply(xp, p(d), p(m), p(rs), p(gam), p(bet), p(mg), p(mgx), p(y), 1, 2, 13, CPc, 1, did, stream))

        assert calls(p(x), CP) == (NX.WM_E_SHAPE,) * 4, dt                       # more than 256 16-byte vectors per pixel
        assert calls(p(x) + x.element_size(), 16) == (NX.WM_E_SHAPE,) * 4, dt    # a misaligned activation
        assert calls(p(x), 16, bet=None)[1:] == (NX.WM_E_BADARG,) * 3, dt        # gamma without beta
        assert calls(p(x), 16, dbt=None)[2] == NX.WM_E_BADARG, dt                # dgamma without dbeta
        assert calls(p(x), 16) == (NX.WM_OK,) * 4, dt
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- Dice
def gdev_of(m):
    return (None if m.get("gdev") is None else f32dev([m["gdev"]])), (None if m.get("gout") is None else f32dev(m["gout"]))


def test_dice_binary():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for key in NX.DICE_BIN_KEYS:
            c = NX.dice_bin_case(*key)
            B, per, P = c.B, c.per, L.wm_dice_nparts(c.per)
            assert P == NX.dice_nparts(per)
            coef_in = torch.from_numpy(c.coef).cuda()
            for off in NX.DICE_OFFSETS:
                pt, tt = placed(c.p, off[0]), placed(c.t, off[1])
                part = torch.full((B * P * 3 + 2,), NX.SENTINEL, dtype=torch.float64, device="cuda")
                _lib.check(L.wm_dice_sums(p(pt), p(tt), B, per, c.pw, p(part[1:]), stream), c.label)
                q = part[1:-1]
                lab = "%s offsets %s" % (c.label, off)
                r.add("dice_sums", [NX.ECmp(lab + " sums per unit", NX.f64(q).reshape(B, P, 3).sum(1), c.S, c.bS),
                                    NX.ECmp(lab + " around the partials", NX.f64(part[[0, -1]]), [NX.SENTINEL] * 2)])
                if off == (0, 0):
                    for red, rid in NX.REDUCTIONS.items():
                        coef = torch.full((B, 2), NX.SENTINEL, dtype=torch.float64, device="cuda")
                        lb, loss = guarded((B if red == "none" else 1,))
                        _lib.check(L.wm_dice_finalize(p(q), B, 1, per, NX.SMOOTH, rid, -1, None, p(coef), p(loss), stream), c.label)
                        r.add("dice_finalize", NX.check_finalize(c.label, coef, loss, NX.f64(q), B, 1, NX.SMOOTH, red) + around(c.label + " loss", lb, loss))
                    l2, _ = ops.dice_binary_fwd(pt.view(B, per), tt.view(B, per), NX.SMOOTH, c.pw, "mean")
                    r.add("dice_finalize", [NX.ECmp(c.label + " ops.dice_binary_fwd, same bits", NX.f64(l2), NX.f64(ops.dice_binary_fwd(pt, tt, NX.SMOOTH, c.pw)[0]))])
                for mode in (NX.BIN_GRAD_MODES if off == (0, 0) else NX.BIN_GRAD_MODES[4:]):
                    if off[0] != off[1] and per > 4097:
                        continue
                    m = NX.resolve_mode(mode, B)
                    gd, go = gdev_of(m)
                    gbuf, grad = guarded((B, per), "f32", off[0], init=NX.store(c.old, "f32").cuda() if m.get("accumulate") else None)
                    _lib.check(L.wm_dice_bwd(p(pt), p(tt), p(coef_in), p(grad), B, per, c.pw, NX.REDUCTIONS[m.get("reduction", "mean")], p(go),
                                             m.get("gscale", 1.0), p(gd), int(m.get("chain", False)), int(m.get("accumulate", False)), stream), c.label)
                    r.add("dice_bwd", c.check_grad(grad, **m) + around(lab + " grad", gbuf, grad, off[0]))


def test_dice_softmax():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for key in NX.dice_soft_keys():
            c = NX.dice_soft_case(*key)
            B, C, HW, P = c.B, c.C, c.HW, L.wm_dice_nparts(c.HW)
            assert P == NX.dice_nparts(HW)
            coef_in, wdev = torch.from_numpy(c.coef).cuda(), f32dev(c.weight)
            big = HW > 4096
            for off in ((0, 1) if HW % 4 == 0 and not big else (0,)):      # HW % 4 == 0 and aligned: VEC; one element on, or HW odd: strided
                zt, tt = placed(c.z, off), placed(c.t, off)
                lab = "%s offset %d" % (c.label, off)
                part = torch.full((B * C * P * 3 + 2,), NX.SENTINEL, dtype=torch.float64, device="cuda")
                _lib.check(L.wm_dice_softmax_sums(p(zt), p(tt), B, C, HW, c.pw, p(part[1:]), stream), c.label)
                q = part[1:-1]
                r.add("dice_softmax_sums", [NX.ECmp(lab + " sums per unit", NX.f64(q).reshape(B, C, P, 3).sum(2), c.S, c.bS),
                                            NX.ECmp(lab + " around the partials", NX.f64(part[[0, -1]]), [NX.SENTINEL] * 2)])
                if off == 0 and not big:
                    for red, ig, wt in (("mean", -1, None), ("sum", 0, c.weight), ("none", C - 1, None)):
                        coef = torch.full((B * C, 2), NX.SENTINEL, dtype=torch.float64, device="cuda")
                        lb, loss = guarded((B if red == "none" else 1,))
                        _lib.check(L.wm_dice_finalize(p(q), B, C, HW, NX.SMOOTH, NX.REDUCTIONS[red], ig, p(wdev if wt is not None else None), p(coef), p(loss),
                                                      stream), c.label)
                        r.add("dice_finalize", NX.check_finalize(c.label, coef, loss, NX.f64(q), B, C, NX.SMOOTH, red, ig, wt) + around(c.label + " loss", lb, loss))
                for mode in (NX.SOFT_GRAD_MODES if off == 0 and not big else NX.SOFT_GRAD_MODES[3:4]):
                    m = NX.resolve_mode(mode, B, C)
                    gd, go = gdev_of(m)
                    gbuf, grad = guarded((B, C, HW), "f32", off, init=NX.store(c.old, "f32").cuda() if m.get("accumulate") else None)
                    _lib.check(L.wm_dice_softmax_bwd(p(zt), p(tt), p(coef_in), p(grad), B, C, HW, c.pw, NX.REDUCTIONS[m.get("reduction", "mean")],
                                                     m.get("ignore_index", -1), p(wdev if m.get("weighted") else None), p(go), m.get("gscale", 1.0), p(gd),
                                                     int(m.get("accumulate", False)), stream), c.label)
                    r.add("dice_softmax_bwd", c.check_grad(grad, **m) + around(lab + " grad", gbuf, grad, off))
        z = torch.zeros(33 * 4, device="cuda")
        part = torch.zeros(33 * 3, dtype=torch.float64, device="cuda")
        assert L.wm_dice_softmax_sums(p(z), p(z), 1, 33, 4, 2.0, p(part), stream) == NX.WM_E_BADARG
        assert L.wm_dice_softmax_bwd(p(z), p(z), p(part), p(z), 1, 33, 4, 2.0, 0, -1, None, None, 1.0, None, 0, stream) == NX.WM_E_BADARG


# ----------------------------------------------------------------------------------------------------------------- two-source mask head
def head_run(r, c, bwd=True):
    _lib, ops, L, stream = _mods()
    did, k = NX.WM_DT[c.dt], "head2 %s " % c.dt
    a, b, w, bias = c.t_a().cuda(), c.t_b().cuda(), f32dev(c.w), f32dev(c.bias)
    ob, out = guarded((c.B, c.Cout, c.hw))
    _lib.check(L.wm_head2_fwd(p(a), c.lda, c.na, p(b), c.ldb, c.nb, p(w), p(bias), p(out), c.B, c.hw, c.Cout, c.act, did, stream), c.label)
    r.add(k + "fwd", c.check_fwd(out) + around(c.label + " out", ob, out))
    if not bwd:
        return
    nparts = L.wm_head2_nparts(c.npix)
    assert nparts == c.nparts == NX.head_nparts(c.npix)
    ncol = c.Cout * (c.na + c.nb + 1)
    gout, saved = f32dev(c.gout), f32dev(c.saved)
    gab, ga = guarded((c.npix, c.lda), c.dt)
    gbb, gb = guarded((c.npix, c.ldb), c.dt)
    part = torch.full((nparts * ncol + 2,), NX.SENTINEL, dtype=torch.float64, device="cuda")
    _lib.check(L.wm_head2_bwd(p(a), c.lda, c.na, p(b), c.ldb, c.nb, p(w), p(gout), p(saved), int(c.chain), p(ga), c.lda, p(gb), c.ldb, p(part[1:]), c.B, c.hw,
                              c.Cout, did, stream), c.label)
    r.add(k + "bwd", c.check_bwd(ga, gb) + c.check_partials(part[1:-1]) + around(c.label + " ga", gab, ga) + around(c.label + " gb", gbb, gb)
          + [NX.ECmp(c.label + " around the partials", NX.f64(part[[0, -1]]), [NX.SENTINEL] * 2)])
    for acc in (False, True):
        wb_, dw = guarded((c.Cout, c.na + c.nb), init=f32dev(c.old_w) if acc else None)
        bb_, db = guarded((c.Cout,), init=f32dev(c.old_b) if acc else None)
        _lib.check(L.wm_head2_finalize(p(part[1:]), nparts, c.Cout, c.na + c.nb, p(dw), p(db), int(acc), stream), c.label)
        r.add(k + "finalize", c.check_params(dw, db, accumulate=acc) + around(c.label + " dw", wb_, dw) + around(c.label + " db", bb_, db))


@pytest.mark.parametrize("dt", NX.DTYPES)
def test_head2_entry_points(dt):
    _lib, ops, L, stream = _mods()
    with Run() as r:
        for key in NX.head_keys(dt):
            head_run(r, NX.head_case(*key))
        c = NX.head_case(*NX.head_keys(dt)[-1])                             # the wrappers: same cases, same comparisons, same bits twice
        a, b = c.t_a().cuda().view(c.B, c.hw, 1, c.lda), c.t_b().cuda().view(c.B, c.hw, 1, c.ldb)
        w, bias = f32dev(c.w), f32dev(c.bias)
        out = ops.head2_fwd(a, c.na, b, c.nb, w, bias, c.act)
        res = ops.head2_bwd(a, c.na, b, c.nb, w, f32dev(c.gout).view(out.shape), f32dev(c.saved).view(out.shape) if c.chain else None)
        res2 = ops.head2_bwd(a, c.na, b, c.nb, w, f32dev(c.gout).view(out.shape), f32dev(c.saved).view(out.shape) if c.chain else None)
        r.add("head2 %s ops" % dt, c.check_fwd(out.view(c.B, c.Cout, c.hw)) + c.check_bwd(res[0].view(c.npix, c.lda), res[1].view(c.npix, c.ldb))
              + c.check_params(res[2], res[3]) + [x for u, v in zip(res, res2) for x in same_bits(c.label + " ops.head2_bwd", u, v)])


def test_head2_second_trip_and_refusals():
    _lib, ops, L, stream = _mods()
    with Run() as r:
        c = NX.head_case(*NX.head_big_key())
        assert c.G == 16 and c.npix == NX.HEAD_FWD_CAP * c.PPB * NX.HEAD_FWD_UNROLL + 1 and L.wm_head2_nparts(c.npix) == NX.HEAD_PARTS_CAP
        head_run(r, c, bwd=False)
    z = torch.zeros(256, device="cuda")
    d = torch.zeros(256, dtype=torch.float64, device="cuda")
    assert L.wm_head2_fwd(p(z), 16, 13, p(z), 16, 5, p(z), None, p(z), 1, 1, 5, 0, 0, stream) == NX.WM_E_SHAPE
    assert L.wm_head2_bwd(p(z), 16, 13, p(z), 16, 5, p(z), p(z), None, 0, p(z), 16, p(z), 16, p(d), 1, 1, 5, 0, stream) == NX.WM_E_SHAPE
    assert L.wm_head2_finalize(p(d), 1, 5, 18, p(z), p(z), 0, stream) == NX.WM_E_BADARG
    assert L.wm_head2_fwd(p(z), 16, 13, p(z), 16, 5, p(z), None, p(z), 1, 1, 4, 0, 0, stream) == NX.WM_OK
    assert [L.wm_head2_nparts(n) for n in (1, 128, 129)] == [NX.head_nparts(n) for n in (1, 128, 129)]
    torch.cuda.synchronize()
