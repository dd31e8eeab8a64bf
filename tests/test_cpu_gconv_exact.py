"""The per-element comparisons of tests/gconv_exact.py without a GPU: float32 numpy imitations that follow each kernel's summation
structure (per-tap chains of MFMA steps, the f32 kernel's interleaved waves, split partials and the fixed-order reduce with its 1 / 4 / 16
split lanes, the 16-bit kernel's 64-pixel chunks and 8-tap groups, the thin kernel's per-row chunks, the two-stage column sums) pass every
comparison in every dtype; each planted defect of the kinds these kernels can have FAILS at the case named for it; and the data holds its
conditions: GRID sums stay below 2**20 grid units, every case takes the path it names, no comparison skips an element.  So a green
tests/test_gpu_gconv_exact.py means something."""
import numpy as np
import pytest
import torch

import gconv_exact as GX
from layers_exact import TORCH, all_ok

f32 = np.float32


def a32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def must_fail(cmps, what):
    assert not all_ok(cmps), "the defect `%s` passed every comparison" % what


def must_pass(cmps):
    for c in cmps:
        c.assert_ok()
        assert c.skipped == 0


def stored(v, dt, truncate=False):
    """float32 values -> what a store of dtype dt keeps (round to nearest even; truncate: the defect), as float64"""
    v = a32(v)
    if dt == "f32":
        return v.astype(np.float64)
    if not truncate:
        return torch.from_numpy(v).to(TORCH[dt]).double().numpy()
    if dt == "bf16":
        return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float64)


def chain(parts):
    """parts [steps, ...] float32 -> their sum taken one after the other in float32 (an accumulator across MFMA steps)"""
    if parts.shape[0] == 0:
        return np.zeros(parts.shape[1:], dtype=f32)
    return np.cumsum(parts, axis=0, dtype=f32)[-1]


# ----------------------------------------------------------------------------------------------------------------- forward / dgrad
def walk(sp, npix):
    """(b, oy, ox) of the flattened pixel index as gconv_kernel walks it: by parity class for the stride-2 input gradient onto an even grid"""
    lin = np.arange(npix)
    if sp.dgrad and sp.s == 2 and not ((sp.OH | sp.OW) & 1):
        hw, hh, per = sp.OW >> 1, sp.OH >> 1, npix >> 2
        cls = lin // per
        idx = lin - cls * per
        return idx // (hw * hh), 2 * ((idx // hw) % hh) + (cls >> 1), 2 * (idx % hw) + (cls & 1)
    return lin // (sp.OW * sp.OH), (lin // sp.OW) % sp.OH, lin % sp.OW


def src_of(sp, oy, ox, ky, kx, defect=None):
    dy, dx = sp.d, (1 if defect == "dilation on ky only" else sp.d)
    if not sp.dgrad:
        sy, sx = oy * sp.s - sp.p + ky * dy, ox * sp.s - sp.p + kx * dx
        ok = (sy >= 0) & (sy < sp.IH) & (sx >= 0) & (sx < sp.IW)
        if defect == "border tap dropped":              # right and bottom edge only
            ok &= ~((sx == sp.IW - 1) & (kx == sp.KW - 1)) & ~((sy == sp.IH - 1) & (ky == sp.KH - 1))
    else:
        ty, tx = oy + sp.p - ky * dy, ox + sp.p - kx * dx
        ok = (ty >= 0) & (tx >= 0) & (ty % sp.s == 0) & (tx % sp.s == 0)
        sy, sx = ty // sp.s, tx // sp.s
        ok &= (sy < sp.IH) & (sx < sp.IW)
    return np.where(ok, sy, 0), np.where(ok, sx, 0), ok


def imit_linear(c, X, W, bias):
    """glinear_small_kernel: lane l chains k = l, l + 64, ... with fused multiply-adds; the 64 lanes meet in a halving tree"""
    P, KC = X.shape
    kp = GX.cdiv(KC, 64) * 64
    prod = np.zeros((P, W.shape[0], kp), dtype=np.float64)
    prod[:, :, :KC] = X.astype(np.float64)[:, None, :] * W.astype(np.float64)[None, :, :]
    acc = np.zeros((P, W.shape[0], 64), dtype=f32)
    for j in range(kp // 64):
        acc = (acc.astype(np.float64) + prod[:, :, 64 * j:64 * j + 64]).astype(f32)      # one rounding: fmaf
    n = 64
    while n > 1:
        n //= 2
        acc = acc[:, :, :n] + acc[:, :, n:2 * n]
    return acc[:, :, 0] + bias


def imit_fwd(c, defect=None):
    sp, dt, KC, NC = c.spec, c.dt, c.KC, c.spec.NC
    npix, ks = sp.npix, GX.KSTEP[dt]
    X, W = a32(c.x).reshape(-1, KC), a32(c.wp)
    bias = a32(c.bias_p) if c.bias_p is not None else np.zeros(NC, dtype=f32)
    if defect == "padding channels not zero":
        bias = bias.copy()
        bias[sp.Nr:] = f32(0.25)
    b, oy, ox = walk(sp, npix)
    pix = (b * sp.OH + oy) * sp.OW + ox
    if c.paths() == {"linear"}:
        res = imit_linear(c, X, W[0], bias)
    else:
        kext = GX.cdiv(KC, ks) * ks
        if defect == "channel tail read" and kext > KC:  # the last step's lanes beyond KC read on: the next pixel's / the next row's channels
            X = np.concatenate([X, np.roll(X, -1, axis=0)[:, :kext - KC]], axis=1)
            Wf = W.reshape(-1, KC)
            W = np.concatenate([Wf, np.roll(Wf, -1, axis=0)[:, :kext - KC]], axis=1).reshape(W.shape[0], NC, kext)
        acc = np.zeros((npix, NC), dtype=f32)
        for tap in range(sp.KH * sp.KW):
            ky, kx = divmod(tap, sp.KW)
            sy, sx, ok = src_of(sp, oy, ox, ky, kx, defect)
            if defect == "class of the wave's first pixel":  # the taps the first pixel's class skips are skipped for the wave
                ok = ok & np.repeat(ok[::16], 16)[:npix]
            patch = np.where(ok[:, None], X[(b * sp.IH + sy) * sp.IW + sx], f32(0))
            Wt = W[tap]
            if defect == "narrow block reads the wide block's rows" and NC % 64 == 16 and NC > 64:
                Wt = Wt.copy()
                Wt[NC - 16:] = Wt[:16]
            for c0 in range(0, X.shape[1], ks):              # one MFMA step per chunk of the channels, chained through the accumulator
                acc += patch[:, c0:c0 + ks] @ Wt[:, c0:c0 + ks].T
        res = acc + bias
    out = np.zeros((npix, NC), dtype=np.float64)
    out[pix] = stored(res, dt, truncate=(defect == "truncating store"))
    return out


FWD_KEYS = [(i, dt) for i in range(len(GX.FWD_SPECS)) for dt in GX.DTYPES]


@pytest.mark.parametrize("i,dt", FWD_KEYS)
def test_fwd_imitation_passes(i, dt):
    c = GX.fwd_case(i, dt)
    c.check_path()
    assert c.units < GX.MAX_UNITS
    must_pass(c.check(imit_fwd(c)))


FWD_DEFECTS = [
    ("border tap dropped", GX.fwd_index("wide", GX.F, npix=16), "f32"),
    ("border tap dropped", GX.fwd_index("wide+narrow", GX.F, npix=65), "bf16"),
    ("class of the wave's first pixel", GX.fwd_index("narrow+parity", GX.G, npix=60), "f32"),
    ("class of the wave's first pixel", GX.fwd_index("wide+narrow+parity", GX.G), "f16"),
    ("narrow block reads the wide block's rows", GX.fwd_index("wide+narrow", GX.F, NC=80), "f32"),
    ("narrow block reads the wide block's rows", GX.fwd_index("wide+narrow", GX.G, NC=80), "bf16"),
    ("channel tail read", GX.fwd_index("wide", GX.F, npix=16), "bf16"),          # KC = 48
    ("channel tail read", GX.fwd_index("narrow", GX.F, npix=5), "f16"),          # KC = 16
    ("dilation on ky only", GX.fwd_index("wide", GX.F, d=2), "f32"),
    ("dilation on ky only", GX.fwd_index("narrow", GX.G, d=3), "bf16"),
    ("padding channels not zero", GX.fwd_index("narrow", GX.F, npix=5), "f32"),
    ("padding channels not zero", GX.fwd_index("wide+narrow", GX.G, npix=105), "f16"),
    ("truncating store", GX.fwd_index("wide", GX.F, npix=63), "bf16"),
    ("truncating store", GX.fwd_index("wide+narrow", GX.F, kind="normal"), "f16"),     # (the grid sums are exact in f16)
    ("truncating store", GX.fwd_index("wide+narrow+parity", GX.G, kind="normal"), "bf16"),
]


@pytest.mark.parametrize("defect,i,dt", FWD_DEFECTS)
def test_fwd_defects_fail(defect, i, dt):
    c = GX.fwd_case(i, dt)
    must_fail(c.check(imit_fwd(c, defect)), defect)


def test_fwd_table_reaches_every_path():
    specs = GX.FWD_SPECS
    for dgrad in (0, 1):
        s = [x for x in specs if x.dgrad == dgrad and x.kind == "grid"]
        assert {x.NC for x in s} >= {16, 48, 64, 80, 144}
        assert any("linear" in x.path for x in s) and {x.KC for x in s if x.path == "linear"} >= {16, 80, 512}
        assert {x.npix for x in s if x.path == "linear"} >= {1, 32} and any(x.npix == 33 and x.KH == 1 for x in s)
        assert {x.d for x in s} >= {1, 2, 3, 8} and {x.entry for x in s if x.d > 1} == {"plain", "dil"}
        assert {x.bias for x in s} == {True, False}
        assert {x.KC for x in s} >= {GX.K0, GX.K1, GX.K2}
    fw = [x for x in specs if not x.dgrad]
    assert {x.npix for x in fw} >= {5, 16, 63, 65, 105}
    assert {x.KH for x in fw} >= {1, 2, 3, 4, 5} and {x.s for x in fw} == {1, 2} and {x.p for x in fw} >= {0, 1, 2, 4}
    assert any(x.KH == 3 and x.p == 4 for x in fw)
    dg = [x for x in specs if x.dgrad]
    assert any("parity" in x.path and (x.npix // 4) % 16 for x in dg) and any("general" in x.path for x in dg)
    assert {x.extra for x in dg if x.s == 2} == {0, 1}
    assert {frozenset(x.path.split("+")) for x in specs if x.kind != "grid"} >= {frozenset(("wide", "narrow")), frozenset(("linear",)),
                                                                                 frozenset(("wide", "narrow", "parity")), frozenset(("wide", "general"))}


# ----------------------------------------------------------------------------------------------------------------- weight gradient
def gather(c, X, b, oy, oxv, ky, kx, defect=None):
    """the input pixel under tap (ky, kx) of output pixel (b, oy, oxv), [n, KC] float32; zero where there is none (b < 0: no pixel)"""
    sp = c.spec
    d = 1 if defect == "dilation ignored" else sp.d
    sy, sx = oy * sp.s - sp.p + ky * d, oxv * sp.s - sp.p + kx * d
    ok = (b >= 0) & (sy >= 0) & (sy < sp.IH) & (sx >= 0) & (sx < sp.IW)
    return np.where(ok[:, None], X[np.where(ok, (b * sp.IH + sy) * sp.IW + sx, 0)], f32(0))


def wgrad_units(c, defect=None):
    """per split: a list of accumulators, each a list of MFMA steps, each arrays (dout row index or -1, b, oy, ox) of the step's pixels.
    f32 kernel: four waves taking interleaved 4-pixel steps; 16-bit kernels: one accumulator over 32-pixel steps of 64-pixel chunks
    (thin: a chunk = 64 pixels of ONE output row, the rest of the chunk empty)"""
    sp, ns, npix = c.spec, c.nsplit, c.spec.npix
    out = []

    def of_lin(lin):
        lin = np.asarray(lin)
        ok = lin < npix
        l0 = np.where(ok, lin, 0)
        return np.where(ok, lin, -1), np.where(ok, l0 // (sp.OW * sp.OH), -1), (l0 // sp.OW) % sp.OH, l0 % sp.OW

    if c.kernel == "f32":
        per = GX.cdiv(npix, ns)
        for s in range(ns):
            p0, p1 = s * per, min(s * per + per, npix)
            if defect == "tail of the last split dropped" and s == ns - 1:
                p1 = p0 + (p1 - p0) // 16 * 16
            waves = []
            for w in range(4):
                steps = []
                for s0 in range(p0 + 4 * w, p1, 16):
                    lin = np.arange(s0, s0 + 4)
                    steps.append(of_lin(np.where(lin < p1, lin, npix)))
                waves.append(steps)
            out.append(waves)
        return out
    if c.kernel == "wgrad16":
        chunks = GX.cdiv(npix, 64)
        cper = GX.cdiv(chunks, ns)
        for s in range(ns):
            steps = []
            for ch in range(s * cper, min(s * cper + cper, chunks)):
                steps += [of_lin(np.arange(ch * 64 + 32 * h, ch * 64 + 32 * h + 32)) for h in range(2)]
            out.append([steps])
        return out
    cx = GX.cdiv(sp.OW, 64)
    chunks = sp.B * sp.OH * cx
    cper = GX.cdiv(chunks, ns)
    for s in range(ns):
        steps = []
        for ch in range(s * cper, min(s * cper + cper, chunks)):
            xs, oy, b = ch % cx, (ch // cx) % sp.OH, ch // (cx * sp.OH)
            for h in range(2):
                ox = xs * 64 + 32 * h + np.arange(32)
                lin = (b * sp.OH + oy) * sp.OW + ox
                if defect == "last OW chunk taken to be full":       # dout read on into the next row; the window still ends at IW
                    ok = lin < npix
                else:
                    ok = ox < sp.OW
                steps.append((np.where(ok, lin, -1), np.where(ok, b, -1), np.full(32, oy), ox))
        out.append([steps])
    return out


def reduce_splits(partial, SL, defect=None):
    """gconv_wreduce_kernel: lane sl chains the splits sl, sl + SL, ...; lane 0 then adds the other lanes' sums in order"""
    lanes = [chain(partial[sl::SL]) for sl in range(SL)]
    s = lanes[0]
    if defect != "reduce without the lanes sl >= 1":
        for k in range(1, SL):
            s = s + lanes[k]
    return s


def imit_colsum(x, nsplit, nlanes, defect=None):
    """gcolsum_kernel + gcolsum_reduce_kernel: per split, pixel lanes that chain every nlanes-th pixel and are added in order; the splits
    go to 16 lanes (k, k + 16, ...) that are added in order"""
    npix = x.shape[0]
    per = GX.cdiv(npix, nsplit)
    part = np.zeros((nsplit, x.shape[1]), dtype=f32)
    for s in range(nsplit):
        blk = x[s * per:min(s * per + per, npix)]
        part[s] = chain(np.stack([chain(blk[l::nlanes]) for l in range(min(nlanes, max(len(blk), 1)))]))
    return chain(np.stack([chain(part[k::16]) for k in range(min(16, nsplit))]))


def imit_wgrad(c, accumulate, defect=None):
    sp = c.spec
    NC, KC, taps = sp.NC, sp.KC, sp.KH * sp.KW
    X, D = a32(c.x).reshape(-1, KC), a32(c.dout).reshape(-1, NC)
    partial = np.zeros((c.nsplit, taps, NC, KC), dtype=f32)
    units = wgrad_units(c, defect)
    for s, accs in enumerate(units):
        for tap in range(taps):
            if defect == "ninth tap's group dropped" and tap // GX.WG_TAPS == 1:
                continue
            ky, kx = divmod(tap, sp.KW)
            sums = []
            for steps in accs:
                if not steps:
                    sums.append(np.zeros((NC, KC), dtype=f32))
                    continue
                li, b, oy, ox = (np.concatenate([st[j] for st in steps]) for j in range(4))
                n = len(steps[0][0])
                dv = np.where(li[:, None] >= 0, D[np.maximum(li, 0)], f32(0)).reshape(len(steps), n, NC)
                xv = gather(c, X, b, oy, ox, ky, kx, defect).reshape(len(steps), n, KC)
                sums.append(chain(np.einsum("spn,spk->snk", dv, xv)))                      # one MFMA per step, chained
            partial[s, tap] = sums[0] if len(sums) == 1 else (sums[0] + sums[1]) + (sums[2] + sums[3])
    red = reduce_splits(partial, c.SL, defect)[:, :sp.Nr, :sp.Kr].transpose(1, 2, 0).reshape(sp.Nr, sp.Kr, sp.KH, sp.KW)
    acc = accumulate and defect != "accumulate ignored"
    dw = (a32(c.dw0) if acc else f32(0)) + red
    db = (a32(c.db0) if acc else f32(0)) + imit_colsum(D, GX.colsum_nsplit(sp.npix), 16)[:sp.Nr]
    return dw, db


@pytest.mark.parametrize("i,dt", GX.wgrad_keys())
def test_wgrad_imitation_passes(i, dt):
    c = GX.wgrad_case(i, dt)
    c.check_path()
    assert c.units < GX.MAX_UNITS
    for acc in (False, True):
        must_pass(c.check(*imit_wgrad(c, acc), accumulate=acc))


WGRAD_DEFECTS = [
    ("tail of the last split dropped", "13 splits", "f32"),
    ("tail of the last split dropped", "dilation 2, two splits", "f32"),
    ("dilation ignored", "dilation 2, two splits", "f32"),
    ("dilation ignored", "dilation 2", "bf16"),
    ("dilation ignored", "KC = 16 but dilated", "f16"),
    ("ninth tap's group dropped", "9 taps", "bf16"),
    ("last OW chunk taken to be full", "k 3; OW = 65", "bf16"),
    ("last OW chunk taken to be full", "OW = 150", "f16"),
    ("last OW chunk taken to be full", "k 4 s 2 p 1; OW = 5", "bf16"),
    ("accumulate ignored", "64 splits", "f32"),
    ("accumulate ignored", "8 taps", "f16"),
    ("accumulate ignored", "odd IW", "bf16"),
    ("reduce without the lanes sl >= 1", "13 splits", "f32"),
    ("reduce without the lanes sl >= 1", "64 splits", "f32"),
    ("reduce without the lanes sl >= 1", "1 tap; 256 chunks", "bf16"),
    ("reduce without the lanes sl >= 1", "k 3; OW = 65", "f16"),
    ("reduce without the lanes sl >= 1", "B 8, OH 64", "bf16"),
]


@pytest.mark.parametrize("defect,why,dt", WGRAD_DEFECTS)
def test_wgrad_defects_fail(defect, why, dt):
    c = GX.wgrad_case(GX.wgrad_index(why, dt), dt)
    must_fail(c.check(*imit_wgrad(c, True, defect), accumulate=True), defect)


def test_wgrad_table_reaches_every_path():
    rows = [(s, dt) + s.dispatch(dt) for s in GX.WGRAD_SPECS for dt in s.dts if s.kind == "grid"]
    for kern in ("f32", "wgrad16", "thin"):
        assert {SL for s, dt, k, ns, SL in rows if k == kern} == {1, 4, 16}, kern
    assert any(ns == 1 for s, dt, k, ns, SL in rows if k == "f32") and any(s.KC == 20 for s, dt, k, ns, SL in rows if k == "f32")
    assert any(GX.cdiv(s.npix, ns) % 16 for s, dt, k, ns, SL in rows if k == "f32" and ns > 1)
    w16 = [s for s, dt, k, ns, SL in rows if k == "wgrad16"]
    assert {s.KH * s.KW for s in w16} >= {1, 8, 9, 25} and {s.NC for s in w16} >= {32, 64, 80} and {s.KC for s in w16} >= {32, 64, 80}
    assert all(s.npix % 64 for s in w16 if s.d == 1) and any(s.d == 2 for s in w16) and any(s.d == 2 and s.KC == 16 for s in w16)
    th = [s for s, dt, k, ns, SL in rows if k == "thin"]
    assert {(s.KH, s.s, s.p) for s in th} >= {(4, 2, 1), (5, 1, 2), (3, 1, 1)} and {s.OW for s in th} >= {5, 64, 65, 150}
    assert any(s.s == 2 and s.IW % 2 for s in th) and any((s.B, s.OH, s.OW) == (8, 64, 8) for s in th)
    assert any(s.Nr < s.NC and s.Kr < s.KC for s, *_ in rows)
    assert {s.kernel for s in GX.WGRAD_SPECS if s.kind != "grid"} == {"f32", "wgrad16", "thin"}
    assert GX.wgrad_nsplit(1, 128, 128, 16, 16, 1, 1) == 64 and GX.thin_nsplit(8, 64, 8) == 64


# ----------------------------------------------------------------------------------------------------------------- column sums
def imit_gcolsum(c, in_double, defect=None):
    x = a32(c.x)
    acc = c.accumulate and defect != "accumulate ignored"
    if in_double:                                         # 256 threads chain pixels t, t + 256, ... in double; one rounding at the end
        s = np.stack([x[t::256].astype(np.float64).sum(0) for t in range(min(256, c.npix))]).sum(0)
        return ((c.out0 if acc else 0.0) + s[:c.Creal]).astype(f32)
    if defect == "splits beyond the cap dropped":        # 256 pixels per split whatever their number: the 513th split's pixel is lost
        x = x[:512 * 256]
    s = imit_colsum(x, c.nsplit, 16)
    return (a32(c.out0) if acc else f32(0)) + s[:c.Creal]


@pytest.mark.parametrize("i,dt", GX.colsum_keys())
def test_colsum_imitation_passes(i, dt):
    c = GX.colsum_case(i, dt)
    assert c.units < GX.MAX_UNITS
    for dbl in (False, True):
        must_pass(c.check(imit_gcolsum(c, dbl), dbl))


def test_colsum_defects_fail_and_table_is_whole():
    keys = GX.colsum_keys()
    acc = next(k for k in keys if GX.COLSUM_SPECS[k[0]][3] == 1 and GX.COLSUM_SPECS[k[0]][1] == 257)
    for dbl in (False, True):
        c = GX.colsum_case(*acc)
        must_fail(c.check(imit_gcolsum(c, dbl, "accumulate ignored"), dbl), "accumulate ignored")
    cap = GX.colsum_case(next(i for i, s in enumerate(GX.COLSUM_SPECS) if s[1] == GX.COLSUM_CAP), "bf16")
    assert cap.nsplit == 512 and GX.cdiv(cap.npix, 256) == 513
    must_fail(cap.check(imit_gcolsum(cap, False, "splits beyond the cap dropped"), False), "splits beyond the cap dropped")
    sp = [s for s in GX.COLSUM_SPECS if s[4] == "grid"]
    assert {s[0] for s in sp} == {16, 32, 48, 64, 80} and {s[1] for s in sp} == {1, 255, 257, 1025, 256 * 512 + 1}
    for C in (16, 32, 48, 64, 80):
        assert {s[3] for s in sp if s[0] == C} == {0, 1} and {s[2] < C for s in sp if s[0] == C} == {True, False}


# ----------------------------------------------------------------------------------------------------------------- pack
def imit_pack(c, defect=None):
    w = stored(a32(c.w), c.dt, truncate=(defect == "truncating store"))
    m = w.reshape(c.Cout, c.Cin, c.KH * c.KW).transpose(2, 0, 1)
    if c.transpose and defect != "not transposed":
        m = m.transpose(0, 2, 1)
    out = np.full((c.KH * c.KW, c.RP, c.CP), 0.5 if defect == "padding channels not zero" else 0.0)
    r, k = min(m.shape[1], c.RP), min(m.shape[2], c.CP)
    out[:, :r, :k] = m[:, :r, :k]
    return out


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_pack_imitation_passes_and_defects_fail(dt):
    for i in range(len(GX.PACK_SPECS)):
        c = GX.pack_case(i, dt)
        must_pass(c.check(imit_pack(c)))
        if c.RP * c.CP > c.Cout * c.Cin:
            must_fail(c.check(imit_pack(c, "padding channels not zero")), "padding channels not zero")
        if c.transpose:
            must_fail(c.check(imit_pack(c, "not transposed")), "not transposed")
        if dt != "f32":
            must_fail(c.check(imit_pack(c, "truncating store")), "truncating store")
