"""GPU: the general convolution family (csrc/gconv.hip: wm_gconv_fwd / _dil_fwd, wm_gconv_wgrad / _dil_wgrad, wm_gconv_pack, wm_gcolsum,
wm_gcolsum_f64) per element against float64 (tests/gconv_exact.py), at the smallest shapes that take each path: the wide and the narrow
form of gconv_kernel and both in one launch (NC = 80, 144), the krem tail of a 32-channel step, pad 4 under a 3x3 filter, dilation 2 / 3 /
8 through both entry points, the stride-2 input gradient walked by parity class with classes that share a wave, onto odd grids, and onto
the grid of a dropped row, the linear kernel and its MFMA twin one pixel later; the f32 weight-gradient kernel with 1, 13 and 64 splits,
gconv_wgrad16_kernel with 1 / 8 / 9 / 25 taps, the thin kernel with OW 5 / 64 / 65 / 150, the reduce with 1, 4 and 16 split lanes; the
column sums up to their 512-split cap, in float32 and in double; the pack in both orientations.

GRID data makes every float32 sum exact in any order: there the comparison is bit for bit (16-bit outputs: within their own rounding).
GENERIC data is accepted within FACTOR * (n + 1) * 2**-24 * sum|terms| for n non-zero terms; no bound is picked.  Every case asserts the
path it names from the host arithmetic restated in Python (wm_gconv_wgrad_nsplit is compared with the library's), runs twice and must give
identical bits (no atomics), and prints one line per comparison (run with -s).  tests/test_cpu_gconv_exact.py shows that these
comparisons fail on the defects they are there to catch.  Where ops.* refuses a shape the C ABI takes (an f32 channel stride of 4 or 20)
the call goes to _lib.lib() directly.

MEASURED on an MI355X (the largest share of its bound any element reached, from the -s output; every GRID comparison of a float32
quantity -- f32 outputs, dw, dbias, column sums, packed filters, padding channels -- was exact, 0 values differ, in all three dtypes):
    forward         f32 0.031 (generic, dilation 3)   bf16 0.996   f16 0.947   -- 16 bit: the output's own rounding, half an ulp
    input gradient  f32 0.073 (generic, parity walk)  bf16 0.996   f16 0.987
    wgrad f32 kernel          generic dw 2.2e-05 of a bound of 1.55, dbias 1.5e-05 of 1.92: below 0.001
    wgrad gconv_wgrad16       generic dw 4.5e-05 of 3.56 (f16), 3.8e-05 of 3.56 (bf16): below 0.001
    wgrad thin kernel         generic dw 4.2e-05 of 4.31 (f16), 3.1e-05 of 4.31 (bf16): below 0.001
    column sums     float32 generic 1.2e-05 of 0.21: below 0.001; in double 0.845 (f32), 0.984 (bf16), 0.993 (f16): the one float32 rounding
    pack            exact
The 16-bit MFMA summed the exactly-summable GRID data exactly in every case: no inexact accumulation was seen."""
import pytest
import torch

import gconv_exact as GX
from layers_exact import TORCH, store, Cmp

pytestmark = pytest.mark.gpu

SENTINEL = 768.0


def dev(a, dt="f32"):
    return None if a is None else store(a, dt).cuda()


def report(cmps, tally):
    for c in cmps:
        print("  ", c.line())
    for c in cmps:
        c.assert_ok()
        assert c.skipped == 0
        tally[0] = max(tally[0], c.worst)


def _mods():
    from video_watermarking_forgery_detection_amd import _lib, ops
    return _lib, ops, ops._p, torch.cuda.current_stream().cuda_stream


def same_bits(a, b, what):
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "%s: two runs of the same call differ" % what


# ----------------------------------------------------------------------------------------------------------------- forward / dgrad
def run_fwd(c, x, wp, bias):
    _lib, ops, _p, stream = _mods()
    sp = c.spec
    if c.KC % 16 == 0:
        if sp.entry == "dil":
            return ops.gconv_dil_fwd(x, wp, bias, (sp.OH, sp.OW), sp.KH, sp.KW, sp.s, sp.p, sp.d, bool(sp.dgrad))
        return ops.gconv_fwd(x, wp, bias, (sp.OH, sp.OW), sp.KH, sp.KW, sp.s, sp.p, dgrad=bool(sp.dgrad), dilation=sp.d)
    L, dtid = _lib.lib(), ops.dt_id(TORCH[c.dt])           # an f32 channel stride below 16: ops.* asks for multiples of 16
    out = torch.full((sp.B, sp.OH, sp.OW, sp.NC), SENTINEL, device="cuda", dtype=TORCH[c.dt])
    if sp.entry == "dil" or sp.d != 1:
        rc = L.wm_gconv_dil_fwd(_p(x), _p(wp), _p(bias), _p(out), sp.B, sp.IH, sp.IW, c.KC, sp.OH, sp.OW, sp.NC, sp.KH, sp.KW, sp.s, sp.p, sp.d,
                                sp.dgrad, dtid, stream)
        _lib.check(rc, "wm_gconv_dil_fwd")
    else:
        rc = L.wm_gconv_fwd(_p(x), _p(wp), _p(bias), _p(out), sp.B, sp.IH, sp.IW, c.KC, sp.OH, sp.OW, sp.NC, sp.KH, sp.KW, sp.s, sp.p, sp.dgrad,
                            dtid, stream)
        _lib.check(rc, "wm_gconv_fwd")
    return out


@pytest.mark.parametrize("dt", GX.DTYPES)
@pytest.mark.parametrize("dgrad", [0, 1], ids=["fwd", "dgrad"])
def test_forward_and_input_gradient(dgrad, dt):
    _lib, ops, _p, _ = _mods()
    print()
    tally = [0.0]
    for i, sp in enumerate(GX.FWD_SPECS):
        if sp.dgrad != dgrad:
            continue
        c = GX.fwd_case(i, dt)
        c.check_path()
        assert c.units < GX.MAX_UNITS
        x, bias = dev(c.x, dt), dev(c.bias_p)
        wp = ops.gconv_pack(dev(c.w), sp.NC, c.KC, bool(sp.dgrad), TORCH[dt])
        cm = [Cmp(c.label + " packed filter", wp, c.wp)]
        out = run_fwd(c, x, wp, bias)
        same_bits(out, run_fwd(c, x, wp, bias), c.label)
        report(cm + c.check(out), tally)
    print("   %s %s: largest share of its bound %.3f" % ("dgrad" if dgrad else "fwd", dt, tally[0]))


# ----------------------------------------------------------------------------------------------------------------- weight gradient
def run_wgrad(c, accumulate, want_bias=True, dil_entry=False):
    _lib, ops, _p, stream = _mods()
    sp, dt = c.spec, c.dt
    x, dout = dev(c.x, dt), dev(c.dout, dt)
    dw = dev(c.dw0) if accumulate else None
    db = dev(c.db0) if accumulate and want_bias else None
    if sp.KC % 16 == 0:
        return ops.gconv_wgrad(dout, x, sp.Nr, sp.Kr, sp.KH, sp.KW, sp.s, sp.p, want_bias=want_bias, dw_acc=dw, db_acc=db, dilation=sp.d,
                               dil_entry=dil_entry)
    L, dtid = _lib.lib(), ops.dt_id(TORCH[dt])
    partial = torch.full((L.wm_gconv_wgrad_scratch_floats(sp.B, sp.OH, sp.OW, sp.KC, sp.NC, sp.KH, sp.KW),), SENTINEL, device="cuda", dtype=torch.float32)
    if dw is None:
        dw = torch.full((sp.Nr, sp.Kr, sp.KH, sp.KW), SENTINEL, device="cuda", dtype=torch.float32)
    if db is None and want_bias:
        db = torch.full((sp.Nr,), SENTINEL, device="cuda", dtype=torch.float32)
    acc = 1 if accumulate else 0
    if sp.d != 1 or dil_entry:
        rc = L.wm_gconv_dil_wgrad(_p(dout), _p(x), _p(partial), _p(dw), _p(db), acc, sp.B, sp.IH, sp.IW, sp.KC, sp.OH, sp.OW, sp.NC, sp.KH, sp.KW,
                                  sp.s, sp.p, sp.d, sp.Nr, sp.Kr, dtid, stream)
        _lib.check(rc, "wm_gconv_dil_wgrad")
    else:
        rc = L.wm_gconv_wgrad(_p(dout), _p(x), _p(partial), _p(dw), _p(db), acc, sp.B, sp.IH, sp.IW, sp.KC, sp.OH, sp.OW, sp.NC, sp.KH, sp.KW,
                              sp.s, sp.p, sp.Nr, sp.Kr, dtid, stream)
        _lib.check(rc, "wm_gconv_wgrad")
    return dw, db


@pytest.mark.parametrize("kernel,dt", [("f32", "f32"), ("wgrad16", "bf16"), ("wgrad16", "f16"), ("thin", "bf16"), ("thin", "f16")])
def test_weight_and_bias_gradient(kernel, dt):
    print()
    tally = [0.0]
    for i, sp in enumerate(GX.WGRAD_SPECS):
        if sp.kernel != kernel or dt not in sp.dts:
            continue
        c = GX.wgrad_case(i, dt)
        c.check_path()
        assert c.units < GX.MAX_UNITS
        for acc in (False, True):
            dw, db = run_wgrad(c, acc)
            dw2, db2 = run_wgrad(c, acc)
            same_bits(dw, dw2, c.label)
            same_bits(db, db2, c.label)
            report(c.check(dw, db, acc), tally)
        dw, db = run_wgrad(c, False, want_bias=False)
        assert db is None
        report(c.check(dw, None, False, " (no dbias)"), tally)
        if sp.d == 1:                                      # dilation 1 through the dilated entry point: the same bits
            dwd, dbd = run_wgrad(c, True, dil_entry=True)
            report(c.check(dwd, dbd, True, " (dil entry)"), tally)
    print("   wgrad %s %s: largest share of its bound %.3f" % (kernel, dt, tally[0]))


def test_wgrad_nsplit_is_the_librarys():
    _lib, ops, _p, _ = _mods()
    L = _lib.lib()
    for sp in GX.WGRAD_SPECS + tuple(GX.WSpec("f32", 0, GX.F32, B, H, W, KC, KC, NC, NC, k, 1, k // 2)
                                     for B, H, W in ((1, 1, 1), (2, 64, 64), (4, 128, 128)) for KC, NC in ((4, 16), (64, 64), (16, 144)) for k in (1, 3, 5)):
        args = (sp.B, sp.OH, sp.OW, sp.KC, sp.NC, sp.KH, sp.KW)
        assert L.wm_gconv_wgrad_nsplit(*args) == GX.wgrad_nsplit(*args), args


# ----------------------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("dt", GX.DTYPES)
def test_column_sums(dt):
    _lib, ops, _p, _ = _mods()
    print()
    tally = [0.0]
    for i, dts in ((i, s[5]) for i, s in enumerate(GX.COLSUM_SPECS)):
        if dt not in dts:
            continue
        c = GX.colsum_case(i, dt)
        assert c.units < GX.MAX_UNITS
        x = dev(c.x, dt).reshape(1, 1, c.npix, c.C)
        for dbl in (False, True):
            outs = [ops.gcolsum(x, c.Creal, out_acc=dev(c.out0) if c.accumulate else None, f64=dbl) for _ in range(2)]
            same_bits(outs[0], outs[1], c.label)
            report(c.check(outs[0], dbl), tally)
    print("   colsum %s: largest share of its bound %.3f" % (dt, tally[0]))


# ----------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("dt", GX.DTYPES)
def test_pack(dt):
    _lib, ops, _p, _ = _mods()
    print()
    tally = [0.0]
    for i in range(len(GX.PACK_SPECS)):
        c = GX.pack_case(i, dt)
        report(c.check(ops.gconv_pack(dev(c.w), c.RP, c.CP, bool(c.transpose), TORCH[dt])), tally)
    print("   pack %s: exact" % dt)
