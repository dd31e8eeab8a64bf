"""The forward half of the 3x3 convolution hot path -- wm_pack_w3x3 / _batch, wm_conv3x3_fwd (csrc/conv3x3_ws.hip, csrc/conv3x3_stream.hip,
the generic 16-bit and float32 kernel of csrc/conv3x3.hip; forward and, with the transposed pack, input gradient), wm_conv3x3_fwd_addin,
wm_concat_side_fwd and wm_concat_side_msg_wgrad -- per element against the float64 restatement of tests/cbr_fwd_exact.py.  Every case
asserts the kernel and the number of statistics rows it reaches against the restated host arithmetic (wm_conv3x3_nparts; the persistent
kernel also by its refusal of a strided output, a host-side check), runs twice (identical bits), runs once more swept the other way
(identical y; the persistent kernel's rows against the restated rows of that direction), and compares y and the statistics rows -- bit
for bit on GRID / SPARSE data, within the derived bounds on dense-data statistics and on the GENERIC cases; no element is skipped.  The
WHOLE / masked form of the persistent kernel cannot be observed from outside the release library: the restated rule (ws_form) names
it.  tests/test_cpu_cbr_fwd_exact.py shows that these comparisons pass for correct arithmetic and fail for the defects such kernels can
have.  With -s every comparison prints its line, and the last test the largest share of a bound per family."""
import collections

import pytest
import torch

import cbr_fwd_exact as FX
from layers_exact import TORCH, SENTINEL

pytestmark = pytest.mark.gpu

WORST = collections.defaultdict(float)            # (family, dtype, quantity) -> largest error / bound
AMBIGUOUS = collections.defaultdict(float)        # (family, dtype) -> largest ambiguous share


def _ptr(t):
    return None if t is None else t.data_ptr()


def run(c, dt, reverse):
    """one call through the library handle (ops.conv3x3_fwd always passes a dense output) -> (ybuf [npix, ldy], rows or None)"""
    from video_watermarking_forgery_detection_amd import _lib, ops
    o = {k: (v.cuda() if v is not None else None) for k, v in c.operands(dt).items()}
    T = TORCH[dt]
    if c.transposed:
        wp = ops.pack_w3x3(o["w"], c.Cin, c.CoutP, T, transpose=True)                 # the layer's weight [Cin here][CoutP here]: [9][CoutP][Cin]
    else:
        wp = ops.pack_w3x3(o["w"], c.CoutP, c.Cin, T)
    assert tuple(wp.shape) == (9, c.CoutP, c.Cin)
    if c.addin:
        x = o["x"].reshape(c.B, c.H, c.W, c.Cin)
        y, st = ops.conv3x3_fwd_addin(x, wp, o["in_scale"], o["in_shift"], o["addend"].reshape(c.B, c.H, c.W, c.CoutP), reverse=reverse)
        torch.cuda.synchronize()
        return y.reshape(-1, c.CoutP), st
    y = o["y0"]
    st = torch.full((c.expected_rows(dt), 2, c.CoutP), SENTINEL, device="cuda", dtype=torch.float32) if c.stats else None
    L = _lib.lib()
    rc = L.wm_conv3x3_fwd(_ptr(o["x"]), c.ldx, _ptr(wp), _ptr(o["bias"]), c.nbias, _ptr(o["in_scale"]), _ptr(o["in_shift"]), _ptr(y), c.ldy, _ptr(st),
                          c.B, c.H, c.W, c.Cin, c.CoutP, ops.dt_id(T), 1 if reverse else 0, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "wm_conv3x3_fwd")
    torch.cuda.synchronize()
    return y, st


def same_bits(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def note(c, dt, cm):
    for x in cm:
        print(x.line())
        if not x.exact:
            k = (c.family + (" f32" if dt == "f32" else ""), dt, c.kind + x.what.split(dt, 1)[1])
            WORST[k] = max(WORST[k], x.worst)
    for x in cm:
        x.assert_ok()
        assert x.skipped == 0
        assert x.exact or c.kind == "normal" or (c.kind == "grid" and " sum y" in x.what), "an exact-data comparison with a bound: " + x.what


@pytest.mark.parametrize("cid,dt", FX.case_keys())
def test_forward_per_element(cid, dt):
    from video_watermarking_forgery_detection_amd import _lib, ops
    c = FX.case(cid)
    kernel = c.check_dispatch(dt, nparts_fn=lambda B, H, W, Cin, CoutP, d: ops.conv3x3_nparts(B, H, W, Cin, CoutP, TORCH[d]))
    # the persistent kernel writes a dense output only: wm_conv3x3_fwd refuses a strided one on the host, before any launch
    one = torch.zeros(64, device="cuda", dtype=TORCH[dt])
    rc = _lib.lib().wm_conv3x3_fwd(one.data_ptr(), c.Cin, one.data_ptr(), None, 0, None, None, one.data_ptr(), c.CoutP + 16, None, 1, 1, 1, c.Cin, c.CoutP,
                                   ops.dt_id(TORCH[dt]), 0, torch.cuda.current_stream().cuda_stream) if kernel == "ws" else 0
    assert (rc != 0) == (kernel == "ws"), "%s: a strided output was not refused" % c.label(dt)
    first, second, other = run(c, dt, c.reverse), run(c, dt, c.reverse), run(c, dt, not c.reverse)
    assert same_bits(first, second), "two runs of %s differ" % c.label(dt)
    assert torch.equal(first[0], other[0]), "sweep_reverse changes y of %s" % c.label(dt)
    note(c, dt, c.check(dt, *first))
    if c.stats:
        note(c, dt, [x for x in c.check(dt, *other, reverse=not c.reverse) if " sum y" in x.what])
    if c.kind == "normal":
        share = c.ref(dt).amb_share
        print("%s: %.2e of a ambiguous" % (c.label(dt), share))
        AMBIGUOUS[(c.family, dt)] = max(AMBIGUOUS[(c.family, dt)], share)


def test_dispatch_predicates_against_the_library():
    from video_watermarking_forgery_detection_amd import _lib, ops
    L = _lib.lib()
    for dt in ("f32",) + FX.DT16:
        T = TORCH[dt]
        for Cin in (4, 12, 16, 32, 48, 64, 112, 128, 256):
            for CoutP in (32, 64, 96, 128):
                assert ops.conv3x3_fwd_elu_supported(Cin, CoutP, T) == FX.fwd_elu_supported(Cin, CoutP, dt), (Cin, CoutP, dt)
                for B, H, W in ((1, 1, 1), (1, 17, 33), (3, 15, 18), (1, 16, 16 * 257), (2, 256, 256), (16, 256, 256)):
                    assert ops.conv3x3_nparts(B, H, W, Cin, CoutP, T) == FX.nparts(B, H, W, Cin, CoutP, dt), (B, H, W, Cin, CoutP, dt)
        for CinP in (8, 16, 32, 48, 64, 128):
            assert ops.conv3x3_dgrad_elufused_supported(CinP, T) == FX.dgrad_elufused_supported(CinP, dt), (CinP, dt)
    for B, H, W in ((1, 1, 1), (1, 17, 33), (1, 16, 16 * 257), (16, 256, 256)):
        assert L.wm_conv3x3_dgrad_elufused_nparts(B, H, W) == FX.dgrad_elufused_nparts(B, H, W)


# ----------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("dt", ("f32",) + FX.DT16)
def test_pack_single_and_batched(dt):
    """every pack shape x transpose through wm_pack_w3x3, bit for bit against the restatement; wm_pack_w3x3_batch over all of them at once
    (ops.PackPlan.refresh) equals the single launches bit for bit"""
    from video_watermarking_forgery_detection_amd import ops
    T = TORCH[dt]
    plan, single, ws = ops.PackPlan(), {}, {}
    for k, (Cout, Cin, CoutP, CinP, pn) in enumerate(FX.PACK_SHAPES):
        ws[k] = torch.from_numpy(FX.pack_weight(k)).float().cuda()
        for t in (0, 1):
            wp = plan.get(ws[k], CoutP, CinP, T, perm=FX.pack_perm(pn), transpose=bool(t))          # not valid yet: one wm_pack_w3x3 launch
            torch.cuda.synchronize()
            single[(k, t)] = wp
            for x in FX.pack_cmps(k, t, dt, wp):
                print(x.line())
                x.assert_ok()
    plan.refresh()
    torch.cuda.synchronize()
    assert plan.njobs == 2 * len(FX.PACK_SHAPES)
    for k, (Cout, Cin, CoutP, CinP, pn) in enumerate(FX.PACK_SHAPES):
        for t in (0, 1):
            got = plan.packed[plan.key(ws[k], CoutP, CinP, T, FX.pack_perm(pn), bool(t))]
            assert torch.equal(got, single[(k, t)]), "batched pack %d transpose=%d differs from the single launch" % (k, t)
            for x in FX.pack_cmps(k, t, dt, got, what="pack (batched)"):
                x.assert_ok()


# ----------------------------------------------------------------------------------------------------------------- the after-concat layer
@pytest.mark.parametrize("dt", FX.DT16)
@pytest.mark.parametrize("key", FX.SIDE_KEYS, ids=["L%d-%dx%dx%d-%s" % (k[0], k[1], k[2], k[3], "bias" if k[4] else "nobias") for k in FX.SIDE_KEYS])
def test_after_concat_layer_per_element(key, dt):
    from video_watermarking_forgery_detection_amd import ops
    r, T = FX.side_ref(*key), TORCH[dt]
    f = lambda a, t=torch.float32: torch.from_numpy(a).to(t).cuda().contiguous()          # noqa: E731
    img, w, msg = f(r.img), f(r.w), f(r.msg)
    bias = f(r.bias) if r.with_bias else None

    def once():
        P = ops.concat_side_fwd(img, w, bias, msg, T, r.c_msg, r.L, r.c_img)
        if r.Cin <= 128:
            wp = ops.pack_w3x3(w, 64, 64, T, perm=r.fperm)                                 # the encoder's channel map: features only
        else:
            wp = ops.pack_w3x3(w[:, r.L:r.L + 64].contiguous(), 64, 64, T)                 # (a channel map holds 128 entries)
        y, st = ops.conv3x3_fwd_addin(f(r.x, T), wp, f(r.in_scale), f(r.in_shift), P)
        dws = []
        for acc in (0, 1):
            dw = torch.full((64, r.Cin, 3, 3), FX.DW_START, device="cuda", dtype=torch.float32)
            ops.concat_side_msg_wgrad(f(r.dy, T), msg, dw, acc, r.c_msg, r.L)
            dws.append(dw)
        torch.cuda.synchronize()
        return P, y, st, dws[0], dws[1]

    first, second = once(), once()
    assert same_bits(first, second), "two runs of %s differ" % r.label(dt)
    P, y, st, dw0, dw1 = first
    cm = r.check_P(dt, P) + r.check_y(dt, y) + r.check_dw(dt, dw0, 0) + r.check_dw(dt, dw1, 1)
    for x in cm:
        print(x.line())
        if not x.exact:
            WORST[("concat_side", dt, "y against the concat's conv2d")] = max(WORST[("concat_side", dt, "y against the concat's conv2d")], x.worst)
    for x in cm:
        x.assert_ok()
        assert x.skipped == 0 and (x.exact or "against the concat" in x.what)


# ----------------------------------------------------------------------------------------------------------------- conv + bias + ELU
@pytest.mark.parametrize("dt", FX.DT16)
@pytest.mark.parametrize("key", FX.ELU_KEYS, ids=["%d-%dx%dx%d-%s" % k for k in FX.ELU_KEYS])
def test_elu_layer_per_element(key, dt):
    """wm_conv3x3_fwd_elu, wm_conv3x3_dgrad_elufused on (g, the out a correct forward stores) and wm_conv3x3_wgrad_bias on the restated gz
    and partial rows, accumulating or not"""
    from video_watermarking_forgery_detection_amd import _lib, ops
    r, T = FX.elu_case(key, dt), TORCH[dt]
    Cin, d = r.Cin, r.bwd[dt]
    f = lambda a, t=torch.float32: torch.from_numpy(a).to(t).cuda().contiguous()          # noqa: E731
    assert ops.conv3x3_fwd_elu_supported(Cin, 64, T) and FX.fwd_elu_supported(Cin, 64, dt)
    assert ops.conv3x3_dgrad_elufused_supported(Cin, T) and FX.dgrad_elufused_supported(Cin, dt)
    nrows = FX.dgrad_elufused_nparts(r.B, r.H, r.W)
    assert _lib.lib().wm_conv3x3_dgrad_elufused_nparts(r.B, r.H, r.W) == nrows
    x, w, bias, g, outq, gzr = f(r.x, T), f(r.w), f(r.bias), f(d["g"], T), f(d["out"], T), f(d["gz"], T)
    rows_in = f(r.wgrad_ref(dt, 0)[4])

    def once():
        out = ops.conv3x3_fwd_elu(x, ops.pack_w3x3(w, 64, Cin, T), bias)
        wpt = ops.pack_w3x3(w, 64, 32 if Cin == 16 else Cin, T, transpose=True)           # 16: packed to 32 rows, the upper 16 zero
        dx, gz, part = ops.conv3x3_dgrad_elufused(g, outq, wpt, dx_stride=16 if Cin == 16 else None)
        res = [out, dx, gz, part]
        for acc in (0, 1):
            dw = torch.full((64, Cin, 3, 3), FX.DW_START, device="cuda", dtype=torch.float32)
            db = torch.full((64,), FX.DB_START, device="cuda", dtype=torch.float32)
            ops.conv3x3_wgrad_bias(x, gzr, dw, acc, rows_in, db, acc)
            res += [dw, db]
        torch.cuda.synchronize()
        return res

    first, second = once(), once()
    assert same_bits(first, second), "two runs of %s differ" % r.label(dt)
    out, dx, gz, part, dw0, db0, dw1, db1 = first
    assert tuple(part.shape) == (nrows, 64) and tuple(dx.shape) == (r.B, r.H, r.W, Cin)
    cm = r.check_out(dt, out) + r.check_dgrad(dt, Cin, dx, gz, part) + r.check_wgrad(dt, 0, dw0, db0) + r.check_wgrad(dt, 1, dw1, db1)
    print("%s: ELU allowance %.3e (numpy float32 deviates %.3e from float64)" % (r.label(dt), r.allow, r.measured))
    for c in cm:
        print(c.line())
        if not c.exact:
            k = ("elu", dt, r.kind + " " + c.what.split(r.kind, 1)[1].split("acc=")[0].strip())
            WORST[k] = max(WORST[k], c.worst)
    if r.kind != "normal":                                  # the kernel's share of the ELU allowance alone: exact z, the store's half ulp taken off
        ref, b = r.out_ref(dt)
        o = out.double().cpu().numpy().reshape(ref.shape)
        live = b > 0
        if live.any():
            import numpy as np
            from layers_exact import half_ulp
            share = float(np.max((np.abs(o - ref)[live] - half_ulp(np.abs(ref), dt)[live]) / r.allow))
            WORST[("elu", dt, r.kind + " kernel's share of the ELU allowance (beyond the half ulp)")] = max(WORST[("elu", dt, r.kind + " kernel's share of the ELU allowance (beyond the half ulp)")], share)
    for c in cm:
        c.assert_ok()
        assert c.skipped == 0
    assert cm[1].exact, "gz is compared bit for bit"


def test_zz_report():
    """with -s: the largest share of each bound per family, dtype and quantity, and the ambiguous shares (filled by the tests above)"""
    for k in sorted(WORST):
        print("largest error / bound  %-12s %-5s %-60s %.3f" % (k[0], k[1], k[2].strip(), WORST[k]))
    for k in sorted(AMBIGUOUS):
        print("largest ambiguous share %-12s %-5s %.2e" % (k[0], k[1], AMBIGUOUS[k]))
    assert all(v <= 1.0 for v in WORST.values()) and all(v <= FX.AMBIGUOUS_CAP for v in AMBIGUOUS.values())
