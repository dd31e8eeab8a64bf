"""The per-element comparisons of tests/cbr_fwd_exact.py without a GPU.  A float32 imitation splits the work as the kernels do -- 16 x 16
tiles with an 18 x 18 halo cut from a canvas that is zero outside the image (the padding follows the transform), a rounded to 16 bits, float32 accumulation per
tile, one statistics row per run of tiles (per tile, per quarter tile) -- and passes every comparison of every case in every dtype, GENERIC
cases included: the bounds and the 1 % cap hold for correct arithmetic.  Each planted defect of the kinds these kernels can have FAILS
at the case named for it, and the first failing comparison names the quantity the defect spoils.  The restatement itself is checked once
against torch's float64 conv2d / conv_transpose2d / autograd on a 97-channel concat, so that a mistake shared by the restatement and the
imitation cannot hide in both.  So a green tests/test_gpu_cbr_fwd_exact.py means something."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cbr_fwd_exact as FX
from layers_exact import TORCH, all_ok, first_bad


def must_pass(cmps):
    for c in cmps:
        c.assert_ok()
        assert c.skipped == 0


def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


# ----------------------------------------------------------------------------------------------------------------- pack
def imitate_pack(w, CoutP, CinP, perm, transpose, dt, defect=None):
    """element by element, as a thread of the pack kernel sees it: output index -> (tap, row, col) -> which weight, if any"""
    Cout, Cin = w.shape[:2]
    rowsP, colsP = (CinP, CoutP) if transpose else (CoutP, CinP)
    out = np.zeros((9, rowsP, colsP), dtype=np.float32)
    if defect == "perm inverted" and perm is not None:
        perm = [perm.index(q) if q in perm else FX.DROP for q in range(Cin)]
    src = {}
    for q in range(Cin):
        p = q if perm is None else perm[q]
        if defect == "dropped channel packed" and p >= CinP:
            p = q % CinP
        src.setdefault(p, q)
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        if transpose != (defect in ("taps flipped in the forward pack", "taps not flipped in the transposed pack")):
            kh, kw = 2 - kh, 2 - kw
        if defect == "kh and kw swapped":
            kh, kw = kw, kh
        for cip in range(CinP):
            ci = src.get(cip)
            v = np.zeros(CoutP, dtype=np.float32)
            if ci is not None:
                v[:Cout] = w[:, ci, kh, kw]
            if defect == "padding rows not zero":
                v[Cout:] = v[0]
            if transpose:
                out[tap, cip, :] = v
            else:
                out[tap, :, cip] = v
    return torch.from_numpy(out).to(TORCH[dt])


PACK_KEYS = [(k, t, dt) for k in range(len(FX.PACK_SHAPES)) for t in (0, 1) for dt in ("f32",) + FX.DT16]


@pytest.mark.parametrize("k,transpose,dt", PACK_KEYS)
def test_faithful_pack_passes(k, transpose, dt):
    Cout, Cin, CoutP, CinP, pn = FX.PACK_SHAPES[k]
    must_pass(FX.pack_cmps(k, transpose, dt, imitate_pack(FX.pack_weight(k), CoutP, CinP, FX.pack_perm(pn), transpose, dt)))


PACK_DEFECTS = (
    ("taps flipped in the forward pack", 0, 0, "bf16", " values"),
    ("taps not flipped in the transposed pack", 0, 1, "f16", " values"),
    ("kh and kw swapped", 2, 0, "f32", " values"),
    ("perm inverted", 5, 0, "bf16", " values"),
    ("dropped channel packed", 3, 1, "bf16", " values"),
    ("dropped channel packed", 4, 0, "f16", " values"),
    ("padding rows not zero", 1, 0, "bf16", " padding"),
    ("padding rows not zero", 1, 1, "f32", " padding"),
)


@pytest.mark.parametrize("defect,k,transpose,dt,quantity", PACK_DEFECTS, ids=["%s@%d-%d-%s" % (d[0].replace(" ", "_"), d[1], d[2], d[3]) for d in PACK_DEFECTS])
def test_planted_pack_defect_fails_at_its_case(defect, k, transpose, dt, quantity):
    Cout, Cin, CoutP, CinP, pn = FX.PACK_SHAPES[k]
    cm = FX.pack_cmps(k, transpose, dt, imitate_pack(FX.pack_weight(k), CoutP, CinP, FX.pack_perm(pn), transpose, dt, defect))
    assert not all_ok(cm), "the defect `%s` passed every comparison" % defect
    assert quantity in first_bad(cm) and dt in first_bad(cm), first_bad(cm)


def test_transposed_pack_is_the_conv_transpose_operand():
    """the restated transposed pack of a layer's weight is the forward pack of conv_transpose2d's equivalent conv2d weight -- what ties
    `transpose` to the input gradient the transposed cases compare with"""
    r = FX.reference(32, 96, 1, 17, 33, False, 0, "grid", None, False, True)
    assert np.array_equal(FX.pack64(r.w_layer, 32, 96, None, True, "bf16"), FX.pack64(r.w, 96, 32, None, False, "bf16"))
    want = F.conv_transpose2d(FX.nchw(r.x), torch.from_numpy(r.w_layer), padding=1)
    assert np.abs(FX.nhwc(want) - r.y).max() <= 1e-12


# ----------------------------------------------------------------------------------------------------------------- forward
def imitate(c, dt, defect=None):
    """-> (ybuf [npix, ldy] of dtype dt, statistics rows [rows,2,CoutP] float32 or None)"""
    o, T = c.operands(dt), TORCH[dt]
    B, H, W, Cin, CoutP = c.B, c.H, c.W, c.Cin, c.CoutP
    x = o["x"][:, :Cin].float().reshape(B, H, W, Cin)
    border = None
    if c.xform:
        a = torch.relu(fma(o["in_scale"], x, o["in_shift"])).to(T).float()
        if defect == "padded before the transform":
            border = torch.relu(o["in_shift"]).to(T).float()
    else:
        a = x
    wl = o["w"]
    w = wl.permute(1, 0, 2, 3).flip(2, 3).contiguous() if c.transposed else wl          # what the pack hands the kernel: already exact in dt
    w = w.to(T).float()
    TL = FX.TILE
    Hp, Wp = FX.cdiv(H, TL) * TL, FX.cdiv(W, TL) * TL
    P = torch.zeros(B, Hp + 2, Wp + 2, Cin)                                              # the canvas of whole tiles, one pixel of halo
    if border is not None:
        P[:] = border
    if defect == "halo clamped":
        P[:, :H + 2, :W + 2] = F.pad(a.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").permute(0, 2, 3, 1)
    else:
        P[:, 1:H + 1, 1:W + 1] = a
    if defect == "halo across samples":
        P[1:, 0, 1:W + 1] = a[:-1, -1]
        P[:-1, H + 1, 1:W + 1] = a[1:, 0]
    bias = torch.zeros(CoutP)
    if c.nbias:
        bias[:c.nbias] = o["bias"]
        if defect == "bias beyond nbias":
            bias[c.nbias:] = o["bias"].repeat(CoutP)[:CoutP - c.nbias]
    acc = torch.zeros(B, Hp, Wp, CoutP)                                                  # the unrounded y of every pixel of every tile
    ybuf = o["y0"].clone().reshape(B, H, W, c.ldy)
    tiles = list(range(FX.ntiles(B, H, W)))
    if c.reverse and defect == "tile skipped under reverse":
        tiles = tiles[:-1]
    for t in tiles:
        b, h0, h1, w0, w1 = FX.tile_box(t, B, H, W)
        patch = P[b, h0:h0 + TL + 2, w0:w0 + TL + 2].clone()
        if defect == "halo zero at a tile seam":
            if h0 > 0: patch[0] = 0
            if h0 + TL < H: patch[-1] = 0
            if w0 > 0: patch[:, 0] = 0
            if w0 + TL < W: patch[:, -1] = 0
        s = F.conv2d(patch.permute(2, 0, 1)[None], w)[0].permute(1, 2, 0) + bias          # [16, 16, CoutP], float32 accumulation
        if c.addin and defect != "addend after the statistics":
            s[:h1 - h0, :w1 - w0] += o["addend"].float().reshape(B, H, W, CoutP)[b, h0:h1, w0:w1]
        acc[b, h0:h0 + TL, w0:w0 + TL] = s
        st = s[:h1 - h0, :w1 - w0]
        if c.addin and defect == "addend after the statistics":
            st = st + o["addend"].float().reshape(B, H, W, CoutP)[b, h0:h1, w0:w1]
        st = st.to(T)
        if defect == "channels swapped":
            st[..., [20, 21]] = st[..., [21, 20]]
        ybuf[b, h0:h1, w0:w1, :CoutP] = st
        if defect == "sentinel touched" and c.ldy > CoutP:
            ybuf[b, h0, w0, CoutP] = 0
    stat = None
    if c.stats:
        rows = FX.stat_rows(c.kernel, B, H, W, c.reverse)
        stat = torch.zeros(len(rows), 2, CoutP)
        for r, boxes in enumerate(rows):
            if defect == "last tile missing from its row" and len(boxes) > 1:
                boxes = boxes[:-1]
            for b, h0, h1, w0, w1 in boxes:
                if defect == "masked pixels counted":
                    h1, w1 = max(h1, min(h0 + TL, Hp)) if c.kernel != "stream" else h1, w0 + TL
                v = acc[b, h0:h1, w0:w1].reshape(-1, CoutP)
                if defect == "statistics of the rounded y":
                    v = v.to(T).float()
                stat[r, 0] += v.sum(0)
                stat[r, 1] += (v * v).sum(0)
    return ybuf.reshape(-1, c.ldy), stat


@pytest.mark.parametrize("cid,dt", FX.case_keys())
def test_faithful_imitation_passes_every_comparison(cid, dt):
    c = FX.case(cid)
    c.check_dispatch(dt)
    cm = c.check(dt, *imitate(c, dt))
    must_pass(cm)
    if c.kind == "normal":
        print("%s: %.2e of a ambiguous" % (c.label(dt), c.ref(dt).amb_share))
        assert c.ref(dt).amb_share <= FX.AMBIGUOUS_CAP
    elif c.kind == "sparse" or not c.stats:
        assert all(x.exact for x in cm), "an exact-data comparison with a bound"
    else:
        assert all(x.exact for x in cm if " sum y" not in x.what), "an exact-data comparison with a bound"


def test_case_table_reaches_every_form():
    fam = {}
    for c in FX.CASES:
        for dt in c.dts:
            fam.setdefault((c.family, dt in FX.DT16), []).append(c)
    for f in ("ws-whole", "ws-masked", "stream", "generic", "addin"):
        assert any(c.kind == "grid" for c in fam[(f, True)]) and any(c.kind == "sparse" for c in fam[(f, True)]) and any(c.kind == "normal" for c in fam[(f, True)]), f
    assert {c.Cin for c in fam[("generic", False)]} >= {4, 12, 16, 64} and {c.CoutP for c in fam[("generic", False)]} == {32, 64}
    masked = fam[("ws-masked", True)]
    assert {(c.Cin, c.CoutP, c.xform, c.stats) for c in masked} >= {(ci, co, xf, st) for ci, co in ((16, 64), (32, 64), (64, 64), (64, 32)) for xf in (0, 1) for st in (0, 1)}
    assert any(c.H % 16 == 0 and c.W % 16 == 0 and not c.xform and not c.stats for c in masked)
    assert FX.ws_form(64, 64, True, True, 16, 16) == "WHOLE" and FX.ws_form(64, 64, True, False, 16, 16) == "masked" and FX.ws_form(16, 64, False, True, 32, 32) == "WHOLE"
    assert FX.ws_form(16, 64, True, True, 16, 16) == "masked" and FX.ws_form(64, 64, True, True, 17, 16) == "masked" and FX.ws_form(32, 64, True, True, 16, 16) == "masked"
    assert FX.nparts(1, 16, 16 * 257, 64, 64, "bf16") == 129 and [len(r) for r in FX.ws_rows(1, 16, 16 * 257)] == [2] * 128 + [1]
    assert FX.ws_rows(1, 16, 16 * 257, True)[0] == [1, 0] and FX.ws_rows(1, 32, 128)[1] == [2] and FX.ws_rows(1, 32, 128)[8] == [1]
    assert FX.nparts(1, 17, 33, 128, 128, "f16") == 4 * 6 and FX.nparts(1, 17, 33, 48, 96, "bf16") == 6 and FX.nparts(1, 17, 33, 64, 64, "f32") == 6
    assert FX.kernel_of(112, 64, "bf16") == "stream" and FX.kernel_of(16, 128, "bf16") == "generic" and FX.kernel_of(64, 64, "f32") == "generic"
    assert FX.kernel_of(32, 32, "bf16") == "generic" and FX.kernel_of(64, 32, "f16") == "ws" and FX.kernel_of(48, 96, "f16") == "generic"
    assert any(c.transposed for c in fam[("ws-masked", True)]) and any(c.transposed for c in fam[("stream", True)]) and any(c.transposed for c in fam[("generic", True)])
    assert any(c.transposed for c in fam[("generic", False)])
    assert all(c.ldy_gap for c in fam[("stream", True)] if c.stats) and any(c.ldx_gap and c.ldy_gap for c in fam[("generic", True)])


# (defect, the case it must fail at, dtype, the quantity its first failing comparison names)
DEFECTS = (
    ("padded before the transform", "ws-masked-64to64-1x17x33-grid-xf-st-b30-rev", "bf16", " y"),
    ("padded before the transform", "stream-128to128-1x17x33-grid-xf-st-b30-ldx-ldy", "f16", " y"),
    ("halo clamped", "ws-whole-16to64-1x16x16-grid-st-b64-rev", "bf16", " y"),
    ("halo clamped", "generic-4to32-2x16x16-grid-st-b30-ldy", "f32", " y"),
    ("halo across samples", "ws-whole-64to64-2x32x32-grid-xf-st-b30-rev", "f16", " y"),
    ("halo across samples", "stream-112to64-2x16x16-grid-st-b30-ldy", "bf16", " y"),
    ("halo zero at a tile seam", "ws-masked-32to64-1x17x33-grid-st-b30-rev", "bf16", " y"),
    ("halo zero at a tile seam", "generic-48to96-1x17x33-grid-st-b30-ldx-ldy", "f16", " y"),
    ("channels swapped", "ws-masked-64to32-3x15x18-grid-b30-ldx", "bf16", " y"),
    ("bias beyond nbias", "ws-masked-16to64-1x1x1-grid-b30", "f16", " y"),
    ("bias beyond nbias", "generic-16to128-1x17x33-grid-st-b30-ldx-ldy", "bf16", " y"),
    ("statistics of the rounded y", "ws-masked-64to64-1x17x33-normal-xf-st-b30", "bf16", " rows sum y"),
    ("statistics of the rounded y", "stream-256to64-1x20x21-grid-st-b30-ldy", "bf16", " column sums of sum y"),
    ("masked pixels counted", "ws-masked-64to64-1x17x33-sparse-xf-st", "bf16", " rows sum y"),
    ("masked pixels counted", "ws-masked-16to64-1x16x1-grid-st-b30-rev-ldx", "f16", " rows sum y"),
    ("masked pixels counted", "stream-128to128-1x17x33-sparse-xf-st-ldy", "f16", " column sums of sum y"),
    ("masked pixels counted", "generic-12to64-1x17x33-grid-xf-st-b30", "f32", " column sums of sum y"),
    ("last tile missing from its row", "ws-whole-64to64-1x16x4112-sparse-xf-st", "bf16", " rows sum y"),
    ("last tile missing from its row", "ws-whole-64to64-1x16x4112-sparse-xf-st-rev", "bf16", " rows sum y"),
    ("tile skipped under reverse", "ws-whole-64to64-1x16x4112-sparse-xf-st-rev", "bf16", " y"),
    ("tile skipped under reverse", "addin-64to64-1x17x33-grid-xf-st-rev", "f16", " y"),
    ("addend after the statistics", "addin-64to64-1x16x16-grid-xf-st", "bf16", " rows sum y"),
    ("addend after the statistics", "addin-64to64-2x32x32-sparse-xf-st", "f16", " rows sum y"),
    ("sentinel touched", "stream-128to128-2x16x16-grid-st-b30-ldy", "bf16", " stride gap"),
    ("sentinel touched", "generic-16to32-1x17x33-grid-st-b30-ldx-ldy", "f16", " stride gap"),
)


@pytest.mark.parametrize("defect,cid,dt,quantity", DEFECTS, ids=["%s@%s-%s" % (d[0].replace(" ", "_"), d[1], d[2]) for d in DEFECTS])
def test_planted_defect_fails_at_its_case(defect, cid, dt, quantity):
    assert cid in FX.CASE_IDS, "the case named for `%s` left the table" % defect
    c = FX.case(cid)
    cm = c.check(dt, *imitate(c, dt, defect))
    assert not all_ok(cm), "the defect `%s` passed every comparison" % defect
    line = first_bad(cm)
    assert c.label(dt) in line and quantity in line, line


def test_permuted_rows_are_told_apart():
    """a persistent kernel that wrote its row at the run's index instead of the workgroup's fails at the 16-workgroup case"""
    c = FX.case("ws-whole-64to64-1x32x128-sparse-xf-st")
    y, st = imitate(c, "bf16")
    perm = [FX.xcd_run(16, g) for g in range(16)]
    assert perm != list(range(16))
    bad = torch.empty_like(st)
    bad[perm] = st
    assert not all_ok(c.check("bf16", y, bad)) and all_ok(c.check("bf16", y, st))


# ----------------------------------------------------------------------------------------------------------------- the after-concat layer
def imitate_side(r, dt, defect=None):
    """float32: P, y = conv64(features) + P through the addin arithmetic, and dw after the message channels' weight gradient"""
    T = TORCH[dt]
    B, H, W, L = r.B, r.H, r.W, r.L
    w = torch.from_numpy(r.w).float()
    img = torch.from_numpy(r.img).float()
    msg = torch.from_numpy(r.msg).float()
    if defect == "msg[0] for every sample":
        msg = msg[:1].expand(B, L)
    inside = torch.from_numpy(FX.taps_inside(H, W)).float()
    if defect == "message taps outside the image":
        inside = torch.ones_like(inside)
    mbias = torch.einsum("olt,bl->bto", w[:, r.c_msg:r.c_msg + L].reshape(64, L, 9), msg)
    P = F.conv2d(img, w[:, r.c_img:r.c_img + 3], padding=1).permute(0, 2, 3, 1) + torch.from_numpy(r.bias).float() + torch.einsum("bto,thw->bhwo", mbias, inside)
    P = P.to(T)
    a = torch.relu(fma(torch.from_numpy(r.in_scale).float(), torch.from_numpy(r.x).float(), torch.from_numpy(r.in_shift).float())).to(T).float()
    y = (F.conv2d(a.permute(0, 3, 1, 2), w[:, L:L + 64], padding=1).permute(0, 2, 3, 1) + P.float()).to(T)
    return P, y


def imitate_msg_wgrad(r, dt, accumulate, defect=None):
    B, H, W, L = r.B, r.H, r.W, r.L
    dy = torch.from_numpy(r.dy).to(TORCH[dt]).float()
    inside = torch.from_numpy(FX.taps_inside(H, W)).float()
    if defect == "message taps outside the image":
        inside = torch.ones_like(inside)
    msg = torch.from_numpy(r.msg).float()
    if defect == "msg[0] for every sample":
        msg = msg[:1].expand(B, L)
    S = torch.einsum("bhwo,thw->bto", dy, inside)
    dw = torch.full((64, r.Cin, 3, 3), FX.DW_START)
    upd = torch.einsum("bl,bto->olt", msg, S).reshape(64, L, 3, 3)
    if defect == "other channels written":
        dw[:, r.c_img] = 0
    if accumulate and defect != "accumulate overwrites":
        dw[:, r.c_msg:r.c_msg + L] += upd
    else:
        dw[:, r.c_msg:r.c_msg + L] = upd
    return dw


@pytest.mark.parametrize("dt", FX.DT16)
@pytest.mark.parametrize("key", FX.SIDE_KEYS, ids=["L%d-%dx%dx%d-%s" % (k[0], k[1], k[2], k[3], "bias" if k[4] else "nobias") for k in FX.SIDE_KEYS])
def test_faithful_after_concat_imitation_passes(key, dt):
    r = FX.side_ref(*key)
    P, y = imitate_side(r, dt)
    must_pass(r.check_P(dt, P) + r.check_y(dt, y))
    for acc in (0, 1):
        must_pass(r.check_dw(dt, imitate_msg_wgrad(r, dt, acc), acc))
    assert np.abs(r.conv_feat + r.P - r.cat_conv()).max() <= 1e-12            # the header's identity, in float64


SIDE_DEFECTS = (
    ("message taps outside the image", (30, 1, 2, 2, True), "bf16", " P", "fwd"),
    ("message taps outside the image", (1, 2, 32, 32, True), "f16", " P", "fwd"),
    ("msg[0] for every sample", (64, 2, 32, 32, False), "bf16", " P", "fwd"),
    ("message taps outside the image", (30, 1, 17, 33, False), "bf16", " dw message channels", "wgrad"),
    ("msg[0] for every sample", (30, 2, 32, 32, True), "f16", " dw message channels", "wgrad"),
    ("accumulate overwrites", (64, 1, 17, 33, True), "bf16", " dw message channels", "wgrad"),
    ("other channels written", (1, 1, 2, 2, True), "f16", " dw other channels", "wgrad"),
)


@pytest.mark.parametrize("defect,key,dt,quantity,which", SIDE_DEFECTS, ids=["%s@L%d-%dx%dx%d-%s" % ((d[0].replace(" ", "_"),) + d[1][:4] + (d[2],)) for d in SIDE_DEFECTS])
def test_planted_after_concat_defect_fails_at_its_case(defect, key, dt, quantity, which):
    assert key in FX.SIDE_KEYS, "the case named for `%s` left the table" % defect
    r = FX.side_ref(*key)
    if which == "fwd":
        P, y = imitate_side(r, dt, defect)
        cm = r.check_P(dt, P) + r.check_y(dt, y)
    else:
        cm = r.check_dw(dt, imitate_msg_wgrad(r, dt, 1, defect), 1)
    assert not all_ok(cm), "the defect `%s` passed every comparison" % defect
    assert r.label(dt) in first_bad(cm) and quantity in first_bad(cm), first_bad(cm)


# ----------------------------------------------------------------------------------------------------------------- the restatement itself
def test_restatement_against_torch_float64_on_a_97_channel_concat():
    """conv64 / stats_ref / SideRef against torch's own float64 conv2d and autograd, written independently of cbr_fwd_exact's helpers"""
    r = FX.side_ref(30, 1, 17, 33, True)
    B, H, W, L = r.B, r.H, r.W, r.L
    planes = torch.from_numpy(r.msg)[:, :, None, None].expand(B, L, H, W)
    feat = torch.relu(torch.from_numpy(r.in_scale)[None, :, None, None] * torch.from_numpy(r.x).permute(0, 3, 1, 2) + torch.from_numpy(r.in_shift)[None, :, None, None])
    cat = torch.cat([planes, feat, torch.from_numpy(r.img)], dim=1)
    assert cat.shape[1] == 97
    w = torch.from_numpy(r.w).clone().requires_grad_(True)
    y = F.conv2d(cat, w, torch.from_numpy(r.bias), padding=1)
    assert np.abs(y.detach().permute(0, 2, 3, 1).numpy() - (r.conv_feat + r.P)).max() <= 1e-12
    y.backward(torch.from_numpy(r.dy).permute(0, 3, 1, 2))
    assert np.abs(w.grad[:, :L].numpy() - r.dwm).max() <= 1e-12
    # the plain forward with transform, bias beyond nbias absent, and its statistics rows
    c = FX.case("ws-masked-64to64-1x17x33-grid-xf-st-b30-rev")
    q = c.ref("bf16")
    a = torch.relu(torch.from_numpy(q.in_scale)[None, :, None, None] * torch.from_numpy(q.x).permute(0, 3, 1, 2) + torch.from_numpy(q.in_shift)[None, :, None, None])
    want = F.conv2d(a, torch.from_numpy(q.w), torch.from_numpy(q.bias), padding=1).permute(0, 2, 3, 1).numpy()
    assert np.abs(want - q.y).max() <= 1e-12 and np.all(q.bias[30:] == 0) and np.any(q.in_shift > 0)
    ref, _ = q.stats_ref(FX.stat_rows("ws", 1, 17, 33))
    assert np.abs(ref[:, 0].sum(0) - want.sum((0, 1, 2))).max() <= 1e-9 and np.abs(ref[:, 1].sum(0) - (want * want).sum((0, 1, 2))).max() <= 1e-7
    assert np.abs(ref[5, 0] - want[0, 16:, 32:].sum((0, 1))).max() <= 1e-12            # tile 5 of 2 x 3: one row, one column


# ----------------------------------------------------------------------------------------------------------------- conv + bias + ELU
def imitate_elu(r, dt, defect=None):
    """float32: out of the forward; gz, dx, the bias partial rows of the input-gradient call on (g, the stored out); dw, db onto the starts"""
    T = TORCH[dt]
    B, H, W, Cin = r.B, r.H, r.W, r.Cin
    x, w = torch.from_numpy(r.x).float(), torch.from_numpy(r.w).float()
    z = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1) + torch.from_numpy(r.bias).float()
    zn = z.numpy()
    if defect == "exp - 1 below the switch, in the storage type":
        h = zn.astype(np.float16)
        small = (np.abs(zn) < FX.ELU_SWITCH) & (zn <= 0)
        e = (np.exp(h) - np.float16(1)).astype(np.float32)
        o32 = np.where(small, e, FX.elu_np32(zn))
    else:
        o32 = FX.elu_np32(zn)
    out = torch.from_numpy(o32).to(T)
    d = r.bwd[dt]
    g, outq = torch.from_numpy(d["g"]).float(), torch.from_numpy(d["out"]).float()
    if defect == "derivative from z":
        fac = torch.where(z > 0, torch.ones(()), torch.exp(z))
    else:
        fac = torch.where(outq > 0, torch.ones(()), outq + 1)
    p = g * fac
    gz = p.to(T)
    wt = w.permute(1, 0, 2, 3).flip(2, 3).contiguous()
    dx = F.conv2d(gz.float().permute(0, 3, 1, 2), wt, padding=1).permute(0, 2, 3, 1).to(T)
    rr = FX.stat_rows("ws", B, H, W)
    rows = torch.zeros(len(rr), 64)
    src = gz.float() if defect == "bias partials of the rounded gz" else p
    for k, boxes in enumerate(rr):
        for b, h0, h1, w0, w1 in boxes:
            rows[k] += src[b, h0:h1, w0:w1].reshape(-1, 64).sum(0)
    res = {"out": out, "gz": gz, "dx": dx, "rows": rows}
    dw1 = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (64, Cin, 3, 3), gz.float().permute(0, 3, 1, 2), padding=1)
    rows_in = torch.from_numpy(r.wgrad_ref(dt, 0)[4]).float()
    for acc in (0, 1):
        keep = acc and defect != "accumulate overwrites"
        res["dw%d" % acc] = dw1 + (FX.DW_START if keep else 0.0)
        res["db%d" % acc] = rows_in.sum(0) + (FX.DB_START if keep else 0.0)
    return res


def elu_cmps(r, dt, res):
    return r.check_out(dt, res["out"]) + r.check_dgrad(dt, r.Cin, res["dx"], res["gz"], res["rows"]) + \
        r.check_wgrad(dt, 0, res["dw0"], res["db0"]) + r.check_wgrad(dt, 1, res["dw1"], res["db1"])


ELU_IDS = ["%d-%dx%dx%d-%s" % k for k in FX.ELU_KEYS]


@pytest.mark.parametrize("dt", FX.DT16)
@pytest.mark.parametrize("key", FX.ELU_KEYS, ids=ELU_IDS)
def test_faithful_elu_imitation_passes(key, dt):
    r = FX.elu_case(key, dt)
    must_pass(elu_cmps(r, dt, imitate_elu(r, dt)))
    assert FX.ELU_FLOOR <= r.allow <= 1e-6, "the measured ELU allowance left its range: %g" % r.allow
    print("%s: ELU allowance %.3e (numpy float32 deviates %.3e)" % (r.label(dt), r.allow, r.measured))


def test_planted_values_are_all_there():
    for dt in FX.DT16:
        r = FX.elu_case((64, 1, 16, 16, "planted"), dt)
        zs = set(np.unique(r.z[..., 0::2])) | set(np.unique(r.z[..., 1::2]))
        for v in (0.0, 1.0 / 64, -1.0 / 64, -2.0 ** -14, -1.0, -20.0, -100.0, 3.0):
            assert v in zs, (dt, v)
        assert np.any(np.signbit(r.x) & (r.x == 0)) and len(set(FX.neighbours16(-1.0 / 64, dt))) == 5
        tie = 1.0 + {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}[dt]
        assert tie in zs and FX.rnd(np.array([tie]), dt)[0] == 1.0                         # to even
        ref, b = r.out_ref(dt)
        assert np.all(ref[r.z <= -20] == -1.0) and np.all(b[r.z <= -20] == 0) and np.all(b[r.z > 0] == 0)
        lo, hi = FX.neighbours16(-1.0 / 64, dt, (1,))[0], FX.neighbours16(-1.0 / 64, dt, (-1,))[0]
        assert abs(lo) >= FX.ELU_SWITCH > abs(hi)                                           # one on each side of the switch


ELU_DEFECTS = (
    ("exp - 1 below the switch, in the storage type", (64, 1, 16, 16, "planted"), "f16", " out"),
    ("derivative from z", (64, 1, 16, 16, "planted"), "bf16", " gz"),
    ("derivative from z", (32, 1, 17, 33, "grid"), "f16", " gz"),
    ("bias partials of the rounded gz", (16, 3, 20, 20, "grid"), "bf16", " bias partial rows"),
    ("accumulate overwrites", (64, 1, 16, 16, "grid"), "f16", " dw"),
)


@pytest.mark.parametrize("defect,key,dt,quantity", ELU_DEFECTS, ids=["%s@%s-%s" % (d[0].replace(" ", "_"), "%d-%dx%dx%d-%s" % d[1], d[2]) for d in ELU_DEFECTS])
def test_planted_elu_defect_fails_at_its_case(defect, key, dt, quantity):
    assert key in FX.ELU_KEYS, "the case named for `%s` left the table" % defect
    r = FX.elu_case(key, dt)
    cm = elu_cmps(r, dt, imitate_elu(r, dt, defect))
    assert not all_ok(cm), "the defect `%s` passed every comparison" % defect
    assert r.label(dt) in first_bad(cm) and quantity in first_bad(cm), first_bad(cm)
