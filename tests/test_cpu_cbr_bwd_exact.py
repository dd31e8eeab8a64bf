"""The per-element comparisons of tests/cbr_bwd_exact.py without a GPU.  A float32 imitation forms dy, dx, the partial rows and the dW
slabs in the pieces the kernels split the work into -- per 8 x 16 tile (one-pass kernels) or 16 x 16 tile (two-kernel routes) with a halo
from the neighbouring tiles, dy and the staged activation rounded to 16 bits, float32 accumulation per tile, one slab and one partial
row per run of tiles (cut the bwd_ws8 way for every kernel: where a run ends moves sums between rows and changes no column sum), the
fixed-order reduction -- and passes every comparison of every case in both 16-bit types, GENERIC cases included: the bounds and the 1 % cap hold for correct
arithmetic.  Each planted defect of the kinds these kernels can have FAILS at the case named for it, and the first failing comparison
names the quantity the defect spoils.  The data holds its conditions: building a GRID reference asserts that dy, a and z are exact and
that every sum stays below 2**24 grid units; every case takes the path it names.  So a green tests/test_gpu_cbr_bwd_exact.py means
something."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cbr_bwd_exact as CX
from layers_exact import TORCH, all_ok, first_bad

C = CX.C


def must_pass(cmps):
    for c in cmps:
        c.assert_ok()
        assert c.skipped == 0


def fma(a, b, c):
    """float32 a*b + c with one rounding (the product of two float32 values is exact in double)"""
    return (a.double() * b.double() + c.double()).float()


def padded(t, mode, border=None):
    """t [B,H,W,K] float32 -> [B,H+2,W+2,K] with the halo ring: zero (the definition), `clamp` (the edge pixel repeated), `sample` (the
    rows of the neighbouring sample: the batch read as one tall image), or `border` [K] (a constant per channel)"""
    B, H, W, K = t.shape
    if mode == "clamp":
        return F.pad(t.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").permute(0, 2, 3, 1).contiguous()
    p = torch.zeros(B, H + 2, W + 2, K)
    if border is not None:
        p[:] = border
    p[:, 1:-1, 1:-1] = t
    if mode == "sample":
        p[1:, 0, 1:-1] = t[:-1, -1]
        p[:-1, -1, 1:-1] = t[1:, 0]
    return p


def imitate(c, dt, defect=None):
    """c: a one-pass Case (8 x 16 tiles) or a two-kernel Route (16 x 16 tiles) -> dict: dy [B,H,W,64] and dx [B,H,W,CinP] of dtype dt,
    partials [nwg,2,64] float32 (None where dx leaves unmasked), dw [64,Cin,3,3] float32.  The tile list is cut into runs the way
    csrc/bwd_ws8.hip cuts it (the first tiles % workgroups runs one longer); csrc/bwd_ws.hip and the two-kernel kernels cut elsewhere,
    which moves sums between rows and slabs and changes no column sum -- the only thing compared."""
    r, o = c.ref(dt), CX.operands(c, dt)
    B, H, W, T = r.B, r.H, r.W, TORCH[dt]
    sc, sh, mu, isd = o["stats4"]
    ca, c1, c2 = o["coef"]
    # dy as csrc/wm_common.h folds it, in float32
    k2 = ca * (isd * c2)
    k3 = fma(k2, mu, ca * c1 if defect == "k3 sign" else -(ca * c1))
    y = o["y"].float()
    if c.gform == "gvec":
        g = (o["gvec"][:1] if defect == "gvec row 0" else o["gvec"])[:, None, None, :].expand(B, 1, 1, C)
    else:
        g = o["g"].float()
    masked = c.gform != "premasked" and defect != "mask dropped"
    gm = torch.where(fma(sc, y, sh) > 0, g.expand_as(y), torch.zeros(())) if masked else g.expand_as(y)
    dy = fma(-k2, y, fma(ca, gm, k3)) if c.gform == "gvec" else fma(ca, gm, fma(-k2, y, k3))
    if defect != "dy in float32":
        dy = dy.to(T).float()
    # the staged activation
    if c.layer == "body":
        xr = o["xr"].float()
        zin = fma(o["in_scale"], xr, o["in_shift"])
        a, mask = torch.relu(zin).to(T).float(), zin > 0
        border = torch.relu(o["in_shift"]).to(T).float() if defect == "a padded before the activation" else None
        w = o["w"]
    else:
        a, mask, border = o["x16"].float(), None, None
        w = torch.zeros(C, c.CinP, 3, 3)
        w[:, :3] = o["w"]
    if not c.dx_masked:
        mask = None
    CinP, CA, TH, TW = c.CinP, a.shape[3], c.tile_h, c.tile_w
    Pa = padded(a, "zero", border)
    Pd = padded(dy, {"halo clamped": "clamp", "halo across samples": "sample"}.get(defect, "zero"))
    wd = w.permute(1, 0, 2, 3).contiguous() if defect == "taps not flipped" else w.permute(1, 0, 2, 3).flip(2, 3).contiguous()
    ty, tx = CX.cdiv(H, TH), CX.cdiv(W, TW)
    tiles = [(b, i, j) for b in range(B) for i in range(ty) for j in range(tx)]
    if c.reverse:
        tiles = tiles[::-1]
        if defect == "tile skipped under reverse":
            tiles = tiles[:-1]
    nwg = c.expected_nwg()
    q, rem = divmod(len(tiles), nwg)
    dx = torch.zeros(B, H, W, CinP, dtype=T)
    rows = torch.zeros(nwg, 2, C)
    slabs = torch.zeros(nwg, C, CA, 3, 3)
    pos = 0
    for wg in range(nwg):
        run = tiles[pos:pos + q + (1 if wg < rem else 0)]
        pos += len(run)
        for k, (b, i, j) in enumerate(run):
            h0, w0 = i * TH, j * TW
            h1, w1 = min(h0 + TH, H), min(w0 + TW, W)
            last_of_many = len(run) > 1 and k == len(run) - 1
            patch = Pd[b, h0:h1 + 2, w0:w1 + 2].clone()
            if defect == "halo zero at a tile seam":
                if h0 > 0: patch[0] = 0
                if h1 < H: patch[-1] = 0
                if w0 > 0: patch[:, 0] = 0
                if w1 < W: patch[:, -1] = 0
            s = F.conv2d(patch.permute(2, 0, 1)[None], wd)[0].permute(1, 2, 0)          # [th, tw, CinP], float32 accumulation
            if mask is not None and defect != "dx not masked":
                s = torch.where(mask[b, h0:h1, w0:w1], s, torch.zeros(()))
            st = s.to(T)
            if defect == "channels swapped":
                st[..., [20, 21]] = st[..., [21, 20]]
            if defect == "padding channels not zero":
                st[..., 3:] = st[..., :1]
            dx[b, h0:h1, w0:w1] = st
            if c.dx_masked and not (defect == "last tile missing from the rows" and last_of_many):
                gz = s if defect == "sums of the unrounded dx" else st.float()
                other = a[b, h0:h1, w0:w1] if defect == "sum gz*a" else xr[b, h0:h1, w0:w1]
                rows[wg, 0] += gz.reshape(-1, C).sum(0)
                rows[wg, 1] += (gz * other).reshape(-1, C).sum(0)
            if defect == "last tile missing from dW" and last_of_many:
                continue
            d2 = dy[b, h0:h1, w0:w1].reshape(-1, C)
            ap = Pa[b, h0:h1 + 2, w0:w1 + 2]
            for kh in range(3):
                for kw in range(3):
                    t = d2.t() @ ap[kh:kh + h1 - h0, kw:kw + w1 - w0].reshape(-1, CA)
                    if defect == "kh and kw swapped":
                        slabs[wg, :, :, kw, kh] += t
                    else:
                        slabs[wg, :, :, kh, kw] += t
    Cin = o["w"].shape[1]
    dw = torch.cumsum(slabs, 0)[-1][:, :Cin]                                           # the fixed-order reduction, float32
    if c.accumulate and defect != "accumulate overwrites":
        dw = o["dw0"] + dw
    return {"dy": dy.to(T), "dx": dx, "partials": rows if c.dx_masked else None, "dw": dw}


def run_case(c, dt, defect=None):
    d = imitate(c, dt, defect)
    if isinstance(c, CX.Case):
        return c.check(dt, d["dx"], d["partials"], d["dw"])
    d.update(dx_b=d["dx"], partials_b=d["partials"])             # wm_conv3x3_dgrad_bwdstats on the route's dy: the same arithmetic
    return c.check(dt, {k: d[k] for k in c.outputs})


@pytest.mark.parametrize("dt", CX.DT16)
@pytest.mark.parametrize("cid", CX.CASE_IDS)
def test_faithful_imitation_passes_every_comparison(cid, dt):
    c = CX.case(cid)
    c.check_dispatch(dt)                                   # building the reference asserts the grid conditions
    cm = run_case(c, dt)
    must_pass(cm)
    if c.kind != "normal":
        assert all(x.exact for x in cm), "a GRID comparison with a bound"


@pytest.mark.parametrize("cid,dt", CX.route_keys())
def test_faithful_imitation_passes_every_route(cid, dt):
    c = CX.route_case(cid)
    c.check_dispatch(dt)
    cm = run_case(c, dt)
    must_pass(cm)
    if c.kind != "normal":
        assert all(x.exact for x in cm), "a GRID comparison with a bound"


@pytest.mark.parametrize("dt", CX.DT16)
@pytest.mark.parametrize("cid", [i for i in CX.CASE_IDS if CX.case(i).kind == "normal"] + [i for i in CX.ROUTE_IDS if CX.route_case(i).kind == "normal"])
def test_generic_cases_keep_the_ambiguity_cap(cid, dt):
    c = CX.case(cid) if cid in CX.CASE_IDS else CX.route_case(cid)
    r = c.ref(dt)
    print("%s: %.2e of the dy elements at a rounding boundary, %.2e at an ambiguous mask" % (c.label(dt), r.amb_r_share, r.amb_z_share))
    assert r.amb_share <= CX.AMBIGUOUS_CAP


def test_route_table_covers_every_route_and_shape():
    for route in CX.ROUTES:
        mine = [c for c in CX.ROUTE_CASES if c.route == route]
        assert {(c.B, c.H, c.W) for c in mine if c.kind != "normal"} >= set(CX.ROUTE_SHAPES) and any(c.kind == "normal" and (c.B, c.H, c.W) == (1, 17, 33) for c in mine)
    assert CX.nparts16(*CX.MANY_TILES) == 129 and CX.nslabs16(*CX.MANY_TILES) == 256 and CX.terms_per_row16(*CX.MANY_TILES) == 512 and CX.nparts16(1, 17, 33) == 6
    assert CX.applyfused_supported(64, 32, "f16") and not CX.applyfused_supported(64, 16, "bf16") and not CX.bwdstats_supported(64, 32, "bf16")
    assert CX.gvfused_supported(64, 32, "bf16") and not CX.gvfused_supported(32, 64, "bf16") and CX.wgrad_bnfused_supported(16, 64, "f16")
    assert not CX.wgrad_bnfused_supported(32, 64, "bf16")


def test_case_table_reaches_every_path():
    by = {k: [c for c in CX.CASES if c.kernel == k] for k in ("ws8", "ws", "ws16")}
    assert all(c.H % 8 == 0 and c.W % 16 == 0 and c.gform != "g" for c in by["ws8"])
    assert any(c.premasked and (c.H % 8 or c.W % 16) for c in by["ws"])                 # premasked on a ragged shape: kernel 1
    assert CX.fused_kernel(7, 15, True, False) == 1 and CX.fused_kernel(8, 16, True, False) == 8 and CX.fused_kernel(8, 16, False, False) == 1
    assert CX.fused_kernel(8, 16, False, True) == 8 and CX.fused_kernel(9, 17, False, True) == 1
    for k in by:
        assert any(CX.ntiles(c.B, c.H, c.W) > CX.MAX_WGS and c.reverse for c in by[k]) and any(c.kind == "normal" for c in by[k])
    assert CX.fused_nwg(3, 80, 144) == 256 and CX.fused_nwg(3, 75, 140) == 256 and CX.fused16_nwg(3, 80, 144) == 256 and CX.fused_nwg(1, 9, 17) == 4
    assert CX.fused16_supported(1, 8, 16, "bf16") and not CX.fused16_supported(1, 9, 16, "f16") and not CX.fused16_supported(1, 8, 16, "f32")


# (defect, the case it must fail at, dtype, the quantity its first failing comparison names)
DEFECTS = (
    ("taps not flipped", "ws8-1x8x16-premasked-grid", "bf16", " dx"),
    ("kh and kw swapped", "ws8-1x8x16-premasked-grid", "f16", " dW"),
    ("halo zero at a tile seam", "ws8-1x16x32-premasked-grid-acc", "bf16", " dx"),
    ("halo across samples", "ws8-2x8x32-premasked-grid", "f16", " dx"),
    ("halo clamped", "ws8-1x8x16-premasked-grid", "bf16", " dx"),
    ("a padded before the activation", "ws8-1x8x16-premasked-grid", "bf16", " dW"),
    ("mask dropped", "ws-1x8x16-g-grid", "f16", " dx"),
    ("dx not masked", "ws-1x7x15-g-grid", "bf16", " dx"),
    ("sums of the unrounded dx", "ws8-2x16x32-premasked-normal-acc", "bf16", " partials"),
    ("sum gz*a", "ws-2x13x37-g-grid-acc", "f16", " partials sum gz*xr"),
    ("k3 sign", "ws-1x9x17-g-grid", "bf16", " dx"),
    ("gvec row 0", "ws8-2x8x16-gvec-grid", "bf16", " dx"),
    ("last tile missing from dW", "ws8-3x80x144-premasked-coarse", "bf16", " dW"),
    ("last tile missing from the rows", "ws-3x75x140-g-coarse", "f16", " partials"),
    ("tile skipped under reverse", "ws8-3x80x144-premasked-coarse-rev-acc", "bf16", " dx"),
    ("accumulate overwrites", "ws-1x16x32-g-grid-acc", "bf16", " dW"),
    ("channels swapped", "ws-2x16x16-g-grid", "f16", " dx"),
    ("dy in float32", "ws-2x13x37-g-normal-acc", "bf16", " dx"),
    ("padding channels not zero", "ws16-1x8x16-g-grid", "bf16", " dx padding channels"),
    ("last tile missing from dW", "ws16-3x80x144-g-coarse-acc", "f16", " dW"),
    ("kh and kw swapped", "ws16-2x8x32-g-grid", "bf16", " dW"),
    ("taps not flipped", "ws16-1x16x32-premasked-grid", "f16", " dx"),
    # the two-kernel routes
    ("dy in float32", "body_two_kernels-1x17x33-normal-acc", "f16", " dx"),
    ("k3 sign", "first_two_kernels-1x16x16-grid-acc", "bf16", " dy_out"),
    ("taps not flipped", "body_two_kernels-1x17x33-grid-rev", "bf16", " dx"),
    ("halo zero at a tile seam", "body_two_kernels-2x32x32-coarse-acc", "f16", " dx"),
    ("halo across samples", "pooled-2x32x32-coarse-acc", "bf16", " dx"),
    ("mask dropped", "dx_only-1x16x16-grid-acc", "bf16", " dx"),
    ("dx not masked", "pooled_feed-1x17x33-grid-rev", "f16", " dx"),
    ("gvec row 0", "pooled_feed-2x32x32-coarse-acc", "bf16", " dx"),
    ("sum gz*a", "body_two_kernels-1x17x33-grid-rev", "f16", " partials sum gz*xr"),
    ("sums of the unrounded dx", "pooled_feed-1x17x33-normal-acc", "bf16", " partials"),
    ("kh and kw swapped", "pooled-1x17x33-grid-rev", "bf16", " dW"),
    ("a padded before the activation", "body_two_kernels-1x16x16-grid-acc", "f16", " dW"),
    ("accumulate overwrites", "first_layer_weights_only-2x32x32-coarse-acc", "bf16", " dW"),
    ("padding channels not zero", "first_two_kernels-1x17x33-grid-rev", "f16", " dx padding channels"),
    ("last tile missing from dW", "body_two_kernels-1x16x4112-coarse-rev", "bf16", " dW"),
    ("last tile missing from the rows", "body_two_kernels-1x16x4112-coarse-rev", "bf16", " partials"),
)


@pytest.mark.parametrize("defect,cid,dt,quantity", DEFECTS, ids=["%s@%s-%s" % (d[0].replace(" ", "_"), d[1], d[2]) for d in DEFECTS])
def test_planted_defect_fails_at_its_case(defect, cid, dt, quantity):
    cm = run_case(CX.case(cid) if cid in CX.CASE_IDS else CX.route_case(cid), dt, defect)
    assert not all_ok(cm), "the defect `%s` passed every comparison" % defect
    line = first_bad(cm)
    assert cid.split("-")[0] + " " + dt in line and quantity in line, line
