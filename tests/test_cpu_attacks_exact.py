"""The tap-by-tap comparisons of tests/attacks_exact.py without a GPU: the dense float64 restatements ARE F.interpolate / F.conv2d in
float64 on every case the GPU tests use, every table row selects the kernel path it is there for, a float32 imitation of each operation
passes the comparison functions the GPU tests call -- and each planted defect of the kinds a kernel can have FAILS them, so a green
tests/test_gpu_attacks_exact.py means something."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attacks_exact as AX
import detgen
from oracle import attacks_ref

CASES = [(n, k) for n in AX.RESAMPLE_NAMES for k in AX.KINDS]
case_ids = ["%s-%s" % (n.replace(" ", "_"), AX.MODE[k]) for n, k in CASES]


# ---------------------------------------------------------------------------------------------------- the restatement is the operation
@pytest.mark.parametrize("name,kind", CASES, ids=case_ids)
def test_dense_restatement_is_interpolate_in_float64(name, kind):
    c = AX.resample_case(name, kind)
    h0, hs, w0, ws = c.rect
    for x in (c.x, c.x_sat):
        xd = x[:, :, h0:h0 + hs, w0:w0 + ws].double().requires_grad_(True)
        y = F.interpolate(xd, size=c.out, mode=AX.MODE[kind], align_corners=False)
        assert float((y.detach() - AX.resample_ref(x, c.rect, c.out, kind)).abs().max()) <= 1e-12
        assert float((y.detach().clamp(0, 1) - AX.resample_ref(x, c.rect, c.out, kind, clamp01=True)).abs().max()) <= 1e-12
    for yc in (None, AX.synthetic_mask_plane(c.gy.shape), c.fwd_expect(True, True)[0].float()):
        g = c.gy.double() if yc is None else c.gy.double() * AX.clamp_mask(yc)
        (gi,) = torch.autograd.grad(y, xd, g, retain_graph=True)
        ref = AX.resample_bwd_ref(c.gy, yc, c.shape[2:], c.rect, c.out, kind)
        assert float((ref[:, :, h0:h0 + hs, w0:w0 + ws] - gi).abs().max()) <= 1e-12
        assert float(ref[:, :, c.outside].abs().max()) == 0 if bool(c.outside.any()) else True


def test_every_row_selects_the_path_it_is_there_for():
    for name, shape, rect, out, want in AX.RESAMPLE_ROWS:
        got = AX.sep_path(shape, rect, out)
        assert {k: got[k] for k in want} == want, (name, got)


def test_the_synthetic_mask_shows_every_value_to_every_row_and_column():
    for name, kind in CASES[::2]:
        m = AX.synthetic_mask_plane(AX.resample_case(name, kind).gy.shape)
        OH, OW = m.shape[2:]
        if OW >= 6:
            assert all(r.view(torch.int32).unique().numel() == 6 for r in m[0, 0])
        if OH >= 6:
            assert all(m[0, 0, :, j].view(torch.int32).unique().numel() == 6 for j in range(OW))
        if OH * OW >= 36:
            assert float(AX.clamp_mask(m).float().mean()) == pytest.approx(0.5, abs=0.15)
    m = AX.synthetic_mask_plane((1, 1, 1, 6))[0, 0, 0]
    assert AX.clamp_mask(m).tolist() == [False, False, False, True, True, True] and bool(torch.signbit(m[1])) and float(m[4]) == 2.0 ** -126


def test_stencil_restatement_is_conv2d_in_float64():
    w9 = AX.asymmetric_w9()
    for shape in AX.STENCIL_SHAPES:
        x = detgen.normal(shape, 31).double().requires_grad_(True)
        gy = detgen.normal(shape, 32)
        C = shape[1]
        w = torch.tensor(w9, dtype=torch.float64).view(1, 1, 3, 3).repeat(C, 1, 1, 1)
        y = F.conv2d(x, w, padding=1, groups=C)
        (gx,) = torch.autograd.grad(y, x, gy.double())
        assert float((y.detach() - AX.stencil3_ref(x.detach(), w9)).abs().max()) <= 1e-12
        assert float((gx - AX.stencil3_bwd_ref(gy, w9)).abs().max()) <= 1e-12
        assert float((AX.stencil3_bwd_ref(gy, w9) - AX.stencil3_ref(gy, w9[::-1])).abs().max()) <= 1e-12   # what GaussianBlur's backward launches


def test_quantiser_restatements_are_the_oracle():
    x = AX.quant_inputs()
    assert x.dtype == np.float32 and np.isfinite(x).all() and x.size == 3 * (512 + 13)
    t = torch.from_numpy(x)
    AX.assert_same_bits(attacks_ref.quantization(t), AX.quant_ref(x), x, "quant_ref")
    ref = AX.clamp_quant_ref(x)
    assert np.array_equal(attacks_ref.quantization(torch.clamp(t, 0, 1)).numpy(), ref)          # (-0 == +0 here: see clamp_quant_ref)
    assert ref.min() == 0 and ref.max() == 1 and not np.signbit(ref).any()
    assert np.unique(ref).size == 256


# ---------------------------------------------------------------------------------------------------- float32 imitations, with defects
def imitate_resample_fwd(c, saturated, clamp01, defect=None):
    """float32 stand-in for wm_resample_fwd: dense weights over the whole image axis (so that a tap may leave the rectangle)"""
    H, W = c.shape[2:]
    h0, hs, w0, ws = c.rect
    bad = defect == "image clamp"
    Rh = AX.axis_matrix_in_image(c.out[0], hs, c.kind, h0, H, clamp_to_image=bad)
    Rw = AX.axis_matrix_in_image(c.out[1], ws, c.kind, w0, W, clamp_to_image=bad)
    y = Rh @ (c.x_sat if saturated else c.x).double() @ Rw.T
    return (y.clamp(0, 1) if clamp01 else y).float()


def _drop_beyond(R, n, out, keep):
    """the candidates of input i beyond the keep-th are never visited"""
    R = R.clone()
    for i in range(n):
        lo, _ = AX.axis_range(i, n, out)
        R[lo + keep:, i] = 0
    return R


def imitate_resample_bwd(c, yc, defect=None):
    H, W = c.shape[2:]
    h0, hs, w0, ws = c.rect
    OH, OW = c.out
    G = c.gy.double()
    if yc is not None:
        G = G * (((yc >= 0) & (yc <= 1)) if defect == "closed mask" else AX.clamp_mask(yc))
    if defect == "image clamp":
        return (AX.axis_matrix_in_image(OH, hs, c.kind, h0, H, True).T @ G @ AX.axis_matrix_in_image(OW, ws, c.kind, w0, W, True)).float()
    Rh, Rw = AX.axis_matrix(OH, hs, c.kind), AX.axis_matrix(OW, ws, c.kind)
    if defect == "24 columns":
        Rw = _drop_beyond(Rw, ws, OW, 24)
    if defect == "12 rows":
        Rh = _drop_beyond(Rh, hs, OH, 12)
    gx = torch.zeros(c.shape, dtype=torch.float64)
    gx[:, :, h0:h0 + hs, w0:w0 + ws] = Rh.T @ G @ Rw
    return gx.float()


def _own_forward(c):
    return imitate_resample_fwd(c, True, True)


@pytest.mark.parametrize("name,kind", CASES, ids=case_ids)
def test_float32_imitation_passes_resample(name, kind):
    c = AX.resample_case(name, kind)
    print()
    for sat in (False, True):
        for clamp in (False, True):
            print("  ", c.check_fwd(imitate_resample_fwd(c, sat, clamp), sat, clamp).line())
    for which in AX.MASKS:
        yc = c.mask_plane(which, _own_forward(c))
        print("  ", c.check_bwd(imitate_resample_bwd(c, yc), yc, which).line())
    if not name.startswith("one"):                      # (a single row, column or output cannot overshoot)
        sat = c.fwd_expect(True, False)[0]
        assert kind == AX.BILINEAR or float(sat.min()) < 0 or float(sat.max()) > 1, "the saturated input does not make the clamp act"


def _fails(fn):
    with pytest.raises(AssertionError):
        fn()


@pytest.mark.parametrize("kind", AX.KINDS, ids=lambda k: AX.MODE[k])
def test_defect_taps_clamped_to_the_image_not_the_rectangle(kind):
    for name in ("crop 0.3 back to full", "very wide", "seam", "one row/col"):
        c = AX.resample_case(name, kind)
        _fails(lambda: c.check_fwd(imitate_resample_fwd(c, False, False, "image clamp"), False, False))
        _fails(lambda: c.check_bwd(imitate_resample_bwd(c, None, "image clamp"), None))


@pytest.mark.parametrize("kind", AX.KINDS, ids=lambda k: AX.MODE[k])
def test_defect_candidates_beyond_the_24th_column_dropped(kind):
    for name in ("very wide", "long rows c"):
        c = AX.resample_case(name, kind)
        _fails(lambda: c.check_bwd(imitate_resample_bwd(c, None, "24 columns"), None))
    c = AX.resample_case("long rows a", kind)                      # at most 24 candidates: nothing dropped, nothing to see
    c.check_bwd(imitate_resample_bwd(c, None, "24 columns"), None)


@pytest.mark.parametrize("kind", AX.KINDS, ids=lambda k: AX.MODE[k])
def test_defect_candidates_beyond_the_12th_row_dropped(kind):
    """bilinear weights vanish beyond one source pixel, so up to 3.3x (Crop's range) the rows beyond the 12th candidate all have weight
    zero: the overflow loop runs there and adds nothing, and only the 7.4x row can see it; bicubic sees it at 3.3x"""
    for name in ("crop 0.3 back to full", "very wide")[kind == AX.BILINEAR:]:
        c = AX.resample_case(name, kind)
        _fails(lambda: c.check_bwd(imitate_resample_bwd(c, None, "12 rows"), None))
    c = AX.resample_case("resize 1.3", kind)
    c.check_bwd(imitate_resample_bwd(c, None, "12 rows"), None)


@pytest.mark.parametrize("kind", AX.KINDS, ids=lambda k: AX.MODE[k])
def test_defect_clamp_mask_closed_interval(kind):
    for name in ("resize 0.7", "seam", "one pixel to 3x4"):
        c = AX.resample_case(name, kind)
        yc = c.mask_plane("synthetic")
        _fails(lambda: c.check_bwd(imitate_resample_bwd(c, yc, "closed mask"), yc))
    c = AX.resample_case("resize 1.3", AX.BICUBIC)                 # the kernel's own forward of the saturated input holds exact 0s and 1s
    yc = c.mask_plane("own forward", _own_forward(c))
    assert int((yc == 0).sum()) > 0 and int((yc == 1).sum()) > 0
    _fails(lambda: c.check_bwd(imitate_resample_bwd(c, yc, "closed mask"), yc))


def test_crop_layer_case_passes_with_the_imitation():
    c = AX.crop_layer_case()
    assert AX.sep_path(c.shape, c.rect, c.out)["y_overflow"]
    c.check_fwd(imitate_resample_fwd(c, False, False), False, False)
    c.check_bwd(imitate_resample_bwd(c, None), None)


@pytest.mark.parametrize("ratio", sorted(AX.RESIZE_SEEDS))
def test_resize_layer_case_has_an_unambiguous_mask(ratio):
    """no unclamped float64 output within the tolerance of 0 or 1 (else: another seed in attacks_exact.RESIZE_SEEDS), and the clamp acts"""
    c = AX.resize_layer_case(ratio)
    print("\n   %s: margin %.3e, needed %.3e (tolerance y %.3e, gx %.3e)" % (c.label, c.margin, c.margin_needed, c.tol_y, c.tol_g))
    assert c.margin > c.margin_needed
    assert int((c.y64 == 0).sum()) > 0 and int((c.y64 == 1).sum()) > 0
    c.check(c.y64.float(), c.gx64.float())
    with pytest.raises(AssertionError):                 # the closed mask again, through both stages
        H, W = c.shape[2:]
        nh, nw = c.mid
        A = [AX.axis_matrix(*a, AX.BICUBIC) for a in ((nh, H), (nw, W), (H, nh), (W, nw))]
        c.check(c.y64.float(), (A[0].T @ (A[2].T @ c.gy.double() @ A[3]) @ A[1]).float())


# ---------------------------------------------------------------------------------------------------- stencil
def test_defect_stencil_taps_transposed():
    w9 = AX.asymmetric_w9()
    wt = torch.tensor(w9).view(3, 3).t().flatten().tolist()
    gauss = attacks_ref.gaussian_kernel().flatten().tolist()
    for shape in AX.STENCIL_SHAPES:
        x = detgen.uniform(shape, 33)
        AX.check_stencil(x, w9, AX.stencil3_ref(x, w9).float())
        AX.check_stencil_bwd(x, w9, AX.stencil3_bwd_ref(x, w9).float())
        if shape[2] > 1 and shape[3] > 1:
            _fails(lambda: AX.check_stencil(x, w9, AX.stencil3_ref(x, wt).float()))
            _fails(lambda: AX.check_stencil(x, w9, AX.stencil3_ref(x, w9[::-1]).float()))             # flipped
            _fails(lambda: AX.check_stencil_bwd(x, w9, AX.stencil3_ref(x, w9).float()))               # "same stencil" as the backward
            AX.check_stencil(x, gauss, AX.stencil3_ref(x, torch.tensor(gauss).view(3, 3).t().flatten().tolist()).float())  # the Gaussian cannot see it


# ---------------------------------------------------------------------------------------------------- median
def imitate_median(x, k):
    """the oracle's value and the stable-rank tap: among the taps equal to the median, the (k*k // 2 - #{taps < y})-th in tap order"""
    y = attacks_ref.median_blur(x, k)
    taps = AX.median_taps(x, k)
    eq = taps == y.unsqueeze(2)
    want = k * k // 2 - (taps < y.unsqueeze(2)).sum(2)
    idx = (eq & (eq.cumsum(2) - 1 == want.unsqueeze(2))).float().argmax(2)
    return y, idx.to(torch.int8)


def imitate_median_bwd(gy, idx, k, defect=False):
    B, C, H, W = gy.shape
    p = k // 2
    gx = torch.zeros(B, C, H, W, dtype=torch.float64)
    hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for t in range(k * k):
        th, tw = hh + t // k - p, ww + t % k - p
        inside = (th >= 0) & (th < H) & (tw >= 0) & (tw < W)
        if defect:                                    # a padded tap's gradient goes to the nearest pixel of the image
            th, tw, inside = th.clamp(0, H - 1), tw.clamp(0, W - 1), torch.ones_like(inside)
        sel = (idx == t) & inside
        for b in range(B):
            for ch in range(C):
                s = sel[b, ch]
                gx[b, ch].index_put_((th[s], tw[s]), gy[b, ch][s].double(), accumulate=True)
    return gx.float()


@pytest.mark.parametrize("k", [3, 5])
def test_median_checks_accept_the_imitation_and_free_ties_and_reject_defects(k):
    rejected_bwd = 0
    for shape in AX.MEDIAN_SHAPES[:-1] + ((1, 1, 12, 40),):
        for data in AX.MEDIAN_DATA:
            x = AX.median_input(shape, data) if shape in AX.MEDIAN_SHAPES else {"continuous": detgen.uniform(shape, 9), "constant": torch.full(shape, 0.25)}.get(data)
            if x is None:
                continue
            gy = detgen.normal(shape, 34)
            y, idx = imitate_median(x, k)
            AX.median_routing_check(x, y, idx, k)
            AX.check_median_bwd(gy, idx, k, imitate_median_bwd(gy, idx, k))
            AX.check_median_bwd(gy, idx, k, AX.median_bwd_ref(gy, idx, k).float())
            taps = AX.median_taps(x, k)
            # a padded tap holds the median at some border pixel (zero padding): its gradient must vanish, not move inwards
            padded = AX.median_taps(torch.ones_like(x), k).gather(2, idx.long().unsqueeze(2)).squeeze(2) == 0
            if bool(padded.any()):
                _fails(lambda: AX.check_median_bwd(gy, idx, k, imitate_median_bwd(gy, idx, k, defect=True)))
                rejected_bwd += 1
            # free ties: another tap of the same value is as good
            other = (taps == y.unsqueeze(2)) & (torch.arange(k * k).view(1, 1, -1, 1, 1) != idx.long().unsqueeze(2))
            if bool(other.any()):
                alt = torch.where(other.any(2), other.float().argmax(2), idx.long()).to(torch.int8)
                assert not torch.equal(alt, idx)
                AX.median_routing_check(x, y, alt, k)
                AX.check_median_bwd(gy, alt, k, imitate_median_bwd(gy, alt, k))
            else:
                assert data == "continuous" and min(shape[2:]) > k
            # defects of the forward: a neighbouring tap, a value that is not the median, an index out of range
            if min(shape[2:]) > k and data == "continuous":
                _fails(lambda: AX.median_routing_check(x, y, ((idx.long() + 1) % (k * k)).to(torch.int8), k))
                _fails(lambda: AX.median_routing_check(x, taps.max(2)[0], taps.argmax(2).to(torch.int8), k))
            _fails(lambda: AX.median_routing_check(x, y, torch.full_like(idx, k * k), k))
    assert rejected_bwd >= 10


# ---------------------------------------------------------------------------------------------------- quantisers
def test_defect_round_half_away_from_zero():
    x = AX.quant_inputs()
    v = x * np.float32(255)
    away = (np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))).astype(np.float32) / np.float32(255)
    exact_ties = int((np.abs(v - np.trunc(v)) == 0.5).sum())
    assert exact_ties >= 100, exact_ties                  # the half-way points that survive x * 255 in float32
    _fails(lambda: AX.assert_same_bits(away, AX.quant_ref(x), x, "half away"))
    c = np.clip(x, 0, 1)
    _fails(lambda: AX.assert_same_bits((np.floor(c * np.float32(255) + np.float32(0.5)) / np.float32(255)).astype(np.float32), AX.clamp_quant_ref(x), x, "half up"))
    _fails(lambda: AX.assert_same_bits(AX.quant_ref(x), AX.clamp_quant_ref(x), x, "no clamp"))
    _fails(lambda: AX.assert_same_bits((np.rint(x * np.float32(255)) * np.float32(1 / 255)).astype(np.float32), AX.quant_ref(x), x, "multiply by the reciprocal"))
    AX.assert_same_bits(AX.quant_ref(x).copy(), AX.quant_ref(x), x, "itself")
