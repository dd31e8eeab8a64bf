"""GPU: the stencil, median, resample and rounding kernels (csrc/attacks.hip, wm_clamp_quant_fwd of csrc/localise.hip) tap by tap against
float64 (tests/attacks_exact.py), at shapes chosen for the kernels' paths: every MAXC of the separable backward's x pass, its LDS and
global-memory forms and their `wide` loops, the y pass's overflow loop, column-block seams, the launch-grid caps, degenerate axes.

Resample tolerances are 4 x the deviation of torch's float32 CPU interpolation from float64 on the same case, measured on the CPU at
test time and printed with the kernels' own deviation (run with -s); stencil and median-backward bounds follow from the number format;
median values, tap indices and the quantisers are exact.  tests/test_cpu_attacks_exact.py shows that these comparisons fail on the
defects they are there to catch."""
import numpy as np
import pytest
import torch

import attacks_exact as AX
from oracle import attacks_ref

pytestmark = pytest.mark.gpu

CASES = [(n, k) for n in AX.RESAMPLE_NAMES for k in AX.KINDS]


# ----------------------------------------------------------------------------------------------------------------- resample
@pytest.mark.parametrize("name,kind", CASES, ids=["%s-%s" % (n.replace(" ", "_"), AX.MODE[k]) for n, k in CASES])
def test_resample_kernels(name, kind):
    from video_watermarking_forgery_detection_amd import ops
    assert (ops.BILINEAR, ops.BICUBIC) == (AX.BILINEAR, AX.BICUBIC)
    c = AX.resample_case(name, kind)
    gy = c.gy.cuda()
    print()
    own = None
    for sat in (False, True):
        x = (c.x_sat if sat else c.x).cuda()
        for clamp in (False, True):
            y = ops.resample_fwd(x, c.rect, c.out, kind, clamp01=clamp)
            print("  ", c.check_fwd(y, sat, clamp).line())
            if sat and clamp:
                own = y
    for which in AX.MASKS:
        yc = c.mask_plane(which, own)
        for separable in (True, False):
            gx = ops.resample_bwd(gy, None if yc is None else yc.cuda(), c.shape[2:], c.rect, kind, separable=separable)
            print("  ", c.check_bwd(gx, yc, "%s, %s" % (which, "separable" if separable else "gather")).line())


def test_crop_layer():
    """Crop()(x, apex) on 32 x 32 with a 10 x 10 rectangle, through autograd: 3.2x, the separable backward's overflow loop"""
    from video_watermarking_forgery_detection_amd.noise_layers import Crop
    c = AX.crop_layer_case()
    h0, hs, w0, ws = c.rect
    x = c.x.cuda().requires_grad_(True)
    y, apex = Crop()(x, apex=(h0, h0 + hs, w0, w0 + ws))
    assert tuple(apex) == (h0, h0 + hs, w0, w0 + ws)
    (y * c.gy.cuda()).sum().backward()
    print()
    print("  ", c.check_fwd(y.detach(), False, False).line())
    print("  ", c.check_bwd(x.grad, None, "autograd").line())


@pytest.mark.parametrize("ratio", sorted(AX.RESIZE_SEEDS))
def test_resize_layer(ratio):
    """Resize()(x, resize_ratio) on a saturated image, through autograd: both stages, the clamp and its mask"""
    from video_watermarking_forgery_detection_amd.noise_layers import Resize
    c = AX.resize_layer_case(ratio)
    assert c.margin > c.margin_needed          # the mask is unambiguous (tests/test_cpu_attacks_exact.py)
    x = c.x.cuda().requires_grad_(True)
    y = Resize()(x, resize_ratio=ratio)
    (y * c.gy.cuda()).sum().backward()
    print()
    for rep in c.check(y.detach(), x.grad):
        print("  ", rep.line())


# ----------------------------------------------------------------------------------------------------------------- stencil
@pytest.mark.parametrize("taps", ["asymmetric", "gaussian"])
def test_stencil_kernel(taps):
    from video_watermarking_forgery_detection_amd import ops
    from video_watermarking_forgery_detection_amd.noise_layers import GaussianBlur
    import detgen
    w9 = AX.asymmetric_w9() if taps == "asymmetric" else GaussianBlur()._w9
    print()
    for i, shape in enumerate(AX.STENCIL_SHAPES):
        x = detgen.uniform(shape, 4610 + i, lo=-1.0)
        print("  ", AX.check_stencil(x, w9, ops.stencil3(x.cuda(), w9), "stencil %s %s" % (taps, shape)))


def test_gaussian_blur_backward_is_the_transpose():
    from video_watermarking_forgery_detection_amd.noise_layers import GaussianBlur
    import detgen
    layer = GaussianBlur()
    x = detgen.uniform(AX.STENCIL_BWD_SHAPE, 4620).cuda().requires_grad_(True)
    gy = detgen.normal(AX.STENCIL_BWD_SHAPE, 4621)
    y = layer(x)
    y.backward(gy.cuda())
    print()
    print("  ", AX.check_stencil(x.detach().cpu(), layer._w9, y.detach(), "GaussianBlur fwd"))
    print("  ", AX.check_stencil_bwd(gy, layer._w9, x.grad, "GaussianBlur bwd"))


# ----------------------------------------------------------------------------------------------------------------- median
def _shifted(t):
    """the same values 4 bytes off a 16-byte boundary: the one-pixel kernels"""
    buf = torch.empty(t.numel() + 1, device="cuda", dtype=t.dtype)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


@pytest.mark.parametrize("shape", AX.MEDIAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("k", [3, 5])
def test_median_kernels(k, shape):
    from video_watermarking_forgery_detection_amd import ops
    gy = AX.median_gy(shape)
    print()
    for data in AX.MEDIAN_DATA:
        xc = AX.median_input(shape, data)
        yref = attacks_ref.median_blur(xc, k)
        for shifted in (False, True) if shape in AX.MEDIAN_SHIFTED else (False,):
            x, g = xc.cuda(), gy.cuda()
            assert x.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
            if shifted:
                x, g = _shifted(x), _shifted(g)
            y, idx = ops.median_fwd(x, k)
            what = "median k=%d %s %s%s" % (k, shape, data, " shifted" if shifted else "")
            assert torch.equal(y.cpu().view(torch.int32), yref.view(torch.int32)), what
            AX.median_routing_check(xc, y, idx, k)
            gx = ops.median_bwd(g, idx, k)
            print("  ", AX.check_median_bwd(gy, idx, k, gx, what))
            y_only, none = ops.median_fwd(x, k, want_idx=False)
            assert none is None and torch.equal(y_only, y), what


# ----------------------------------------------------------------------------------------------------------------- quantisers
def test_quantisers_at_every_level_and_half_way_point():
    from video_watermarking_forgery_detection_amd import ops
    x = AX.quant_inputs()
    xg = torch.from_numpy(x).cuda()
    AX.assert_same_bits(ops.quant(xg), AX.quant_ref(x), x, "ops.quant")
    AX.assert_same_bits(ops.clamp_quant(xg), AX.clamp_quant_ref(x), x, "ops.clamp_quant")
    inside = x[(x >= 0) & (x <= 1) & ~np.signbit(x)]
    AX.assert_same_bits(ops.clamp_quant(torch.from_numpy(inside).cuda()), AX.quant_ref(inside), inside, "ops.clamp_quant inside [0, 1]")
