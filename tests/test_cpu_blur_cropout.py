"""CPU: the host side of the any-size blur, GF and Cropout -- taps, limits, surfaces, the bound model of tests/blur_restate.py (which the
GPU tests hold the kernels to) against a float32 imitation of the kernel's summation order and against the mistakes it must catch, and the
fixture tests/golden/blur.npz.  No kernel runs here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import blur_restate as BR
import instnorm_restate as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video_watermarking_forgery_detection_amd")


@pytest.fixture(scope="module")
def blur(golden):
    return golden("blur")


# ----------------------------------------------------------------------------- taps and weights
def test_layer_taps_are_the_restated_taps_rounded_once():
    from video_watermarking_forgery_detection_amd.noise_layers.gaussian_blur import GaussianBlur, gaussian_taps
    from video_watermarking_forgery_detection_amd.noise_layers.gaussian_filter import GF, kornia_taps
    for k in range(5, 16, 2):
        t = np.array(GaussianBlur(k)._taps, np.float64)
        assert np.array_equal(t, BR.gaussian_taps(k).astype(np.float64)) and np.array_equal(t, np.array(gaussian_taps(k)))
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t)              # float32 values
        assert np.array_equal(t, t[::-1]) and abs(t.sum() - 1.0) <= k * BR.EPS and GaussianBlur(k)._w9 is None
    for k, sigma in ((3, 0.5), (7, 2.0), (5, 1.0), (15, 3.0)):
        t = np.array(GF(sigma, k)._taps, np.float64)
        assert np.array_equal(t, BR.kornia_taps(k, sigma).astype(np.float64)) and np.array_equal(t, np.array(kornia_taps(k, sigma)))
        assert abs(t.sum() - 1.0) <= k * BR.EPS and np.argmax(t) == k // 2
    assert GF(2.0).kernel == 7 and GF(2.0).sigma == 2.0
    # the 3 x 3 layer keeps its nine stencil weights (the reference's own float32 expression) and no separable taps
    g3 = GaussianBlur()
    assert g3.kernel_size == 3 and g3._taps is None and len(g3._w9) == 9
    assert g3._w9 == g3.get_gaussian_kernel().flatten().tolist()


def test_golden_weights_against_the_outer_product(blur):
    """the reference's float32 2-D weights vs outer(t, t) of the layer's taps: the 2-D weights deviate from the exact expression by the
    fixture's own wdev, each tap by one rounding (2^-24), so the relative difference stays below wdev + 3 * 2^-24"""
    from video_watermarking_forgery_detection_amd.noise_layers.gaussian_blur import GaussianBlur
    for k in (5, 7):
        layer = GaussianBlur(k)
        w = blur["w2d/%d" % k]
        assert w.dtype == np.float32 and w.shape == (k, k)
        o = BR.outer64(np.array(layer._taps, np.float32))
        rel = float(np.max(np.abs(w.astype(np.float64) - o) / o))
        bound = float(blur["wdev/%d" % k]) + 3 * BR.EPS
        print("k = %d: relative difference %.3e (bound %.3e)" % (k, rel, bound))
        assert rel < bound
        # get_gaussian_kernel keeps returning the reference's 2-D float32 weights, bit for bit
        got = layer.get_gaussian_kernel()
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), w)


# ----------------------------------------------------------------------------- the bound model
SHAPES = lambda k: ((k // 2 + 1, k // 2 + 1), (k, k + 2), (19, 23))     # noqa: E731


def _data(k, H, W):
    rs = np.random.RandomState(100 * k + H + W)
    return rs.standard_normal((2, H, W)).astype(np.float32), rs.standard_normal((2, H, W)).astype(np.float32)


@pytest.mark.parametrize("border", [BR.ZERO, BR.REFLECT])
@pytest.mark.parametrize("k", BR.KS)
def test_imitation_of_the_kernels_order_passes_the_bound_model(k, border):
    t = BR.unsym_taps(k)
    assert np.all(t[:k // 2] != t[::-1][:k // 2])
    for H, W in SHAPES(k):
        x, g = _data(k, H, W)
        BR.Cmp("fwd k=%d border=%d %dx%d" % (k, border, H, W), BR.imitate_fwd(x, t, border), BR.fwd64(x, t, border), BR.bound_fwd(x, t, border)).assert_ok()
        BR.Cmp("bwd k=%d border=%d %dx%d" % (k, border, H, W), BR.imitate_bwd(g, t, border), BR.bwd64(g, t, border), BR.bound_bwd(g, t, border)).assert_ok()
        # the restated transpose is the transpose: <A x, g> = <x, A^T g> in float64
        a = float(np.sum(BR.fwd64(x, t, border) * g.astype(np.float64)))
        b = float(np.sum(x.astype(np.float64) * BR.bwd64(g, t, border)))
        assert abs(a - b) <= 1e-12 * float(np.sum(BR.fwd_abs64(x, t, border) * np.abs(g)))
    # the restated reflect padding is torch's
    if border == BR.REFLECT:
        x = _data(k, k, k + 1)[0]
        want = torch.nn.functional.pad(torch.from_numpy(x).double()[None], (k // 2,) * 4, mode="reflect")[0].numpy()
        assert np.array_equal(BR.pad64(x, k // 2, BR.REFLECT), want)


@pytest.mark.parametrize("k", BR.KS)
def test_named_defects_fail_the_bound_model(k):
    """each mistake the issue names must leave the bound somewhere; the same call without the defect stays inside it"""
    t, tc = BR.unsym_taps(k), BR.unsym_taps(k, seed=1)
    H, W = 19, 23
    x, g = _data(k, H, W)

    def frac(got, ref, bound):
        return BR.Cmp("", got, ref, bound).frac

    ref_bz, b_bz = BR.bwd64(g, t, BR.ZERO), BR.bound_bwd(g, t, BR.ZERO)
    assert frac(BR.imitate_bwd(g, t, BR.ZERO), ref_bz, b_bz) <= 1.0
    assert frac(BR.imitate_bwd(g, t, BR.ZERO, defect="no_reverse"), ref_bz, b_bz) > 1.0            # taps not reversed, zero border
    ref_br, b_br = BR.bwd64(g, t, BR.REFLECT), BR.bound_bwd(g, t, BR.REFLECT)
    assert frac(BR.imitate_bwd(g, t, BR.REFLECT), ref_br, b_br) <= 1.0
    assert frac(BR.imitate_bwd(g, t, BR.REFLECT, defect="no_fold"), ref_br, b_br) > 1.0            # the fold omitted
    for border in (BR.ZERO, BR.REFLECT):
        ref, b = BR.fwd64(x, t, border), BR.bound_fwd(x, t, border)
        assert frac(BR.imitate_fwd(x, t, border), ref, b) <= 1.0
        assert frac(BR.imitate_fwd(x, t, border, defect="halo_shift"), ref, b) > 1.0               # the halo off by one
        # column pass before row pass: visible with distinct row and column taps (an unsymmetric 2-D kernel) ...
        ref2, b2 = BR.fwd64(x, t, border, taps_col=tc), BR.bound_fwd(x, t, border, taps_col=tc)
        assert frac(BR.imitate_fwd(x, t, border, taps_col=tc), ref2, b2) <= 1.0
        assert frac(BR.imitate_fwd(x, t, border, taps_col=tc, defect="swap_passes"), ref2, b2) > 1.0
        # ... and, with the kernel's single tap vector, the same operator: only the rounding differs, inside the bound
        assert frac(BR.imitate_fwd(x, t, border, defect="swap_passes"), ref, b) <= 1.0
    # the fold only matters where the window reaches the halo: an impulse r or more pixels from every border gives the zero-border transpose
    imp = np.zeros((1, H, W), np.float32)
    imp[0, H // 2, W // 2] = 1.0
    assert k // 2 <= H // 2 and H // 2 + k // 2 <= H - 1
    assert np.array_equal(BR.bwd64(imp, t, BR.REFLECT), BR.bwd64(imp, t, BR.ZERO))


def test_imitation_against_the_fixture(blur):
    """what the GPU module tests ask of GaussianBlur(5), GaussianBlur(7) and GF, asked of the host imitation first: the fixture's bounds
    (bound_of(the reference's own float32 deviation, amax)) and the bound model leave room for the kernel's order"""
    x, gw = blur["x"], blur["gw"]
    assert x.shape == (2, 3, 12, 10) and "restatement" in str(blur["gf/source"])
    for k in (5, 7):
        t = BR.gaussian_taps(k)
        for q, got in (("out", BR.imitate_fwd(x, t, BR.ZERO)), ("gx", BR.imitate_bwd(gw, t, BR.ZERO))):
            key = "gb%d/%s" % (k, q)
            NR.check(key, NR.maxdiff(got, blur[key]), NR.bound_of(float(blur["dev32/" + key]), float(blur["amax/" + key])))
    for k in (7, 5):
        t = blur["gf%d/taps" % k]
        assert np.array_equal(t, BR.kornia_taps(k, float(blur["gf%d/sigma" % k])))
        BR.Cmp("gf%d out" % k, BR.imitate_fwd(x, t, BR.REFLECT), blur["gf%d/out" % k], BR.bound_fwd(x, t, BR.REFLECT)).assert_ok()
        BR.Cmp("gf%d gx" % k, BR.imitate_bwd(gw, t, BR.REFLECT), blur["gf%d/gx" % k], BR.bound_bwd(gw, t, BR.REFLECT)).assert_ok()


# ----------------------------------------------------------------------------- limits and surfaces
def test_the_limits_raise():
    from video_watermarking_forgery_detection_amd.noise_layers.gaussian_blur import GaussianBlur
    from video_watermarking_forgery_detection_amd.noise_layers.gaussian_filter import GF
    for k in (1, 2, 4, 6, 16, 17, 21, 0, -3):
        with pytest.raises(NotImplementedError, match=r"odd and in 3\.\.15"):
            GaussianBlur(k)
        with pytest.raises(NotImplementedError, match=r"odd and in 3\.\.15"):
            GF(2.0, k)
    with pytest.raises(ValueError, match="sigma"):
        GF(0.0)
    for k in range(3, 16, 2):
        assert GaussianBlur(k).kernel_size == k and GF(1.5, k).kernel == k
    x = torch.rand(1, 3, 16, 16)
    for call in (lambda: GaussianBlur(5)(x), lambda: GF(2.0)([x, x]), lambda: GF(2.0).apply_attack(x)):
        with pytest.raises(RuntimeError, match="HIP path only"):
            call()


def test_library_refuses_bad_sizes_before_any_launch():
    """the argument checks of the four entry points come before the launch, so they answer without a GPU (the pointers are host arrays that
    nothing dereferences): every refused call returns WM_E_BADARG through the raw handle and raises through the checked one"""
    from video_watermarking_forgery_detection_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    raw, chk = _lib.lib(), _lib.checked()
    buf, out, taps = (ctypes.c_float * 64)(), (ctypes.c_float * 64)(), (ctypes.c_float * 17)()
    for fn in (raw.wm_gauss_sep_fwd, raw.wm_gauss_sep_bwd):
        for k in (1, 2, 4, 16, 17, 0, -1):
            assert fn(buf, out, 1, 8, 8, taps, k, BR.ZERO, None) == -1
        assert fn(buf, out, 1, 8, 8, taps, 5, 2, None) == -1                              # no such border
        assert fn(buf, out, 1, 2, 8, taps, 5, BR.REFLECT, None) == -1                     # r = 2 >= H = 2
        assert fn(buf, out, 1, 8, 3, taps, 7, BR.REFLECT, None) == -1                     # r = 3 >= W = 3
        assert fn(buf, out, 1, 7, 7, taps, 15, BR.REFLECT, None) == -1
        assert fn(None, out, 1, 8, 8, taps, 5, BR.ZERO, None) == -1 and fn(buf, out, 1, 8, 8, None, 5, BR.ZERO, None) == -1
        assert fn(buf, out, 0, 8, 8, taps, 5, BR.ZERO, None) == -1
    assert b"reflected border" in raw.wm_last_error_string() or b"bad arguments" in raw.wm_last_error_string()
    for rect in ((4, 4, 0, 8), (0, 8, 5, 5), (5, 3, 0, 8), (-1, 4, 0, 8), (0, 9, 0, 8), (0, 8, 0, 9), (8, 12, 0, 8), (0, 8, 8, 10)):
        assert raw.wm_cropout_fwd(buf, buf, out, 1, 8, 8, *rect, None) == -1
        assert raw.wm_cropout_bwd(buf, out, None, 1, 8, 8, *rect, None) == -1
    with pytest.raises(RuntimeError, match=r"wm_gauss_sep_fwd failed \(rc=-1\).*odd and in 3\.\.15"):
        chk.wm_gauss_sep_fwd(buf, out, 1, 8, 8, taps, 4, BR.ZERO, None)
    with pytest.raises(RuntimeError, match=r"wm_cropout_fwd failed \(rc=-1\).*empty or not inside"):
        chk.wm_cropout_fwd(buf, buf, out, 1, 8, 8, 4, 4, 0, 8, None)


def test_new_layers_live_in_their_submodules_only():
    import video_watermarking_forgery_detection_amd.noise_layers as nl
    from video_watermarking_forgery_detection_amd.noise_layers import crop, gaussian_filter
    for name in ("GF", "Cropout", "JpegTest"):
        assert not hasattr(nl, name)
    assert not hasattr(crop, "JpegTest") and not hasattr(gaussian_filter, "JpegTest")
    gf, co = gaussian_filter.GF(2.0), crop.Cropout(0.5, 0.25)
    assert isinstance(gf, torch.nn.Module) and gf.name == "GF" and gf.capturable is True and not getattr(gf, "needs_cover", False)
    assert isinstance(co, torch.nn.Module) and co.name == "Cropout" and co.capturable is False and co.needs_cover is True
    assert (co.height_ratio, co.width_ratio) == (0.5, 0.25)
    for layer in (gf, co, nl.GaussianBlur(5)):
        assert callable(layer.fwd) and callable(layer.bwd)
    assert callable(gf.apply_attack) and callable(co.apply_attack)
    assert nl.GaussianBlur.capturable is True and nl.GaussianBlur(7).name == "G_Blur"
    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="HIP path only"):
        co([x, x])
    with pytest.raises(ValueError, match="cover"):
        co.fwd(x)
    for call in (lambda: co.apply_attack(x), lambda: co([x, None])):      # a missing cover is named, on any device
        with pytest.raises(ValueError, match="cover"):
            call()
    # Hybrid takes the new children as they are
    h = nl.Hybrid([nl.GaussianBlur(5), gf, co])
    assert h.needs_cover is True and len(h.layers) == 3


def test_cropout_rectangle_is_crops_under_a_seeded_numpy_rng():
    from video_watermarking_forgery_detection_amd.noise_layers.crop import Crop, Cropout
    for shape, hr, wr in (((2, 3, 16, 20), 0.5, 0.5), ((1, 3, 33, 7), 0.3, 0.9), ((1, 1, 8, 8), 1.0, 0.5), ((1, 1, 8, 8), 1.0, 1.0)):
        np.random.seed(123)
        a = [Cropout(hr, wr).get_random_rectangle_inside(shape, hr, wr) for _ in range(5)]
        after_a = np.random.rand()
        np.random.seed(123)
        b = [Crop().get_random_rectangle_inside(shape, hr, wr) for _ in range(5)]
        assert a == b and after_a == np.random.rand()                      # the same rectangles and the same number of draws
        for h0, h1, w0, w1 in a:
            assert 0 <= h0 < h1 <= shape[2] and 0 <= w0 < w1 <= shape[3] and h1 - h0 == int(hr * shape[2]) and w1 - w0 == int(wr * shape[3])
    # the layer draws through that method, once per call, and refuses ratios that leave nothing
    co = Cropout(0.5, 0.5)
    np.random.seed(5)
    want = Crop().get_random_rectangle_inside((1, 3, 16, 20), 0.5, 0.5)
    np.random.seed(5)
    assert co._rect(torch.empty(1, 3, 16, 20)) == want and co.last_rect == want
    with pytest.raises(ValueError, match="empty rectangle"):
        Cropout(0.01, 0.5)._rect(torch.empty(1, 3, 16, 20))


def test_attack_table_option_file_and_cycle_keys():
    """options/train/train_hidden_c3_blur.yml is train_hidden_c3.yml with the new layers in the cycle; a layer that says capturable = False
    (Cropout: a host-drawn rectangle per call) makes the cycle answer None -- that step runs eagerly -- and every other layer keeps its key"""
    from video_watermarking_forgery_detection_amd.models.IRNrhi_model import _AttackCycle
    from video_watermarking_forgery_detection_amd.noise_layers import Crop, GaussianBlur, Resize
    from video_watermarking_forgery_detection_amd.noise_layers.crop import Cropout
    from video_watermarking_forgery_detection_amd.noise_layers.gaussian_filter import GF
    from video_watermarking_forgery_detection_amd.options import options
    opt = options.parse(os.path.join(PKG, "options", "train", "train_hidden_c3_blur.yml"), is_train=True)
    base = options.parse(os.path.join(PKG, "options", "train", "train_hidden_c3.yml"), is_train=True)
    assert opt["train"]["attacks"] == ["Jpeg50", "GaussianBlur5", "GaussianBlur7", "GF7", "Cropout", "Resize", "Crop"]
    assert {k: v for k, v in opt["train"].items() if k != "attacks"} == {k: v for k, v in base["train"].items() if k != "attacks"}
    assert opt["datasets"] == base["datasets"]
    cyc = _AttackCycle([GaussianBlur(5), GF(2.0), Cropout(0.5, 0.5), Resize(), Crop()])
    keys = []
    for k in range(5):
        cyc.k = k
        keys.append(cyc.capture_key())
    assert keys[2] is None and cyc.name == "Crop"
    assert [k[1:] for k in keys if k is not None] == [(0, "GaussianBlur"), (1, "GF"), (3, "Resize"), (4, "Crop")]


def test_tile_constants_of_ops_are_the_kernels():
    from video_watermarking_forgery_detection_amd import ops
    src = open(os.path.join(PKG, "csrc", "gauss_sep.hip")).read()
    m = re.search(r"constexpr int TH = (\d+), TW = (\d+)", src)
    assert m and (int(m.group(1)), int(m.group(2))) == ops.GAUSS_SEP_TILE
    hdr = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    assert "#define WM_GAUSS_SEP_MAX_K %d" % ops.GAUSS_SEP_MAX_K in hdr and ops.GAUSS_SEP_MAX_K == BR.MAX_K
    assert "#define WM_BORDER_ZERO %d" % ops.BORDER_ZERO in hdr and "#define WM_BORDER_REFLECT %d" % ops.BORDER_REFLECT in hdr
    assert (ops.BORDER_ZERO, ops.BORDER_REFLECT) == (BR.ZERO, BR.REFLECT)
