"""GPU: the separable blur (csrc/gauss_sep.hip: wm_gauss_sep_fwd / wm_gauss_sep_bwd) and Cropout (wm_cropout_fwd / wm_cropout_bwd), through
ops, the layers GaussianBlur(k) / GF / Cropout, Hybrid and the trainer.

The blur is held per element to the float64 restatement of tests/blur_restate.py within its bound model (derived there from the kernel's
summation order, nothing measured); Cropout, the float4-vs-scalar paths, repeated runs and GaussianBlur(3) are compared bit for bit; the
layers GaussianBlur(5) / (7) to the reference's own output in tests/golden/blur.npz within bound_of(the reference's own float32 deviation,
amax), as tests/test_gpu_swin.py does; GF to its restated fixture within the bound model."""
import functools
import os

import numpy as np
import pytest
import torch

import blur_restate as BR
import detgen
import instnorm_restate as NR

pytestmark = pytest.mark.gpu

N = 3
BORDERS = (BR.ZERO, BR.REFLECT)


def _ops():
    from video_watermarking_forgery_detection_amd import ops
    return ops


def _sizes(k, tile):
    r = k // 2
    return sorted({r + 1, k, tile - 1, tile, tile + 1, 2 * tile + 3})


@functools.lru_cache(maxsize=None)
def _planes(H, W, seed):
    """x and g [1, N, H, W] ~ N(0, 1) on the host, made once per shape and shared"""
    rs = np.random.RandomState(seed + 1000 * H + W)
    return rs.standard_normal((1, N, H, W)).astype(np.float32), rs.standard_normal((1, N, H, W)).astype(np.float32)


def _offset_view(t):
    """the same values in a contiguous cuda tensor whose storage starts 4 bytes past a 16-byte boundary (the kernels' element-by-element path)"""
    buf = torch.empty(t.numel() + 1, device="cuda", dtype=torch.float32)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _both(x, g, taps, border):
    ops = _ops()
    tl = [float(v) for v in taps]
    y = ops.gauss_sep(torch.from_numpy(x).cuda(), tl, border)
    gx = ops.gauss_sep_bwd(torch.from_numpy(g).cuda(), tl, border)
    return y.cpu().numpy(), gx.cpu().numpy()


def _check(label, x, g, taps, border):
    y, gx = _both(x, g, taps, border)
    a = BR.Cmp(label + " fwd", y, BR.fwd64(x, taps, border), BR.bound_fwd(x, taps, border))
    b = BR.Cmp(label + " bwd", gx, BR.bwd64(g, taps, border), BR.bound_bwd(g, taps, border))
    return a, b, y, gx


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("k", BR.KS)
def test_every_plane_edge_per_element(k, border):
    """H x W over {r+1, k, tile-1, tile, tile+1, 2 tile+3} of the kernel's tile, random planes and unsymmetric taps, forward and transpose; and
    the adjoint identity <A x, g> = <x, A^T g> of the two GPU results in float64, to the sum of the two bound models"""
    TH, TW = _ops().GAUSS_SEP_TILE
    taps = BR.unsym_taps(k)
    worst = []
    for H in _sizes(k, TH):
        for W in _sizes(k, TW):
            x, g = _planes(H, W, 11)
            a, b, y, gx = _check("k=%d border=%d %dx%d" % (k, border, H, W), x, g, taps, border)
            worst += [a, b]
            lhs = float(np.sum(y.astype(np.float64) * g))
            rhs = float(np.sum(x.astype(np.float64) * gx))
            room = float(np.sum(BR.bound_fwd(x, taps, border) * np.abs(g)) + np.sum(BR.bound_bwd(g, taps, border) * np.abs(x)))
            assert abs(lhs - rhs) <= room, (k, border, H, W, lhs, rhs, room)
    for c in sorted(worst, key=lambda c: -c.frac)[:4]:
        c.assert_ok()
    assert all(c.ok for c in worst), [(c.label, c.frac) for c in worst if not c.ok]


@pytest.mark.parametrize("k", BR.KS)
def test_widths_1_to_8_across_the_float4_split(k):
    """W = 1..8 (4 and 8 take the float4 path, the others the scalar one; both from an aligned and from an offset base); the reflected border
    where torch's limit r < W allows it"""
    taps, r = BR.unsym_taps(k), k // 2
    ops = _ops()
    for W in range(1, 9):
        for H in (r + 1, 9):
            x, g = _planes(H, W, 23)
            for border in BORDERS:
                if border == BR.REFLECT and (r >= W or r >= H):
                    continue
                a, b, y, gx = _check("k=%d border=%d %dx%d" % (k, border, H, W), x, g, taps, border)
                assert a.ok and b.ok, (a.label, a.frac, b.frac)
                tl = [float(v) for v in taps]
                xo, go = _offset_view(torch.from_numpy(x)), _offset_view(torch.from_numpy(g))
                yo = ops.gauss_sep(xo, tl, border, out=_offset_view(torch.zeros(x.shape)))
                gxo = ops.gauss_sep_bwd(go, tl, border, out=_offset_view(torch.zeros(x.shape)))
                assert np.array_equal(yo.cpu().numpy().view(np.int32), y.view(np.int32)), (k, border, H, W)
                assert np.array_equal(gxo.cpu().numpy().view(np.int32), gx.view(np.int32)), (k, border, H, W)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("k", BR.KS)
def test_impulses_at_corners_and_tile_seams(k, border):
    """one impulse per plane set: the four corners, both sides of the tile seams in each direction and the seam crossing; the forward spreads
    the reversed taps around it and the transpose the taps, folded at a reflected border -- every element against the restatement"""
    TH, TW = _ops().GAUSS_SEP_TILE
    H, W = 2 * TH + 3, 2 * TW + 3
    taps = BR.unsym_taps(k)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (TH - 1, TW - 1), (TH, TW), (TH - 1, TW), (TH, TW - 1), (2 * TH, 2 * TW),
             (2 * TH - 1, 5), (7, 2 * TW - 1), (1, 1), (H - 2, W - 2)]
    for lo in range(0, len(spots), N):
        x = np.zeros((1, N, H, W), np.float32)
        for n, (h, w) in enumerate(spots[lo:lo + N]):
            x[0, n, h, w] = 1.0 + n
        a, b, _, _ = _check("impulses %s k=%d border=%d" % (spots[lo:lo + N], k, border), x, x, taps, border)
        assert a.ok and b.ok, (a.label, a.frac, b.frac)


@pytest.mark.parametrize("border", BORDERS)
def test_float4_and_scalar_paths_agree_and_runs_repeat_bit_for_bit(border):
    """W % 4 == 0 from an aligned base takes float4 loads and stores; the same values one element past the boundary take the scalar ones"""
    ops = _ops()
    for k in (5, 15):
        taps = [float(v) for v in BR.unsym_taps(k)]
        for H, W in ((35, 72), (67, 132), (9, 8)):
            x, g = (torch.from_numpy(a).cuda() for a in _planes(H, W, 31))
            assert x.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
            for fn, t in ((ops.gauss_sep, x), (ops.gauss_sep_bwd, g)):
                y1 = fn(t, taps, border)
                assert y1.data_ptr() % 16 == 0
                y2 = fn(t, taps, border)
                assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))                      # two runs, the same bits
                ys = fn(_offset_view(t), taps, border, out=_offset_view(torch.zeros_like(t)))
                assert torch.equal(y1.view(torch.int32), ys.view(torch.int32)), (k, H, W, fn.__name__)
                ym = fn(_offset_view(t), taps, border)                                               # scalar loads, float4 stores
                assert torch.equal(y1.view(torch.int32), ym.view(torch.int32))


def test_refusals_launch_nothing():
    """a bad size or a reflected border wider than the plane is WM_E_BADARG: the raw handle returns -1, ops raises, the output keeps its values"""
    from video_watermarking_forgery_detection_amd import _lib
    ops = _ops()
    x = torch.rand(1, N, 6, 6, device="cuda")
    y = torch.full_like(x, 7.0)
    taps = (np.ones(17, np.float32) / 17).tolist()
    raw = _lib.lib()
    for k, border in ((4, BR.ZERO), (17, BR.ZERO), (1, BR.ZERO), (13, BR.REFLECT), (15, BR.REFLECT)):
        t = ops._host_floats(taps[:max(k, 1)])
        assert raw.wm_gauss_sep_fwd(x.data_ptr(), y.data_ptr(), N, 6, 6, t, k, border, None) == -1
        assert raw.wm_gauss_sep_bwd(x.data_ptr(), y.data_ptr(), N, 6, 6, t, k, border, None) == -1
    with pytest.raises(RuntimeError, match="wm_gauss_sep_fwd failed"):
        ops.gauss_sep(x, taps[:13], BR.REFLECT)
    with pytest.raises(RuntimeError, match="wm_gauss_sep_bwd failed"):
        ops.gauss_sep_bwd(x, taps[:4])
    for rect in ((2, 2, 0, 6), (0, 6, 6, 8), (0, 7, 0, 6)):
        with pytest.raises(RuntimeError, match="wm_cropout_fwd failed"):
            ops.cropout_fwd(x, x, rect)
        with pytest.raises(RuntimeError, match="wm_cropout_bwd failed"):
            ops.cropout_bwd(x, rect)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ----------------------------------------------------------------------------- layers
def test_gaussian_blur_3_is_the_stencil_bit_for_bit():
    from video_watermarking_forgery_detection_amd.noise_layers import GaussianBlur
    from video_watermarking_forgery_detection_amd.noise_layers.gaussian_blur import _gaussian_weights
    ops = _ops()
    layer = GaussianBlur()
    w9 = _gaussian_weights(3).flatten().tolist()
    assert layer._w9 == w9
    x = detgen.uniform((2, 3, 37, 41), 5100).cuda()
    g = detgen.normal((2, 3, 37, 41), 5101).cuda()
    want = ops.stencil3(x, w9)
    xr = x.clone().requires_grad_(True)
    y = layer(xr)
    y.backward(g)
    assert torch.equal(y.detach().view(torch.int32), want.view(torch.int32)) and layer.name == "GaussianBlur"
    assert torch.equal(xr.grad.view(torch.int32), ops.stencil3(g, w9[::-1]).view(torch.int32))
    yf, c = layer.fwd(x)
    assert torch.equal(yf.view(torch.int32), want.view(torch.int32)) and torch.equal(layer.bwd(c, g), xr.grad)


@pytest.mark.parametrize("k", [5, 7])
def test_gaussian_blur_k_against_the_reference_fixture(golden, k):
    """GaussianBlur(k) -- module call with autograd, and fwd / bwd -- against the reference's own layer run in float64 (tests/golden/blur.npz)"""
    from video_watermarking_forgery_detection_amd.noise_layers import GaussianBlur
    blur = golden("blur")
    layer = GaussianBlur(k)
    x = torch.from_numpy(blur["x"]).cuda().requires_grad_(True)
    gw = torch.from_numpy(blur["gw"]).cuda()
    y = layer(x)
    (y * gw).sum().backward()
    yf, c = layer.fwd(x.detach())
    assert layer.name == "GaussianBlur" and torch.equal(yf, y.detach()) and torch.equal(layer.bwd(c, gw), x.grad)
    for q, got in (("out", y.detach()), ("gx", x.grad)):
        key = "gb%d/%s" % (k, q)
        NR.check(key, NR.maxdiff(got.cpu().numpy(), blur[key]), NR.bound_of(float(blur["dev32/" + key]), float(blur["amax/" + key])))


@pytest.mark.parametrize("k", [7, 5])
def test_gf_against_its_restated_fixture(golden, k):
    """GF(sigma, k) against the fixture's torch restatement (F.pad(reflect) + conv2d in float64; kornia is not installed) within the bound model"""
    from video_watermarking_forgery_detection_amd.noise_layers.gaussian_filter import GF
    blur = golden("blur")
    layer = GF(float(blur["gf%d/sigma" % k]), k)
    taps = blur["gf%d/taps" % k]
    assert np.array_equal(np.array(layer._taps, np.float32), taps)
    x = torch.from_numpy(blur["x"]).cuda().requires_grad_(True)
    gw = torch.from_numpy(blur["gw"]).cuda()
    y = layer([x, None])
    (y * gw).sum().backward()
    BR.Cmp("GF%d out" % k, y.detach().cpu().numpy(), blur["gf%d/out" % k], BR.bound_fwd(blur["x"], taps, BR.REFLECT)).assert_ok()
    BR.Cmp("GF%d gx" % k, x.grad.cpu().numpy(), blur["gf%d/gx" % k], BR.bound_bwd(blur["gw"], taps, BR.REFLECT)).assert_ok()
    yf, c = layer.fwd(x.detach())
    assert torch.equal(yf, y.detach()) and torch.equal(layer.bwd(c, gw), x.grad) and torch.equal(layer.apply_attack(x.detach()), yf)


# ----------------------------------------------------------------------------- Cropout
def _rects(H, W):
    return {"top": (0, 4, 3, 7), "bottom": (H - 4, H, 3, 7), "left": (2, 6, 0, 5), "right": (2, 6, W - 6, W), "one pixel": (4, 5, 5, 6),
            "full plane": (0, H, 0, W), "splits a float4 (1..3)": (1, H - 1, 1, 3), "splits two (2..7)": (1, H - 1, 2, 7),
            "inside one float4 (5..7)": (3, 4, 5, 7), "corner": (0, 1, 0, 1), "far corner": (H - 1, H, W - 1, W)}


@pytest.mark.parametrize("W", [12, 11, 260])
def test_cropout_kernels_bit_for_bit(W):
    """forward and both gradients are selections: equal to torch.where on the rectangle's mask, bit for bit; the cover is only read; gcover
    may be absent.  W = 12: float4 rows (and the same from an offset base: scalar); 11: scalar rows; 260: a second column block"""
    ops = _ops()
    H = 9
    x, cover, g = (detgen.normal((1, N, H, W), 6100 + i).cuda() for i in range(3))
    cover_before = cover.clone()
    for name, (h0, h1, w0, w1) in _rects(H, W).items():
        m = torch.zeros(1, 1, H, W, dtype=torch.bool, device="cuda")
        m[..., h0:h1, w0:w1] = True
        zero = torch.zeros_like(g)
        for off in (False, True):
            xx, cc, gg = (_offset_view(t) if off else t for t in (x, cover, g))
            y = ops.cropout_fwd(xx, cc, (h0, h1, w0, w1))
            assert torch.equal(y.view(torch.int32), torch.where(m, x, cover).view(torch.int32)), (name, off)
            gx, gc = ops.cropout_bwd(gg, (h0, h1, w0, w1), want_cover=True)
            assert torch.equal(gx.view(torch.int32), torch.where(m, g, zero).view(torch.int32)), (name, off)
            assert torch.equal(gc.view(torch.int32), torch.where(m, zero, g).view(torch.int32)), (name, off)
            gx2, none = ops.cropout_bwd(gg, (h0, h1, w0, w1))                                        # gcover = NULL
            assert none is None and torch.equal(gx2.view(torch.int32), gx.view(torch.int32))
    assert torch.equal(cover.view(torch.int32), cover_before.view(torch.int32))


def test_cropout_layer():
    from video_watermarking_forgery_detection_amd.noise_layers.crop import Crop, Cropout
    layer = Cropout(0.5, 0.25)
    image = detgen.uniform((2, 3, 16, 20), 6200).cuda().requires_grad_(True)
    cover = detgen.uniform((2, 3, 16, 20), 6201).cuda().requires_grad_(True)
    cover_before = cover.detach().clone()
    g = detgen.normal((2, 3, 16, 20), 6202).cuda()
    np.random.seed(77)
    h0, h1, w0, w1 = Crop().get_random_rectangle_inside(image.shape, 0.5, 0.25)
    np.random.seed(77)
    y = layer([image, cover])
    assert layer.last_rect == (h0, h1, w0, w1) and (h1 - h0, w1 - w0) == (8, 5)
    want = cover_before.clone()
    want[:, :, h0:h1, w0:w1] = image.detach()[:, :, h0:h1, w0:w1]                 # what the reference writes into cover_image
    assert torch.equal(y.detach(), want) and torch.equal(cover.detach(), cover_before) and y.data_ptr() != cover.data_ptr()
    y.backward(g)
    m = torch.zeros_like(g, dtype=torch.bool)
    m[:, :, h0:h1, w0:w1] = True
    assert torch.equal(image.grad, torch.where(m, g, torch.zeros_like(g))) and torch.equal(cover.grad, torch.where(m, torch.zeros_like(g), g))
    np.random.seed(77)
    yf, c = layer.fwd(image.detach(), cover=cover.detach())
    assert torch.equal(yf, want) and torch.equal(layer.bwd(c, g), image.grad)
    np.random.seed(77)
    assert torch.equal(layer.apply_attack(image.detach(), cover.detach()), want)


# ----------------------------------------------------------------------------- Hybrid and the trainer
def test_hybrid_step_with_the_new_children():
    """Hybrid takes GaussianBlur(5), GF and Cropout children unchanged (they expose fwd / bwd): one forward and backward; with one-hot weights
    the mix reduces to the chosen child, and the backward to that child's"""
    from video_watermarking_forgery_detection_amd.noise_layers import GaussianBlur, Hybrid, Identity
    from video_watermarking_forgery_detection_amd.noise_layers.crop import Cropout
    from video_watermarking_forgery_detection_amd.noise_layers.gaussian_filter import GF
    blur5 = GaussianBlur(5)
    h = Hybrid([Identity(), blur5, GF(2.0), Cropout(0.5, 0.5)])
    x = detgen.uniform((4, 3, 32, 32), 6300).cuda().requires_grad_(True)
    cover = detgen.uniform((4, 3, 32, 32), 6301).cuda()
    np.random.seed(3)
    torch.manual_seed(3)
    y = h(x, cover)
    loss = (y * y).mean()
    loss.backward()
    assert y.shape == x.shape and bool(torch.isfinite(y).all()) and np.isfinite(float(loss.detach())) and bool(torch.isfinite(x.grad).all())
    assert float(x.grad.abs().max()) > 0
    w = torch.zeros(4, 4, device="cuda")
    w[:, 1] = 1.0
    x2 = x.detach().clone().requires_grad_(True)
    y2 = h(x2, cover, weights=w)
    g = detgen.normal((4, 3, 32, 32), 6302).cuda()
    y2.backward(g)
    assert torch.equal(y2.detach(), blur5.fwd(x.detach())[0]) and torch.equal(x2.grad, blur5.bwd(None, g))


def test_c3_cycle_from_the_blur_option_file(tmp_path):
    """options/train/train_hidden_c3_blur.yml through IRNrhiModel at 2 images of 32 x 32 instead of its 16 of 256 x 256: one step through every
    layer of the cycle (GaussianBlur5, GaussianBlur7, GF7 replayed from their graphs, Cropout eagerly) runs forward and backward with finite
    losses and moves the encoder"""
    from video_watermarking_forgery_detection_amd.models.IRNrhi_model import IRNrhiModel
    from video_watermarking_forgery_detection_amd.noise_layers import GaussianBlur
    from video_watermarking_forgery_detection_amd.noise_layers.crop import Cropout
    from video_watermarking_forgery_detection_amd.noise_layers.gaussian_filter import GF
    from video_watermarking_forgery_detection_amd.options import options
    pkg = os.path.dirname(os.path.abspath(options.__file__))
    opt = options.parse(os.path.join(pkg, "train", "train_hidden_c3_blur.yml"), is_train=True)
    opt["datasets"]["train"].update(GT_size=32, batch_size=2)
    opt["path"] = {"models": str(tmp_path / "models"), "training_state": str(tmp_path / "state")}
    torch.manual_seed(0)
    np.random.seed(0)
    m = IRNrhiModel(options.dict_to_nonedict(opt))
    layers = m.attack.layers
    assert [type(l) for l in layers[1:5]] == [GaussianBlur, GaussianBlur, GF, Cropout]
    assert (layers[1].kernel_size, layers[2].kernel_size, layers[3].kernel, layers[3].sigma) == (5, 7, 7, 2.0)
    for net in (m.netG.encoder, m.netG.decoder, m.discriminator):
        detgen.fill_module(net)
    before = m.netG.encoder.final_layer.weight.detach().clone()
    seen = []
    for step in range(1, 11):
        m.feed_data({"GT": detgen.uniform((2, 3, 32, 32), 6400 + step), "mask": torch.zeros(2, 1, 32, 32), "messages": detgen.bits((2, 30), 6500 + step)})
        logs, _ = m.optimize_parameters(step, None)
        if step > 2:
            seen.append(m.attack.name)
            vals = [float(v) for _, v in logs if not isinstance(v, str)]
            assert vals and all(np.isfinite(v) for v in vals), (step, list(logs))
    assert {"GaussianBlur", "GF", "Cropout"} <= set(seen), seen
    assert layers[4].last_rect is not None
    assert not torch.equal(before, m.netG.encoder.final_layer.weight.detach())
