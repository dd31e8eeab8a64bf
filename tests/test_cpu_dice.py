"""CPU: the Dice losses without a GPU.
  * the torch restatement (tests/dice_restate.py) reproduces the reference's outputs stored in tests/golden/dice.npz: run at float32 its
    losses and gradients are the reference's float32 ones, run at float64 the float64 ones.  Same ops, same order: bit equality is what a
    single-threaded run gives (the fixture was made with one thread); a multi-threaded torch may split the sums differently, so where
    equality fails the difference is bounded by the reference's OWN float32-vs-float64 deviation stored in the file (float32 run) or by
    1e-12 relative (float64 run);
  * an all-zero target gives 1 - smooth/den, neither 0 nor NaN; the weighted restatement is the weighted sum of the per-class losses;
  * the closed-form backward the kernels implement equals autograd of the restatement to float64 rounding;
  * the public module refuses CPU input and bad reductions, keeps the reference's assertion messages; header <-> exports; the C5 Dice
    configuration parses."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dice_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video_watermarking_forgery_detection_amd")


def _same(a, want, bound, scale=None):
    a, want = np.asarray(a), np.asarray(want)
    if np.array_equal(a, want):
        return True
    s = np.abs(want.astype(np.float64)) if scale is None else scale
    return bool(np.all(np.abs(a.astype(np.float64) - want.astype(np.float64)) <= bound * s))


@pytest.mark.parametrize("red", R.REDUCTIONS)
@pytest.mark.parametrize("p", R.POWERS)
@pytest.mark.parametrize("case", ("b0", "b1"))
def test_restatement_reproduces_reference_binary(golden, case, p, red):
    g = golden("dice")
    x, t = R.fixture_case(g, case)
    tag = "%s_p%d_%s_" % (case, p, red)
    dev_l, dev_g = float(g["dev_loss_max_binary"]), float(g["dev_grad_max_binary"])
    fn = lambda a: R.binary_dice(a, t.to(a.dtype), 1, p, red)  # noqa: E731
    l32, l64 = fn(x), fn(x.double())
    g32 = R.grad_of(fn, x)
    assert l32.dtype == torch.float32 and l64.dtype == torch.float64
    assert _same(l32.numpy(), g[tag + "loss32"], dev_l)
    assert _same(l64.numpy(), g[tag + "loss64"], 1e-12)
    assert _same(g32.numpy(), g[tag + "grad32"], dev_g, scale=float(np.abs(g[tag + "grad32"]).max()))


@pytest.mark.parametrize("red", R.REDUCTIONS)
@pytest.mark.parametrize("ig", (None, 1))
@pytest.mark.parametrize("case", ("m0", "m1"))
def test_restatement_reproduces_reference_multiclass(golden, case, ig, red):
    g = golden("dice")
    x, t = R.fixture_case(g, case)
    tag = "%s_i%s_%s_" % (case, "-" if ig is None else ig, red)
    dev_l, dev_g = float(g["dev_loss_max_multi"]), float(g["dev_grad_max_multi"])
    fn = lambda a: R.dice(a, t.to(a.dtype), None, ig, 1, 2, red)  # noqa: E731
    l32, l64 = fn(x), fn(x.double())
    assert _same(l32.numpy(), g[tag + "loss32"], dev_l)
    assert _same(l64.numpy(), g[tag + "loss64"], 1e-12)
    if tag + "grad32" in g.files:
        want = g[tag + "grad32"]
        assert _same(R.grad_of(fn, x).numpy(), want, dev_g, scale=float(np.abs(want).max()))


def test_fixture_holds_what_the_issue_asks(golden):
    g = golden("dice")
    assert [tuple(g[k + "_x"].shape) for k in ("b0", "b1", "m0", "m1")] == list(R.BINARY_SHAPES + R.MULTI_SHAPES)
    x, t = R.fixture_case(g, "b1")
    assert float(t[2].sum()) == 0 and float(t[0].sum()) > 0      # the all-zero target
    loss = R.binary_dice(x.double(), t.double(), 1, 2, "none")
    want = 1 - 1 / (float((x[2].double() ** 2).sum()) + 1)
    assert abs(float(loss[2]) - want) <= 1e-15 and 0 < want < 1
    assert abs(float(g["b1_p2_none_loss64"][2]) - want) <= 1e-12
    for k in ("m0", "m1"):
        _, t = R.fixture_case(g, k)
        assert torch.equal(t.sum(1), torch.ones_like(t[:, 0]))   # one-hot
    # the deviations that calibrate the GPU tolerances (1e-6 loss, 2e-6 gradient) leave the margin the tolerances claim
    assert float(g["dev_loss_max_binary"]) < 1e-6 / 10 and float(g["dev_grad_max_binary"]) < 2e-6 / 8
    assert float(g["dev_loss_max_multi"]) < 1e-6 / 8 and float(g["dev_grad_max_multi"]) < 2e-6 / 4


def test_weighted_restatement_is_the_weighted_class_sum(golden):
    g = golden("dice")
    x, t = (v.double() for v in R.fixture_case(g, "m0"))
    w = torch.tensor([0.5, 2.0, 1.0, 0.25], dtype=torch.float64)
    s = torch.softmax(x, 1)
    for red in R.REDUCTIONS:
        want = sum(w[c] * R.binary_dice(s[:, c], t[:, c], 1, 2, red) for c in range(4) if c != 2) / 4
        assert torch.allclose(R.dice(x, t, w, 2, 1, 2, red), want, rtol=1e-14, atol=0)


def _formula_binary(x, t, smooth, p, gout):
    """the backward wm_dice_bwd implements: gout_b * (num * p * x^(p-1) - t * den) / den^2"""
    n = x.shape[0]
    xf, tf = x.reshape(n, -1), t.reshape(n, -1)
    num = (xf * tf).sum(1, keepdim=True) + smooth
    den = (xf.pow(p) + tf.pow(p)).sum(1, keepdim=True) + smooth
    return (gout.reshape(n, 1) * (num * p * xf.pow(p - 1) - tf * den) / den ** 2).reshape(x.shape)


@pytest.mark.parametrize("p", R.POWERS)
def test_backward_formula_equals_autograd(golden, p):
    g = golden("dice")
    x, t = (v.double() for v in R.fixture_case(g, "b1"))
    gout = torch.tensor([0.3, -1.2, 2.0], dtype=torch.float64)
    ga = R.grad_of(lambda a: R.binary_dice(a, t, 1e-3, p, "none"), x, gout)
    gf = _formula_binary(x, t, 1e-3, p, gout)
    assert float((ga - gf).abs().max()) <= 1e-12 * float(ga.abs().max())
    # the softmax form: dz_c = s_c (g_c - sum_k g_k s_k) with g_c the binary formula of class c times weight_c / C (0 when ignored)
    z, y = (v.double() for v in R.fixture_case(g, "m0"))
    w = torch.tensor([0.5, 2.0, 1.0, 0.25], dtype=torch.float64)
    go = torch.tensor([0.7, -0.4], dtype=torch.float64)
    ga = R.grad_of(lambda a: R.dice(a, y, w, 1, 1, p, "none"), z, go)
    s = torch.softmax(z, 1)
    gc = torch.stack([(0.0 if c == 1 else w[c] / 4) * _formula_binary(s[:, c], y[:, c], 1, p, go) for c in range(4)], 1)
    gf = s * (gc - (gc * s).sum(1, keepdim=True))
    assert float((ga - gf).abs().max()) <= 1e-12 * float(ga.abs().max())


NEW_ENTRY_POINTS = {"wm_dice_nparts": 1, "wm_dice_sums": 7, "wm_dice_softmax_sums": 8, "wm_dice_finalize": 11, "wm_dice_bwd": 14,
                    "wm_dice_softmax_bwd": 16}


def test_header_declares_entry_points_and_library_exports_them():
    from video_watermarking_forgery_detection_amd import _lib, dice_loss, ops
    sigs = _lib.signatures()
    for name, nargs in NEW_ENTRY_POINTS.items():
        assert name in sigs and len(sigs[name][1]) == nargs, name
    assert os.path.exists(os.path.join(PKG, "csrc", "dice.hip"))
    for mod, names in ((dice_loss, ("make_one_hot", "BinaryDiceLoss", "DiceLoss")),
                       (ops, ("dice_binary", "dice_binary_fwd", "dice_binary_bwd", "dice_softmax", "dice_softmax_fwd", "dice_softmax_bwd"))):
        for n in names:
            assert callable(getattr(mod, n)), (mod.__name__, n)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libwm_hip.so is not built: the export check needs it (python -m video_watermarking_forgery_detection_amd.build)")
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(h, name), name + " is not exported by the built library"
    fn = h.wm_dice_nparts      # host-only: the partial count, 1 .. 64, 0 for an empty sample
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_size_t]
    assert [fn(n) for n in (0, 1, 30 * 43, 4096, 4097, 65536, 10 ** 9)] == [0, 1, 1, 1, 2, 16, 64]


def test_module_surface_and_refusals():
    from video_watermarking_forgery_detection_amd import dice_loss, ops
    a, t = torch.rand(2, 1, 8, 8), torch.zeros(2, 1, 8, 8)
    b = dice_loss.BinaryDiceLoss()
    assert (b.smooth, b.p, b.reduction) == (1, 2, 'mean')
    d = dice_loss.DiceLoss(weight=None, ignore_index=3, smooth=2, p=1, reduction='sum')
    assert d.kwargs == {'smooth': 2, 'p': 1, 'reduction': 'sum'} and d.ignore_index == 3 and d.weight is None
    with pytest.raises(TypeError):
        dice_loss.DiceLoss(beta=1)
    with pytest.raises(RuntimeError, match="HIP path only"):
        b(a, t)
    with pytest.raises(RuntimeError, match="HIP path only"):
        dice_loss.DiceLoss()(a, t)
    for call in (lambda: ops.dice_binary(a, t), lambda: ops.dice_softmax(a, t), lambda: ops.dice_binary_fwd(a, t),
                 lambda: ops.dice_binary_bwd(a, t, torch.zeros(2, 2, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    for bad in (lambda: dice_loss.BinaryDiceLoss(reduction='avg')(a, t), lambda: dice_loss.DiceLoss(reduction='avg')(a, t),
                lambda: ops.dice_binary(a, t, reduction='avg'), lambda: ops.dice_softmax(a, t, reduction=None)):
        with pytest.raises(Exception, match="Unexpected reduction"):
            bad()
    with pytest.raises(AssertionError, match="predict & target batch size don't match"):
        b(a, t[:1])
    with pytest.raises(AssertionError, match="predict & target shape do not match"):
        dice_loss.DiceLoss()(a, t[:, :, :4])
    with pytest.raises(AssertionError, match=r"Expect weight shape \[1\], get\[3\]"):
        dice_loss.DiceLoss(weight=np.ones(3))(a, t)
    labels = torch.tensor([[[0, 2], [1, 1]]]).unsqueeze(0)            # [1,1,2,2]
    oh = dice_loss.make_one_hot(labels, 3)
    assert oh.shape == (1, 3, 2, 2) and oh.dtype == torch.float32
    assert torch.equal(oh.argmax(1, keepdim=True), labels) and torch.equal(oh.sum(1), torch.ones(1, 2, 2))


def test_c5_dice_configuration_parses_and_the_default_is_off():
    from video_watermarking_forgery_detection_amd.options import options
    opt = options.parse(os.path.join(PKG, "options", "train", "train_hidden_c5_dice.yml"), is_train=True)
    assert opt["train"]["dice_weight"] == 1.0 and opt["train"]["localizer"] is True
    base = options.parse(os.path.join(PKG, "options", "train", "train_hidden_c5.yml"), is_train=True)
    assert options.dict_to_nonedict(base)["train"]["dice_weight"] is None     # absent: the trainer reads 0 = off
    drop = lambda o: {k: v for k, v in o["train"].items() if k != "dice_weight"}  # noqa: E731
    assert drop(opt) == drop(base) and opt["datasets"] == base["datasets"]
