"""CPU: SSIM / PSNR / mask scores without a GPU.
  * the torch restatement (tests/metrics_restate.py) reproduces the reference's outputs stored in tests/golden/metrics.npz: run at float32
    its values and gradients are the reference's float32 ones, run at float64 the float64 ones.  Same ops, same order: bit equality is what
    a single-threaded run gives (the fixture was made with one thread); a multi-threaded torch may split the convolution's and the mean's
    sums differently, so where equality fails the difference is bounded by the reference's OWN float32-vs-float64 deviation stored in the
    file (float32 run) or by 1e-12 (float64 run: a few hundred ulp of values of order 1);
  * PSNR and EdgeAccuracy to 1 ulp, the empty-mask and equal-image conventions;
  * the closed-form backward the kernel implements equals autograd of the restatement to float64 rounding;
  * the confusion formulas against a plain count; header <-> exports; CPU input refused; ssim_weight in the signature and the graph key."""
import inspect
import os
import types

import numpy as np
import pytest
import torch

import metrics_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (0, 1, 2)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("si", SMALL)
def test_restatement_reproduces_reference_values(golden, si, kind):
    g = golden("metrics")
    tag = "s%d_%s_" % (si, kind)
    x, y = R.case_inputs(si, kind)
    n = x.numel()
    dev_mean = max(float(g["s%d_%s_dev_mean" % (i, k)]) for i in range(4) for k in R.KINDS)
    dev_img = max(float(g["s%d_%s_dev_img" % (i, k)]) for i in range(4) for k in R.KINDS)
    dev_grad = max(float(g["s%d_%s_dev_grad" % (i, k)]) for i in range(4) for k in R.KINDS)
    with torch.no_grad():
        m32, i32 = R.ssim(x, y, True).numpy(), R.ssim(x, y, False).numpy()
        m64, i64 = R.ssim(x.double(), y.double(), True).numpy(), R.ssim(x.double(), y.double(), False).numpy()
    g32 = R.ssim_autograd(x, y, True).numpy()
    print(tag, "d mean32 %.3e img32 %.3e mean64 %.3e img64 %.3e grad32 %.3e" % (
        abs(float(m32) - float(g[tag + "mean32"])), np.abs(i32 - g[tag + "img32"]).max(), abs(float(m64) - float(g[tag + "mean64"])),
        np.abs(i64 - g[tag + "img64"]).max(), n * np.abs(g32.astype(np.float64) - g[tag + "grad32"]).max()))
    assert m32.dtype == np.float32 and m64.dtype == np.float64
    assert np.array_equal(m32, g[tag + "mean32"]) or abs(float(m32) - float(g[tag + "mean32"])) <= dev_mean
    assert np.array_equal(i32, g[tag + "img32"]) or np.abs(i32.astype(np.float64) - g[tag + "img32"]).max() <= dev_img
    assert np.array_equal(m64, g[tag + "mean64"]) or abs(float(m64) - float(g[tag + "mean64"])) <= 1e-12
    assert np.array_equal(i64, g[tag + "img64"]) or np.abs(i64 - g[tag + "img64"]).max() <= 1e-12
    assert np.array_equal(g32, g[tag + "grad32"]) or n * np.abs(g32.astype(np.float64) - g[tag + "grad32"]).max() <= dev_grad
    if kind == "equal":
        assert float(m32) == 1.0 and float(m64) == 1.0


@pytest.mark.parametrize("kind", ("near", "smooth"))
def test_restatement_reproduces_reference_at_256(golden, kind):
    """the C2-sized case: float32 value, the stored stride sample of the gradient and sum |g|"""
    g = golden("metrics")
    tag = "s3_%s_" % kind
    x, y = R.case_inputs(3, kind)
    n = x.numel()
    dev_mean = max(float(g["s%d_%s_dev_mean" % (i, k)]) for i in range(4) for k in R.KINDS)
    dev_grad = max(float(g["s%d_%s_dev_grad" % (i, k)]) for i in range(4) for k in R.KINDS)
    with torch.no_grad():
        m32 = R.ssim(x, y, True).numpy()
    g32 = R.ssim_autograd(x, y, True)
    sample = g32.reshape(-1)[::R.GRAD_STRIDE].numpy()
    assert np.array_equal(m32, g[tag + "mean32"]) or abs(float(m32) - float(g[tag + "mean32"])) <= dev_mean
    assert np.array_equal(sample, g[tag + "grad32_sample"]) or n * np.abs(sample.astype(np.float64) - g[tag + "grad32_sample"]).max() <= dev_grad
    # sum |g| over n elements each within dev_grad / n of the reference's
    assert abs(float(g32.double().abs().sum()) - float(g[tag + "grad32_abs"])) <= dev_grad


@pytest.mark.parametrize("si", (0, 1, 2, 3))
def test_psnr_and_edge_accuracy_reproduce_reference(golden, si):
    g = golden("metrics")
    for kind in R.KINDS:
        x, y = R.case_inputs(si, kind)
        tag = "s%d_%s_" % (si, kind)
        p1, p255 = R.psnr(x, y, 1.0), R.psnr(255 * x, 255 * y, 255.0)
        if kind == "equal":   # the convention: an integer zero
            assert int(g[tag + "psnr1"]) == 0 and int(p1) == 0 and not p1.dtype.is_floating_point
        else:
            assert _ulps(p1.numpy(), g[tag + "psnr1"]) <= 1 and _ulps(p255.numpy(), g[tag + "psnr255"]) <= 1
    pred, gt = R.case_masks(si)
    prec, rec = R.edge_accuracy(gt, pred, 0.5)
    assert _ulps(prec.numpy(), g["m%d_prec" % si]) <= 1 and _ulps(rec.numpy(), g["m%d_rec" % si]) <= 1
    assert 0 < float(prec) < 1 and 0 < float(rec) < 1


def test_empty_mask_convention(golden):
    g = golden("metrics")
    z = torch.zeros(1, 1, 8, 8)
    prec, rec = R.edge_accuracy(z, z)
    assert int(prec) == 1 and int(rec) == 1 and int(g["empty_prec"]) == 1 and int(g["empty_rec"]) == 1


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("si", SMALL)
def test_backward_formula_equals_autograd(si, kind):
    """both sides use the same window at float64: the difference is summation order, ~1e-13 of max |g|; 1e-10 leaves room"""
    x, y = (t.double() for t in R.case_inputs(si, kind))
    B = x.shape[0]
    n = x.numel()
    for wrt in (0, 1):
        a, b = (x, y) if wrt == 0 else (y, x)
        ga = R.ssim_autograd(x, y, True, wrt=wrt)
        gf = R.ssim_backward_formula(a, b, torch.full((B, 1, 1, 1), 1.0 / n, dtype=torch.float64))
        scale = max(float(ga.abs().max()), 1.0 / n)
        assert float((ga - gf).abs().max()) <= 1e-10 * scale, (wrt, float((ga - gf).abs().max()), scale)
        gout = R.case_gout(si).double()
        ga = R.ssim_autograd(x, y, False, gout=gout, wrt=wrt)
        gf = R.ssim_backward_formula(a, b, (gout * B / n).reshape(B, 1, 1, 1))
        scale = max(float(ga.abs().max()), 1.0 / n)
        assert float((ga - gf).abs().max()) <= 1e-10 * scale


def test_confusion_formulas_against_a_plain_count():
    for si in range(3):
        pred, gt = R.case_masks(si)
        TN, TP, FN, FP = R.confusion(pred.numpy(), gt.numpy(), 0.5, 0.5)
        p, t = pred.numpy().reshape(-1) > 0.5, gt.numpy().reshape(-1) > 0.5
        cnt = [0, 0, 0, 0]
        for a, b in zip(p.tolist(), t.tolist()):
            cnt[(1 if a else 0) if a == b else (2 if not a else 3)] += 1
        assert [TN, TP, FN, FP] == cnt and min(cnt) > 0
        s = R.mask_scores(TN, TP, FN, FP)
        assert s["F1"] == 2 * TP / (2 * TP + FP + FN) and s["ACC"] == (TP + TN) / p.size
        assert s["BER"] == 0.5 * (FP / (FP + TN) + FN / (FN + TP)) and s["TPR"] == TP / (TP + FN) and s["FPR"] == FP / (FP + TN)
    s = R.mask_scores(10, 0, 0, 0)
    assert np.isnan(s["F1"]) and np.isnan(s["TPR"]) and s["FPR"] == 0.0 and s["ACC"] == 1.0


NEW_ENTRY_POINTS = ("wm_ssim_nparts", "wm_ssim_fwd", "wm_ssim_finalize", "wm_ssim_bwd", "wm_psnr_partials", "wm_psnr_finalize",
                    "wm_confusion_nparts", "wm_confusion_counts")


def test_header_declares_entry_points_and_package_exports_names():
    from video_watermarking_forgery_detection_amd import _lib
    sigs = _lib.signatures()
    for name in NEW_ENTRY_POINTS:
        assert name in sigs, name
    assert len(sigs["wm_ssim_bwd"][1]) == 15 and len(sigs["wm_ssim_fwd"][1]) == 10
    from video_watermarking_forgery_detection_amd import metrics, ops, pytorch_ssim
    for mod, names in ((pytorch_ssim, ("SSIM", "ssim")), (metrics, ("PSNR", "EdgeAccuracy", "mask_scores")),
                       (ops, ("ssim", "ssim_bwd", "confusion_counts", "psnr"))):
        for n in names:
            assert callable(getattr(mod, n)), (mod.__name__, n)
    assert os.path.exists(os.path.join(ROOT, "video_watermarking_forgery_detection_amd", "csrc", "ssim.hip"))
    with pytest.raises(NotImplementedError):
        pytorch_ssim.SSIM(window_size=7)
    with pytest.raises(NotImplementedError):
        pytorch_ssim.ssim(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16), window_size=5)


def test_cpu_tensors_are_refused():
    from video_watermarking_forgery_detection_amd import metrics, ops, pytorch_ssim
    a = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="HIP path only"):
        pytorch_ssim.SSIM()(a, a)
    with pytest.raises(RuntimeError, match="HIP path only"):
        pytorch_ssim.ssim(a, a)
    with pytest.raises(RuntimeError, match="HIP path only"):
        metrics.PSNR(1.0)(a, a)
    with pytest.raises(RuntimeError, match="HIP path only"):
        metrics.EdgeAccuracy()(a[:, :1], a[:, :1])
    with pytest.raises(RuntimeError, match="HIP path only"):
        metrics.mask_scores(a[:, :1], a[:, :1], 0.5)
    for call in (lambda: ops.ssim(a, a), lambda: ops.psnr(a, a, 1.0), lambda: ops.confusion_counts(a, a, 0.5, 0.5),
                 lambda: ops.ssim_bwd(torch.zeros(3, 1, 3, 16, 16), a, a)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


def test_hidden_takes_ssim_weight_and_keys_the_graph_on_it():
    from video_watermarking_forgery_detection_amd.hidden_models.hidden import Hidden
    p = inspect.signature(Hidden.__init__).parameters["ssim_weight"]
    assert p.default == 0.0
    h = object.__new__(Hidden)   # host logic only: the key is a function of attributes (a real Hidden needs a device)
    h.noise_id, h.keep_dead_discriminator_grads, h.lazy_losses, h.two_streams, h.skip_zero_attack_gradient = None, True, True, False, True
    h.encoder_decoder = types.SimpleNamespace(encoder=types.SimpleNamespace(compute_dtype=torch.bfloat16))
    h.optimizer_discrim = h.optimizer_enc_dec = types.SimpleNamespace(decoupled=False)
    img, msg = torch.zeros(2, 3, 32, 32), torch.zeros(2, 30)
    keys = []
    for w in (0.0, 0.1, 0.01, 0.1):
        h.ssim_weight = w
        keys.append(h._graph_key(img, msg, True))
    assert keys[0] != keys[1] and keys[1] != keys[2] and keys[1] == keys[3] and len({hash(k) for k in keys}) == 3
    h.ssim_weight = 0.0
    assert h._ssim_term(img, img) == (None, None)   # weight 0: nothing is launched (on CPU tensors anything else would raise)
