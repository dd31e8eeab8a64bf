"""CPU: the float64 restatement of the GAN objectives (tests/advloss_restate.py) against the reference's recorded results
(tests/golden/advloss.npz), the tolerance rule the GPU tests use, the module surface and the header."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import advloss_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video_watermarking_forgery_detection_amd")


def _close(got, want, what):
    """float64 against float64: agreement to rounding of a handful of operations (inf where both are inf)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    tol = 1e-12 * np.maximum(np.abs(want), np.max(np.abs(want)) * 1e-3 + 1e-300)
    assert (np.abs(got - want) <= tol).all(), (what, float(np.max(np.abs(got - want))))


def test_element_objectives_match_the_reference_at_float64(golden):
    g = golden("advloss")
    for case, (variant, n) in R.CASES.items():
        objective, label, family, _ = R.VARIANTS[variant]
        x = g["x_%s_n%d" % (family, n)]
        assert x.dtype == np.float32 and np.array_equal(x, R.gen_input(family, n)), case
        loss, grad = R.adv_loss(objective, x, None if label is None else R.f32(label))
        _close(loss, g[case + "_loss64"], case + " loss")
        _close(grad, g[case + "_grad64"], case + " grad")
        # the recorded float32 results are inside their own bound, trivially: the rule is self-consistent and never zero-width
        R.check(case + " reference float32 loss", g[case + "_loss32"], loss, g[case + "_dev_loss"])
        R.check(case + " reference float32 grad", g[case + "_grad32"], grad, g[case + "_dev_grad"])


def test_planted_branch_points_are_in_the_inputs(golden):
    g = golden("advloss")
    p, h, z = g["x_prob_n257"], g["x_hinge_n257"], g["x_logit_n257"]
    assert p[0] == 0.0 and p[1] == 1.0 and 0 < p[2] < 1e-12 and ((p[3:] > 0) & (p[3:] < 1)).all()
    assert h[0] == -1.0 and h[1] == 1.0 and z[0] == 40.0 and z[1] == -40.0
    # the -100 clamp and the 1e-12 denominator, exactly
    v, dv = R.elem("bce_prob", p[:3], 1.0)
    assert v[0] == 100.0 and dv[0] == -1.0 / R.BCE_EPS and v[1] == 0.0 and dv[1] == 0.0
    v, dv = R.elem("bce_prob", p[:3], 0.0)
    assert v[1] == 100.0 and dv[1] == 1.0 / R.BCE_EPS
    # nn.ReLU's subgradient at the kink is 0
    assert R.elem("hinge_disc", h[:2], 1.0)[1][0] == 0.0 and R.elem("hinge_disc", h[:2], -1.0)[1][1] == 0.0
    assert float(g["hinge_fake_n257_grad32"][0]) == 0.0 and float(g["hinge_real_n257_grad32"][1]) == 0.0


def test_bilinear_restatement_is_torchs_upsample():
    for (so, sm) in R.MASK_SHAPES.values():
        m = torch.rand(sm, dtype=torch.float64, generator=torch.Generator().manual_seed(sm[2]))
        want = torch.nn.functional.interpolate(m, size=so[2:], mode="bilinear", align_corners=False)
        _close(R.bilinear(m.numpy(), so[2:]), want.numpy(), "bilinear %s -> %s" % (sm, so))
    same = np.arange(16.0).reshape(1, 1, 4, 4)
    assert np.array_equal(R.bilinear(same, (4, 4)), same)


def test_masked_labels_match_the_reference_at_float64(golden):
    g = golden("advloss")
    for case, (shape, kind, typ) in R.MASK_CASES.items():
        o, m = g[case + "_out"], g[case + "_mask"]
        assert o.shape == R.MASK_SHAPES[shape][0] and m.shape == R.MASK_SHAPES[shape][1]
        assert (kind == "bin") == bool(np.isin(m, (0.0, 1.0)).all())
        loss, grad = R.adv_loss("bce_prob" if typ == "nsgan" else "mse", o, R.masked_labels(m, o.shape, R.MASK_REAL_LABEL))
        _close(loss, g[case + "_loss64"], case + " loss")
        _close(grad, g[case + "_grad64"], case + " grad")


def test_cw_margin_matches_the_reference_ties_included(golden):
    """the gradient is compared EXACTLY: every entry is 0, +-1/2 or +-1, and which column gets it is torch's tie behaviour"""
    g = golden("advloss")
    for case, (B, K, targeted, kappa) in R.CW_CASES.items():
        z, t = g[case + "_logits"], g[case + "_target"]
        loss, grad = R.cw_margin(z, t, targeted, kappa)
        _close(loss, g[case + "_loss64"], case + " loss")
        assert np.array_equal(grad, g[case + "_grad64"]) and np.array_equal(grad, g[case + "_grad32"].astype(np.float64)), case
        if B >= 3:
            sg = 1.0 if targeted else -1.0
            assert not grad[0].any()                                                        # the clamp wins
            assert grad[1, 0] == -0.5 * sg and grad[1, 2] == 0.5 * sg                       # the tie at kappa
            assert grad[2, 1] == sg and grad[2, 3] == 0.0 and grad[2, K - 1] == -sg         # equal maxima: the lowest column
        if B >= 4:
            assert np.count_nonzero(grad[3]) == (0 if targeted else 1) and grad[3, 2] == (0.0 if targeted else 1.0)


def test_bound_rule():
    assert R.bound(0.0, 1.0) == 2 * 2.0 ** -23 and R.bound(1e-3, 1.0) == 4e-3 and R.bound(1e-3, 1.0, scale=-2.0) == 8e-3
    assert 0 < R.bound(0.0, 0.0) < 1e-44
    R.check("exact", np.array([0.0, 1.0]), np.array([0.0, 1.0]), 0.0)
    for bad in (np.array([1e-30, 1.0]), np.array([0.0, 1.0 + 3 * 2.0 ** -23]), np.array([0.0, np.nan])):
        with pytest.raises(AssertionError):
            R.check("planted", bad, np.array([0.0, 1.0]), 0.0)


ENTRY_POINTS = {"wm_advloss_nparts": 1, "wm_advloss_elem": 20, "wm_advloss_finalize": 4, "wm_cw_margin": 14}


def test_header_declares_entry_points_and_library_exports_them():
    from video_watermarking_forgery_detection_amd import _lib, build, ops
    sigs = _lib.signatures()
    for name, nargs in ENTRY_POINTS.items():
        assert name in sigs and len(sigs[name][1]) == nargs, name
    hdr = open(build.HEADER).read()
    for k, v in ops.ADV_OBJECTIVES.items():
        assert "#define WM_ADV_%s %d\n" % (k.upper(), v) in hdr
    assert os.path.exists(os.path.join(PKG, "csrc", "advloss.hip")) and "advloss.hip" in build.NO_SPILL
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libwm_hip.so is not built: the export check needs it (python -m video_watermarking_forgery_detection_amd.build)")
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(h, name), name + " is not exported by the built library"
    fn = h.wm_advloss_nparts
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_size_t]
    assert [fn(n) for n in (0, 1, 4096, 4097, 1 << 20, 1 << 34)] == [0, 1, 1, 2, 256, 256]


def test_module_surface_is_the_references(golden):
    from video_watermarking_forgery_detection_amd import loss as loss_mod
    from video_watermarking_forgery_detection_amd.models.modules.loss import CWLoss, GANLoss
    p = inspect.signature(loss_mod.AdversarialLoss.__init__).parameters
    assert [(k, v.default) for k, v in list(p.items())[1:]] == [("type", "nsgan"), ("target_real_label", 1.0), ("target_fake_label", 0.0)]
    p = inspect.signature(loss_mod.AdversarialLoss.__call__).parameters
    assert [(k, v.default) for k, v in list(p.items())[1:]] == [("outputs", inspect.Parameter.empty), ("is_real", inspect.Parameter.empty),
                                                               ("is_disc", None), ("mask", None)]
    m = loss_mod.AdversarialLoss("lsgan", 0.9, 0.1)
    assert list(m.state_dict().keys()) == list(golden("advloss")["adv_state_dict_keys"]) == ["real_label", "fake_label"]
    assert m.state_dict()["real_label"].dtype == torch.float32 and float(m.state_dict()["fake_label"]) == R.f32(0.1)
    m2 = loss_mod.AdversarialLoss("lsgan")
    m2.load_state_dict(m.state_dict())
    assert m2._labels == (R.f32(0.9), R.f32(0.1))
    with pytest.raises(ValueError, match="nsgan, lsgan or hinge"):
        loss_mod.AdversarialLoss("wgan")
    p = inspect.signature(CWLoss.forward).parameters
    assert [(k, v.default) for k, v in list(p.items())[1:]] == [("logits", inspect.Parameter.empty), ("target", inspect.Parameter.empty),
                                                               ("is_targeted", inspect.Parameter.empty), ("num_classes", 1000), ("kappa", 0)]
    p = inspect.signature(GANLoss.__init__).parameters
    assert [(k, v.default) for k, v in list(p.items())[1:]] == [("gan_type", inspect.Parameter.empty), ("real_label_val", 1.0), ("fake_label_val", 0.0)]
    for t in ("gan", "RaGAN", "lsgan", "wgan-gp"):
        assert GANLoss(t).gan_type == t.lower()
    with pytest.raises(NotImplementedError, match=r"GAN type \[hinge\] is not found"):
        GANLoss("hinge")
    x = torch.zeros(2, 3)
    assert GANLoss("wgan-gp").get_target_label(x, True) is True
    assert torch.equal(GANLoss("gan", 0.9, 0.1).get_target_label(x, False), torch.full((2, 3), 0.1))


def test_modules_and_ops_refuse_cpu_tensors_and_bad_arguments():
    from video_watermarking_forgery_detection_amd import loss as loss_mod, ops
    from video_watermarking_forgery_detection_amd.models.modules.loss import CWLoss, GANLoss
    a, t = torch.rand(1, 1, 4, 4), torch.zeros(3, dtype=torch.int64)
    for call in (lambda: loss_mod.AdversarialLoss()(a, True, True), lambda: loss_mod.AdversarialLoss("hinge")(a, True, False),
                 lambda: GANLoss("gan")(a, True), lambda: GANLoss("wgan-gp")(a, False), lambda: CWLoss()(torch.rand(3, 5), t, True, 5)):
        with pytest.raises(RuntimeError, match="HIP path only"):
            call()
    for call in (lambda: ops.adv_loss(a, "mse", 1.0), lambda: ops.cw_margin(torch.rand(3, 5), t, True)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    with pytest.raises(ValueError, match="objective must be one of"):
        ops.adv_loss(a, "wgan", 1.0)


def test_literal_lsgan_configuration_parses():
    from video_watermarking_forgery_detection_amd.options import options
    opt = options.parse(os.path.join(PKG, "options", "train", "train_literal_lsgan.yml"), is_train=True)
    assert opt["train"]["gan_type"] == "lsgan" and opt["train"]["gradient_clipping"] == 1.0
    base = options.parse(os.path.join(PKG, "options", "train", "train_hidden_c3.yml"), is_train=True)
    assert options.dict_to_nonedict(base)["train"]["gan_type"] is None      # absent: the step's own BCE terms
