"""CPU: the float64 restatement of the reconstruction, gradient and exclusion losses (tests/imgloss_restate.py) against the reference's
recorded results (tests/golden/imgloss.npz), the module surface, the header, and -- on planted defects -- the comparison functions the GPU
tests call (check_value / check_grad with the fixture's bounds: 4 x the reference's own float32-vs-float64 deviation)."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import imgloss_restate as R

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_watermarking_forgery_detection_amd")


def test_restatement_equals_the_reference_float64(golden):
    g = golden("imgloss")
    for name in R.CASES:
        a, b, level = R.fixture_case(g, name)
        a, b = a.double(), b.double()
        tag = name + "_excl_"
        if a.shape[1] != b.shape[1]:
            assert int(g[tag + "reference_raises"]) == 1      # the reference cannot run C1 != C2: the restatement alone defines it
            loss, means = R.exclusion(a, b, level, want_terms=True)
            assert means.shape == (level, 2, a.shape[1] * b.shape[1]) and float(loss) > 0
            continue
        loss, means = R.exclusion(a, b, level, want_terms=True)
        assert R.rel_dev(loss.numpy(), g[tag + "loss64"]) <= 1e-12
        assert R.rel_dev(means.numpy(), g[tag + "means64"]) <= 1e-12
        g1, g2 = R.grad_of(lambda x, y: R.exclusion(x, y, level), a, b)
        dg = float(g[tag + "dev_grad"])
        assert 0 < dg < 1e-5
        for got, ref32 in ((g1, g[tag + "grad1_32"]), (g2, g[tag + "grad2_32"])):    # the float32 gradients: within the recorded deviation
            assert R.grad_dev(ref32, got.numpy()) <= dg * (1 + 1e-6)
    for name in R.IMAGE_CASES:
        a, b, _ = R.fixture_case(g, name)
        a, b = a.double(), b.double()
        for kind in R.KINDS:
            for eps in R.EPS:
                tag = "%s_recon_%s_%g_" % (name, kind, eps)
                assert R.rel_dev(R.recon(a, b, kind, eps).numpy(), g[tag + "loss64"]) <= 1e-12
                if tag + "grad32" in g.files:
                    (gx,) = R.grad_of(lambda x: R.recon(x, b, kind, eps), a)
                    assert R.grad_dev(g[tag + "grad32"], gx.numpy()) <= float(g[tag + "dev_grad"]) * (1 + 1e-6)
        tag = name + "_gradl_"
        assert R.rel_dev(R.gradient_loss(a).numpy(), g[tag + "loss64"]) <= 1e-12
        if tag + "grad32" in g.files:
            (ga,) = R.grad_of(R.gradient_loss, a)
            assert R.grad_dev(g[tag + "grad32"], ga.numpy()) <= float(g[tag + "dev_grad"]) * (1 + 1e-6)


def test_bounds_come_from_the_fixture(golden):
    g = golden("imgloss")
    b = R.bounds(g)
    assert set(b) == {"loss_excl", "mean_excl", "grad_excl", "loss_recon", "grad_recon", "loss_gradl", "grad_gradl"}
    for k, v in b.items():
        assert v == 4.0 * float(g["dev_" + k.replace("_", "_max_")]) and 1e-8 < v < 1e-4, (k, v)
    # each per-case deviation lies within the stored maximum
    for k in g.files:
        for q in ("loss", "mean", "grad"):
            if k.endswith("_dev_" + q):
                fam = "excl" if "_excl_" in k else ("recon" if "_recon_" in k else "gradl")
                assert float(g[k]) <= float(g["dev_%s_max_%s" % (q, fam)]), k
    assert int(g["const_image_grad_is_nan"]) == 1 and float(g["const_image_loss"]) == 0.0


def test_a_vanished_term_has_a_zero_gradient_in_the_restatement():
    a, b = R.gen_pair((1, 3, 16, 16), (1, 3, 16, 16), 5)
    a = a.double()
    a[:, 1] = 0.5
    loss, means = R.exclusion(a, b.double(), 3, want_terms=True)
    assert (means[:, :, [1, 4, 7]] == 0).all() and (means[:, :, [0, 2, 3, 5, 6, 8]] > 0).all() and float(loss) > 0
    g1, g2 = R.grad_of(lambda x, y: R.exclusion(x, y, 3), a, b.double())
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all() and (g1[:, 1] == 0).all() and float(g1[:, 0].abs().max()) > 0


def test_reconstruction_module_quirks_match_the_fixture(golden, capsys):
    from video_watermarking_forgery_detection_amd.models.modules.loss import ReconstructionLoss
    g = golden("imgloss")
    sig = inspect.signature(ReconstructionLoss.__init__).parameters
    assert sig["losstype"].default == "l_char" and sig["eps"].default == 1e-6
    assert inspect.signature(ReconstructionLoss.forward).parameters["losstype"].default == "l_char"
    m = ReconstructionLoss(losstype="l2", eps=1e-3)
    assert m.losstype == "l2" and m.eps == 1e-3
    a, b, _ = R.fixture_case(g, "e2")
    a, b = a.double(), b.double()
    # the fixture's values of the reference built with losstype='l2': a default call is l_char all the same, a call with 'l1' is l1
    assert R.rel_dev(R.recon(a, b, "l_char", 1e-3).numpy(), g["quirk_ctor_l2_default_call"]) <= 1e-12
    assert R.rel_dev(R.recon(a, b, "l1", 1e-3).numpy(), g["quirk_ctor_l2_call_l1"]) <= 1e-12
    assert abs(float(g["quirk_ctor_l2_default_call"]) - float(R.recon(a, b, "l2"))) > 1.0
    # the unknown type: the reference's message and 0, before anything looks at the tensors
    assert m(a, b, "nonsense") == 0 and "reconstruction loss type error!" in capsys.readouterr().out
    # a valid type reaches the kernels: CPU tensors are refused whatever the constructor said
    with pytest.raises(RuntimeError, match="HIP path only"):
        m(a.float(), b.float())


NEW_ENTRY_POINTS = {"wm_recon_nparts": 1, "wm_recon_sums": 8, "wm_recon_finalize": 5, "wm_recon_bwd": 12, "wm_gradloss_nparts": 2,
                    "wm_gradloss_sums": 6, "wm_gradloss_finalize": 6, "wm_gradloss_bwd": 10, "wm_excl_nparts": 3, "wm_excl_fwd": 10,
                    "wm_excl_finalize": 11, "wm_excl_bwd": 16}


def test_header_declares_entry_points_and_library_exports_them():
    from video_watermarking_forgery_detection_amd import _lib, build, ops
    from video_watermarking_forgery_detection_amd import loss as loss_mod
    sigs = _lib.signatures()
    for name, nargs in NEW_ENTRY_POINTS.items():
        assert name in sigs and len(sigs[name][1]) == nargs, name
    assert os.path.exists(os.path.join(PKG, "csrc", "imgloss.hip")) and "imgloss.hip" in build.NO_SPILL
    for n in ("recon_loss", "recon_loss_fwd", "recon_loss_bwd", "gradient_loss", "gradient_loss_bwd", "exclusion", "exclusion_fwd", "exclusion_bwd"):
        assert callable(getattr(ops, n)), n
    assert ops.RECON_KINDS == {"l2": 0, "l_char": 1, "l1": 2}
    for n in ("ExclusionLoss", "GradientLoss"):
        assert callable(getattr(loss_mod, n))
    for n in ("compute_gradient", "_all_comb", "get_gradients"):      # deliberately not carried over
        assert not hasattr(loss_mod.ExclusionLoss, n)
    assert inspect.signature(loss_mod.ExclusionLoss.__init__).parameters["level"].default == 3
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libwm_hip.so is not built: the export check needs it (python -m video_watermarking_forgery_detection_amd.build)")
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(h, name), name + " is not exported by the built library"
    fn = h.wm_excl_nparts      # host-only: 16 x 32 tiles per sample
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 3
    assert [fn(*a) for a in ((0, 8, 8), (1, 8, 8), (2, 32, 32), (1, 30, 43), (1, 133, 70), (16, 256, 256))] == [0, 1, 4, 4, 27, 2048]
    fn = h.wm_recon_nparts
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_size_t]
    assert [fn(n) for n in (0, 1, 4096, 4097, 3 * 256 * 256)] == [0, 1, 1, 2, 48]


def test_modules_and_ops_refuse_cpu_tensors():
    from video_watermarking_forgery_detection_amd import loss as loss_mod, ops
    from video_watermarking_forgery_detection_amd.models.modules.loss import ReconstructionLoss
    a, b = torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8)
    for call in (lambda: loss_mod.ExclusionLoss()(a, b), lambda: loss_mod.GradientLoss()(a), lambda: ReconstructionLoss()(a, b, "l2")):
        with pytest.raises(RuntimeError, match="HIP path only"):
            call()
    c = torch.zeros(3, 2, 9, dtype=torch.float64)
    for call in (lambda: ops.recon_loss(a, b, "l2", 1e-6), lambda: ops.recon_loss_fwd(a, b), lambda: ops.recon_loss_bwd(a, b),
                 lambda: ops.gradient_loss(a), lambda: ops.gradient_loss_bwd(a), lambda: ops.exclusion(a, b, 3), lambda: ops.exclusion_bwd(a, b, c)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    with pytest.raises(ValueError, match="kind must be one of"):
        ops.recon_loss(a, b, "huber")


def test_hidden_takes_recon_weight_and_keys_the_graph_on_it():
    import types
    from video_watermarking_forgery_detection_amd.hidden_models.hidden import Hidden
    p = inspect.signature(Hidden.__init__).parameters
    assert p["recon_weight"].default == 0.0 and p["recon_type"].default == "l2"
    h = object.__new__(Hidden)   # host logic only: the key is a function of attributes (a real Hidden needs a device)
    h.noise_id, h.keep_dead_discriminator_grads, h.lazy_losses, h.two_streams, h.skip_zero_attack_gradient = None, True, True, False, True
    h.encoder_decoder = types.SimpleNamespace(encoder=types.SimpleNamespace(compute_dtype=torch.bfloat16))
    h.optimizer_discrim = h.optimizer_enc_dec = types.SimpleNamespace(decoupled=False)
    h.ssim_weight = 0.0
    img, msg = torch.zeros(2, 3, 32, 32), torch.zeros(2, 30)
    keys = []
    for w, kind in ((0.0, "l2"), (1e-4, "l2"), (1e-4, "l_char"), (1e-4, "l2")):
        h.recon_weight, h.recon_type = w, kind
        keys.append(h._graph_key(img, msg, True))
    assert len(set(keys)) == 3 and keys[1] == keys[3]
    h.recon_weight = 0.0
    assert h._recon_term(img, img) == (None, None)   # weight 0: nothing is launched (on CPU tensors anything else would raise)


def test_c3_char_configuration_parses_and_the_default_is_off():
    from video_watermarking_forgery_detection_amd.options import options
    opt = options.parse(os.path.join(PKG, "options", "train", "train_hidden_c3_char.yml"), is_train=True)
    assert opt["train"]["lambda_fit_forw"] == 1e-5 and opt["train"]["pixel_criterion_forw"] == "l_char"
    base = options.parse(os.path.join(PKG, "options", "train", "train_hidden_c3.yml"), is_train=True)
    assert options.dict_to_nonedict(base)["train"]["lambda_fit_forw"] is None     # absent: the trainer reads 0 = off
    drop = lambda o: {k: v for k, v in o["train"].items() if k not in ("lambda_fit_forw", "pixel_criterion_forw")}  # noqa: E731
    assert drop(opt) == drop(base) and opt["datasets"] == base["datasets"]


# ----------------------------------------------------------------------------- the GPU tests' comparisons catch planted defects
def _caught(fn):
    with pytest.raises(AssertionError):
        fn()


def test_comparisons_fail_on_planted_defects(golden, capsys):
    g = golden("imgloss")
    bd = R.bounds(g)
    a43, b43, _ = (v.double() if torch.is_tensor(v) else v for v in R.fixture_case(g, "e1"))     # 1 x 3 x 30 x 43
    a70, b70 = (v.double() for v in R.gen_pair((1, 3, 133, 70), (1, 3, 133, 70), 77))

    def excl_checks(a, b, defect):
        loss, means = R.exclusion(a, b, 3, want_terms=True)
        bad_loss, bad_means = R.exclusion(a, b, 3, want_terms=True, defect=defect)
        g_ok = R.grad_of(lambda x, y: R.exclusion(x, y, 3), a, b)
        g_bad = R.grad_of(lambda x, y: R.exclusion(x, y, 3, defect=defect), a, b)
        return ((lambda: R.check_value(defect + " means", bad_means.numpy(), means.numpy(), bd["mean_excl"])),
                (lambda: R.check_value(defect + " loss", bad_loss.numpy(), loss.numpy(), bd["loss_excl"])),
                (lambda: R.check_grad(defect + " grad1", g_bad[0].numpy(), g_ok[0].numpy(), bd["grad_excl"])))

    # the unharmed restatement passes every comparison against itself
    loss, means = R.exclusion(a43, b43, 3, want_terms=True)
    assert R.check_value("self", means.numpy(), means.numpy(), bd["mean_excl"]) == 0.0
    # one pixel's difference dropped, at the largest shape of the GPU test (the smallest relative change: about 1 / (H W))
    for chk in excl_checks(a70, b70, "pixel_dropped"):
        _caught(chk)
    # one row of differences at an interior multiple of 4 (a tile seam) dropped
    for chk in excl_checks(a70, b70, "row_dropped"):
        _caught(chk)
    # ceil instead of floor pooling at 30 x 43: level 1 becomes 15 x 22 instead of 15 x 21
    for chk in excl_checks(a43, b43, "ceil_pool"):
        _caught(chk)
    # gradx and grady swapped: the means change places (the loss, their symmetric sum, cannot tell: the per-term comparison must)
    _caught(excl_checks(a43, b43, "swapped")[0])
    # the same for the gradient loss
    for defect in ("pixel_dropped", "row_dropped", "swapped"):
        ok, bad = R.gradient_loss(a70), R.gradient_loss(a70, defect=defect)
        _caught(lambda: R.check_value(defect, bad.numpy(), ok.numpy(), bd["loss_gradl"]))
    (g_ok,), (g_bad,) = R.grad_of(R.gradient_loss, a70), R.grad_of(lambda x: R.gradient_loss(x, defect="row_dropped"), a70)
    _caught(lambda: R.check_grad("row_dropped", g_bad.numpy(), g_ok.numpy(), bd["grad_gradl"]))
    # reconstruction: abs added to l1, eps ignored (both eps), one element dropped
    for kind, eps, defect in (("l1", 1e-6, "l1_abs"), ("l_char", 1e-6, "eps_ignored"), ("l_char", 1e-3, "eps_ignored"), ("l2", 1e-6, "pixel_dropped"),
                              ("l_char", 1e-3, "pixel_dropped")):
        ok, bad = R.recon(a43, b43, kind, eps), R.recon(a43, b43, kind, eps, defect=defect)
        _caught(lambda: R.check_value(defect, bad.numpy(), ok.numpy(), bd["loss_recon"]))
    for kind, eps, defect in (("l1", 1e-6, "l1_abs"), ("l_char", 1e-3, "eps_ignored"), ("l_char", 1e-6, "eps_ignored")):
        (g_ok,), (g_bad,) = R.grad_of(lambda x: R.recon(x, b43, kind, eps), a43), R.grad_of(lambda x: R.recon(x, b43, kind, eps, defect=defect), a43)
        _caught(lambda: R.check_grad(defect, g_bad.numpy(), g_ok.numpy(), bd["grad_recon"]))
    # NaN is never within a bound
    _caught(lambda: R.check_value("nan", np.array([np.nan]), np.array([1.0]), 1.0))
    _caught(lambda: R.check_grad("nan", np.array([np.nan, 1.0]), np.array([1.0, 1.0]), 1.0))
    capsys.readouterr()
