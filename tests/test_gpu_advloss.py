"""GPU: the GAN-objective kernels (csrc/advloss.hip), their ops wrappers (ops.adv_loss, ops.cw_margin), the public modules
(loss.AdversarialLoss, models.modules.loss.GANLoss / CWLoss) and the literal step's train.gan_type, against the float64 restatement
(tests/advloss_restate.py).

Tolerances: nothing is chosen here.  For every case the fixture (tests/golden/advloss.npz) holds the deviation of the REFERENCE's own float32
CPU result from the float64 restatement on the same inputs -- one figure for the loss, one per element for the gradient.  The bound is
4 x that deviation with a floor of 2 float32 ulp of the value (advloss_restate.bound); a gradient asked with an upstream factor k scales
the recorded deviation by |k|.  The Carlini-Wagner gradient (entries 0, +-1/2, +-1) and every planted branch point are compared exactly.
Every figure is printed before it is asserted.

The reference's own float32-vs-float64 deviations (tests/golden/make_golden_advloss.py; the largest per family, the loss relative to its
value, the gradient relative to max |grad64|) and what the rule makes of them.  The per-case figures in the fixture are what is asserted:

    family                                        reference's deviation      bound (4 x, floor 2 ulp = 2.4e-7 relative at most)
    element objectives, loss   (78 cases)         1.28e-7 (-mean(x), n 1027)  5.13e-7;  a case the reference hits exactly: 2 ulp
    element objectives, gradient per element      1.42e-7 (bce_logits)        5.67e-7 of max |grad|, per element from its own deviation
    masked labels, loss        (20 cases)         1.35e-7                     5.40e-7
    masked labels, gradient per element           8.92e-7 (nsgan, x near 1)   3.57e-6 of max |grad|
    Carlini-Wagner margin, loss (16 cases)        6.23e-8                     2.49e-7
    Carlini-Wagner margin, gradient               0 (exact)                   compared exactly
The kernels evaluate every element in double and round once, so they are expected within 1 ulp, inside every bound.  The kernels' own
figures on the MI355X have NOT been recorded here yet: no GPU could be had while this was written (the test prints them).
"""
import numpy as np
import pytest
import torch

import advloss_restate as R
import detgen

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g(golden):
    return golden("advloss")


def _np(t):
    return t.detach().cpu().double().numpy()


def _dev(v):
    return torch.full((1,), float(v), device="cuda")


_WANT = {}


def _want(key, fn):
    """the float64 restatement of a case, computed once"""
    if key not in _WANT:
        _WANT[key] = fn()
    return _WANT[key]


def _offset_view(a, off):
    """a's values in a contiguous CUDA view that starts `off` elements past a 16-byte boundary"""
    a = torch.as_tensor(a)
    store = torch.zeros(a.numel() + 4, device="cuda", dtype=a.dtype)
    v = store[off:off + a.numel()].view(a.shape)
    v.copy_(a)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


@pytest.mark.parametrize("variant", tuple(R.VARIANTS))
def test_element_objectives_against_float64(g, variant):
    """every size (scalar only, head / body / tail, more than one block's stride), x aligned and offset by one element, the gradient buffer
    aligned with x and not (the all-scalar path), accumulation with a host, a device and an upstream factor"""
    from video_watermarking_forgery_detection_amd import ops
    objective, label, family, _ = R.VARIANTS[variant]
    lab = None if label is None else R.f32(label)
    k = 0.75 * 1024.0 * -1.5
    for n in R.SIZES:
        case = "%s_n%d" % (variant, n)
        x = g["x_%s_n%d" % (family, n)]
        loss64, grad64 = _want(case, lambda: R.adv_loss(objective, x, lab))
        for off in (0, 1):
            what = "%s offset %d" % (case, off)
            xd = _offset_view(x, off)
            loss = ops.adv_loss(xd, objective, label)
            assert loss.shape == (1,) and loss.dtype == torch.float32
            R.check(what + " loss", _np(loss)[0], loss64, g[case + "_dev_loss"])
            l2, grad = ops.adv_loss(xd, objective, label, want_grad=True)
            assert torch.equal(l2, loss) and grad.shape == xd.shape
            R.check(what + " grad", _np(grad), grad64, g[case + "_dev_grad"])
            base = (detgen.uniform((n,), 70 + n, lo=-1.0, hi=1.0) * float(np.abs(k * grad64).max())).float()
            buf = _offset_view(base, 1 - off if n > 3 else off)
            l3, acc = ops.adv_loss(xd, objective, label, want_grad=True, gscale=0.75, gscale_dev=_dev(1024.0), gout=_dev(-1.5), grad_out=buf)
            assert acc.data_ptr() == buf.data_ptr() and torch.equal(l3, loss)
            R.check(what + " accumulate", _np(buf), base.double().numpy() + k * grad64, g[case + "_dev_grad"], scale=k)
    # the planted branch points: a gradient that is exactly 0 in the restatement is exactly 0 here (x == t of bce_prob, the hinge's kink)
    gr = _np(ops.adv_loss(torch.from_numpy(g["x_%s_n257" % family]).cuda(), objective, label, want_grad=True)[1])
    want = R.adv_loss(objective, g["x_%s_n257" % family], lab)[1]
    assert np.array_equal(gr == 0.0, want == 0.0)
    if family == "prob" and label in (0.0, 1.0):
        assert want[int(label)] == 0.0 and abs(want[1 - int(label)]) == 1.0 / R.BCE_EPS / 257      # x == t; the 1e-12 denominator
    if family == "hinge":
        assert want[0 if label > 0 else 1] == 0.0 and want[2] != 0.0


@pytest.mark.parametrize("case", tuple(R.MASK_CASES))
def test_masked_labels_against_float64(g, case):
    """the bilinear sample inside the loss kernel: down, up, identity, a mask per channel and one broadcast over the channels"""
    from video_watermarking_forgery_detection_amd import loss as loss_mod, ops
    shape, kind, typ = R.MASK_CASES[case]
    objective = "bce_prob" if typ == "nsgan" else "mse"
    o, m = g[case + "_out"], g[case + "_mask"]
    loss64, grad64 = _want(case, lambda: R.adv_loss(objective, o, R.masked_labels(m, o.shape, R.MASK_REAL_LABEL)))
    od, md = torch.from_numpy(o).cuda(), torch.from_numpy(m).cuda()
    loss, grad = ops.adv_loss(od, objective, mask=md, real_label=R.MASK_REAL_LABEL, want_grad=True)
    R.check(case + " loss", _np(loss)[0], loss64, g[case + "_dev_loss"])
    R.check(case + " grad", _np(grad), grad64.reshape(o.shape), g[case + "_dev_grad"])
    # the module: the mask counts only when not is_real, and no gradient reaches it
    mod = loss_mod.AdversarialLoss(typ, R.MASK_REAL_LABEL, 0.0).cuda()
    x, mk = od.clone().requires_grad_(True), md.clone().requires_grad_(True)
    out = mod(x, False, True, mask=mk)
    assert out.shape == () and torch.equal(out.detach().reshape(1), loss)
    out.backward()
    assert torch.equal(x.grad, grad) and mk.grad is None
    assert torch.equal(mod(od, True, True, mask=md), mod(od, True, True)) and torch.equal(mod(od, True, True).reshape(1),
                                                                                          ops.adv_loss(od, objective, R.MASK_REAL_LABEL))


@pytest.mark.parametrize("case", tuple(R.CW_CASES))
def test_cw_margin_against_float64(g, case):
    """the loss within the bound; the gradient EXACTLY (clamped rows, the tie at kappa, equal maxima, `other` at the target's own slot)"""
    from video_watermarking_forgery_detection_amd import ops
    B, K, targeted, kappa = R.CW_CASES[case]
    z, t = g[case + "_logits"], g[case + "_target"]
    loss64, grad64 = _want(case, lambda: R.cw_margin(z, t, targeted, kappa))
    for off in (0, 1):
        zd, td = _offset_view(z, off), torch.from_numpy(t).cuda()
        loss = ops.cw_margin(zd, td, targeted, kappa)
        assert loss.shape == (1,)
        R.check("%s offset %d loss" % (case, off), _np(loss)[0], loss64, g[case + "_dev_loss"])
        l2, grad = ops.cw_margin(zd, td, targeted, kappa, want_grad=True)
        assert torch.equal(l2, loss) and np.array_equal(_np(grad), grad64)
    base = detgen.uniform((B, K), 90 + K, lo=-1.0, hi=1.0).float()
    buf = base.cuda()
    _, acc = ops.cw_margin(zd, td, targeted, kappa, want_grad=True, gscale=0.5, gscale_dev=_dev(4.0), gout=_dev(-1.5), grad_out=buf)
    assert acc.data_ptr() == buf.data_ptr()
    R.check(case + " accumulate", _np(buf), base.double().numpy() - 3.0 * grad64, g[case + "_dev_grad"], scale=-3.0)


def test_cw_margin_target_out_of_range_and_argument_errors():
    """a target outside [0, K) is never used as an index: the loss and that row's gradient are NaN, every other row is as it should be;
    check_target=True raises on the host instead"""
    from video_watermarking_forgery_detection_amd import ops
    from video_watermarking_forgery_detection_amd.models.modules.loss import CWLoss
    z = detgen.normal((5, 6), 11, std=3.0)
    good = torch.tensor([0, 5, 2, 3, 1])
    _, want = R.cw_margin(z.numpy(), good.numpy(), True, 0.0)
    for bad_row, bad in ((1, 6), (3, -1), (0, 2 ** 40), (4, -2 ** 62)):
        t = good.clone()
        t[bad_row] = bad
        loss, grad = ops.cw_margin(z.cuda(), t.cuda(), True, 0.0, want_grad=True)
        torch.cuda.synchronize()
        gr = _np(grad)
        ok = [r for r in range(5) if r != bad_row]
        assert np.isnan(_np(loss)[0]) and np.isnan(gr[bad_row]).all() and np.array_equal(gr[ok], want[ok])
        with pytest.raises(ValueError, match=r"target outside \[0, 6\)"):
            ops.cw_margin(z.cuda(), t.cuda(), True, 0.0, check_target=True)
        assert torch.isnan(CWLoss()(z.cuda(), t.cuda(), False, num_classes=6))
    assert torch.isfinite(ops.cw_margin(z.cuda(), good.cuda(), True, 0.0, check_target=True)).all()
    with pytest.raises(ValueError, match="K >= 2"):
        ops.cw_margin(z.cuda()[:, :1].contiguous(), torch.zeros(5, dtype=torch.int64, device="cuda"), True)
    with pytest.raises(ValueError, match="num_classes = 1000, but logits has 6 columns"):
        CWLoss()(z.cuda(), good.cuda(), True)
    with pytest.raises(TypeError, match="int64"):
        ops.cw_margin(z.cuda(), good.int().cuda(), True)
    with pytest.raises(TypeError, match="contiguous float32"):
        ops.cw_margin(z.cuda().double(), good.cuda(), True)


def test_op_argument_errors():
    from video_watermarking_forgery_detection_amd import ops
    x, m = torch.rand(2, 1, 4, 4, device="cuda"), torch.rand(2, 1, 8, 8, device="cuda")
    for kw, err, match in ((dict(objective="hinge_disc", label=0.5), ValueError, "hinge_disc takes the sign"),
                           (dict(objective="hinge_disc", label=1.0, mask=m), ValueError, "hinge_disc takes the sign"),
                           (dict(objective="neg_mean", label=1.0), ValueError, "neither a label nor a mask"),
                           (dict(objective="mse"), ValueError, "needs a scalar label or a mask"),
                           (dict(objective="mse", label=1.0, mask=m), ValueError, "not both"),
                           (dict(objective="mse", mask=m[:1]), ValueError, "masked labels need"),
                           (dict(objective="mse", mask=m.expand(2, 3, 8, 8).contiguous()), ValueError, "masked labels need"),
                           (dict(objective="mse", label=1.0, grad_out=torch.zeros_like(x)), ValueError, "need want_grad"),
                           (dict(objective="bce_logits", label=1.0, mask=None, want_grad=True, grad_out=torch.zeros(3, device="cuda")), AssertionError, ""),
                           (dict(objective="lsgan", label=1.0), ValueError, "objective must be one of")):
        with pytest.raises(err, match=match):
            ops.adv_loss(x, **kw)
    with pytest.raises(TypeError, match="contiguous float32"):
        ops.adv_loss(x[..., ::2], "mse", 1.0)
    with pytest.raises(TypeError, match="contiguous float32"):
        ops.adv_loss(x.double(), "mse", 1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.adv_loss(x, "mse", mask=m.cpu())
    # a probability outside [0, 1] is not hidden: NaN
    assert torch.isnan(ops.adv_loss(torch.tensor([0.5, 1.5], device="cuda"), "bce_prob", 1.0))


def test_modules_under_autograd_give_the_op_level_results(g):
    from video_watermarking_forgery_detection_amd import loss as loss_mod, ops
    from video_watermarking_forgery_detection_amd.models.modules.loss import CWLoss, GANLoss
    assert list(loss_mod.AdversarialLoss().state_dict().keys()) == list(g["adv_state_dict_keys"])
    n = 257
    for variant, (objective, label, family, (cls, typ, labels, args)) in R.VARIANTS.items():
        case = "%s_n%d" % (variant, n)
        x64 = g["x_%s_n%d" % (family, n)]
        loss64, grad64 = _want(case, lambda: R.adv_loss(objective, x64, None if label is None else R.f32(label)))
        mod = (loss_mod.AdversarialLoss(typ, *labels) if cls == "adv" else GANLoss(typ, *labels)).cuda()
        xd = torch.from_numpy(x64).cuda().reshape(1, 1, 1, n)
        x = xd.clone().requires_grad_(True)
        out = mod(x * 1.0, *args)              # a non-leaf input and a scaled result
        assert out.shape == () and torch.equal(out.detach().reshape(1), ops.adv_loss(xd, objective, label))
        R.check(variant + " module loss", float(out), loss64, g[case + "_dev_loss"])
        (out * 2.0).backward()
        R.check(variant + " module grad", _np(x.grad).reshape(-1), 2.0 * grad64, g[case + "_dev_grad"], scale=2.0)
    case = "cw_65x7_t_k0.5"
    z, t = torch.from_numpy(g[case + "_logits"]).cuda().requires_grad_(True), torch.from_numpy(g[case + "_target"]).cuda()
    out = CWLoss()(z, t, True, num_classes=7, kappa=0.5)
    assert out.shape == () and torch.equal(out.detach().reshape(1), ops.cw_margin(z.detach(), t, True, 0.5))
    (2 * out).backward()          # the reference's trainers: 2 * criterion_adv(label_pred, label_GT, is_targeted)
    assert np.array_equal(_np(z.grad), 2.0 * R.cw_margin(g[case + "_logits"], g[case + "_target"], True, 0.5)[1])
    assert torch.equal(CWLoss()(z.detach(), t.int(), True, 7, 0.5), out.detach())      # target.long(), as the reference
    with pytest.raises(ValueError, match="nsgan, lsgan or hinge"):
        loss_mod.AdversarialLoss("wgan")
    with pytest.raises(NotImplementedError):
        GANLoss("hinge")
    with pytest.raises(RuntimeError, match="HIP path only"):
        loss_mod.AdversarialLoss()(torch.rand(1, 1, 2, 2), True, True)
    with pytest.raises(TypeError, match="float32"):
        GANLoss("gan")(torch.rand(1, 1, 2, 2, device="cuda").half(), True)


def test_two_runs_and_a_captured_run_are_bit_identical(g):
    """forward + gradient of every objective, the masked labels and the margin twice, then captured into one graph and replayed: the same
    bits (no atomics, a fixed reduction order), and nothing in the calls reads back to the host"""
    from video_watermarking_forgery_detection_amd import glayers, ops
    x = {f: torch.from_numpy(g["x_%s_n1027" % f]).cuda() for f in ("prob", "logit", "plain", "hinge")}
    o, m = (torch.from_numpy(g["mask_down_frac_nsgan" + k]).cuda() for k in ("_out", "_mask"))
    z, t = (torch.from_numpy(g["cw_65x7_u_k0.5" + k]).cuda() for k in ("_logits", "_target"))
    big = torch.sigmoid(detgen.normal((3, 1, 61, 67), 5, std=2.0)).cuda()      # three workgroups
    scale = _dev(4096.0)

    def run():
        res = []
        for objective, label, family, _ in R.VARIANTS.values():
            res += ops.adv_loss(x[family], objective, label, want_grad=True, gscale=0.5, gscale_dev=scale)
        res += ops.adv_loss(o, "bce_prob", mask=m, real_label=0.9, want_grad=True, gscale_dev=scale)
        res += ops.adv_loss(big, "bce_prob", 1.0, want_grad=True)
        res += ops.cw_margin(z, t, False, 0.5, want_grad=True, gscale_dev=scale)
        return tuple(res)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r1 = run()
        r2 = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for u, v in zip(r1, r2):
        assert torch.equal(u, v) and u.data_ptr() != v.data_ptr()
    step = glayers.CapturedStep(run)
    step.replay()
    torch.cuda.synchronize()
    for u, v in zip(r1, step.result):
        assert torch.equal(u, v)
    want = R.adv_loss("bce_prob", _np(big).astype(np.float32), 1.0)
    R.check("three workgroups loss", _np(r1[-4])[0], want[0], 0.0)
    R.check("three workgroups grad", _np(r1[-3]), want[1].reshape(big.shape), 0.0)


# ----------------------------------------------------------------------------- the literal step (train.gan_type), at tests/test_gpu_literal.py's size
def _literal(**train):
    from video_watermarking_forgery_detection_amd.models.IRNrhi_literal import IRNrhiLiteralModel
    torch.manual_seed(1)
    t = {"lr_D": 2e-4, "beta1": 0.9, "beta2": 0.999, "weight_decay_G": 0.01, "gradient_clipping": 1.0, "compute_dtype": "f32"}
    t.update(train)
    model = IRNrhiLiteralModel({"gpu_ids": [0], "is_train": True, "dist": False, "network": {"nc": [16, 32, 48, 64], "nb": 1}, "train": t})
    with torch.no_grad():
        model.localizer.BayarConv2D.weight.copy_(detgen.uniform((3, 3, 5, 5), 77).cuda() + 0.5)
    return model


def _steps(model, n=2, bs=2):
    logs = []
    for it in range(n):
        base = detgen.uniform((bs, 3, 32, 32), 500 + it)
        model.feed_data(([torch.clamp(base + 0.02 * q * detgen.normal((bs, 3, 32, 32), 600 + 10 * it + q), -0.1, 1.1) for q in range(6)], None))
        logs.append((model.optimize_parameters(it)[0], model.last["dis_loss"], model.last["l_simul_sum"]))
    return logs


def _weights(model):
    return [p.detach().clone() for net in (model.generator, model.localizer, model.discriminator) for p in net.state_dict().values()]


def test_gan_type_absent_is_the_step_as_it_was(monkeypatch):
    """no key and a key that is None (what a yml without it parses to): no advloss launch (the op is made to raise), the same logs and
    bit-identical weights after two steps"""
    from video_watermarking_forgery_detection_amd import ops

    def boom(*a, **k):
        raise AssertionError("an advloss kernel was launched without train.gan_type")
    monkeypatch.setattr(ops, "adv_loss", boom)
    a, b = _literal(), _literal(gan_type=None)
    assert a.adversarial_loss is None and b.adversarial_loss is None and a.gan_type is None
    la, lb = _steps(a), _steps(b)
    assert la == lb and [k for k, _ in la[-1][0]] == ['l_simul_bayar', 'FW_GAN', 'lQF', 'PSSIMU', 'qfsimu']
    assert "dis_real" not in a.last
    for pa, pb in zip(_weights(a), _weights(b)):
        assert torch.equal(pa, pb)
    with pytest.raises(ValueError, match="train.gan_type must be nsgan, lsgan or hinge"):
        _literal(gan_type="wgan-gp")


@pytest.mark.parametrize("gan_type", ("lsgan", "hinge"))
def test_gan_type_routes_the_adversarial_terms_and_replays_bit_for_bit(gan_type):
    """the logged adversarial values are the restatement of the objective on the step's OWN discriminator outputs.  Bounds: FW_GAN is one
    kernel result, double sums rounded once -> the rule's floor, 2 float32 ulp.  dis_loss = (real + fake) / 2 is formed by torch in float32
    from two such results: each term's floor halved, plus one rounding of the sum -> ulp(real) + ulp(fake) + ulp(dis_loss)"""
    a, b = _literal(gan_type=gan_type), _literal(gan_type=gan_type)
    assert a.adversarial_loss.type == gan_type
    la, lb = _steps(a), _steps(b)
    assert la == lb
    for pa, pb in zip(_weights(a), _weights(b)):
        assert torch.equal(pa, pb)
    logs, dis_loss, _ = la[-1]
    f = lambda k: a.last[k].cpu().numpy()  # noqa: E731
    if gan_type == "lsgan":
        real, fake, gen = R.adv_loss("mse", f("dis_real"), 1.0)[0], R.adv_loss("mse", f("dis_fake"), 0.0)[0], R.adv_loss("mse", f("gen_fake"), 1.0)[0]
    else:
        real, fake = R.adv_loss("hinge_disc", f("dis_real"), -1.0)[0], R.adv_loss("hinge_disc", f("dis_fake"), 1.0)[0]
        gen = R.adv_loss("neg_mean", f("gen_fake"))[0]
    R.check(gan_type + " FW_GAN", dict(logs)["FW_GAN"], gen, 0.0)
    want = (real + fake) / 2
    err, bound = abs(dis_loss - want), float(R.ulp32(real) + R.ulp32(fake) + R.ulp32(want))
    print("%s dis_loss: |got - want| %.3e (bound %.3e)" % (gan_type, err, bound))
    assert err <= bound
