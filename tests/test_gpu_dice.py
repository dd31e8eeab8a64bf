"""GPU: the Dice kernels (csrc/dice.hip), the ops wrappers, the public dice_loss module and the train.dice_weight term of the localiser,
against the float64 restatement (tests/dice_restate.py).

Tolerances: loss within 1e-6 relative, gradient within 2e-6 of max |grad|.  They come from the reference, not from the kernels: its own
float32 run deviates from its float64 run on the fixture's inputs by up to 5.6e-8 (loss) and 1.4e-7 of max |grad| (binary, p in {1, 2, 3},
the three reductions), 1.1e-7 and 4.0e-7 (multi-class, with and without an ignored class) -- tests/golden/dice.npz, dev_*_max_* --; the
bounds leave about 10 x (binary) and 4 x (multi-class gradient) for what legitimately differs: f32 products summed in double instead of an
f32 tree, f32 per-sample coefficients in the backward, expf instead of torch's exp.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import detgen
import dice_restate as R

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL = 1e-6, 2e-6
SMOOTHS = (1, 1e-3)


def _binary_case(golden, name):
    return R.big_case() if name == "big" else R.fixture_case(golden("dice"), name)


def _gout(B, seed):
    return detgen.uniform((B,), seed, lo=-1.5, hi=2.0)


def _check_loss(what, got, want):
    got, want = np.atleast_1d(got.detach().cpu().double().numpy()), np.atleast_1d(want.detach().double().numpy())
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = float(np.max(np.abs(got - want) / np.abs(want)))
    print("%s loss rel %.3e (bound %.1e)" % (what, d, LOSS_TOL))
    assert np.isfinite(got).all() and d <= LOSS_TOL, (what, d)


def _check_grad(what, got, want, base=None):
    """got (device f32) against want (float64); base: what the buffer held before an accumulating call"""
    got = got.detach().cpu().double()
    if base is not None:
        got = got - base.double()
    m = float(want.abs().max())
    d = float((got.reshape(want.shape) - want).abs().max()) / m
    print("%s grad %.3e of max |grad| = %.3e (bound %.1e)" % (what, d, m, GRAD_TOL))
    assert torch.isfinite(got).all() and m > 0 and d <= GRAD_TOL, (what, d)


@pytest.mark.parametrize("p", R.POWERS)
@pytest.mark.parametrize("case", ("b0", "b1", "big"))
def test_binary_op_against_float64(golden, case, p):
    """every reduction, smooth in {1, 1e-3}, the sigmoid chain on and off; reduction none takes a per-sample upstream gradient; then the
    device loss scale and accumulation into a non-zero buffer"""
    from video_watermarking_forgery_detection_amd import ops
    x, t = _binary_case(golden, case)
    B = x.shape[0]
    xd, td, x64, t64 = x.cuda(), t.cuda(), x.double(), t.double()
    for smooth in SMOOTHS:
        for red in R.REDUCTIONS:
            fn = lambda a: R.binary_dice(a, t64, smooth, p, red)  # noqa: E731
            what = "%s p%d %s smooth %g" % (case, p, red, smooth)
            loss, coef = ops.dice_binary_fwd(xd, td, smooth, p, red)
            assert loss.shape == ((B,) if red == "none" else (1,)) and coef.shape == (B, 2) and coef.dtype == torch.float64
            _check_loss(what, loss.reshape(-1) if red == "none" else loss[0], fn(x64))
            gout = _gout(B, 7 + p) if red == "none" else None
            g64 = R.grad_of(fn, x64, None if gout is None else gout.double())
            for chain in (False, True):
                g = ops.dice_binary_bwd(xd, td, coef, p, red, gout=None if gout is None else gout.cuda(), chain_sigmoid=chain)
                assert g.shape == xd.shape and g.dtype == torch.float32
                _check_grad(what + (" chain" if chain else ""), g, R.chain_sigmoid(g64, x64) if chain else g64)
    # the trainer's call: gscale, the device loss scale, accumulated into a buffer that already holds a gradient of the same size
    fn = lambda a: R.binary_dice(a, t64, 1, p, "mean")  # noqa: E731
    want = 0.5 * 1024.0 * R.chain_sigmoid(R.grad_of(fn, x64), x64)
    base = (detgen.uniform(tuple(x.shape), 31, lo=-1.0, hi=1.0) * float(want.abs().max())).float()
    buf = base.cuda()
    scale = torch.full((1,), 1024.0, device="cuda")
    loss, g = ops.dice_binary(xd, td, 1.0, p, "mean", want_grad=True, chain_sigmoid=True, gscale=0.5, gscale_dev=scale, grad_out=buf)
    assert g.data_ptr() == buf.data_ptr()
    _check_loss("%s p%d trainer call (unscaled)" % (case, p), loss[0], fn(x64))
    _check_grad("%s p%d accumulate, gscale 0.5 x device 1024" % (case, p), buf, want, base=base)
    loss2, none = ops.dice_binary(xd, td, 1.0, p, "mean", want_grad=False)
    assert none is None and torch.equal(loss2, loss)


def _offset_view(t):
    """t's values on the device in a [1:] view of a buffer one element longer: 4 bytes past a 16-byte boundary, contiguous"""
    buf = torch.empty(t.numel() + 1, device="cuda", dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("p", R.POWERS)
def test_binary_op_with_differently_aligned_tensors(p):
    """(3, 1, 30, 43): a sample is 1290 floats, so samples start 0, 8 and 0 bytes past a 16-byte boundary -- but in every tensor alike.  Here
    the prediction alone sits 4 bytes off: no element reaches a boundary in both tensors and the kernels must take every element singly.
    Then the converse: aligned inputs and a gradient buffer 4 bytes off, accumulated into"""
    from video_watermarking_forgery_detection_amd import ops
    x, t = R.gen_binary((3, 1, 30, 43), 90 + p)
    x64, t64 = x.double(), t.double()
    fn = lambda a: R.binary_dice(a, t64, 1, p, "mean")  # noqa: E731
    g64 = R.chain_sigmoid(R.grad_of(fn, x64), x64)
    xo, td = _offset_view(x), t.cuda()
    assert td.data_ptr() % 16 == 0
    loss, coef = ops.dice_binary_fwd(xo, td, 1, p, "mean")
    _check_loss("p%d prediction 4 bytes off" % p, loss[0], fn(x64))
    g = ops.dice_binary_bwd(xo, td, coef, p, "mean", chain_sigmoid=True)
    _check_grad("p%d prediction 4 bytes off" % p, g, g64)
    base = (detgen.uniform(tuple(x.shape), 33, lo=-1.0, hi=1.0) * float(g64.abs().max())).float()
    buf = _offset_view(base)
    xd = x.cuda()
    assert xd.data_ptr() % 16 == 0
    loss, coef = ops.dice_binary_fwd(xd, td, 1, p, "mean")
    _check_loss("p%d aligned" % p, loss[0], fn(x64))
    out = ops.dice_binary_bwd(xd, td, coef, p, "mean", chain_sigmoid=True, out=buf, accumulate=True)
    assert out.data_ptr() == buf.data_ptr()
    _check_grad("p%d gradient buffer 4 bytes off, accumulate" % p, buf, g64, base=base)


def _multi_case(golden, name):
    if name == "odd":   # neither H*W % 4 == 0 nor a whole tile: the scalar path of the plane kernels
        return R.gen_multi((2, 5, 30, 43), 77)
    return R.fixture_case(golden("dice"), name)


@pytest.mark.parametrize("p", R.POWERS)
@pytest.mark.parametrize("case", ("m0", "m1", "odd"))
def test_softmax_op_against_float64(golden, case, p):
    from video_watermarking_forgery_detection_amd import ops
    z, t = _multi_case(golden, case)
    B, C = z.shape[:2]
    zd, td, z64, t64 = z.cuda(), t.cuda(), z.double(), t.double()
    w = detgen.uniform((C,), 5, lo=0.25, hi=2.0)
    for smooth in SMOOTHS:
        for red in R.REDUCTIONS:
            for ig, weight in ((None, None), (1, None), (None, w), (C - 1, w)):
                fn = lambda a: R.dice(a, t64, None if weight is None else weight.double(), ig, smooth, p, red)  # noqa: E731
                what = "%s p%d %s smooth %g ignore %s%s" % (case, p, red, smooth, ig, " weighted" if weight is not None else "")
                wd = None if weight is None else weight.cuda()
                loss, coef = ops.dice_softmax_fwd(zd, td, smooth, p, red, ig, wd)
                assert loss.shape == ((B,) if red == "none" else (1,)) and coef.shape == (B * C, 2)
                _check_loss(what, loss.reshape(-1) if red == "none" else loss[0], fn(z64))
                gout = _gout(B, 11 + p) if red == "none" else None
                g = ops.dice_softmax_bwd(zd, td, coef, p, red, ig, wd, gout=None if gout is None else gout.cuda())
                _check_grad(what, g, R.grad_of(fn, z64, None if gout is None else gout.double()))
    fn = lambda a: R.dice(a, t64, None, 1, 1, p, "mean")  # noqa: E731
    want = 0.25 * 512.0 * R.grad_of(fn, z64)
    base = (detgen.uniform(tuple(z.shape), 32, lo=-1.0, hi=1.0) * float(want.abs().max())).float()
    buf = base.cuda()
    loss, g = ops.dice_softmax(zd, td, 1.0, p, "mean", ignore_index=1, gscale=0.25, gscale_dev=torch.full((1,), 512.0, device="cuda"), grad_out=buf)
    assert g.data_ptr() == buf.data_ptr()
    _check_loss("%s p%d softmax trainer-style call" % (case, p), loss[0], fn(z64))
    _check_grad("%s p%d softmax accumulate" % (case, p), buf, want, base=base)


def test_class_limit_and_argument_errors():
    from video_watermarking_forgery_detection_amd import ops
    z, t = R.gen_multi((1, 33, 8, 8), 3)
    with pytest.raises(RuntimeError, match=r"wm_dice_softmax_sums failed \(rc=-1\)"):
        ops.dice_softmax_fwd(z.cuda(), t.cuda())
    z, t = R.gen_multi((1, 32, 8, 8), 3)
    loss, _ = ops.dice_softmax(z.cuda(), t.cuda())
    _check_loss("32 classes", loss[0], R.dice(z.double(), t.double()))
    x, y = R.gen_binary((2, 1, 8, 8), 4)
    with pytest.raises(RuntimeError, match=r"wm_dice_sums failed \(rc=-1\)"):
        ops.dice_binary_fwd(x.cuda(), y.cuda(), pw=0.0)
    with pytest.raises(ValueError, match="accumulate needs the buffer"):
        ops.dice_binary_bwd(x.cuda(), y.cuda(), torch.ones(2, 2, device="cuda", dtype=torch.float64), accumulate=True)


def test_refusal_raises_from_the_checked_handle_and_the_next_call_runs():
    """33 classes, one past the kernel's 32: the library refuses the arguments before it launches anything, the checked handle ops calls
    through raises with the refusing function's name, and the same op on 2 classes directly afterwards gives a finite loss -- on the release
    build and on the debug build's checked twin alike"""
    from video_watermarking_forgery_detection_amd import _lib, ops

    def refused_then_served():
        z, t = R.gen_multi((1, 33, 2, 2), 3)
        with pytest.raises(RuntimeError, match="wm_dice_softmax_sums"):
            ops.dice_softmax_fwd(z.cuda(), t.cuda())
        z, t = R.gen_multi((1, 2, 2, 2), 3)
        loss, _ = ops.dice_softmax_fwd(z.cuda(), t.cuda())
        assert loss.shape == (1,) and torch.isfinite(loss).all()
    refused_then_served()
    with _lib.use_debug_library():
        refused_then_served()


def test_modules_under_autograd_give_the_op_level_results(golden):
    from video_watermarking_forgery_detection_amd import dice_loss, ops
    x, t = R.fixture_case(golden("dice"), "b1")
    xd, td = x.cuda(), t.cuda()
    B = x.shape[0]
    for p in R.POWERS:
        for red in R.REDUCTIONS:
            a = xd.clone().requires_grad_(True)
            loss = dice_loss.BinaryDiceLoss(smooth=1e-3, p=p, reduction=red)(a, td)
            assert loss.shape == ((B,) if red == "none" else ())
            gout = _gout(B, 3).cuda() if red == "none" else None
            (loss if gout is None else (loss * gout).sum()).backward()
            l_op, coef = ops.dice_binary_fwd(xd, td, 1e-3, p, red)
            assert torch.equal(loss.detach().reshape(-1), l_op.reshape(-1))
            assert torch.equal(a.grad, ops.dice_binary_bwd(xd, td, coef, p, red, gout=gout))
            fn = lambda v: R.binary_dice(v, t.double(), 1e-3, p, red)  # noqa: E731
            _check_loss("module binary p%d %s" % (p, red), loss.reshape(-1) if red == "none" else loss, fn(x.double()))
            _check_grad("module binary p%d %s" % (p, red), a.grad, R.grad_of(fn, x.double(), None if gout is None else gout.cpu().double()))
    # a non-leaf prediction: the gradient flows on through torch's sigmoid
    zl = detgen.normal(tuple(x.shape), 9, std=2.0)
    a = zl.cuda().requires_grad_(True)
    dice_loss.BinaryDiceLoss()(torch.sigmoid(a), td).backward()
    want = R.grad_of(lambda v: R.binary_dice(torch.sigmoid(v), t.double()), zl.double())
    _check_grad("module binary through torch.sigmoid", a.grad, want)

    z, y = R.fixture_case(golden("dice"), "m0")
    zd, yd = z.cuda(), y.cuda()
    w = np.array([0.5, 2.0, 1.0, 0.25], dtype=np.float32)
    for ig, weight in ((None, None), (1, None), (2, w), (None, torch.from_numpy(w))):
        for red in R.REDUCTIONS:
            a = zd.clone().requires_grad_(True)
            loss = dice_loss.DiceLoss(weight=weight, ignore_index=ig, reduction=red, smooth=1, p=2)(a, yd)
            assert loss.shape == ((z.shape[0],) if red == "none" else ())
            loss.sum().backward()
            w64 = None if weight is None else torch.as_tensor(weight).double()
            fn = lambda v: R.dice(v, y.double(), w64, ig, 1, 2, red)  # noqa: E731
            what = "module multi-class ignore %s weight %s %s" % (ig, weight is not None, red)
            _check_loss(what, loss.reshape(-1) if red == "none" else loss, fn(z.double()))
            _check_grad(what, a.grad, R.grad_of(fn, z.double()))
            l_op, g_op = ops.dice_softmax(zd, yd, 1, 2, red, ignore_index=ig, weight=None if weight is None else torch.as_tensor(weight).cuda())
            assert torch.equal(loss.detach().reshape(-1), l_op.reshape(-1))
            if red != "none":      # (none: autograd hands a vector of ones, the op-level call no vector: the same numbers)
                assert torch.equal(a.grad, g_op)
    oh = dice_loss.make_one_hot(y.argmax(1, keepdim=True).cuda(), 4)
    assert torch.equal(oh, y)


def test_two_runs_and_a_captured_run_are_bit_identical():
    """forward + backward of the 16 x 1 x 256 x 256 case twice, then captured into a graph and replayed: the same bits (no atomics, a fixed
    reduction order), and nothing in the calls reads back to the host"""
    from video_watermarking_forgery_detection_amd import glayers, ops
    x, t = R.big_case()
    xd, td = x.cuda(), t.cuda()
    scale = torch.full((1,), 4096.0, device="cuda")

    def run():
        return ops.dice_binary(xd, td, 1.0, 2.0, "mean", want_grad=True, chain_sigmoid=True, gscale=0.5, gscale_dev=scale)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        l1, g1 = run()
        l2, g2 = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and l1.data_ptr() != l2.data_ptr()
    z, y = R.gen_multi((4, 3, 64, 64), 201)
    s1, s2 = (ops.dice_softmax(z.cuda(), y.cuda(), ignore_index=1) for _ in range(2))
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1])
    step = glayers.CapturedStep(run)
    step.replay()
    torch.cuda.synchronize()
    lg, gg = step.result
    assert torch.equal(lg, l1) and torch.equal(gg, g1)


# ----------------------------------------------------------------------------- the trainer (models/IRNrhi_model.py, train.dice_weight)
def _model(tmp_path, tag, size=32, **train):
    from video_watermarking_forgery_detection_amd.models.IRNrhi_model import IRNrhiModel
    from video_watermarking_forgery_detection_amd.options.options import dict_to_nonedict
    t = {"compute_dtype": "f32", "attacks": ["JpegSS50", "GaussianBlur"], "lr_G": 1e-3, "manual_seed": 10, "save_interval": 3000,
         "localizer": True, "gradient_clipping": 1.0}
    t.update(train)
    torch.manual_seed(0)
    m = IRNrhiModel(dict_to_nonedict({"gpu_ids": [0], "dist": False, "is_train": True, "datasets": {"train": {"GT_size": size, "batch_size": 2}},
                                      "train": t, "path": {"models": str(tmp_path / tag / "models"), "training_state": str(tmp_path / tag / "state")}}))
    for net in (m.netG.encoder, m.netG.decoder, m.discriminator, m.localizer):
        detgen.fill_module(net)
    return m


def _feed(m, step, size=32):
    mask = torch.zeros(2, 1, size, size)
    mask[0, :, 4:size // 2, 6:20] = 1
    mask[1, :, size // 2:size - 3, 2:9] = 1
    m.feed_data({"GT": detgen.uniform((2, 3, size, size), 500 + step), "mask": mask, "messages": detgen.bits((2, 30), 600 + step)})


def _run(m, steps=5, size=32):
    """two batches to fill the history, then steps - 2 trained steps -> the logs of the trained steps"""
    out = []
    for step in range(1, steps + 1):
        _feed(m, step, size)
        logs, _ = m.optimize_parameters(step, None)
        if step > 2:
            out.append(list(logs))
    return out


def test_dice_weight_zero_and_absent_are_the_step_as_it_was(tmp_path, monkeypatch):
    """dice_weight 0 and no dice_weight: no Dice launch (the op is made to raise), the same logs and bit-identical parameters after three
    trained steps.  (That these equal the step of the commit before the Dice term was checked once by running that commit's
    IRNrhi_model.py on the same feeds: DESIGN.md section 7.)"""
    from video_watermarking_forgery_detection_amd import ops

    def boom(*a, **k):
        raise AssertionError("a Dice kernel was launched with dice_weight off")
    for name in ("dice_binary", "dice_binary_fwd", "dice_binary_bwd"):
        monkeypatch.setattr(ops, name, boom)
    a, b = _model(tmp_path, "zero", dice_weight=0), _model(tmp_path, "absent")
    assert a.dice_weight == 0.0 and b.dice_weight == 0.0
    la, lb = _run(a), _run(b)
    assert len(la) == 3 and la == lb
    names = [k for k, _ in la[0]]
    assert "Dice" not in names and names[names.index("CE") + 1] == "Kind"
    for pa, pb in zip(list(a.netG.parameters()) + [a.localizer.flat_params], list(b.netG.parameters()) + [b.localizer.flat_params]):
        assert torch.equal(pa, pb)


def test_dice_weight_joins_the_bce_gradient_and_is_logged(tmp_path):
    from video_watermarking_forgery_detection_amd import ops
    from video_watermarking_forgery_detection_amd.models.IRNrhi_model import DeferredLogs
    m = _model(tmp_path, "half", dice_weight=0.5)
    off = _model(tmp_path, "off")
    assert m.dice_weight == 0.5
    m.keep_outputs = True
    seen = []
    inner = m.localizer.bwd

    def spy(ctx, g_out, *a, **k):
        seen.append(g_out.detach().clone())
        return inner(ctx, g_out, *a, **k)
    m.localizer.bwd = spy
    for step in range(1, 4):
        _feed(m, step)
        logs, _ = m.optimize_parameters(step, None)
        _feed(off, step)
        logs_off, _ = off.optimize_parameters(step, None)
    names = [k for k, _ in logs]
    assert names[names.index("CE") + 1] == "Dice" and names[names.index("Dice") + 1] == "Kind"
    assert [k for k in names if k != "Dice"] == [k for k, _ in logs_off]
    d, d_off = dict(logs), dict(logs_off)
    # the first trained step starts from the same parameters: the BCE value is the run's without the Dice term
    assert d["CE"] == d_off["CE"] and isinstance(d["Dice"], float)
    pred, mask = m.last_outputs["pred"], m.mask
    want = R.binary_dice(pred.cpu().double(), mask.cpu().double())
    rel = abs(d["Dice"] - float(want)) / float(want)
    print("logged Dice %.9g restatement %.9g rel %.3e" % (d["Dice"], float(want), rel))
    assert rel <= LOSS_TOL and 0 < d["Dice"] < 1
    assert len(seen) == 1 and seen[0].shape == pred.shape
    _, g_bce = ops.bce_logits_target(pred, mask, m.localizer_weight, chain_sigmoid=True)
    _, g_dice = ops.dice_binary(pred, mask, 1.0, 2.0, "mean", chain_sigmoid=True)
    want_g = g_bce.cpu().double() + 0.5 * g_dice.cpu().double()
    _check_grad("gradient handed to the UNet backward", seen[0], want_g.reshape(pred.shape))
    assert float((0.5 * g_dice).abs().max()) > 1e-3 * float(g_bce.abs().max())     # the Dice part is not lost in the tolerance
    # deferred logs: the same list, read later
    e, f = _model(tmp_path, "now", dice_weight=0.5, deferred_logs=False), _model(tmp_path, "later", dice_weight=0.5, deferred_logs=True)
    le, lf = _run(e, 4), _run(f, 4)
    assert le == lf and all("Dice" in dict(x) for x in le)
    _feed(f, 5)
    assert isinstance(f.optimize_parameters(5, None)[0], DeferredLogs)


def test_f16_step_with_the_device_scaler_logs_the_unscaled_dice(tmp_path):
    from video_watermarking_forgery_detection_amd import ops
    m = _model(tmp_path, "f16", size=64, compute_dtype="f16", dice_weight=0.5)
    assert m.amp is not None
    m.keep_outputs = True
    w0 = m.localizer.flat_params.clone()
    logs = _run(m, 6, size=64)
    assert len(logs) == 4
    d = dict(logs[-1])
    pred, mask = m.last_outputs["pred"], m.mask
    loss, _ = ops.dice_binary(pred, mask, 1.0, 2.0, "mean", want_grad=False)
    want = float(R.binary_dice(pred.cpu().double(), mask.cpu().double()))
    print("f16: logged Dice %.9g, f32 loss of its pred %.9g, restatement %.9g, loss scale %g" % (d["Dice"], float(loss), want, m.amp.get_scale()))
    assert m.amp.get_scale() >= 1024.0                       # the scale is far from 1: a scaled loss could not equal the unscaled one
    assert d["Dice"] == float(loss) and abs(d["Dice"] - want) <= LOSS_TOL * want
    assert all(np.isfinite(v) for x in logs for v in dict(x).values() if isinstance(v, float))
    assert not torch.equal(w0, m.localizer.flat_params) and torch.isfinite(m.localizer.flat_params).all()
    for p in m.netG.parameters():
        assert torch.isfinite(p).all()
    assert m.amp.step_count(m.optimizer_localizer.amp_slot) >= 1
