"""GPU: the SSIM / PSNR / confusion-count kernels (csrc/ssim.hip), the public pytorch_ssim / metrics modules, the SSIM fidelity term of the
training step and the evaluation report, against the float64 restatement (tests/metrics_restate.py).

Tolerances come from the reference, not from the kernels: tests/golden/metrics.npz stores, per fixture case, how far the reference's own
float32 run is from its float64 run.  Value bound = 4 x the largest such deviation (batch mean / per-image mean); gradient bound =
4 x the largest N * max |g32 - g64| (N = B C H W: the gradient of the map's sum).  The factor 4 covers what legitimately differs from the
reference: separable instead of 2-D window summation, FMA contraction, another reduction tree.  Measured kernel deviations: DESIGN.md section 7.
Host reads are counted with torch.cuda.set_sync_debug_mode("error") around evaluate_on_batch."""
import numpy as np
import pytest
import torch

import detgen
import metrics_restate as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bounds(golden):
    g = golden("metrics")
    def mx(k):
        return max(float(g["s%d_%s_%s" % (i, kind, k)]) for i in range(4) for kind in R.KINDS)
    b = {"mean": 4 * mx("dev_mean"), "img": 4 * mx("dev_img"), "grad": 4 * mx("dev_grad")}
    print("bounds", b)
    return b


_REF = {}


def _ref64(si, kind):
    """float64 restatement of one case: values, and the gradients wrt either image of the mean and of sum(gout * per-image means)"""
    if (si, kind) not in _REF:
        x, y = R.case_inputs(si, kind)
        x64, y64 = x.double(), y.double()
        gout = R.case_gout(si)
        with torch.no_grad():
            r = {"mean": float(R.ssim(x64, y64, True)), "img": R.ssim(x64, y64, False).numpy()}
        for wrt in (0, 1):
            r["g_mean%d" % wrt] = R.ssim_autograd(x64, y64, True, wrt=wrt)
            r["g_img%d" % wrt] = R.ssim_autograd(x64, y64, False, gout=gout.double(), wrt=wrt)
        _REF[(si, kind)] = r
    return _REF[(si, kind)]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("si", range(4))
def test_ssim_forward(bounds, si, kind):
    from video_watermarking_forgery_detection_amd import ops
    x, y = (t.cuda() for t in R.case_inputs(si, kind))
    r = _ref64(si, kind)
    m = float(ops.ssim(x, y, True))
    im = ops.ssim(x, y, False).cpu().double().numpy()
    dm, di = abs(m - r["mean"]), float(np.abs(im - r["img"]).max())
    print("ssim fwd", R.SHAPES[si], kind, "d mean %.3e (bound %.3e)  d img %.3e (bound %.3e)" % (dm, bounds["mean"], di, bounds["img"]))
    assert dm <= bounds["mean"] and di <= bounds["img"]
    if kind == "equal":
        assert abs(m - 1.0) <= bounds["mean"] and np.abs(im - 1.0).max() <= bounds["img"]
    m2, dpl = ops.ssim(x, y, True, want_grad=True)   # the planes' forward is the same forward
    assert float(m2) == m and dpl.shape == (3,) + tuple(x.shape)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("si", range(4))
def test_ssim_backward(bounds, si, kind):
    """both arguments, mean and per-image upstream; then accumulate with a device gradient scale: the accumulated result is
    buf + (the scaled gradient), to 1 ulp of the result (the kernel's add may contract into an FMA)"""
    from video_watermarking_forgery_detection_amd import ops
    x, y = (t.cuda() for t in R.case_inputs(si, kind))
    n = x.numel()
    B = x.shape[0]
    r = _ref64(si, kind)
    gout = R.case_gout(si).cuda()
    one = torch.ones(1, device="cuda")
    for wrt in (0, 1):
        a, b = (x, y) if wrt == 0 else (y, x)
        _, dpl = ops.ssim(a, b, True, want_grad=True)
        for mode, go, per in (("mean", one, False), ("img", gout, True)):
            g = ops.ssim_bwd(dpl, a, b, gout=go, per_image=per)
            ref = r["g_%s%d" % (mode, wrt)]
            d = n * float((g.cpu().double() - ref).abs().max())
            # the per-image weights of the fixture are <= 1.5 and each image's mean has B times the mean's weight per pixel: N there is C H W
            nd = d / B if per else d
            print("ssim bwd", R.SHAPES[si], kind, "wrt", wrt, mode, "N max|g - g64| %.3e (bound %.3e; gout <= 1.5: %.3e)" % (nd, bounds["grad"], 1.5 * bounds["grad"]))
            assert nd <= bounds["grad"] * (1.5 if per else 1.0)
            if kind == "equal":
                assert n * float(g.abs().max()) / (B if per else 1) <= bounds["grad"] * (1.5 if per else 1.0)
        sd = torch.full((1,), 0.5, device="cuda")
        plain = ops.ssim_bwd(dpl, a, b, gout=one, gscale=-0.25, gscale_dev=sd)
        ref = -0.125 * r["g_mean%d" % wrt]
        assert n * float((plain.cpu().double() - ref).abs().max()) <= 0.125 * bounds["grad"] + 1e-30
        buf = detgen.normal(tuple(x.shape), 9950 + si, std=1e-6).cuda()
        acc = ops.ssim_bwd(dpl, a, b, gout=one, gscale=-0.25, gscale_dev=sd, out=buf.clone(), accumulate=True)
        want = (buf.double() + plain.double()).cpu().numpy()
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(acc.cpu().double().numpy() - want) <= ulp)


def test_ssim_is_bitwise_reproducible():
    from video_watermarking_forgery_detection_amd import ops
    x, y = (t.cuda() for t in R.case_inputs(3, "near"))
    runs = []
    for _ in range(2):
        v, dpl = ops.ssim(x, y, True, want_grad=True)
        vi = ops.ssim(x, y, False)
        g = ops.ssim_bwd(dpl, x, y)
        runs.append((v.clone(), vi.clone(), dpl.clone(), g.clone()))
    for p, q in zip(*runs):
        assert torch.equal(p, q)


def test_public_ssim_autograd_both_arguments(bounds):
    from video_watermarking_forgery_detection_amd import pytorch_ssim
    si, kind = 1, "near"
    x, y = (t.cuda() for t in R.case_inputs(si, kind))
    r = _ref64(si, kind)
    n = x.numel()
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    v = pytorch_ssim.SSIM()(a, b)
    (-0.1 * v).backward()
    assert abs(float(v) - r["mean"]) <= bounds["mean"]
    for t, wrt in ((a, 0), (b, 1)):
        assert n * float((t.grad.cpu().double() + 0.1 * r["g_mean%d" % wrt]).abs().max()) <= 0.1 * bounds["grad"]
    a.grad = None
    gout = R.case_gout(si).cuda()
    vi = pytorch_ssim.ssim(a, y, size_average=False)
    assert vi.shape == (x.shape[0],)
    (vi * gout).sum().backward()
    assert n / x.shape[0] * float((a.grad.cpu().double() - r["g_img0"]).abs().max()) <= 1.5 * bounds["grad"]


@pytest.mark.parametrize("dtype", (torch.float32, torch.uint8))
def test_confusion_counts_exact(golden, dtype):
    from video_watermarking_forgery_detection_amd import metrics, ops
    g = golden("metrics")
    cases = [R.case_masks(si) for si in range(4)]
    B = 16
    gt = (detgen.uniform((B, 1, 256, 256), 9990) < 0.4).float()
    cases += [(torch.zeros_like(gt), torch.zeros_like(gt)), (torch.ones_like(gt), torch.ones_like(gt)), (torch.zeros_like(gt), gt),
              (torch.ones_like(gt), gt)]
    for ci, (pred, gt) in enumerate(cases):
        if dtype == torch.uint8:
            pred, thr = (pred > 0.5).to(torch.uint8) * 255, 127.0
        else:
            thr = 0.5
        c = ops.confusion_counts(pred.cuda(), gt.cuda(), thr, 0.5).cpu().numpy()
        want = np.array([R.confusion(pred[b].numpy(), gt[b].numpy(), thr, 0.5) for b in range(pred.shape[0])])
        assert c.dtype == np.int64 and np.array_equal(c[1:], want) and np.array_equal(c[0], want.sum(0)), ci
        TN, TP, FN, FP = (int(v) for v in c[0])
        if dtype == torch.float32:
            s = metrics.mask_scores(pred.cuda(), gt.cuda(), 0.5)
            ref = R.mask_scores(TN, TP, FN, FP)
            for k, v in ref.items():
                got = float(s[k])
                assert (np.isnan(v) and np.isnan(got)) or abs(got - v) <= np.spacing(abs(v)), (ci, k, got, v)
            prec, rec = metrics.EdgeAccuracy(0.5)(gt.cuda(), pred.cuda())
            rp, rr = R.edge_accuracy(gt, pred, 0.5)
            assert abs(float(prec) - float(rp)) <= np.spacing(np.float32(float(rp))) and abs(float(rec) - float(rr)) <= np.spacing(np.float32(float(rr)))
            if ci < 4:
                assert abs(float(prec) - float(g["m%d_prec" % ci])) <= np.spacing(np.float32(g["m%d_prec" % ci]))
    z = torch.zeros(1, 1, 8, 8, device="cuda")
    prec, rec = metrics.EdgeAccuracy()(z, z)
    assert float(prec) == 1.0 and float(rec) == 1.0


def test_psnr_against_restatement():
    """bound: the kernel sums (a - b)^2 in double and rounds the mean once (relative 6e-8); 10 log10 of that moves the result by < 3e-7 dB,
    the two logf calls and the float32 result each add an ulp of ~40 dB (4e-6): 2e-5 dB in all, against the float64 restatement"""
    from video_watermarking_forgery_detection_amd import metrics, ops
    for si in range(4):
        for kind in R.KINDS:
            x, y = R.case_inputs(si, kind)
            for mv, s in ((1.0, 1.0), (255.0, 255.0)):
                got = float(metrics.PSNR(mv)((s * x).cuda(), (s * y).cuda()))
                ref = float(R.psnr((s * x).double(), (s * y).double(), mv))
                print("psnr", R.SHAPES[si], kind, mv, got, ref)
                if kind == "equal":
                    assert got == 0.0 and ref == 0.0
                else:
                    assert abs(got - ref) <= (2e-5 if s == 1.0 else 4e-5)   # 255 x: the inputs' own float32 rounding doubles the mse error
    # psnr255 (the int-truncated form the literal step logs) is what it was
    x, y = R.case_inputs(2, "near")
    xi, yi = (255 * x.clamp(0, 1)).int().double(), (255 * y.clamp(0, 1)).int().double()
    want = 20 * np.log10(255.0) - 10 * np.log10(float(((xi - yi) ** 2).mean()))
    assert abs(float(ops.psnr255(x.cuda(), y.cuda())) - want) < 1e-3


# ----------------------------------------------------------------------------- the training step
def _hidden(H, noiser, w, dtype=torch.float32):
    from video_watermarking_forgery_detection_amd.hidden_models import Hidden
    from video_watermarking_forgery_detection_amd.options import HiDDenConfiguration
    h = Hidden(HiDDenConfiguration(H=H, W=H), torch.device("cuda"), noiser, None, compute_dtype=dtype, ssim_weight=w)
    for m in (h.encoder_decoder.encoder, h.encoder_decoder.decoder, h.discriminator):
        detgen.fill_module(m)
    return h


def _noiser(name):
    from video_watermarking_forgery_detection_amd.noise_layers import Identity, Jpeg
    return Identity() if name == "Identity" else Jpeg(50)


@pytest.mark.parametrize("nname", ("Identity", "Jpeg50"))
@pytest.mark.parametrize("B,H", ((2, 32), (16, 256)))
def test_step_gradient_gains_the_ssim_term(bounds, B, H, nname):
    """g_enc (the gradient of the generator's loss wrt the encoded image, read by an extra_encoded_grad callable that only clones it) at
    weight 0.1 differs from the weight-0 one by 0.1 * d(-SSIM(encoded, cover))/d encoded of the float64 restatement"""
    images, messages = detgen.uniform((B, 3, H, H), 2100), detgen.bits((B, 30), 2101)
    got = {}
    for w in (0.0, 0.1):
        h = _hidden(H, _noiser(nname), w)
        box = {}

        def grab(encoded, cover, g_enc):
            box["g"], box["enc"] = g_enc.clone(), encoded.clone()
            return []
        losses, _ = h.train_on_batch([images, messages], extra_encoded_grad=grab)
        got[w] = (box["g"], box["enc"], losses)
    assert torch.equal(got[0.0][1], got[0.1][1])        # the same first forward
    enc = got[0.1][1].cpu()
    g64 = R.ssim_autograd(enc.double(), images.double(), True, wrt=0)
    n = enc.numel()
    diff = (got[0.1][0].double() - got[0.0][0].double()).cpu()
    # g_enc is a float32 sum of O(1e-6..1e-3) terms: adding the SSIM gradient rounds at the sum's magnitude, one ulp of max |g_enc|
    ulp = float(np.spacing(np.float32(got[0.1][0].abs().max().item())))
    d = n * float((diff + 0.1 * g64).abs().max())
    print("step g_enc", B, H, nname, "N max|dg - 0.1 g64| %.3e (bound %.3e + N ulp %.3e)" % (d, 0.1 * bounds["grad"], n * ulp))
    assert d <= 0.1 * bounds["grad"] + n * ulp
    extra = dict(got[0.1][2]["_extra"])
    assert abs(float(extra["SSFW"]) - float(R.ssim(enc.double(), images.double()))) <= bounds["mean"]
    assert "_extra" not in got[0.0][2]
    for k in ('loss           ', 'encoder_mse    '):   # 'loss' keeps its three-term meaning
        assert got[0.0][2][k] == got[0.1][2][k]


def _run_steps(h, images, messages, steps):
    out = []
    for _ in range(steps):
        losses, (e, nz, d) = h.train_on_batch([images, messages])
        extra = losses.pop("_extra", [])
        out.append((np.array([losses[k] for k in sorted(losses)]), [float(v) for _, v in extra], e.clone(), d.clone()))
    torch.cuda.synchronize()
    flats = [m.flat_params.clone() for m in (h.encoder_decoder.encoder, h.encoder_decoder.decoder, h.discriminator)]
    return out, flats


@pytest.mark.parametrize("nname", ("Identity", "Jpeg50"))
@pytest.mark.parametrize("B,H,dtype", ((2, 32, torch.float32), (16, 256, torch.bfloat16)))
def test_step_with_term_captured_and_two_chain_equal_eager(B, H, dtype, nname):
    images, messages = detgen.uniform((B, 3, H, H), 2200).cuda(), detgen.bits((B, 30), 2201).cuda()
    runs = {}
    for mode in ("eager", "graph", "two", "two_graph"):
        h = _hidden(H, _noiser(nname), 0.1, dtype)
        h.two_streams = mode.startswith("two")
        if mode.endswith("graph"):
            h.enable_graph()
        runs[mode] = _run_steps(h, images, messages, 4 + (2 if mode.endswith("graph") else 0))
        if mode.endswith("graph"):
            g = next(iter(h._graphs.values()))
            assert g.graph is not None and g.failed is None
        assert len(runs[mode][0][0][1]) == 1          # SSFW is logged
    for mode in ("graph", "two", "two_graph"):
        for (la, xa, ea, da), (lb, xb, eb, db) in zip(runs["eager"][0][:4], runs[mode][0][:4]):
            assert np.array_equal(la, lb) and xa == xb and torch.equal(ea, eb) and torch.equal(da, db), mode
    for p, q in zip(runs["eager"][1], runs["two"][1]):
        assert torch.equal(p, q)
    for p, q in zip(runs["graph"][1], runs["two_graph"][1]):
        assert torch.equal(p, q)


@pytest.mark.parametrize("nname", ("Jpeg50", "Identity"))
def test_weight_zero_step_launches_no_ssim_kernel_and_matches_golden(golden, monkeypatch, nname):
    from video_watermarking_forgery_detection_amd import ops

    def boom(*a, **k):
        raise AssertionError("an SSIM kernel was launched at ssim_weight = 0")
    monkeypatch.setattr(ops, "ssim", boom)
    monkeypatch.setattr(ops, "ssim_bwd", boom)
    g = golden("step")
    h = _hidden(32, _noiser(nname), 0.0)
    images, messages = detgen.uniform((4, 3, 32, 32), 2000), detgen.bits((4, 30), 2001)
    keys = ("loss           ", "encoder_mse    ", "dec_mse        ", "bitwise-error  ", "adversarial_bce", "discr_cover_bce", "discr_encod_bce")
    for it in range(2):
        losses, _ = h.train_on_batch([images, messages])
        assert "_extra" not in losses
        np.testing.assert_allclose(np.array([losses[k] for k in keys]), g[f"step_{nname}/losses_it{it}"], rtol=5e-3 if it else 1e-3, atol=1e-4)
    for tag, m in (("wE", h.encoder_decoder.encoder), ("wDec", h.encoder_decoder.decoder), ("wD", h.discriminator)):
        diffs = []
        for n, p in m.state_dict().items():
            ref_w = g[f"step_{nname}/{tag}/{n}"]
            got_w = detgen.subsample(p.float(), 31).cpu().numpy()
            if n.endswith("num_batches_tracked"):
                assert np.array_equal(got_w, ref_w)
                continue
            d = np.abs(got_w - ref_w)
            assert d.max() <= 4e-3 + 1e-3 * np.abs(ref_w).max(), (tag, n)     # test_gpu_hidden.py::test_full_step_golden's bounds
            diffs.append(d)
        d = np.concatenate(diffs)
        assert d.mean() < 3e-4 and (d > 1e-3).mean() < 0.1


# ----------------------------------------------------------------------------- evaluation
def test_evaluate_on_batch_one_host_read(bounds):
    from video_watermarking_forgery_detection_amd.noise_layers import Identity, Jpeg
    B, H = 4, 64
    h = _hidden(H, Jpeg(50), 0.0)
    images, messages = detgen.uniform((B, 3, H, H), 2300).cuda(), detgen.bits((B, 30), 2301).cuda()
    h.train_on_batch([images, messages])     # running statistics and the pack plans exist
    noisers = [Identity(), Jpeg(50), Jpeg(90)]
    h.evaluate_on_batch([images, messages], noisers)   # warm: first-call allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        vals, names = h.evaluate_on_batch([images, messages], noisers)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    host = vals.tolist()          # the report's one device -> host read
    assert names == ["PSNR", "SSIM", "BER/Identity", "dec_mse/Identity", "BER/Jpeg50", "dec_mse/Jpeg50", "BER/Jpeg90", "dec_mse/Jpeg90"]
    rep = dict(zip(names, host))
    ed = h.encoder_decoder
    ed.eval()
    with torch.no_grad():
        enc, _ = ed.encoder.fwd(images, messages, training=False)
        assert abs(rep["PSNR"] - float(R.psnr(enc.cpu().double(), images.cpu().double(), 1.0))) <= 2e-5
        assert abs(rep["SSIM"] - float(R.ssim(enc.cpu().double(), images.cpu().double()))) <= bounds["mean"]
        for n in noisers:
            nz, _ = n.fwd(enc)
            dec, _ = ed.decoder.fwd(nz, training=False)
            dec = dec.float().cpu()
            ber = float((dec.round().clamp(0, 1) - messages.cpu()).abs().sum()) / (B * 30)
            assert abs(rep["BER/" + n.name] - ber) <= 1e-7          # k / 120 rounded to float32
            assert abs(rep["dec_mse/" + n.name] - float(((dec.double() - messages.cpu().double()) ** 2).mean())) <= 1e-6
    ed.train()


def _model(tmp_path, localizer, eval_metrics, size=64):
    from video_watermarking_forgery_detection_amd.models.IRNrhi_model import IRNrhiModel
    from video_watermarking_forgery_detection_amd.options.options import dict_to_nonedict
    torch.manual_seed(0)
    return IRNrhiModel(dict_to_nonedict({
        "gpu_ids": [0], "dist": False, "is_train": True, "datasets": {"train": {"GT_size": size, "batch_size": 4}},
        "train": {"compute_dtype": "f32", "attacks": ["Jpeg50", "GaussianBlur", "Crop"], "lr_G": 1e-3, "manual_seed": 10, "save_interval": 3000,
                  "localizer": localizer, "eval_metrics": eval_metrics},
        "path": {"models": str(tmp_path / "models"), "training_state": str(tmp_path / "state")}}))


def test_robustness_report_and_evaluate_keys(tmp_path):
    m = _model(tmp_path, True, False)
    B, S = 4, 64
    mask = torch.zeros(B, 1, S, S)
    mask[:, :, 16:40, 8:48] = 1
    for k in range(3):
        m.feed_data((detgen.uniform((B, 3, S, S), 2400 + k), mask))
        m.optimize_parameters(k)
    m.feed_data((detgen.uniform((B, 3, S, S), 2410), mask))
    logs, _ = m.evaluate()
    assert [k for k, _ in logs] == ["loss", "encoder_mse", "dec_mse", "bitwise-error", "adversarial_bce", "discr_cover_bce", "discr_encod_bce"]
    m.feed_data((detgen.uniform((B, 3, S, S), 2410), mask))
    msgs = detgen.bits((B, 30), 2411).cuda()
    rep = m.robustness_report(msgs)
    names = [k for k, _ in rep]
    for want in ("PSNR", "SSIM", "BER/Jpeg50", "BER/GaussianBlur", "BER/Crop", "F1/Jpeg50", "precision/Jpeg50", "recall/GaussianBlur"):
        assert want in names, (want, names)
    assert "F1/Crop" not in names and all(isinstance(v, float) for _, v in rep)
    rep = dict(rep)
    # F1 exactly from the thresholded masks: rebuild the tampered batch and the localiser's mask, count on the host
    from video_watermarking_forgery_detection_amd import ops
    images = m.real_H.clamp(0, 1)
    m.netG.eval()
    with torch.no_grad():
        enc, _ = m.netG.encoder.fwd(images, msgs, training=False)
        _, tampered, _ = ops.splice_fwd(enc, real=images, prev=m.previous_images, mask=m.mask)
        att, _ = m.attack.fwd(tampered, id=0, cover=images)
        pred = m.localise_mask(ops.clamp_quant(att.contiguous()))
    m.netG.train()
    TN, TP, FN, FP = R.confusion(pred.cpu().numpy(), mask.numpy(), 0.5, 0.5)
    ref = R.mask_scores(TN, TP, FN, FP)["F1"]
    got = rep["F1/Jpeg50"]
    assert (np.isnan(ref) and np.isnan(got)) or abs(got - ref) <= np.spacing(np.float32(ref))
    m2 = _model(tmp_path, False, True)
    for k in range(3):
        m2.feed_data(detgen.uniform((B, 3, S, S), 2400 + k))
        m2.optimize_parameters(k)
    m2.feed_data(detgen.uniform((B, 3, S, S), 2410))
    logs, _ = m2.evaluate()
    assert [k for k, _ in logs][:7] == ["loss", "encoder_mse", "dec_mse", "bitwise-error", "adversarial_bce", "discr_cover_bce", "discr_encod_bce"]
    assert {"PSNR", "SSIM", "BER/Jpeg50", "BER/Crop"} <= {k for k, _ in logs}
