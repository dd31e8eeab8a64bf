"""GPU: the kernels of csrc/ssim3.hip (SSIM_Loss's map, its backward, the fused mean; ExtendedL1Loss, NonBlurryLoss, GrayLoss), their ops
wrappers, the public modules and the trainer's ssim3_weight term, against the float64 values of tests/golden/ssim3.npz.

Tolerances.  SSIM_Loss: per case, MARGIN = 4 x the reference's OWN float32-vs-float64 deviation on the very inputs compared, stored by
the generator (ssim3_restate.bounds): map absolute, mean relative, gradients relative to max |grad64| over the pixels no clamp kink
reaches (ssim3_restate.grad_keep; at most 1 % of the outputs are kinked, none in the uniform cases).  Why 4: the kernel adds the nine taps
in the reference's order, so the map carries the reference's roundings, but it forms the gradient as a 27-term gather where autograd
scatters through five pooled paths -- another realisation of rounding errors of the same size, whose largest element can exceed the
reference's largest by a small factor (2) --, and its block sums run in double with one final rounding, at most 2^-24 relative; the
remaining factor 2 is headroom.  The mean alone has a floor of 2 float32 ulp (2^-22 relative, as the GAN-objective tests): one float32
mean can land on the float64 one by luck, and 4 x nothing bounds nothing.  Calibrated on the reference alone, never on the kernel.
The three reductions: sums in double and one rounding to float32, bound 2^-23 relative (ssim3_restate.RED_BOUND).
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import detgen
import ssim3_restate as R

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().double().numpy()


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


@pytest.mark.parametrize("name", tuple(R.CASES))
def test_map_backward_and_fused_mean_against_float64(golden, name):
    from video_watermarking_forgery_detection_amd import loss as loss_mod, ops
    g = golden("ssim3")
    bd = R.bounds(g, name)
    x, y, up = _dev(g[name + "_x"], g[name + "_y"], g[name + "_g"])
    keep = R.grad_keep(g[name + "_x"], g[name + "_y"])
    assert 1.0 - keep.mean() <= 9 * R.KINK_SHARE and float(g[name + "_kink_share"]) <= R.KINK_SHARE
    m = ops.ssim3_map_fwd(x, y)
    assert m.shape == x.shape and m.dtype == torch.float32
    R.check(name + " map abs", R.abs_dev(_np(m), g[name + "_map64"]), bd["map"])
    gx, gy = ops.ssim3_map_bwd(x, y, up)
    R.check(name + " map bwd x", R.grad_dev(_np(gx), g[name + "_gmap64_x"], keep), bd["gmap"])
    R.check(name + " map bwd y", R.grad_dev(_np(gy), g[name + "_gmap64_y"], keep), bd["gmap"])
    only_y = ops.ssim3_map_bwd(x, y, up, want=(False, True))
    assert only_y[0] is None and torch.equal(only_y[1], gy)
    val, gmx = ops.ssim3_mean(x, y, want_grad=True)
    want = g[name + "_map64"].mean()
    R.check(name + " mean rel", abs(float(val) - want) / want, bd["mean"])
    R.check(name + " mean grad x", R.grad_dev(_np(gmx), g[name + "_gmean64_x"], keep), bd["gmean"])
    _, gmy = ops.ssim3_mean_bwd(x, y, want=(False, True))
    R.check(name + " mean grad y", R.grad_dev(_np(gmy), g[name + "_gmean64_y"], keep), bd["gmean"])
    # the device scalars and accumulation: 0.5 (host) * 4 (device) * 0.25 (upstream) = 0.5, a power of two -> exact
    base = torch.full_like(x, 0.125)
    acc = ops.ssim3_mean_bwd(x, y, (True, False), torch.tensor([0.25], device="cuda"), 0.5, torch.tensor([4.0], device="cuda"), (base.clone(), None), True)[0]
    assert torch.equal(acc, base + 0.5 * gmx)
    # autograd through the module's map and .mean(): torch hands the backward a map filled with 1.f * (1.f / N) -- the weight the fused
    # path forms -- and the kernel is the same, so the two gradients agree bit for bit
    xa, ya = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    out = loss_mod.SSIM_Loss()(xa, ya)
    assert torch.equal(out, m)
    out.mean().backward()
    assert torch.equal(xa.grad, gmx) and torch.equal(ya.grad, gmy)
    # two runs are bit-identical
    assert torch.equal(ops.ssim3_map_fwd(x, y), m) and torch.equal(ops.ssim3_mean(x, y), val)
    again = ops.ssim3_map_bwd(x, y, up)
    assert torch.equal(again[0], gx) and torch.equal(again[1], gy)


def test_equal_images_give_exactly_zero_and_a_finite_gradient(golden):
    from video_watermarking_forgery_detection_amd import ops
    (x,) = _dev(golden("ssim3")["same_x"])
    m = ops.ssim3_map_fwd(x, x.clone())
    assert float(m.abs().max()) == 0.0
    val, gx = ops.ssim3_mean(x, x.clone(), want_grad=True)
    assert float(val) == 0.0 and bool(torch.isfinite(gx).all())
    gx, gy = ops.ssim3_map_bwd(x, x.clone(), torch.ones_like(x))
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gy).all())


def test_module_refuses_what_the_reference_cannot_pad():
    from video_watermarking_forgery_detection_amd import loss as loss_mod, ops
    s = loss_mod.SSIM_Loss()
    a = torch.rand(1, 1, 1, 4, device="cuda")
    for bad in (a, a.permute(0, 1, 3, 2)):
        with pytest.raises(ValueError, match="at least 2"):
            s(bad, bad)
        with pytest.raises(ValueError, match="at least 2"):
            ops.ssim3_map_fwd(bad.contiguous(), bad.contiguous())
    with pytest.raises(TypeError):
        s(torch.rand(1, 1, 4, 4, device="cuda").double(), torch.rand(1, 1, 4, 4, device="cuda").double())
    with pytest.raises(ValueError):
        s(torch.rand(1, 1, 4, 4, device="cuda"), torch.rand(1, 1, 4, 5, device="cuda"))
    with pytest.raises(ValueError):
        s(torch.rand(4, 4, device="cuda"), torch.rand(4, 4, device="cuda"))


def _rel(got, want):
    """max |got - want| / |want| elementwise; an exact zero must be matched exactly"""
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    assert got.shape == want.shape and np.isfinite(got).all()
    z = want == 0
    assert (got[z] == 0).all()
    return float(np.max(np.abs(got[~z] - want[~z]) / np.abs(want[~z]))) if (~z).any() else 0.0


@pytest.mark.parametrize("sname", tuple(R.RED_SHAPES))
def test_mask_and_gray_losses_against_float64(golden, sname):
    from video_watermarking_forgery_detection_amd import loss as loss_mod
    g = golden("ssim3")
    d = R.red_inputs(sname)
    E = loss_mod.ExtendedL1Loss()
    for mcase in ("binary", "zeros", "zeromask"):
        a, b, m = _dev(*d[mcase])
        a.requires_grad_(True); b.requires_grad_(True)
        val = E(a, b, m)
        t = "%s_extl1_%s_" % (sname, mcase)
        if mcase == "zeromask":
            assert not bool(torch.isfinite(val)) and not np.isfinite(g[t + "val"])      # 0 / 0, unguarded as the reference
            continue
        assert val.shape == () and val.dtype == torch.float32
        val.backward()
        R.check(t + "val", _rel(_np(val), g[t + "val"]), R.RED_BOUND)
        R.check(t + "ga", _rel(_np(a.grad), g[t + "ga"]), R.RED_BOUND)
        R.check(t + "gb", _rel(_np(b.grad), g[t + "gb"]), R.RED_BOUND)
        a2 = a.detach().clone().requires_grad_(True)       # one gradient alone
        E(a2, b.detach(), m).backward()
        assert torch.equal(a2.grad, a.grad)
    if sname == "r57":          # a [B,1,H,W] mask broadcasts over the channels
        a, b, m = _dev(*d["binary"])
        assert torch.equal(E(a, b, m[:, :1]), E(a, b, m[:, :1].expand_as(a).contiguous()))
    for mod, key in ((loss_mod.NonBlurryLoss(), "nonblurry"), (loss_mod.GrayLoss(), "gray")):
        (x,) = _dev(d["x"])
        x.requires_grad_(True)
        val = mod(x)
        (2.0 * val).backward()
        R.check("%s %s val" % (sname, key), _rel(_np(val), g["%s_%s_val" % (sname, key)]), R.RED_BOUND)
        R.check("%s %s gx" % (sname, key), _rel(_np(x.grad), 2.0 * g["%s_%s_gx" % (sname, key)]), R.RED_BOUND)
        assert torch.equal(mod(x.detach()), val.detach())


def test_reductions_at_an_unaligned_length_with_vector_body():
    """a view 4 bytes off a 16-byte boundary, long enough for float4 groups, more than one workgroup: head, body and tail"""
    from video_watermarking_forgery_detection_amd import ops
    rs = np.random.RandomState(7950)
    n = 2 * 4096 + 7
    buf = [torch.from_numpy(rs.rand(n + 1).astype(np.float32)).cuda() for _ in range(3)]
    a, b, m = (t[1:] for t in buf)
    loss, coef = ops.extended_l1_fwd(a, b, m)
    an, bn, mn = (_np(t) for t in (a, b, m))
    R.check("unaligned extl1", _rel(_np(loss)[0], R.extended_l1(an, bn, mn)), R.RED_BOUND)
    ga, gb = ops.extended_l1_bwd(a, b, m, coef)
    wa, wb = R.extended_l1_grads(an, bn, mn)
    R.check("unaligned extl1 ga", _rel(_np(ga), wa), R.RED_BOUND)
    R.check("unaligned extl1 gb", _rel(_np(gb), wb), R.RED_BOUND)
    loss, coef = ops.gray_loss_fwd(a)
    R.check("unaligned gray", _rel(_np(loss)[0], R.gray_loss(an)), R.RED_BOUND)
    R.check("unaligned gray gx", _rel(_np(ops.gray_loss_bwd(a, coef)), R.gray_loss_grad(an)), R.RED_BOUND)


# ----------------------------------------------------------------------------- the training step
def _hidden(w=None, H=32):
    from video_watermarking_forgery_detection_amd.hidden_models import Hidden
    from video_watermarking_forgery_detection_amd.noise_layers import Identity
    from video_watermarking_forgery_detection_amd.options import HiDDenConfiguration
    kw = {} if w is None else {"ssim3_weight": w}
    h = Hidden(HiDDenConfiguration(H=H, W=H), torch.device("cuda"), Identity(), None, compute_dtype=torch.float32, **kw)
    for m in (h.encoder_decoder.encoder, h.encoder_decoder.decoder, h.discriminator):
        detgen.fill_module(m)
    return h


def _flats(h):
    return [m.flat_params.clone() for m in (h.encoder_decoder.encoder, h.encoder_decoder.decoder, h.discriminator)]


def test_weight_zero_is_the_step_as_it_was(monkeypatch):
    """ssim3_weight = 0 and a model built without the argument: no ssim3 launch (the ops are made to raise), bit-equal losses and weights"""
    from video_watermarking_forgery_detection_amd import ops

    def boom(*a, **k):
        raise AssertionError("an ssim3 kernel was launched at ssim3_weight = 0")
    for n in ("ssim3_mean", "ssim3_mean_fwd", "ssim3_mean_bwd", "ssim3_map_fwd", "ssim3_map_bwd"):
        monkeypatch.setattr(ops, n, boom)
    images, messages = detgen.uniform((2, 3, 32, 32), 3100), detgen.bits((2, 30), 3101)
    res = []
    for w in (0.0, None):
        h = _hidden(w)
        assert h.ssim3_weight == 0.0
        steps = []
        for _ in range(2):
            losses, _ = h.train_on_batch([images, messages])
            assert "_extra" not in losses
            steps.append(dict(losses))
        res.append((steps, _flats(h)))
    assert res[0][0] == res[1][0]
    for p, q in zip(res[0][1], res[1][1]):
        assert torch.equal(p, q)


def test_weight_adds_exactly_the_fused_term_to_the_encoder_gradient(golden):
    """g_enc at weight 0.5 minus g_enc at weight 0 against 0.5 x the standalone gradient, and the standalone gradient itself against
    float64: both within the bound of the largest fixture case of uniform images (s1733: 4 x its recorded deviation)"""
    from video_watermarking_forgery_detection_amd import ops
    images, messages = detgen.uniform((2, 3, 32, 32), 3200), detgen.bits((2, 30), 3201)
    got = {}
    for w in (0.0, 0.5):
        h = _hidden(w)
        box = {}

        def grab(encoded, cover, g_enc):
            box["g"], box["enc"] = g_enc.clone(), encoded.clone()
            return []
        losses, _ = h.train_on_batch([images, messages], extra_encoded_grad=grab)
        got[w] = (box["g"], box["enc"], losses)
    assert torch.equal(got[0.0][1], got[0.5][1])
    enc, cover = got[0.5][1], images.cuda()
    val, alone = ops.ssim3_mean(enc, cover, want_grad=True)
    bound = R.bounds(golden("ssim3"), "s1733")["gmean"]
    diff = got[0.5][0].double() - got[0.0][0].double()
    # the term enters g_enc through float32 additions (g_enc + term, then + the attack's gradient, on either side of the difference): three
    # roundings of at most half an ulp of max |g_enc| each, whatever the kernel computes
    ulp = float(np.spacing(np.float32(max(got[0.5][0].abs().max().item(), got[0.0][0].abs().max().item()))))
    d = float((diff - 0.5 * alone.double()).abs().max())
    scale = 0.5 * float(alone.abs().max())
    print("g_enc difference against 0.5 x the standalone gradient: %.3e = %.3e of max |term| %.3e (bound %.3e) = %.2f ulp of max |g_enc| "
          "(allowance 2 ulp = %.3e; the ulp allowance is %.1f %% of the whole bound)"
          % (d, d / scale, scale, bound, d / ulp, 2 * ulp, 100 * 2 * ulp / (bound * scale + 2 * ulp)))
    assert d <= bound * scale + 2 * ulp
    g64 = R.ssim3_mean_grads(_np(enc), _np(cover))[0]
    keep = R.grad_keep(_np(enc), _np(cover))
    R.check("standalone gradient", R.grad_dev(_np(alone), g64, keep), bound)
    extra = dict(got[0.5][2]["_extra"])
    assert float(extra["SS3FW"]) == float(val) and "_extra" not in got[0.0][2]
    for k in ('loss           ', 'encoder_mse    '):   # 'loss' keeps its three-term meaning
        assert got[0.0][2][k] == got[0.5][2][k]


def test_step_with_term_captured_and_two_chain_equal_eager():
    """as tests/test_gpu_graph.py: the replayed and the two-stream step equal the eager one bit for bit, with the term on"""
    images, messages = detgen.uniform((2, 3, 32, 32), 3300).cuda(), detgen.bits((2, 30), 3301).cuda()
    runs = {}
    for mode in ("eager", "graph", "two", "two_graph"):
        h = _hidden(0.5)
        h.two_streams = mode.startswith("two")
        if mode.endswith("graph"):
            h.enable_graph()
        out = []
        for _ in range(4 + (2 if mode.endswith("graph") else 0)):
            losses, (e, _, dcd) = h.train_on_batch([images, messages])
            extra = losses.pop("_extra", [])
            assert [k for k, _ in extra] == ["SS3FW"]
            out.append((np.array([losses[k] for k in sorted(losses)]), [float(v) for _, v in extra], e.clone(), dcd.clone()))
        torch.cuda.synchronize()
        if mode.endswith("graph"):
            gr = next(iter(h._graphs.values()))
            assert gr.graph is not None and gr.failed is None
        runs[mode] = (out, _flats(h))
    for mode in ("graph", "two", "two_graph"):
        for (la, xa, ea, da), (lb, xb, eb, db) in zip(runs["eager"][0][:4], runs[mode][0][:4]):
            assert np.array_equal(la, lb) and xa == xb and torch.equal(ea, eb) and torch.equal(da, db), mode
    for p, q in zip(runs["eager"][1], runs["two"][1]):
        assert torch.equal(p, q)
    for p, q in zip(runs["graph"][1], runs["two_graph"][1]):
        assert torch.equal(p, q)


def test_option_file_reaches_the_trainer_and_logs_the_term(tmp_path):
    """options/train/train_hidden_c3_ssim3.yml through IRNrhiModel, at 2 frames of 32 x 32 instead of its 16 of 256 x 256: the key arrives
    in Hidden, the term is logged on every trained step with the value of the standalone op, and the other logs keep their names"""
    import os
    from video_watermarking_forgery_detection_amd import ops
    from video_watermarking_forgery_detection_amd.models.IRNrhi_model import IRNrhiModel
    from video_watermarking_forgery_detection_amd.options import options
    pkg = os.path.dirname(os.path.abspath(options.__file__))
    names = {}
    for yml in ("train_hidden_c3_ssim3.yml", "train_hidden_c3.yml"):
        opt = options.parse(os.path.join(pkg, "train", yml), is_train=True)
        opt["datasets"]["train"].update(GT_size=32, batch_size=2)
        opt["path"] = {"models": str(tmp_path / yml / "models"), "training_state": str(tmp_path / yml / "state")}
        torch.manual_seed(0)
        m = IRNrhiModel(options.dict_to_nonedict(opt))
        for net in (m.netG.encoder, m.netG.decoder, m.discriminator):
            detgen.fill_module(net)
        assert m.hidden.ssim3_weight == (0.5 if "ssim3" in yml else 0.0)
        m.keep_outputs = True
        for step in range(1, 5):
            m.feed_data({"GT": detgen.uniform((2, 3, 32, 32), 3400 + step), "mask": torch.zeros(2, 1, 32, 32), "messages": detgen.bits((2, 30), 3500 + step)})
            logs, _ = m.optimize_parameters(step, None)
            if step > 2:
                names[yml] = [k for k, _ in logs]
                if "ssim3" in yml:
                    want = ops.ssim3_mean(m.last_outputs["encoded"].float().contiguous(), m.real_H.float().contiguous())
                    assert float(dict(logs)["SS3FW"]) == float(want)
    assert "SS3FW" in names["train_hidden_c3_ssim3.yml"]
    assert [k for k in names["train_hidden_c3_ssim3.yml"] if k != "SS3FW"] == names["train_hidden_c3.yml"]
