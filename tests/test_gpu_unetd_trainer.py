"""UNetDiscriminator as the trained tamper localiser (train.localizer_arch: unetd; models/IRNrhi_model.py).

  * Two training steps of the model's own localiser-step code (unetd_localiser_step: forward, BCEWithLogits on the sigmoid output, backward
    into the flat gradient buffer, FlatAdam) against tests/golden/unetd_step.npz -- the REFERENCE's UNetDiscriminator under
    nn.BCEWithLogitsLoss and torch.optim.Adam in float64 (tests/golden/make_golden_unetd_step.py).  Bound per quantity: MARGIN = 4 x the
    reference's own float32-vs-float64 deviation of that quantity, stored by the generator, at least 2 float32 ulp of its largest |value|
    (tests/unetd_restate.py); never calibrated on the device.  Step 2 catches a wrong Adam hook-up (moments, step count) and a lost u / v.
  * IRNrhiModel with the option at the smallest size tests/test_gpu_model_surface.py uses (32 x 32), two frames.
  * Two data-parallel replicas: as tests/test_gpu_distributed.py does it -- two host threads on one card exchanging their buckets through
    its PairSync stand-in for distributed.GradSync (a pytest process that has initialised the GPU starts no children here) -- so this runs
    on one GPU and is not skipped.
Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import detgen
import unetd_restate as R
import unetd_step_restate as S
from test_gpu_model_surface import make_opt

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def g(golden):
    return golden("unetd_step")


def _mod():
    from video_watermarking_forgery_detection_amd.models import IRNrhi_model
    return IRNrhi_model


def make_trainee(dtype=torch.float32, fused=True, lr=S.LR):
    """(net, flat, optimizer) built the way IRNrhiModel builds them, with the fixture's parameters"""
    from video_watermarking_forgery_detection_amd import glayers as G
    from video_watermarking_forgery_detection_amd.optim import FlatAdam
    net = R.fill_net(_mod().build_unetd_localizer("cpu", dtype, 16, fused), S.NAME).to(DEV).train()
    flat = G.FlatParameters(net)
    return net, flat, FlatAdam([flat], lr=lr)


def two_steps(fused=True, sync=None, x=None, steps=2):
    net, flat, opt = make_trainee(fused=fused)
    x0, mask = (t.to(DEV) for t in S.step_inputs())
    x0 = x0 if x is None else x
    srm0 = net.SRMConv2D.weight.detach().clone()
    q = {}
    for n in range(1, steps + 1):
        loss, dice, pred, gx = _mod().unetd_localiser_step(net, flat, opt, x0, mask, grad_sync=sync)
        assert dice is None and tuple(pred.shape) == (2, 1, 20, 28)
        q[f"loss{n}"] = loss.double().cpu().numpy().reshape(())
        if n == 1:
            q["gx1"] = gx.double().cpu().numpy()
        for k, p in net.named_parameters():
            q[f"p{n}/{k}"] = p.detach().double().cpu().numpy()
        for k, v in net.state_dict().items():
            if k.endswith("weight_u") or k.endswith("weight_v"):
                q[f"uv{n}/{k}"] = v.double().cpu().numpy()
    assert torch.equal(srm0, net.SRMConv2D.weight) and net.SRMConv2D.weight.grad is None      # frozen, outside the flat buffer
    return q, net, flat


@pytest.mark.parametrize("fused", [True, False])
def test_two_steps_against_the_reference(g, fused):
    q, net, flat = two_steps(fused)
    want, b = S.unpack(g), S.bounds(g)
    assert sorted(q) == sorted(want), set(q) ^ set(want)
    assert flat.flat_params.numel() == sum(p.numel() for p in net.parameters() if p.requires_grad)
    failed = []
    for k in sorted(q):
        try:
            R.check(f"fused={fused}: {k}", R.maxdiff(np.ravel(S.stored(k, q[k])), np.ravel(want[k])), b[k])
        except AssertionError as e:
            failed.append(e.args[0])
    assert not failed, failed


def run_model(tmp_path, steps, seed=0, frames=2, **train):
    """an IRNrhiModel with the unetd localiser through `steps` working steps (the first two calls only fill the previous-batch buffers);
    -> (model, [logs of every working step as a dict], {working step: {parameter name: clone}} of the localiser and the encoder)"""
    torch.manual_seed(seed)
    np.random.seed(seed)
    t = dict(localizer=True, localizer_arch="unetd", attacks=["JpegSS50"])
    t.update(train)
    m = _mod().IRNrhiModel(make_opt(tmp_path, **t))
    logs, snaps = [], {}
    for step in range(1, steps + 3):
        clip = detgen.uniform((1, 3, frames, 32, 32), 100 + step)
        mask = torch.zeros(1, 1, frames, 32, 32)
        mask[..., 8:24, 4:20] = 1
        m.feed_data((clip, mask))
        lg, _ = m.optimize_parameters(step, None)
        if step > 2:
            logs.append(dict(lg))
            snaps[step - 2] = {"loc": {k: v.detach().clone() for k, v in m.localizer.state_dict().items()},
                               "enc": m.netG.encoder.flat_params.detach().clone()}
    return m, logs, snaps


def test_model_trains_the_unetd_localiser(tmp_path):
    from video_watermarking_forgery_detection_amd.models.networks import UNetDiscriminator
    torch.manual_seed(0)
    m0 = _mod().IRNrhiModel(make_opt(tmp_path, localizer=True, localizer_arch="unetd", attacks=["JpegSS50"]))
    before = {k: v.detach().clone() for k, v in m0.localizer.named_parameters()}
    del m0
    m, logs, snaps = run_model(tmp_path, 10)
    net = m.localizer
    assert isinstance(net, UNetDiscriminator)
    assert (net.use_sigmoid, net.in_channels, net.out_channels, net.dim, net.use_SRM, net.fused_head, net.dtype) == (True, 3, 1, 16, True, True, torch.float32)
    assert len(net.middle) == 2 and type(net.encoder_1[0]).__name__ == "SpectralNormConv2d" and not net.additional_conv
    after3 = snaps[3]["loc"]
    for k, v in before.items():       # (the same seed: `before` holds the parameters this model started from)
        if k == "SRMConv2D.weight":
            assert torch.equal(v, after3[k]), "the frozen SRM filters moved"
        else:
            assert not torch.equal(v, after3[k]), k + " did not change in three steps"
    for lg in logs:
        assert {"lB", "CE", "Kind", "LocKind"} <= set(lg) and np.isfinite(lg["CE"]) and np.isfinite(lg["loss"])
    for p in net.parameters():
        assert torch.isfinite(p).all()
    # the localiser's loss reaches the encoder: with localizer_weight 0 the encoder's first update is another one
    _, _, snaps0 = run_model(tmp_path, 1, localizer_weight=0.0)
    assert not torch.equal(snaps[1]["enc"], snaps0[1]["enc"])


def test_fused_and_unfused_heads_agree_and_repeat(tmp_path, golden):
    runs = {(fused, rep): run_model(tmp_path, 3, localizer_fused_head=fused) for fused in (True, False) for rep in (0, 1)}
    ce = {fused: runs[(fused, 0)][1][0]["CE"] for fused in (True, False)}
    # d BCEWithLogits(p, t) / dp = sigmoid(p) - t lies in (-1, 1): the mean loss moves by no more than the mask's largest change
    R.check("first-step CE, fused vs unfused head", abs(ce[True] - ce[False]), R.bounds(golden("unetd"), "srm")["x"])
    for fused in (True, False):
        a, b = runs[(fused, 0)][2][3]["loc"], runs[(fused, 1)][2][3]["loc"]
        for k in a:
            assert torch.equal(a[k], b[k]), (fused, k)
        assert runs[(fused, 0)][0].localizer.fused_head is fused


def test_checkpoint_round_trip_and_eval_mode(tmp_path):
    m, _, _ = run_model(tmp_path, 1)
    paths = m.save(12)
    assert os.path.basename(paths[-1]) == "12_localizer.pth"
    sd = torch.load(paths[-1])
    assert list(sd.keys()) == list(m.localizer.state_dict().keys())
    assert "decoder_0.0.weight" in sd and "encoder_1.0.weight_orig" in sd and "encoder_1.0.weight_u" in sd and "SRMConv2D.weight" in sd
    x = detgen.uniform((2, 3, 32, 32), 77)
    uv = {k: v.detach().clone() for k, v in m.localizer.state_dict().items() if k.endswith(("weight_u", "weight_v"))}
    mask = m.localise_mask(x)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (2, 1, 32, 32) and m.localizer.training
    for k, v in uv.items():           # eval mode: no power iteration
        assert torch.equal(v, m.localizer.state_dict()[k]), k
    torch.manual_seed(5)              # a model with other initial parameters
    opt = make_opt(tmp_path, localizer=True, localizer_arch="unetd", attacks=["JpegSS50"])
    opt["path"]["pretrain_model_localizer"] = paths[-1]
    fresh = _mod().IRNrhiModel(opt)
    assert torch.equal(fresh.localise_mask(x), mask)


def test_fp16_runs_under_the_scaler(tmp_path, g):
    m, logs, _ = run_model(tmp_path, 3, compute_dtype="fp16")
    assert m.amp is not None and m.localizer.dtype == torch.float16
    assert all(np.isfinite(lg["CE"]) and np.isfinite(lg["loss"]) for lg in logs)
    for p in m.localizer.parameters():
        assert torch.isfinite(p).all()
    assert m.amp.step_count(m.optimizer_localizer.amp_slot) == 3, "the scaler skipped a localiser step"
    _, logs32, _ = run_model(tmp_path, 1)
    if int(g["has_f16"]) != 1:
        pytest.skip("the fixture's generator could not run the reference in float16 on the CPU: no bound for the float16 loss")
    R.check("first CE, float16 against the float32 device run", abs(logs[0]["CE"] - logs32[0]["CE"]),
            R.bound_of(g["dev16/loss1"], max(abs(logs32[0]["CE"]), float(g["loss1"]))))


def test_two_replicas_share_the_flat_gradient():
    """world size 2: after one step both ranks hold the same flat gradient bit for bit -- the SUM of the two single-rank gradients, whose half
    (the 1 / world the optimiser kernel applies) is their mean within 2 float32 ulp of the largest magnitude; weight_u stays per rank and
    differs exactly when the ranks' inputs do"""
    from test_gpu_distributed import _run_pair
    xs = [S.step_inputs()[0].to(DEV), detgen.uniform(R.NET_SHAPE, 9710).to(DEV)]
    single = [two_steps(x=xs[k], steps=1)[2].flat_grads.clone() for k in range(2)]
    out = {}

    def make(k, sync):
        return sync

    def step(k, sync):
        _, net, flat = two_steps(sync=sync, x=xs[k], steps=1)
        out[k] = (flat.flat_grads.clone(), net.encoder_1[0].weight_u.clone(), sync.log)

    _run_pair(make, step)
    assert torch.equal(out[0][0], out[1][0])
    assert out[0][2] == out[1][2] == [single[0].numel()]                       # one bucket: the whole flat gradient
    mean = (single[0].double() + single[1].double()) / 2
    err = float((out[0][0].double() * 0.5 - mean).abs().max())
    R.check("half the exchanged sum against the mean of the single-rank gradients", err, 2 * R.ulp32(float(mean.abs().max())))
    # the power iteration reads the weights alone, and both ranks started from the same ones: u may differ between ranks only through
    # their inputs, and after one step it does not differ at all
    assert torch.equal(out[0][1], out[1][1])
