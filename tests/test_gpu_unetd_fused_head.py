"""UNetDiscriminator(fused_head=True): decoder_0 + sigmoid + the NCHW conversion as the one two-source mask-head node (glayers._Head2Fn,
csrc/mask_head.hip) inside the network -- case `srm` of tests/unetd_restate.py against the EXISTING fixture tests/golden/unetd.npz.

Every quantity tests/test_gpu_unetd.py::test_network_against_the_reference checks (e0, x, d2, d1, the input gradient, every parameter
gradient, weight_u / weight_v and the Bayar filter after the step) must meet the SAME R.bounds(g, "srm"): 4 x the reference's own
float32-vs-float64 deviation, stored by the generator; the 16-bit runs the `dev bf16` / `dev f16` bounds against the float32 device run of
the fused network.  Nothing here is calibrated on the kernel; every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import unetd_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAME = "srm"


@pytest.fixture(scope="module")
def g(golden):
    return golden("unetd")


def make(dtype=torch.float32, fused=True, **kw):
    from video_watermarking_forgery_detection_amd.models.networks import UNetDiscriminator
    return R.fill_net(UNetDiscriminator(dtype=dtype, fused_head=fused, **dict(R.net_kwargs(NAME), **kw)), NAME).to(DEV).train()


def run_net(dtype=torch.float32, fused=True):
    """one forward + backward: {quantity: float64 numpy array} with the fixture's keys, and the SRM filter's .grad"""
    from video_watermarking_forgery_detection_amd import glayers as G
    x, gy, g2, g1 = (t.to(DEV) for t in R.net_inputs(NAME))
    with torch.no_grad():
        e0 = G.to_nchw(make(dtype, fused).first_block(x), R.NET_KW["dim"])
    net = make(dtype, fused)
    x.requires_grad_(True)
    y, (d2, d1) = net(x)
    assert y.dtype == d2.dtype == d1.dtype == torch.float32
    assert tuple(y.shape) == (2, 1, 20, 28) and tuple(d2.shape) == (2, 32, 10, 14) and tuple(d1.shape) == (2, 16, 20, 28)
    ((y * gy).sum() + (d2 * g2).sum() + (d1 * g1).sum()).backward()
    q = {"e0": e0, "x": y, "d2": d2, "d1": d1, "gx": x.grad}
    srm_grad = "absent"
    for k, p in net.named_parameters():
        if k == "SRMConv2D.weight":
            srm_grad = p.grad
        else:
            q["g/" + k] = p.grad
    for k, v in net.state_dict().items():
        if k.endswith("weight_u") or k.endswith("weight_v") or k == "BayarConv2D.weight":
            q["after/" + k] = v
    return {k: v.detach().double().cpu().numpy() for k, v in q.items()}, srm_grad


_RUN = {}


def f32_run():
    if "f32" not in _RUN:
        _RUN["f32"] = run_net()
    return _RUN["f32"]


def test_fused_network_against_the_reference(g):
    q, srm_grad = f32_run()
    b = R.bounds(g, NAME)
    assert sorted(q) == sorted(b), set(q) ^ set(b)
    assert srm_grad is None
    failed = []
    for k in sorted(q):
        assert np.isfinite(q[k]).all(), k
        try:
            R.check(f"fused {NAME}: {k}", R.maxdiff(R.sub(q[k], R.stride_of(k, q[k].size)), g[f"{NAME}/{k}"]), b[k])
        except AssertionError as e:
            failed.append(e.args[0])
    assert not failed, failed


def test_fused_two_runs_bit_identical():
    a, b = f32_run()[0], run_net()[0]
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("tag,dtype", [("bf16", torch.bfloat16), ("f16", torch.float16)])
def test_fused_network_16_bit(g, tag, dtype):
    assert int(g[f"{NAME}/has_{tag}"]) == 1
    q, _ = run_net(dtype)
    ref = f32_run()[0]
    b = R.bounds(g, NAME, "dev" + tag)
    failed = []
    for k in sorted(q):
        assert np.isfinite(q[k]).all() and q[k].shape == ref[k].shape, k
        try:
            R.check(f"fused {NAME} {tag}: {k} against the float32 device result", R.maxdiff(q[k], ref[k]), b[k])
        except AssertionError as e:
            failed.append(e.args[0])
    assert not failed, failed


def test_state_dict_keys_and_refusal():
    from video_watermarking_forgery_detection_amd.models.networks import UNetDiscriminator
    fused, plain = make(fused=True), make(fused=False)
    assert list(fused.state_dict().keys()) == list(plain.state_dict().keys())
    assert tuple(fused.state_dict()["decoder_0.0.weight"].shape) == (1, 32, 1, 1) and tuple(fused.state_dict()["decoder_0.0.bias"].shape) == (1,)
    plain.load_state_dict(fused.state_dict())                      # the same parameters serve both tails
    with pytest.raises(ValueError):
        UNetDiscriminator(additional_conv=True, fused_head=True, **{k: v for k, v in R.net_kwargs(NAME).items() if k != "additional_conv"})


def test_eval_forward_matches_the_unfused_tail(g):
    """the same parameters through both tails, no gradient: the mask agrees within the fixture's bound of x"""
    x = R.net_inputs(NAME)[0].to(DEV)
    with torch.no_grad():
        a = make(fused=True).eval()(x)[0]
        b = make(fused=False).eval()(x)[0]
    R.check("fused vs unfused mask (eval)", R.maxdiff(a.double().cpu().numpy(), b.double().cpu().numpy()), 2 * R.bounds(g, NAME)["x"])
