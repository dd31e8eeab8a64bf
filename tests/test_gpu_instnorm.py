"""glayers.InstanceNorm2d (csrc/instnorm.hip), Subnet_constructor.ResBlock and the embedder built on it, on the GPU.

The layer against tests/instnorm_restate.py -- the float64 statement that tests/test_cpu_instnorm.py pins to torch's nn.InstanceNorm2d
(+ ReLU) -- on four shapes x affine on / off x act none / ReLU x float32 / bfloat16 / float16: y, dx, dgamma, dbeta.
Bound (restate.torch_bounds, measured in each test): 4 x the deviation of torch's own CPU run in that dtype from float64 on the same
inputs, at least 2 float32 ulp of the quantity's largest |value|.  Exact: padding channels of y and dx are zero (the input's hold 7.0); the constant
plane gives y = beta (0 without affine) and, behind the ReLU, dx = 0 (beta is negative there: with beta > 0 the plane passes the ReLU and
dx = gamma * rstd * (dy - mean dy), as in torch); two runs agree bit for bit.  The cancellation case x = 1000 + N(0,1) in float32 is held
to the same bound.  ResBlock(3, 9) against tests/golden/instnorm_resblock.npz, results of the REFERENCE's own class: each quantity within
4 x the reference's float32-vs-float64 deviation stored with it.  The embedder with the instance-normalised subnet: rev(forward(x)) = x
within 4 x the round-trip error of the same embedder (same seeded parameters by key, same input) with the ELU subnet; finite gradients in
every parameter; the two-stream schedule of the s / t subnets equals the one-stream one bit for bit.

Measured on an MI355X (largest share of its bound): float32 y 0.27, dx 0.33, dgamma 0.31, dbeta 0.25; bfloat16 y 0.23, dx 0.23; float16
y 0.24, dx 0.18 (dgamma / dbeta of the 16-bit runs below 0.005: float32 sums here, 16-bit values in torch); the cancellation case y 0.15,
dx 0.27, dgamma 0.25, dbeta 0.25; ResBlock out 0.51, gx 0.56, g/conv1.0.weight 0.48, g/conv5.bias 0.13; the embedder's round trip 0.86
(5.424e-06 of 6.318e-06)."""
import numpy as np
import pytest
import torch

import detgen
import instnorm_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD_FILL = 7.0


def _G():
    from video_watermarking_forgery_detection_amd import glayers as G
    return G


def nhwc(a, tag):
    """[B,C,H,W] float32 numpy -> NHWC device tensor of dtype `tag`, channel stride rounded up to 16, the padding channels PAD_FILL"""
    B, C, H, W = a.shape
    out = torch.full((B, H, W, _G().cpad(C)), PAD_FILL, dtype=R.TORCH_DT[tag], device=DEV)
    out[..., :C] = torch.from_numpy(a).to(DEV).permute(0, 2, 3, 1).to(R.TORCH_DT[tag])
    return out.contiguous()


def run_layer(x, dy, gamma, beta, relu, tag):
    """the layer through autograd -> ({y, dx[, dgamma, dbeta]} float64 NCHW numpy, (y, dx) the NHWC device tensors)"""
    G = _G()
    C = x.shape[1]
    m = G.InstanceNorm2d(C, eps=R.EPS, affine=gamma is not None, act="relu" if relu else None).to(DEV)
    if gamma is not None:
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(gamma))
            m.bias.copy_(torch.from_numpy(beta))
    xt = nhwc(x, tag).requires_grad_(True)
    y = m(xt)
    assert y.dtype == xt.dtype and y.shape == xt.shape
    y.backward(nhwc(dy, tag))
    raw = {"y": y.detach(), "dx": xt.grad}
    q = {k: v[..., :C].permute(0, 3, 1, 2).double().cpu().numpy() for k, v in raw.items()}
    if gamma is not None:
        assert m.weight.grad.dtype == m.bias.grad.dtype == torch.float32 and tuple(m.weight.grad.shape) == (C,)
        q.update(dgamma=m.weight.grad.double().cpu().numpy(), dbeta=m.bias.grad.double().cpu().numpy())
    return q, raw


def compare(label, x, dy, gamma, beta, relu, tag):
    want = R.restate(x, dy, gamma, beta, relu)
    bounds = R.torch_bounds(x, dy, gamma, beta, relu, tag, want)
    got, raw = run_layer(x, dy, gamma, beta, relu, tag)
    assert sorted(got) == sorted(want)
    failed = []
    for k in sorted(want):
        try:
            R.check(f"{label}: {k}", R.maxdiff(got[k], want[k]), bounds[k])
        except AssertionError as e:
            failed.append(e.args[0])
    assert not failed, failed
    return got, raw


@pytest.mark.parametrize("tag", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_layer_against_the_restatement(name, affine, relu, tag):
    x, dy, gamma, beta = R.inputs(name)
    x, dy = R.rounded(x, tag), R.rounded(dy, tag)
    if not affine:
        gamma = beta = None
    C = x.shape[1]
    got, raw = compare(f"{name} affine={affine} relu={relu} {tag}", x, dy, gamma, beta, relu, tag)
    # exact conditions
    for k, t in raw.items():
        assert t.shape[3] == C or float(t[..., C:].abs().max()) == 0.0, k
    again, raw2 = run_layer(x, dy, gamma, beta, relu, tag)
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    assert all(torch.equal(raw[k], raw2[k]) for k in raw)


@pytest.mark.parametrize("tag", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_constant_plane_is_exact(name, tag):
    """one plane of the input the constant 2.5: y is exactly beta there (0 without affine, 0 behind the ReLU: beta = -0.5), and behind the
    ReLU dx is exactly 0; the rest of the tensor stays finite"""
    x, dy, gamma, beta = R.inputs(name, const=True)
    x, dy = R.rounded(x, tag), R.rounded(dy, tag)
    for affine in (False, True):
        for relu in (False, True):
            got, _ = run_layer(x, dy, gamma if affine else None, beta if affine else None, relu, tag)
            assert all(np.isfinite(v).all() for v in got.values())
            assert (got["y"][R.CONST_B, R.CONST_C] == (0.0 if relu or not affine else R.CONST_BETA)).all(), (affine, relu)
            if relu:
                assert (got["dx"][R.CONST_B, R.CONST_C] == 0.0).all(), (affine, relu)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("affine", [False, True])
def test_cancellation_case(affine, relu):
    """x = 1000 + N(0,1) in float32 on the plane that spans several workgroups: sum x^2 is 1e6 x the variance"""
    x, dy, gamma, beta = R.inputs(R.CANCEL_CASE, cancel=True)
    if not affine:
        gamma = beta = None
    compare(f"cancellation affine={affine} relu={relu}", x, dy, gamma, beta, relu, "f32")


def test_refusals_on_the_device():
    G = _G()
    with pytest.raises(ValueError, match=r"Expected more than 1 spatial element when training, got input size torch.Size\(\[2, 8, 1, 1\]\)"):
        G.InstanceNorm2d(8)(torch.zeros(2, 1, 1, 16, device=DEV))
    with pytest.raises(ValueError, match="NHWC activation of 8 channels"):
        G.InstanceNorm2d(8)(torch.zeros(2, 4, 4, 32, device=DEV))
    m = G.InstanceNorm2d(8, act="relu")
    x = torch.randn(2, 4, 4, 16, device=DEV)
    assert torch.equal(m.train()(x), m.eval()(x))          # no running statistics: both modes normalise with the input's own


def test_resblock_against_the_reference_fixture(golden):
    from video_watermarking_forgery_detection_amd.models.modules import Subnet_constructor as S
    G = _G()
    g = golden("instnorm_resblock")
    block = S.ResBlock(3, 9)
    block.load_state_dict({k.split(":")[0]: torch.from_numpy(g["p/" + k.split(":")[0]]) for k in g["keys"]})
    block = block.to(DEV).train()
    x = torch.from_numpy(g["x"]).to(DEV).requires_grad_(True)
    out = G.to_nchw(block(G.to_nhwc(x, torch.float32)), 9)
    assert tuple(out.shape) == (2, 9, 8, 12)
    (out * torch.from_numpy(g["gy"]).to(DEV)).sum().backward()
    params = dict(block.named_parameters())
    got = {"out": out, "gx": x.grad, "g/conv1.0.weight": params["conv1.0.weight"].grad, "g/conv5.bias": params["conv5.bias"].grad}
    failed = []
    for k, v in got.items():
        try:
            R.check(f"ResBlock: {k}", R.maxdiff(v.detach().double().cpu().numpy(), g[k]), R.bound_of(g["dev32/" + k], g["amax/" + k]))
        except AssertionError as e:
            failed.append(e.args[0])
    assert not failed, failed


def _embedder(constructor):
    from video_watermarking_forgery_detection_amd.models.invertible_net import Inveritible_Decolorization_PAMI
    return detgen.fill_f2(Inveritible_Decolorization_PAMI(dims_in=[[4, 16, 16]], block_num=[1, 1, 1], subnet_constructor=constructor)).to(DEV).train()


def _embedder_step(net, x):
    """forward, reverse and backward -> (y, recovered, middle, {parameter: gradient})"""
    net.zero_grad(set_to_none=True)
    y = net(x)
    back, mid = net(y, rev=True)
    ((y * detgen.normal(tuple(y.shape), 9801).to(DEV)).sum() + (back ** 2).mean() + (mid ** 2).mean()).backward()
    return y.detach(), back.detach(), mid.detach(), {k: p.grad for k, p in net.named_parameters() if p.requires_grad}


_STEP = {}


def _two_stream_step():
    """the instance-normalised embedder, its input, and one step with the s / t subnets on two streams (the default), run once"""
    from video_watermarking_forgery_detection_amd.models.modules import Subnet_constructor as S
    if not _STEP:
        x = detgen.uniform((2, 4, 16, 16), 9800).to(DEV)
        net = _embedder(S.ResBlock)
        _STEP.update(x=x, net=net, out=_embedder_step(net, x))
    return _STEP["net"], _STEP["x"], _STEP["out"]


def test_embedder_round_trip():
    """rev(forward(x)) against x, bound 4 x the same error of the ELU embedder with the same seeded parameters on the same input.

    Measured on an MI355X: 5.424e-06 against a bound of 6.318e-06 (4 x the ELU embedder's 1.580e-06), 0.86 of it.  The margin is the
    network's, not the layer's: with the normalisation composed from torch operators entirely in float64 the same embedder returns
    5.811e-06 (0.92).  The reverse pass evaluates each subnet at an input that differs from the forward's by float32 rounding, and an
    instance-normalised subnet magnifies that difference by its planes' rstd (up to 39.9 on this input; the deepest planes have four
    pixels) where the ELU subnet does not.  This is why the kernels form xhat = (x - mean) * rstd in double and round once
    (csrc/instnorm.hip in_xhat): with the difference and the product rounded separately in float32 the round trip was 7.093e-06, 1.12
    of the bound."""
    from video_watermarking_forgery_detection_amd.models import invertible_net as inn
    net, x, (y, back, mid, _) = _two_stream_step()
    with torch.no_grad():
        elu = _embedder(inn.ResBlock)
        err_elu = float((elu(elu(x), rev=True)[0] - x).abs().max())
    assert tuple(y.shape) == (2, 4, 16, 16) and tuple(mid.shape) == (2, 256, 2, 2) and torch.isfinite(y).all()      # the deepest plane is 2 x 2
    R.check("embedder round trip (bound: 4 x the ELU embedder's %.3e)" % err_elu, float((back - x).abs().max()), 4.0 * err_elu)


def test_embedder_backward_reaches_every_parameter():
    net, _, (_, _, _, grads) = _two_stream_step()
    named = dict(net.named_parameters())
    assert len(grads) == 5 * 4 * 10 and sorted(grads) == sorted(k for k, p in named.items() if p.requires_grad)
    for k, gr in grads.items():
        assert gr is not None and torch.isfinite(gr).all(), k


def test_embedder_two_streams_equal_one_stream():
    """the s / t subnets side by side on two streams (invertible_net._pair, unchanged) and one after the other: the same bits"""
    from video_watermarking_forgery_detection_amd.models import invertible_net as inn
    net, x, (y, back, mid, grads) = _two_stream_step()
    grads = {k: v.clone() for k, v in grads.items()}
    inn.PARALLEL_SUBNETS = False
    try:
        y1, back1, mid1, grads1 = _embedder_step(net, x)
    finally:
        inn.PARALLEL_SUBNETS = True
    assert torch.equal(y, y1) and torch.equal(back, back1) and torch.equal(mid, mid1)
    for k in grads:
        assert torch.equal(grads[k], grads1[k]), k
