"""UNetDiscriminator on the GPU (models/networks.py) and the kernels added for it, against tests/golden/unetd.npz -- float64 results of the
reference's OWN models.networks.UNetDiscriminator / torch operators (tests/golden/make_golden_unetd.py).

Tolerances (tests/unetd_restate.py holds the rule and prints every figure before asserting it):
  * reflection pad forward: EXACT, it copies.  Its adjoint: per element n x 2^-24 x sum |terms|, n <= 9 the number of padded positions the
    pixel receives from (its term count: n - 1 float32 additions, each rounding a partial sum no larger than sum |terms|, the nth to spare);
  * Bayar constraint: EXACT against torch's float32 result -- tests/test_cpu_unetd.py shows that the kernel's sum order (NOT left to right:
    eight lane sums, then the 25th tap and the lanes from the left) is torch.sum's on the fixture;
  * dilated convolution (forward, input gradient, weight gradient) and both network cases (e0, x, d2, d1, the input gradient, every
    parameter gradient, weight_u / weight_v after the step): bound = MARGIN = 4 x the REFERENCE'S OWN float32-vs-float64 deviation of that
    quantity on the same inputs (max over the whole tensor, stored by the generator, calibrated on the reference alone, never on a kernel):
    another summation order of the same terms x 2, headroom x 2; where the stored deviation is (nearly) 0 the bound is 2 float32 ulp of the
    tensor's largest |value|, the floor of tests/test_gpu_ssim3.py and tests/test_gpu_advloss.py;
  * bfloat16 / float16 activations: the network runs, is finite, and stays within 4 x the deviation of the reference run in that dtype on
    the CPU from float64 (torch's CPU build has every operator: the generator stored both), measured against this package's own float32
    device result; parameters and the spectral norm stay float32 here, so the state after the step is held to the same bound.
Two runs are bit-identical (no atomics anywhere on the path); dilation 1 through the new entry points is the old entry points bit for bit.

The bias gradient of the output convolution is a single sum over all 1120 pixels of terms of both signs when out_channels is 1; the network
asks for it in double (glayers.Conv2d(bias_grad_f64=True) -> wm_gcolsum_f64, tested on its own below).

Measured on an MI355X (largest share of its bound, per family): reflection-pad adjoint 0.50; Bayar 0 of 225 elements differ; dilated
convolution y 0.46, gx 0.88, gw 0.14; network cases: outputs and input gradient at most 0.43, g/decoder_0.2.bias of `plain` 0.61 (4.05e-07
of 6.66e-07; 1.24e-06 with the float32 column sums it had first); 16-bit at most 0.39 of the bound."""
import numpy as np
import pytest
import torch

import unetd_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def g(golden):
    return golden("unetd")


def _ops():
    from video_watermarking_forgery_detection_amd import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype).contiguous()


def nhwc(x, dtype=torch.float32):
    """[B,C,H,W] numpy -> NHWC device tensor with the channel stride rounded up to 16, padding zero"""
    ops = _ops()
    B, C, H, W = x.shape
    out = torch.zeros(B, H, W, ops.cpad(C), dtype=dtype, device=DEV)
    out[..., :C] = dev(x).permute(0, 2, 3, 1).to(dtype)
    return out


def nchw(t, C):
    return t[..., :C].permute(0, 3, 1, 2).double().cpu().numpy()


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("name", sorted(R.PAD_CASES))
def test_reflect_pad_and_adjoint(g, name):
    ops = _ops()
    B, H, W, CP, p = R.PAD_CASES[name]
    x, gr = R.pad_inputs(name)
    y = ops.reflect_pad_fwd(dev(x), p)
    assert tuple(y.shape) == (B, H + 2 * p, W + 2 * p, CP)
    assert np.array_equal(y.double().cpu().numpy(), g[f"pad/{name}/y64"])                    # exact
    gx = ops.reflect_pad_bwd(dev(gr), p).double().cpu().numpy()
    n = np.outer(R.pad_terms(H, p), R.pad_terms(W, p))[None, :, :, None]                      # term count per pixel, <= 9
    assert n.max() <= 9
    bound = n * 2.0 ** -24 * R.reflect_pad_adj(np.abs(gr), p)
    err = np.abs(gx - g[f"pad/{name}/gx64"])
    print("%s: adjoint, largest error / bound over the elements %.3f (largest error %.3e, term counts up to %d)"
          % (name, float((err / bound).max()), float(err.max()), int(n.max())))
    assert (err <= bound).all()
    again = ops.reflect_pad_bwd(dev(gr), p).double().cpu().numpy()
    assert np.array_equal(gx, again)
    for dt in (torch.bfloat16, torch.float16):                                               # the 16-bit twins copy exactly too
        x16 = dev(x, dt)
        y16 = ops.reflect_pad_fwd(x16, p)
        assert torch.equal(y16.float().cpu(), torch.from_numpy(R.reflect_pad(x16.float().cpu().numpy(), p)).float())
    with pytest.raises(ValueError):
        ops.reflect_pad_fwd(dev(x), min(H, W))                                               # p <= min(H, W) - 1


@pytest.mark.parametrize("name", R.BAYAR_CASES)
def test_bayar_constraint_exact(g, name):
    ops = _ops()
    got = ops.bayar_constrain_(dev(R.bayar_inputs(name)), torch_order=True).cpu().numpy()
    want = g[f"bayar/{name}/out32"]
    print("bayar %s: elements that differ from torch's float32 result: %d of %d" % (name, int((got != want).sum()), want.size))
    assert np.array_equal(got, want)
    assert np.all(got[:, :, 2, 2] == -1.0)


@pytest.mark.parametrize("name", sorted(R.CONV_CASES))
def test_dilated_conv(g, name):
    ops = _ops()
    B, Cin, Cout, IH, IW, pad, dil = R.CONV_CASES[name]
    x, w, gr = R.conv_inputs(name)
    OH, OW = gr.shape[2:]
    xd, gd, wd = nhwc(x), nhwc(gr), dev(w)
    KC, NC = xd.shape[3], gd.shape[3]
    y = ops.gconv_fwd(xd, ops.gconv_pack(wd, NC, KC, False, torch.float32), None, (OH, OW), 3, 3, 1, pad, dilation=dil)
    gx = ops.gconv_fwd(gd, ops.gconv_pack(wd, KC, NC, True, torch.float32), None, (IH, IW), 3, 3, 1, pad, dgrad=True, dilation=dil)
    gw, _ = ops.gconv_wgrad(gd, xd, Cout, Cin, 3, 3, 1, pad, want_bias=False, dilation=dil)
    assert float(y[..., Cout:].abs().max() if NC > Cout else 0) == 0.0
    for q, got in (("y", nchw(y, Cout)), ("gx", nchw(gx, Cin)), ("gw", gw.double().cpu().numpy())):
        want = g[f"conv/{name}/{q}64"]
        bound = R.bound_of(g[f"conv/{name}/dev32_{q}"], g[f"conv/{name}/amax_{q}"])
        R.check(f"dilated conv {name}: {q}", R.maxdiff(R.sub(got, R.conv_stride(got.size)), want), bound)
    with pytest.raises(RuntimeError):
        ops.gconv_dil_fwd(xd, ops.gconv_pack(wd, NC, KC, False, torch.float32), None, (OH, OW), 3, 3, 2, pad, dil)      # dilation with stride 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dilation_one_is_the_existing_entry_point(dtype):
    ops = _ops()
    rs = np.random.RandomState(8400)
    x, w, gr = rs.randn(2, 24, 7, 6).astype(np.float32), (0.1 * rs.randn(40, 24, 3, 3)).astype(np.float32), rs.randn(2, 40, 7, 6).astype(np.float32)
    xd, gd, wd = nhwc(x, dtype), nhwc(gr, dtype), dev(w)
    KC, NC = xd.shape[3], gd.shape[3]
    wp, wt = ops.gconv_pack(wd, NC, KC, False, dtype), ops.gconv_pack(wd, KC, NC, True, dtype)
    assert torch.equal(ops.gconv_dil_fwd(xd, wp, None, (7, 6), 3, 3, 1, 1, 1), ops.gconv_fwd(xd, wp, None, (7, 6), 3, 3, 1, 1))
    assert torch.equal(ops.gconv_dil_fwd(gd, wt, None, (7, 6), 3, 3, 1, 1, 1, dgrad=True), ops.gconv_fwd(gd, wt, None, (7, 6), 3, 3, 1, 1, dgrad=True))
    a = ops.gconv_wgrad(gd, xd, 40, 24, 3, 3, 1, 1, want_bias=True, dil_entry=True)
    b = ops.gconv_wgrad(gd, xd, 40, 24, 3, 3, 1, 1, want_bias=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_column_sums_in_double(dtype):
    """wm_gcolsum_f64 (the output layer's bias gradient): n terms added in double, one rounding to float32 -> within half a float32 ulp of
    the float64 sum plus n x 2^-53 x sum |terms|; 1120 pixels of both signs, 5 real channels of a stride of 16 (the padding is not summed);
    accumulation onto an existing value; two runs bit-identical"""
    ops = _ops()
    rs = np.random.RandomState(8500)
    x = dev(rs.randn(2, 20, 28, 16).astype(np.float32), dtype)
    want = x.double().cpu().numpy().reshape(-1, 16).sum(0)[:5]
    slack = 1120 * 2.0 ** -53 * np.abs(x.double().cpu().numpy()).reshape(-1, 16).sum(0)[:5]
    got = ops.gcolsum(x, 5, f64=True)
    assert tuple(got.shape) == (5,) and got.dtype == torch.float32
    err = np.abs(got.double().cpu().numpy() - want)
    bound = 0.5 * np.array([R.ulp32(v) for v in want]) + slack
    print("column sums in double, %s: error / bound %s" % (dtype, np.round(err / bound, 3)))
    assert (err <= bound).all()
    assert torch.equal(got, ops.gcolsum(x, 5, f64=True))
    base = dev(np.arange(5, dtype=np.float32))
    acc = ops.gcolsum(x, 5, out_acc=base.clone(), f64=True).double().cpu().numpy()
    want2 = want + np.arange(5)
    assert (np.abs(acc - want2) <= 0.5 * np.array([R.ulp32(v) for v in want2]) + slack).all()


# ----------------------------------------------------------------------------- the network
def run_net(name, dtype=torch.float32):
    """one forward + backward of case `name`: {quantity: float64 numpy array} with the fixture's keys, and the SRM filter's .grad"""
    from video_watermarking_forgery_detection_amd import glayers as G
    from video_watermarking_forgery_detection_amd.models.networks import UNetDiscriminator

    def make():
        return R.fill_net(UNetDiscriminator(dtype=dtype, **R.net_kwargs(name)), name).to(DEV).train()

    x, gy, g2, g1 = (t.to(DEV) for t in R.net_inputs(name))
    with torch.no_grad():
        e0 = G.to_nchw(make().first_block(x), R.NET_KW["dim"])        # (its own instance: the first block constrains the Bayar filter in place)
    net = make()
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


_RUNS = {}


def f32_run(name):
    if name not in _RUNS:
        _RUNS[name] = run_net(name)
    return _RUNS[name]


@pytest.mark.parametrize("name", sorted(R.NET_CASES))
def test_network_against_the_reference(g, name):
    q, srm_grad = f32_run(name)
    b = R.bounds(g, name)
    assert sorted(q) == sorted(b), set(q) ^ set(b)
    assert srm_grad is None if name == "srm" else srm_grad == "absent"
    failed = []
    for k in sorted(q):
        assert np.isfinite(q[k]).all(), k
        try:
            R.check(f"{name}: {k}", R.maxdiff(R.sub(q[k], R.stride_of(k, q[k].size)), g[f"{name}/{k}"]), b[k])
        except AssertionError as e:
            failed.append(e.args[0])
    assert not failed, failed


@pytest.mark.parametrize("name", sorted(R.NET_CASES))
def test_network_two_runs_bit_identical(name):
    a, b = f32_run(name)[0], run_net(name)[0]
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("tag,dtype", [("bf16", torch.bfloat16), ("f16", torch.float16)])
@pytest.mark.parametrize("name", sorted(R.NET_CASES))
def test_network_16_bit(g, name, tag, dtype):
    assert int(g[f"{name}/has_{tag}"]) == 1        # the reference ran in this dtype on the CPU: the bound exists
    q, _ = run_net(name, dtype)
    ref = f32_run(name)[0]
    b = R.bounds(g, name, "dev" + tag)
    failed = []
    for k in sorted(q):
        assert np.isfinite(q[k]).all() and q[k].shape == ref[k].shape, k
        try:
            R.check(f"{name} {tag}: {k} against the float32 device result", R.maxdiff(q[k], ref[k]), b[k])
        except AssertionError as e:
            failed.append(e.args[0])
    assert not failed, failed
