"""CPU side of the UNetDiscriminator work (tests/golden/unetd.npz, generated from the reference's own models.networks.UNetDiscriminator by
tests/golden/make_golden_unetd.py):

  * the float64 restatements of tests/unetd_restate.py reproduce what torch computed for the fixture (reflection pad, its adjoint, the
    dilated convolution and its two gradients, the Bayar constraint), so the GPU tests may lean on either;
  * the Bayar sum order: a plain left-to-right float32 sum of the 25 taps does NOT equal torch.sum over the last two axes on the fixture;
    the order of unetd_restate.plane_sums(.., 'torch') -- eight lane sums, then the 25th tap and the lanes from the left -- does, on every
    plane, and the whole float32 restatement then equals torch's float32 result BIT FOR BIT: which is why csrc/gelem.hip's
    bayar_kernel<true> sums in that order and tests/test_gpu_unetd.py asks it for exact equality;
  * the adjoint identity, the constrained filter's centre and sum, the state_dict contract, the default SRM bank, the refusals, the header."""
import os
import re

import numpy as np
import pytest
import torch

import unetd_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g(golden):
    return golden("unetd")


def networks():
    from video_watermarking_forgery_detection_amd.models import networks as N
    return N


@pytest.mark.parametrize("name", sorted(R.PAD_CASES))
def test_pad_restatement_and_adjoint(g, name):
    p = R.PAD_CASES[name][4]
    x, gr = R.pad_inputs(name)
    y, gx = R.reflect_pad(x, p), R.reflect_pad_adj(gr, p)
    assert np.array_equal(y, g[f"pad/{name}/y64"])                       # a copy: exact
    R.check(f"{name}: adjoint restatement vs torch float64", R.maxdiff(gx, g[f"pad/{name}/gx64"]), 1e-14)
    lhs, rhs = float((y * gr.astype(np.float64)).sum()), float((x.astype(np.float64) * gx).sum())
    R.check(f"{name}: <pad(x), g> - <x, pad_bwd(g)>", abs(lhs - rhs), 1e-12 * max(abs(lhs), 1.0))
    H, W = R.PAD_CASES[name][1:3]
    assert R.pad_terms(H, p).max() <= 3 and R.pad_terms(W, p).max() <= 3 and R.pad_terms(H, p).sum() == H + 2 * p
    if name.startswith("p2_3x4"):
        assert list(R.pad_terms(3, 2)) == [2, 3, 2]        # the middle pixel of the 3-long axis: itself and both mirrors


@pytest.mark.parametrize("name", sorted(R.CONV_CASES))
def test_dilated_conv_restatement(g, name):
    B, Cin, Cout, IH, IW, pad, dil = R.CONV_CASES[name]
    x, w, gr = R.conv_inputs(name)
    for q, got in (("y", R.dil_conv(x, w, pad, dil)), ("gx", R.dil_conv_dgrad(gr, w, pad, dil, (IH, IW))), ("gw", R.dil_conv_wgrad(gr, x, pad, dil))):
        want = g[f"conv/{name}/{q}64"]
        R.check(f"{name}: {q} restatement vs torch float64", R.maxdiff(R.sub(got, R.conv_stride(got.size)), want),
                1e-13 * float(g[f"conv/{name}/amax_{q}"]))
        assert float(g[f"conv/{name}/dev32_{q}"]) > 0


@pytest.mark.parametrize("name", R.BAYAR_CASES)
def test_bayar_restatement_sum_order_and_constraint(g, name):
    w = R.bayar_inputs(name)
    masked = w.reshape(-1, 25).copy()
    masked[:, 12] = 0
    want = g[f"bayar/{name}/sum32"].reshape(-1)
    assert np.array_equal(R.plane_sums(masked, np.float32, "torch"), want)          # on every plane of the fixture
    left = R.plane_sums(masked, np.float32, "left")
    print("planes on which the left-to-right float32 sum differs from torch's:", int((left != want).sum()), "of", want.size)
    assert (left != want).any()          # (why the kernel may not simply add from the left)
    out32 = R.bayar(w, np.float32)
    assert out32.dtype == np.float32 and np.array_equal(out32.reshape(3, 3, 5, 5), g[f"bayar/{name}/out32"])     # bit for bit
    out64 = R.bayar(w, np.float64).reshape(3, 3, 5, 5)
    R.check(f"bayar {name}: float64 restatement vs torch float64", R.maxdiff(out64, g[f"bayar/{name}/out64"]), 1e-15)
    assert np.all(out64[:, :, 2, 2] == -1.0)
    off = out64.reshape(9, 25).sum(1) + 1.0
    R.check(f"bayar {name}: |off-centre sum - 1|", np.abs(off - 1.0).max(), 1e-14)
    if name == "neg":
        assert (g[f"bayar/{name}/sum32"] < 0).any()


def test_bayar_zero_sum_is_not_guarded():
    w = np.ones((1, 1, 5, 5), np.float32)
    w[0, 0, :2, :] = -1.0
    w[0, 0, 2, :2] = -1.0            # 12 x -1 and 12 x +1 beside the centre: the 24 taps sum to 0 exactly, in any order
    out = R.bayar(w, np.float32)
    assert np.isnan(out[0, 2, 2]) and np.isinf(out[0, 0, 0])


@pytest.mark.parametrize("name", sorted(R.NET_CASES))
def test_state_dict_contract(g, name):
    N = networks()
    net = R.fill_net(N.UNetDiscriminator(**R.net_kwargs(name)), name)
    keys = [f"{k}:{tuple(v.shape)}" for k, v in net.state_dict().items()]
    assert keys == list(g[f"{name}/keys"])
    for k, v in net.state_dict().items():       # the regenerated parameters are the ones the reference ran with
        assert np.array_equal(v.reshape(-1)[::101].numpy(), g[f"{name}/probe/{k}"]), k
    frozen = [k for k, p in net.named_parameters() if not p.requires_grad]
    assert frozen == [k[len(name) + 8:] for k in g.files if k.startswith(f"{name}/nograd/")]
    assert frozen == (["SRMConv2D.weight"] if name == "srm" else [])
    if name == "srm":
        assert float(g[f"{name}/bayar_min_abs_sum"]) > 0.5


def test_default_srm_bank():
    N = networks()
    net = N.UNetDiscriminator(in_channels=3, out_channels=1, residual_blocks=1, dim=16)
    w = net.SRMConv2D.weight
    assert tuple(w.shape) == (9, 3, 5, 5) and not w.requires_grad and isinstance(w, torch.nn.Parameter)
    assert torch.equal(w, N.default_srm_weight())
    assert torch.all(w.reshape(9, -1).sum(1).abs() < 1e-6) and torch.all(w.reshape(9, -1).abs().sum(1) > 0)
    for f in range(3):
        for c in range(3):           # filter 3 f + c reads colour channel c only
            assert sorted(torch.nonzero(w[3 * f + c].abs().sum((1, 2))).reshape(-1).tolist()) == [c]
    custom = torch.randn(9, 4, 5, 5)
    net4 = N.UNetDiscriminator(in_channels=4, residual_blocks=1, dim=16, srm_weight=custom)
    assert torch.equal(net4.SRMConv2D.weight, custom) and not net4.SRMConv2D.weight.requires_grad
    with pytest.raises(ValueError):
        N.UNetDiscriminator(in_channels=4, residual_blocks=1, dim=16)


def test_init_weights_keeps_weight_orig_default():
    N = networks()
    torch.manual_seed(0)
    a = N.UNetDiscriminator(residual_blocks=1, dim=16, init_weights=True)
    torch.manual_seed(0)
    b = N.UNetDiscriminator(residual_blocks=1, dim=16, init_weights=False)
    for k in ("encoder_1.0.weight_orig", "decoder_2.0.weight_orig", "middle.0.conv_block.1.weight_orig"):
        bound = 1.0 / np.sqrt(np.prod(a.state_dict()[k].shape[1:]))
        assert a.state_dict()[k].abs().max() <= bound          # nn.Conv2d's default U(-1/sqrt(fan_in), 1/sqrt(fan_in)), not kaiming_normal_
    assert float(a.decoder_0[0].bias.detach().abs().max()) == 0.0 and float(b.decoder_0[0].bias.detach().abs().max()) > 0.0


def test_refusals():
    N = networks()
    with pytest.raises(NotImplementedError, match="with_attn"):
        N.UNetDiscriminator(with_attn=True)
    with pytest.raises(NotImplementedError, match="InstanceNorm2d"):
        N.ResnetBlock(16, dilation=2, use_spectral_norm=False)
    net = N.UNetDiscriminator(**R.net_kwargs("srm"))
    with pytest.raises(ValueError, match=r"\(2, 3, 20, 28\)"):
        net(torch.zeros(2, 3, 20, 28))                      # a CPU tensor
    with pytest.raises(ValueError, match=r"\(2, 3, 22, 28\)"):
        net(torch.zeros(2, 3, 22, 28))                      # 22 is no multiple of 4
    with pytest.raises(ValueError, match=r"\(2, 3, 8, 28\)"):
        net(torch.zeros(2, 3, 8, 28))                       # H / 4 = 2: the dilation-2 reflection pad needs 3
    from video_watermarking_forgery_detection_amd import glayers as G
    with pytest.raises(ValueError):
        G.Conv2d(8, 8, 3, stride=2, dilation=2)


def test_header_declares_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    for sym in ("wm_gconv_dil_fwd", "wm_gconv_dil_wgrad", "wm_reflect_pad_fwd", "wm_reflect_pad_bwd", "wm_bayar_constrain", "wm_bayar_constrain_torch_order", "wm_gcolsum_f64"):
        assert re.search(r"\bint %s\(" % sym, text), sym
    assert re.search(r"int wm_gconv_dil_fwd\([^;]*int pad, int dil, int dgrad", text)
    assert re.search(r"int wm_gconv_fwd\([^;]*int pad, int dgrad", text)       # the existing signature is untouched
