"""The LayerNorm and window-attention kernels (csrc/swin.hip) per element against the float64 bound models of tests/swin_restate.py, and the
Swin modules against the fixture made from the reference's network/SUNet_detail.py (tests/golden/swin.npz)."""
import os

import numpy as np
import pytest
import torch

import instnorm_restate as NR
import swin_restate as SR

GX = SR.GX
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swin.npz")
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def dev(a, dt):
    return GX.store(a, dt).cuda()


def report(cmps):
    for c in cmps:
        print("  ", c.line())
    for c in cmps:
        c.assert_ok()


def _same_bits(a, b):
    return all(torch.equal(s.contiguous().view(torch.uint8), t.contiguous().view(torch.uint8)) for s, t in zip(a, b))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _run_ln(c):
    from video_watermarking_forgery_detection_amd import ops
    x, g = dev(c.x, c.dt).view(1, 1, c.T, c.cp), dev(c.g, c.dt).view(1, 1, c.T, c.cp)
    gamma, beta = dev(c.gamma, "f32"), dev(c.beta, "f32")
    y, mean, rstd = ops.layernorm_fwd(x, c.C, gamma, beta, SR.EPS)
    dx, dgamma, dbeta = ops.layernorm_bwd(x, g, c.C, gamma, mean, rstd)
    return y.view(c.T, c.cp), mean, rstd, dx.view(c.T, c.cp), dgamma, dbeta


@pytest.mark.parametrize("dt", SR.KERNEL_DTYPES)
def test_layernorm_per_element(dt):
    """every width of swin_restate.LN_C (the reference's 96 / 192 / 384 / 768 among them: up to three channel blocks of the parameter
    kernel) x every token count of LN_T (workgroup tails, the slice boundary), and in f32 the 16 515-token case whose slice is 65 tokens:
    a constant row (variance 0), a 1000 + N(0, 1) row (cancellation), SENTINEL in the inputs' padding channels, exact zeros in the
    outputs'; two runs give the same bits.  The worst error-to-bound fraction of each quantity is printed at the end"""
    worst = {}
    for key in SR.ln_keys(dt):
        c = SR.LnCase(*key)
        got = _run_ln(c)
        cmps = c.check(*got)
        report(cmps)
        for m in cmps:
            worst[m.what.split()[-1]] = max(worst.get(m.what.split()[-1], 0.0), m.worst)
        assert _same_bits(got, _run_ln(c)), c.label + ": two runs differ"
    print("worst fractions layernorm %s: %s" % (dt, ", ".join("%s %.3f" % kv for kv in worst.items())))


def _run_attn(c):
    from video_watermarking_forgery_detection_amd import ops
    qkv, gout, table = dev(c.qkv, c.dt), dev(c.gout, c.dt), dev(c.table, "f32")
    out, lse = ops.winattn_fwd(qkv, table, c.C, c.nH, c.ws, c.shift, c.scale)
    gqkv, gtable = ops.winattn_bwd(gout, qkv, table, lse, c.C, c.nH, c.ws, c.shift, c.scale)
    return out, lse, gqkv, gtable


@pytest.mark.parametrize("shape", SR.ATTN_SHAPES, ids=lambda s: "ws%d_hd%d_nh%d_s%d_%dx%d" % s)
@pytest.mark.parametrize("dt", SR.KERNEL_DTYPES)
def test_attention_core_per_element(dt, shape):
    """forward (out, LSE) and backward (g_qkv, g_table), batch 2; one row's scores spread over more than 100, so where the window is
    shifted a masked key still carries that row; padding channels of out and g_qkv exact zeros; two runs give the same bits"""
    c = SR.AttnCase(dt, *shape)
    if c.N > 1:
        assert c.spread > 100, c.spread
        assert c.shift == 0 or c.masked_p > 0.5, c.masked_p
    out, lse, gqkv, gtable = _run_attn(c)
    cmps = c.check_fwd(out, lse) + c.check_bwd(gqkv, gtable)
    report(cmps)
    print("fractions winattn %s: %s" % (dt, ", ".join("%s %.3f" % (m.what.split()[-1], m.worst) for m in cmps)))
    assert _same_bits((out, lse, gqkv, gtable), _run_attn(c)), c.label + ": two runs differ"


@pytest.mark.parametrize("name", SR.CORE_CASES)
def test_attention_core_on_the_reference_s_qkv(golden, name):
    """the reference's own qkv of the two shifted blocks (float64 run, stored on the token grid) through the kernel in float32: its
    attention output within the bound model"""
    H, W, C, nH, ws, s, scale = SR.geometry(name)
    c = SR.AttnCase("f32", ws, C // nH, nH, s, H, W, qkv=golden["core/%s/qkv" % name], table=golden["core/%s/table" % name], scale=scale)
    out, lse, _, _ = _run_attn(c)
    report(c.check_fwd(out, lse))
    want = GX.rnd(golden["core/%s/qkv" % name], "f32")
    NR.check(name + " core vs the fixture", NR.maxdiff(out.double().cpu().numpy()[..., :C], SR.attention_core64(want, c.table, nH, ws, s, scale)), float(c.out[1].max()))


def _hip_build(dtype, fused=True):
    from video_watermarking_forgery_detection_amd.network import SUNet_detail as D

    class Blk(D.SwinTransformerBlock):
        def __init__(self, **kw):
            super().__init__(**kw, fused=fused)
    return {k: m.cuda() for k, m in SR.build((Blk, D.BasicLayer), torch.float32, dtype=dtype).items()}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_blocks_and_layer_against_the_fixture(golden, tag, fused):
    """the three blocks and the BasicLayer -- output, input gradient and four parameter gradients each -- within
    instnorm_restate.bound_of(the reference's own deviation in this dtype from float64, the quantity's largest value); fused and composed
    (fused=False: the attention composed from the host partition helpers) are both held to it.  Each error is printed as a fraction"""
    q = SR.run_cases(_hip_build(TORCH_DT[tag], fused), SR.case_inputs(), lambda t: t.cuda().clone())
    dev_key = "dev32/" if tag == "f32" else "devbf16/"
    worst, top = [], 0.0
    for k in sorted(q):
        bound = NR.bound_of(float(golden[dev_key + k]), float(golden["amax/" + k]))
        err = NR.maxdiff(q[k], golden[k])
        top = max(top, err / bound)
        print("%-62s %.3e (bound %.3e, %.2f of it)" % (tag + " " + k, err, bound, err / bound))
        if not err <= bound:
            worst.append((k, err, bound))
    print("worst fraction %s %s: %.3f" % (tag, "fused" if fused else "composed", top))
    assert not worst, worst


def test_reference_format_state_dict_round_trips(golden):
    from video_watermarking_forgery_detection_amd.network import SUNet_detail as D
    ref = SR.build((SR.SwinTransformerBlock, SR.BasicLayer), torch.float32)["layer"]
    sd = ref.state_dict()
    kw = SR.CASES["layer"][1]
    net = D.BasicLayer(**kw).cuda()
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = net.state_dict()
    assert list(back) == list(sd)
    for k in sd:
        assert torch.equal(back[k].cpu(), sd[k]), k
    x = SR.case_inputs()["layer/x"]
    got = net(x.cuda()).detach().cpu().numpy()
    NR.check("loaded layer(x) vs the fixture", NR.maxdiff(got, golden["layer/out"]), NR.bound_of(float(golden["dev32/layer/out"]), float(golden["amax/layer/out"])))


def test_window_attention_module_takes_windows():
    """WindowAttention.forward on (num_windows*B, N, C) with the block's mask equals the block's own fused path; a foreign mask raises"""
    from video_watermarking_forgery_detection_amd.network import SUNet_detail as D
    blk = SR.fill_swin(D.SwinTransformerBlock(**SR.CASES["blk1"][1])).cuda()
    H, W, C, nH, ws, s, _ = SR.geometry("blk1")
    x = SR.case_inputs()["blk1/x"].cuda()
    grid = torch.roll(x.view(-1, H, W, C), shifts=(-s, -s), dims=(1, 2))
    a = blk.attn(D.window_partition(grid, ws).view(-1, ws * ws, C), mask=blk.attn_mask)
    a = torch.roll(D.window_reverse(a.view(-1, ws, ws, C), ws, H, W), shifts=(s, s), dims=(1, 2))
    want = D.grid_to_tokens(blk.attn.forward_grid(D.tokens_to_grid(x, H, W, torch.float32), s), C)
    assert torch.equal(a.reshape(-1, H * W, C), want)
    with pytest.raises(NotImplementedError):
        blk.attn(D.window_partition(grid, ws).view(-1, ws * ws, C), mask=torch.zeros_like(blk.attn_mask))
