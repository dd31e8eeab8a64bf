"""tests/swin_restate.py against the fixture made from the reference's network/SUNet_detail.py (tests/golden/swin.npz), and the HIP modules'
state_dict surface.  No GPU: construction and float64 arithmetic only."""
import os

import numpy as np
import pytest
import torch

import instnorm_restate as NR
import swin_restate as SR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swin.npz")
D53 = 2.0 ** -53


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_restated_modules_match_the_fixture(golden):
    """every stored quantity of the four cases from the restated modules in float64: within the float64 round-off of sums of a few thousand
    terms of the quantity's size (2**-53 x 4096 x amax; the two sides add in different orders)"""
    q = SR.run_cases(SR.build((SR.SwinTransformerBlock, SR.BasicLayer), torch.float64), SR.case_inputs(), lambda t: t.double().clone())
    assert sorted(q) == sorted(k for k in golden if k.split("/")[0] in SR.CASES)
    for k in sorted(q):
        NR.check(k, NR.maxdiff(q[k], golden[k]), 4096 * D53 * max(float(golden["amax/" + k]), 1.0))


@pytest.mark.parametrize("name", SR.CORE_CASES)
def test_restated_core_matches_the_fixture(golden, name):
    """attention_core64 (gather by token_of, the index and mask rule, softmax, scatter) on the reference's own qkv gives the reference's
    attention output, on the token grid"""
    H, W, C, nH, ws, s, scale = SR.geometry(name)
    got = SR.attention_core64(golden["core/%s/qkv" % name], golden["core/%s/table" % name], nH, ws, s, scale)
    want = golden["core/%s/out" % name]
    NR.check(name + " core", NR.maxdiff(got, want), 4096 * D53 * max(float(np.abs(want).max()), 1.0))


def test_core_backward_is_the_gradient_of_the_core():
    """attention_core_bwd64 against torch autograd through the restated float64 forward written in torch (one small shifted case)"""
    ws, hd, nH, s, H, W = 2, 5, 3, 1, 4, 4
    c = SR.AttnCase("f32", ws, hd, nH, s, H, W)
    C = nH * hd
    qkv = torch.from_numpy(c.qkv[..., :3 * C]).requires_grad_(True)
    table = torch.from_numpy(c.table).requires_grad_(True)
    g = torch.roll(qkv, shifts=(-s, -s), dims=(1, 2))
    win = SR.window_partition(g, ws).view(-1, ws * ws, 3, nH, hd).permute(2, 0, 3, 1, 4)
    att = (win[0] * c.scale) @ win[1].transpose(-2, -1)
    att = att + table[torch.from_numpy(SR.rel_index_rule(ws)).view(-1)].view(ws * ws, ws * ws, -1).permute(2, 0, 1).unsqueeze(0)
    mask = torch.from_numpy(SR.mask_rule(H, W, ws, s))
    att = (att.view(-1, mask.shape[0], nH, ws * ws, ws * ws) + mask.unsqueeze(1).unsqueeze(0)).view(-1, nH, ws * ws, ws * ws)
    o = SR.window_reverse((att.softmax(-1) @ win[2]).transpose(1, 2).reshape(-1, ws, ws, C), ws, H, W)
    o = torch.roll(o, shifts=(s, s), dims=(1, 2))
    (o * torch.from_numpy(c.gout[..., :C])).sum().backward()
    gq, gt = SR.attention_core_bwd64(c.qkv[..., :3 * C], c.table, c.gout[..., :C], nH, ws, s, c.scale)
    NR.check("core forward", NR.maxdiff(SR.attention_core64(c.qkv[..., :3 * C], c.table, nH, ws, s, c.scale), o.detach().numpy()), 1e-12 * 300)
    NR.check("g_qkv", NR.maxdiff(gq, qkv.grad.numpy()), 1e-12 * max(1.0, float(np.abs(gq).max())))
    NR.check("g_table", NR.maxdiff(gt, table.grad.numpy()), 1e-12 * max(1.0, float(np.abs(gt).max())))
    assert c.spread > 100 and c.masked_p > 0.5, (c.spread, c.masked_p)


@pytest.mark.parametrize("name", [n for n, (kind, _) in SR.CASES.items() if kind == "block"])
def test_index_and_mask_rule_equal_the_reference_buffers(golden, name):
    """what the kernel computes per token pair equals the buffers the reference builds, exactly"""
    H, W, C, nH, ws, s, _ = SR.geometry(name)
    assert np.array_equal(SR.rel_index_rule(ws), golden["buf/%s/relative_position_index" % name])
    key = "buf/%s/attn_mask" % name
    if s:
        assert np.array_equal(SR.mask_rule(H, W, ws, s), golden[key].astype(np.float64))
    else:
        assert key not in golden and not SR.mask_rule(H, W, ws, s).any()


def test_rule_for_every_kernel_shape():
    """the rule against the reference's construction (written out here from SUNet_detail.py:86-96, 202-221) for the kernel tests' shapes"""
    for ws, _, _, s, H, W in SR.ATTN_SHAPES:
        co = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij")).flatten(1)
        rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0).contiguous()
        rel[:, :, 0] += ws - 1
        rel[:, :, 1] += ws - 1
        rel[:, :, 0] *= 2 * ws - 1
        assert np.array_equal(SR.rel_index_rule(ws), rel.sum(-1).numpy())
        if s:
            img = torch.zeros(1, H, W, 1)
            cnt = 0
            for h in (slice(0, -ws), slice(-ws, -s), slice(-s, None)):
                for w in (slice(0, -ws), slice(-ws, -s), slice(-s, None)):
                    img[:, h, w, :] = cnt
                    cnt += 1
            mw = SR.window_partition(img, ws).view(-1, ws * ws)
            am = mw.unsqueeze(1) - mw.unsqueeze(2)
            am = am.masked_fill(am != 0, -100.0).masked_fill(am == 0, 0.0)
            assert np.array_equal(SR.mask_rule(H, W, ws, s), am.double().numpy())


def test_hip_modules_have_the_reference_state_dict(golden):
    """keys, order and shapes of the HIP modules' state_dicts equal the reference's; the buffers carry the reference's values"""
    from video_watermarking_forgery_detection_amd.network import SUNet_detail as D
    for name, (kind, kw) in SR.CASES.items():
        m = (D.SwinTransformerBlock if kind == "block" else D.BasicLayer)(**kw)
        assert SR.keys_of(m) == list(golden["keys/" + name]), name
        if kind == "block":
            assert np.array_equal(m.attn.relative_position_index.numpy(), golden["buf/%s/relative_position_index" % name])
            if m.attn_mask is not None:
                assert np.array_equal(m.attn_mask.numpy(), golden["buf/%s/attn_mask" % name])
            assert (m.window_size, m.shift_size) == SR.geometry(name)[4:6]
    assert SR.keys_of(SR.build((SR.SwinTransformerBlock, SR.BasicLayer))["layer"]) == list(golden["keys/layer"])


def test_limits_raise():
    from video_watermarking_forgery_detection_amd.network import SUNet_detail as D
    with pytest.raises(NotImplementedError):
        D.BasicLayer(24, (8, 8), 2, 2, 4, use_checkpoint=True)
    with pytest.raises(NotImplementedError):
        D.BasicLayer(24, (8, 8), 2, 2, 4, downsample=D.PatchMerging)
    for cls in (D.PatchEmbed, D.PatchMerging, D.UpSample, D.SUNet):
        with pytest.raises(NotImplementedError):
            cls()
    blk = D.SwinTransformerBlock(24, (8, 8), 2, window_size=4, drop_path=0.1)
    with pytest.raises(RuntimeError, match="GPU"):
        blk(torch.zeros(2, 64, 24))
    with pytest.raises(RuntimeError, match="GPU"):
        D.WindowAttention(24, (4, 4), 2)(torch.zeros(4, 16, 24))
