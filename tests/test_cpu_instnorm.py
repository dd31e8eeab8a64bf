"""InstanceNorm2d and the instance-normalised coupling subnet, the parts that need no GPU: the float64 restatement
(tests/instnorm_restate.py) against torch's own nn.InstanceNorm2d (+ ReLU) in float64 on every case the GPU tests run, the C ABI's
declarations, state_dict keys against the reference's (tests/golden/instnorm_resblock.npz), the refusals, subnet()'s dispatch."""
import itertools
import re

import numpy as np
import pytest
import torch

import instnorm_restate as R

MODES = list(itertools.product((False, True), (False, True)))      # (affine, relu)


def _run(x, dy, gamma, beta, affine, relu):
    ga, be = (gamma, beta) if affine else (None, None)
    return R.restate(x, dy, ga, be, relu), R.torch_run(x, dy, ga, be, relu, torch.float64)


@pytest.mark.parametrize("affine,relu", MODES)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_is_torch_float64(name, affine, relu):
    """every quantity within 1e-12 of its largest magnitude: two float64 evaluations of the same formulas in different orders"""
    x, dy, gamma, beta = R.inputs(name)
    mine, ref = _run(x, dy, gamma, beta, affine, relu)
    assert sorted(mine) == sorted(ref) == (["dbeta", "dgamma", "dx", "y"] if affine else ["dx", "y"])
    for k in ref:
        R.check(f"{name} affine={affine} relu={relu}: {k}", R.maxdiff(mine[k], ref[k]), 1e-12 * max(1.0, np.max(np.abs(ref[k]))))


@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_restatement_is_torch_float64_on_rounded_inputs(tag):
    """the 16-bit GPU runs start from inputs rounded to the dtype: the statement holds there as well"""
    x, dy, gamma, beta = R.inputs("c24_5x7")
    x, dy = R.rounded(x, tag), R.rounded(dy, tag)
    assert np.array_equal(R.rounded(gamma, tag), gamma) and np.array_equal(R.rounded(beta, tag), beta)
    mine, ref = _run(x, dy, gamma, beta, True, True)
    for k in ref:
        R.check(f"{tag}: {k}", R.maxdiff(mine[k], ref[k]), 1e-12 * max(1.0, np.max(np.abs(ref[k]))))


def test_restatement_on_the_cancellation_case():
    """x = 1000 + N(0,1): the two-pass variance of the restatement agrees with torch's float64; relative 1e-9 of each quantity (the mean
    carries 1e-13 relative error at 1000, i.e. 1e-10 of xhat)"""
    x, dy, gamma, beta = R.inputs(R.CANCEL_CASE, cancel=True)
    assert abs(float(x.mean()) - 1000.0) < 0.1 and 0.9 < float(x.std()) < 1.1
    for affine, relu in MODES:
        mine, ref = _run(x, dy, gamma, beta, affine, relu)
        for k in ref:
            R.check(f"cancellation affine={affine} relu={relu}: {k}", R.maxdiff(mine[k], ref[k]), 1e-9 * max(1.0, np.max(np.abs(ref[k]))))


def test_constant_plane_of_the_statement():
    """the constant plane: y = beta (0 without affine) and, behind the ReLU, dx = 0"""
    x, dy, gamma, beta = R.inputs("c16_33x47", const=True)
    assert (x[R.CONST_B, R.CONST_C] == R.CONST_V).all() and beta[R.CONST_C] == R.CONST_BETA < 0
    for affine, relu in MODES:
        q = R.restate(x, dy, gamma if affine else None, beta if affine else None, relu)
        want = 0.0 if relu or not affine else R.CONST_BETA
        assert (q["y"][R.CONST_B, R.CONST_C] == want).all()
        if relu:
            assert (q["dx"][R.CONST_B, R.CONST_C] == 0).all()


def test_header_declares_the_entry_points():
    import ctypes
    from video_watermarking_forgery_detection_amd import _lib
    sigs = _lib.signatures()
    names = sorted(n for n in sigs if n.startswith("wm_instnorm_"))
    assert names == ["wm_instnorm_apply", "wm_instnorm_bwd_apply", "wm_instnorm_bwd_sums", "wm_instnorm_scratch_doubles", "wm_instnorm_splits",
                     "wm_instnorm_stats"]
    assert sigs["wm_instnorm_scratch_doubles"][0] is ctypes.c_size_t and sigs["wm_instnorm_splits"][0] is ctypes.c_int
    for n in names[:3] + names[5:]:
        restype, args = sigs[n]
        assert restype is ctypes.c_int and args[-1] is ctypes.c_void_p and args[-2] is ctypes.c_int, n     # (..., int dtype, void* stream)
    assert ctypes.c_double in sigs["wm_instnorm_stats"][1]        # eps


def test_plane_splits():
    """the host-side geometry (it launches nothing): one workgroup up to 256 pixels, at most 64 of them; the third GPU case is split"""
    from video_watermarking_forgery_detection_amd import _lib
    L = _lib.lib()
    assert [L.wm_instnorm_splits(n) for n in (1, 2, 256, 257, 1551, 16384, 16385, 1 << 20)] == [1, 1, 1, 2, 7, 64, 64, 64]
    assert L.wm_instnorm_scratch_doubles(2, 1551, 16) == 2 * 7 * 2 * 16
    B, C, H, W = R.CASES["c16_33x47"]
    assert L.wm_instnorm_splits(H * W) > 1 and (H * W) % 256 != 0


def test_layer_state_dict_is_torchs(golden):
    from video_watermarking_forgery_detection_amd import glayers as G
    g = golden("instnorm_resblock")
    plain, affine = (s.split(",") if s else [] for s in g["norm_keys"])
    assert plain == [] and affine == ["weight", "bias"]
    assert list(G.InstanceNorm2d(64).state_dict()) == plain
    assert list(G.InstanceNorm2d(64, act="relu").state_dict()) == plain
    m = G.InstanceNorm2d(64, affine=True)
    assert list(m.state_dict()) == affine and list(dict(m.named_buffers())) == []
    ref = torch.nn.InstanceNorm2d(64, affine=True)
    assert all(torch.equal(m.state_dict()[k], ref.state_dict()[k]) for k in affine)
    m.load_state_dict(ref.state_dict())
    assert m.train().training and not m.eval().training


def test_resblock_keys_are_the_references(golden):
    from video_watermarking_forgery_detection_amd.models.modules import Subnet_constructor as S
    g = golden("instnorm_resblock")
    b = S.ResBlock(3, 9)
    assert [f"{k}:{tuple(v.shape)}" for k, v in b.state_dict().items()] == list(g["keys"])
    assert [k.split(":")[0] for k in g["keys"]] == ["conv1.0.weight", "conv1.0.bias", "conv2.0.weight", "conv2.0.bias", "conv3.0.weight", "conv3.0.bias",
                                                    "conv4.0.weight", "conv4.0.bias", "conv5.weight", "conv5.bias"]
    b.load_state_dict({k.split(":")[0]: torch.from_numpy(g["p/" + k.split(":")[0]]) for k in g["keys"]})
    for i in (1, 2, 3, 4):
        stage = getattr(b, f"conv{i}")
        assert len(stage) == 3 and stage[1].act == "relu" and not stage[1].affine and list(stage[1].state_dict()) == list(stage[2].state_dict()) == []


def test_refusals():
    from video_watermarking_forgery_detection_amd import glayers as G
    with pytest.raises(NotImplementedError, match="track_running_stats"):
        G.InstanceNorm2d(8, track_running_stats=True)
    with pytest.raises(ValueError, match="act"):
        G.InstanceNorm2d(8, act="elu")
    with pytest.raises(RuntimeError, match="GPU only"):
        G.InstanceNorm2d(8)(torch.zeros(1, 4, 4, 16))
    with pytest.raises(RuntimeError, match="GPU only"):                # (the device is refused before the shape)
        G.InstanceNorm2d(8).eval()(torch.zeros(1, 1, 1, 16))


def test_subnet_dispatch():
    from video_watermarking_forgery_detection_amd.models.modules import Subnet_constructor as S
    c = S.subnet("Resnet")
    b = c(6, 10)
    assert isinstance(b, S.ResBlock) and b.conv1[0].in_channels == 6 and b.conv5.in_channels == 70 and b.conv5.out_channels == 10
    assert isinstance(S.subnet("Resnet", "kaiming")(2, 2), S.ResBlock)
    with pytest.raises(NotImplementedError, match="LeakyReLU dense block"):
        S.subnet("DBNet")
    assert S.subnet("anything else")(6, 10) is None           # the reference: "not supported" -> None


def test_embedder_takes_the_subnet():
    """construction only (the forward needs the GPU): every coupling subnet is the instance-normalised ResBlock, with the reference's keys"""
    from video_watermarking_forgery_detection_amd.models.invertible_net import Inveritible_Decolorization_PAMI
    from video_watermarking_forgery_detection_amd.models.modules import Subnet_constructor as S
    net = Inveritible_Decolorization_PAMI(dims_in=[[4, 16, 16]], block_num=[1, 1, 1], subnet_constructor=S.ResBlock)
    keys = list(net.state_dict())
    assert "operations_down.1.s1.conv1.0.weight" in keys and "operations_down.1.t2.conv5.bias" in keys
    assert all(re.fullmatch(r"operations_(up|down)\.\d+\.[st][12]\.(conv[1-4]\.0|conv5)\.(weight|bias)", k) for k in keys if "conv" in k)
    assert sum(isinstance(m, S.ResBlock) for m in net.modules()) == 4 * 5
