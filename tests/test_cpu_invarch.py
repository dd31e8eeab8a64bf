"""The invertible rescaling generator (models/modules/Inv_arch.py, Subnet_constructor.DenseBlock, networks.define_G) without a GPU: the
float64 restatement against the fixture made from the reference's own modules, the state_dict surface, the initialisers, the refusals and
the C ABI's new symbols."""
import ctypes
import os

import numpy as np
import pytest
import torch

import detgen
import invarch_restate as IR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "invarch.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("wm_invblock_shift", "wm_invblock_shift_bwd", "wm_invblock_affine", "wm_invblock_affine_bwd", "wm_invblock_scratch_doubles")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _mods():
    from video_watermarking_forgery_detection_amd.models import networks
    from video_watermarking_forgery_detection_amd.models.modules import Inv_arch as A
    from video_watermarking_forgery_detection_amd.models.modules import Subnet_constructor as S
    return A, S, networks


def test_restatement_equals_the_fixture(golden):
    """float64 against float64: round-off only -- 1e-12 of each quantity's largest value (the two sides order a few sums differently)"""
    db, net = IR.build(torch.float64)
    q = IR.run_cases(db, net, IR.case_inputs(), lambda t: t.double().clone(), IR.middle_nchw)
    stored = [k for k in golden if not k.startswith(("keys/", "amax/", "dev32/", "devbf16/"))]
    assert sorted(stored) == sorted(q)
    for k in stored:
        err, bound = float(np.max(np.abs(q[k] - golden[k]))), 1e-12 * max(float(golden["amax/" + k]), 1.0)
        print("%-52s %.3e (bound %.3e)" % (k, err, bound))
        assert q[k].shape == golden[k].shape and err <= bound, (k, err, bound)


def test_fixture_is_not_the_identity(golden):
    assert float(np.max(np.abs(golden["net/fwd"] - IR.case_inputs()["net/x"].double().numpy()))) > 0.1
    assert float(golden["amax/net/jac"]) > 0.1 and float(golden["amax/db/out"]) > 0.1


def test_state_dict_keys_and_shapes(golden):
    A, S, _ = _mods()
    assert IR.keys_of(S.DenseBlock(IR.DB_CIN, IR.DB_COUT)) == list(golden["keys/db"])
    assert IR.keys_of(A.InvRescaleNet(3, 3, S.DenseBlock, IR.NET_BLOCKS, IR.NET_DOWN)) == list(golden["keys/net"])
    assert IR.keys_of(A.AttackNet(3, 3)) == list(golden["keys/attack"])
    # and the restatement's own, which the fill relies on
    assert IR.keys_of(IR.InvRescaleNet(3, 3, IR.DenseBlock, IR.NET_BLOCKS, IR.NET_DOWN)) == list(golden["keys/net"])
    assert IR.keys_of(IR.AttackNet(3, 3)) == list(golden["keys/attack"])


def test_haar_weights_are_the_unscaled_frozen_filters():
    A, _, _ = _mods()
    h = A.HaarDownsampling(3)
    assert torch.equal(h.haar_weights, IR.haar_unscaled(3)) and not h.haar_weights.requires_grad
    assert set(h.haar_weights.unique().tolist()) == {-1.0, 1.0}


def test_define_G_reads_a_network_G_block():
    A, S, networks = _mods()
    opt = {"network_G": {"which_model_G": {"subnet_type": "DBNet"}, "in_nc": 3, "out_nc": 3, "block_num": [6, 6], "scale": 4, "init": "xavier"}}
    net = networks.define_G(opt, "DBNet", [2, 1])
    assert isinstance(net, A.InvRescaleNet) and net.down_num == 2 and len(net.operations) == 5 and len(net.operations_inverse) == 5
    b = net.operations[1]
    assert isinstance(b, A.InvBlockExp) and isinstance(b.F, S.DenseBlock) and (b.split_len1, b.split_len2) == (3, 9) and b.fused
    assert (net.operations[4].split_len1, net.operations[4].split_len2) == (3, 45)
    assert b.F.conv1.in_channels == 9 and b.F.conv5.out_channels == 3 and b.G.conv5.out_channels == 9
    opt["network_G"].update(scale=2, init=None, in_nc=1, out_nc=1)
    net = networks.define_G(opt, "Resnet", [1])
    assert net.down_num == 1 and isinstance(net.operations[1].H, S.ResBlock) and net.operations[1].split_len2 == 3


@pytest.mark.parametrize("init", ["xavier", "kaiming"])
def test_initialisers_leave_conv5_zero(init):
    _, S, _ = _mods()
    torch.manual_seed(3)
    b = S.DenseBlock(12, 3, init)
    assert not b.conv5.weight.any() and not b.conv5.bias.any()
    for c in (b.conv1, b.conv2, b.conv3, b.conv4):
        fan_in, fan_out = c.in_channels * 9, c.out_channels * 9
        std = 0.1 * (np.sqrt(2.0 / (fan_in + fan_out)) if init == "xavier" else np.sqrt(2.0 / fan_in))
        assert not c.bias.any() and 0.8 * std < float(c.weight.detach().std()) < 1.2 * std


def test_subnet_DBNet_still_refuses():
    _, S, _ = _mods()
    with pytest.raises(NotImplementedError, match="LeakyReLU dense block") as e:
        S.subnet("DBNet")
    assert "DenseBlock" in str(e.value) and "define_G" in str(e.value)


def test_every_module_refuses_a_cpu_tensor():
    A, S, _ = _mods()
    x16 = torch.zeros(1, 4, 4, 16)
    with pytest.raises(RuntimeError, match="GPU only"):
        S.DenseBlock(9, 3)(x16)
    with pytest.raises(RuntimeError, match="GPU only"):
        A.HaarDownsampling(3)(x16)
    for fused in (True, False):
        blk = A.InvBlockExp(S.DenseBlock, 12, 3, fused=fused)
        for rev in (False, True):
            with pytest.raises(RuntimeError, match="GPU only"):
                blk(x16, rev)
    img = torch.zeros(1, 3, 8, 8)
    for net in (A.InvRescaleNet(3, 3, S.DenseBlock, [1, 1], 2), A.AttackNet(3, 3)):
        for rev in (False, True):
            with pytest.raises(RuntimeError, match="GPU only"):
                net(img, rev)


def test_jacobian_needs_the_flag():
    A, S, _ = _mods()
    with pytest.raises(RuntimeError, match="cal_jacobian"):
        A.InvBlockExp(S.DenseBlock, 12, 3).jacobian(torch.zeros(1, 4, 4, 16))


def test_new_symbols_are_declared_and_exported():
    from video_watermarking_forgery_detection_amd import _lib
    sigs = _lib.signatures()
    for name in SYMBOLS:
        assert name in sigs, name
    assert sigs["wm_invblock_scratch_doubles"][0] is ctypes.c_size_t and len(sigs["wm_invblock_affine"][1]) == 16
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libwm_hip.so is not built: run `python -m video_watermarking_forgery_detection_amd.build`")
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(h, name), name


def test_bound_model_accepts_a_faithful_float32_imitation_and_rejects_defects():
    """the kernels' arithmetic imitated in numpy float32 passes its own bound model; dropping the clamp, reading a padding channel or
    leaving the output padding unwritten does not"""
    f32 = np.float32
    for key in IR.affine_keys("f32")[:16]:
        c = IR.AffineCase(*key)
        n1, n2 = c.n1, c.n2
        x, h, g = (a.astype(f32) for a in (c.x[:, n1:n1 + n2], c.h[:, :n2], c.g[:, :n2]))
        with np.errstate(over="ignore"):
            s = f32(c.clamp) * (f32(2) / (f32(1) + np.exp(-h)) - f32(1))
        ex = np.exp(s)
        v = ((x - g) / ex) if c.rev else (ex * x + g)
        out = np.zeros((c.npix, c.ostride))
        out[:, c.vo:c.vo + n2] = v
        if c.whole:
            out[:, :n1] = c.other[:, :n1]
        jac = s.astype(np.float64).reshape(c.B, -1).sum(1).astype(f32)
        assert IR.GX.all_ok(c.check_fwd(out, jac)), IR.GX.first_bad(c.check_fwd(out, jac))
        bad = out.copy()
        bad[:, c.vo:c.vo + n2] = ((x - g) / np.exp(f32(2) * s)) if c.rev else (np.exp(f32(2) * s) * x + g)
        assert not IR.GX.all_ok(c.check_fwd(bad)) or c.clamp == 0.0
        bad = out.copy()
        bad[:, -1] = IR.SENTINEL
        assert not IR.GX.all_ok(c.check_fwd(bad)) or c.vo + n2 == c.ostride
    for key in IR.shift_keys("f32")[:8]:
        c = IR.ShiftCase(*key)
        out = np.zeros((c.npix, c.ostride))
        out[:, :c.n1] = c.x[:, :c.n1].astype(f32) + f32(c.sign) * c.f[:, :c.n1].astype(f32)
        if c.whole:
            out[:, c.n1:c.n1 + c.n2] = c.other[:, :c.n2]
        assert IR.GX.all_ok(c.check_fwd(out)), IR.GX.first_bad(c.check_fwd(out))
        out[:, :c.n1] = c.x[:, :c.n1] - c.sign * c.f[:, :c.n1]
        assert not IR.GX.all_ok(c.check_fwd(out))
