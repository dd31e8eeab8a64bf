"""CPU side of the copy-move forgery (csrc/localise.hip copymove_kernel, ops.copymove_fwd, train.tamper_cycle of models/IRNrhi_model.py):
the restatement the GPU tests measure the kernel against (tests/copymove_restate.py) equals, bit for bit in float32, what the REFERENCE's own
copy_move() produced (tests/golden/copymove.npz, recorded by tests/golden/make_golden_copymove.py); the trainer's host-side pieces -- the
schedule, the shift draws -- and the refusals of ops.copymove_fwd that need no GPU; the option file."""
import os

import numpy as np
import pytest
import torch

import copymove_restate as R
from make_golden_copymove import FRAC, SHIFTS

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_watermarking_forgery_detection_amd")
CASES = [(si, mk, name, s) for si in range(len(R.GOLDEN_SHAPES)) for mk in ("binary", "fractional") for name, s in SHIFTS]


def _mod():
    from video_watermarking_forgery_detection_amd.models import IRNrhi_model
    return IRNrhi_model


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_golden_holds_every_case(golden):
    g = golden("copymove")
    assert len(CASES) == 24 and sorted({k.rsplit("_", 1)[0] for k in g.files if k.count("_") == 3}) == sorted("%d_%s_%s" % c[:3] for c in CASES)
    signs = {(np.sign(s[0]), np.sign(s[1])) for _, s in SHIFTS}
    assert {(1, 1), (-1, -1), (0, 0), (1, -1), (-1, 1)} <= signs          # positive, negative, zero, mixed both ways


@pytest.mark.parametrize("si,mk,name,shift", CASES, ids=["%d-%s-%s" % c[:3] for c in CASES])
def test_restatement_equals_the_reference_bit_for_bit(golden, si, mk, name, shift):
    g = golden("copymove")
    src, mask, tag = g["%d_%s_src" % (si, mk)], g["%d_%s_mask" % (si, mk)], "%d_%s_%s_" % (si, mk, name)
    assert src.shape == R.GOLDEN_SHAPES[si] and tuple(g[tag + "shifts"]) == shift
    if mk == "binary":
        assert set(np.unique(mask)) == {0.0, 1.0}
    else:
        assert 0 < float(mask[mask > 0].min()) < 1 and float(mask.max()) == 1.0
    shifts = [shift] * src.shape[0]                                        # the reference moves the whole batch by one draw
    q, tam, ms = R.copymove(src, mask, shifts, np.float32, quantise=False)
    assert _same_bits(q, src) and _same_bits(tam, g[tag + "tampered"]) and _same_bits(ms, g[tag + "mask_shifted"])
    assert _same_bits(R.clamp_quant32(src), src)                          # the recorded input is on the 1/255 grid: quantising is the identity
    # the reference's own padding construction, restated in torch, agrees with the index identity -- at float64 too
    t2, m2 = R.copymove_pad_torch(torch.from_numpy(src), torch.from_numpy(mask), shifts)
    assert _same_bits(t2.numpy(), tam) and _same_bits(m2.numpy(), ms)
    _, tam64, ms64 = R.copymove(src, mask, shifts, np.float64, quantise=False)
    t3, m3 = R.copymove_pad_torch(torch.from_numpy(src).double(), torch.from_numpy(mask).double(), shifts)
    assert np.array_equal(t3.numpy(), tam64) and np.array_equal(m3.numpy(), ms64)
    assert float(np.abs(tam64 - tam).max()) <= 4 * 2.0 ** -24
    if name != "zero":
        assert not np.array_equal(ms, mask)                                # the case moves something


def test_restatement_edge_shifts_and_the_inline_form():
    """shifts of a whole frame or more leave an all-zero mask and tampered == q; per-frame shifts; a mask outside [0, 1] is clamped, as the
    inline form clamps it (IRNp_model.py:591)"""
    enc, mask = R.gen_inputs((3, 2, 6, 10), 5, "fractional")
    q, tam, ms = R.copymove(enc, mask, [(6, 0), (0, -10), (9, 13)])
    assert not ms.any() and _same_bits(tam, q) and _same_bits(q, R.clamp_quant32(enc))
    q, tam, ms = R.copymove(enc, mask, [(0, 0), (-5, 9), (2, -3)])
    assert _same_bits(ms[0], mask[0]) and ms[1, 0, 0, 9] == mask[1, 0, 5, 0] and np.count_nonzero(ms[1]) <= 1
    assert ms[2, 0, 2, 0] == mask[2, 0, 0, 3] and tam[2, 1, 5, 6] == np.float32(q[2, 1, 5, 6] * (np.float32(1) - ms[2, 0, 5, 6]) + q[2, 1, 3, 9] * ms[2, 0, 5, 6])
    _, _, wide = R.copymove(enc, mask * 3 - 1, [(1, 1)] * 3)
    assert float(wide.min()) == 0 and float(wide.max()) == 1
    t2, m2 = R.copymove_pad_torch(torch.from_numpy(q), torch.from_numpy(mask * 3 - 1), [(1, 1)] * 3)
    assert _same_bits(m2.numpy(), wide)


def test_draws_reproduce_the_recorded_shifts(golden):
    """draw_copymove_shifts on the recorded draws gives the recorded shifts (the reference's order: rows, then columns; int() truncates
    towards zero, also below zero), one draw for the whole batch"""
    draw = _mod().draw_copymove_shifts
    g = golden("copymove")
    for si, mk, name, shift in CASES:
        B, _, H, W = R.GOLDEN_SHAPES[si]
        tag = "%d_%s_%s_" % (si, mk, name)
        rand = R.scripted(g[tag + "draws"].tolist())
        assert draw(B, H, W, frac=FRAC, rand=rand) == [tuple(int(v) for v in g[tag + "shifts"])] * B == [shift] * B
        assert rand.left() == 0
    # truncation towards zero, not floor: 10 * (0.26 - 0.5) = -2.4 -> -2;  14 * (0.99 - 0.5) = 6.86 -> 6; the inline form's range is frac = 1
    assert draw(2, 10, 14, rand=R.scripted([0.26, 0.99])) == [(-2, 6)] * 2
    assert draw(1, 10, 14, frac=1.0, rand=R.scripted(R.draws_for(-4, 6, 10, 14))) == [(-4, 6)]
    assert draw(1, 256, 256, frac=0.25, rand=R.scripted([0.0, 0.999])) == [(-32, 31)]
    np.random.seed(3)
    a = draw(4, 64, 64)
    np.random.seed(3)
    r = np.random.rand(2)
    assert a == [(int(64 * (r[0] - 0.5)), int(64 * (r[1] - 0.5)))] * 4     # the default source is np.random.rand


def test_per_clip_draws_repeat_over_the_clip():
    draw = _mod().draw_copymove_shifts
    rand = R.scripted(R.draws_for(3, -2, 32, 32) + R.draws_for(-7, 0, 32, 32) + R.draws_for(0, 11, 32, 32))
    s = draw(6, 32, 32, per_clip_T=2, rand=rand)
    assert s == [(3, -2)] * 2 + [(-7, 0)] * 2 + [(0, 11)] * 2 and rand.left() == 0
    with pytest.raises(ValueError):
        draw(5, 32, 32, per_clip_T=2, rand=R.scripted([0.5] * 8))


def test_tamper_cycle_option():
    m = _mod()
    assert m.tamper_cycle({}) == ["splicing"] and m.tamper_cycle(None) == ["splicing"] and m.tamper_cycle({"tamper_cycle": None}) == ["splicing"]
    ref = {"tamper_cycle": ["splicing", "copymove", "splicing"]}
    assert m.tamper_cycle(ref) == list(m.REFERENCE_TAMPER_CYCLE)
    assert [m.tamper_cycle(ref)[s % 3] for s in range(1, 7)] == ["copymove", "splicing", "splicing"] * 2     # copy-move where step % 3 == 1
    assert m.tamper_cycle({"tamper_cycle": "copymove"}) == ["copymove"]
    for bad in (["splicing", "inpainting"], [], ["Copymove"], "move"):
        with pytest.raises(ValueError, match="tamper_cycle"):
            m.tamper_cycle({"tamper_cycle": bad})


def test_unknown_tamper_kind_is_refused_before_anything_is_built():
    from video_watermarking_forgery_detection_amd.options.options import dict_to_nonedict
    opt = dict_to_nonedict({"gpu_ids": None, "dist": False, "is_train": True, "datasets": {"train": {"GT_size": 32}},
                            "train": {"localizer": True, "tamper_cycle": ["splicing", "erase"]}, "path": {}})
    with pytest.raises(ValueError, match="tamper_cycle"):
        _mod().IRNrhiModel(opt)


def test_ops_refuse_without_a_gpu_and_bad_arguments():
    from video_watermarking_forgery_detection_amd import ops
    enc, mask = torch.zeros(2, 3, 6, 8), torch.zeros(2, 1, 6, 8)
    ok = [(0, 0), (1, -1)]
    with pytest.raises(RuntimeError, match="HIP path only"):
        ops.copymove_fwd(enc, mask, ok)
    with pytest.raises(RuntimeError, match="HIP path only"):
        ops.copymove_fwd(enc, mask, torch.zeros(2, 2, dtype=torch.int32), real=enc)
    for args in ((enc[0], mask, ok), (enc.double(), mask, ok), (enc, mask[:, :, :5], ok), (enc, mask.expand(2, 3, 6, 8), ok),
                 (enc, mask.half(), ok), (enc, mask, ok[:1]), (enc, mask, [(0, 0, 0), (1, 1, 1)]), (enc, mask, [(0.5, 0), (1, 1)]),
                 (enc, mask, torch.zeros(2, 2, dtype=torch.int64)), (enc, mask, torch.zeros(3, 2, dtype=torch.int32)),
                 (enc, mask, [(0, 0), (2 ** 20 + 1, 0)]), (enc, mask, [(0, -2 ** 20 - 1), (0, 0)])):
        with pytest.raises(ValueError, match="copymove_fwd"):
            ops.copymove_fwd(*args)
    with pytest.raises(ValueError, match="copymove_fwd"):
        ops.copymove_fwd(enc, mask, ok, real=enc[:, :2])
    with pytest.raises(RuntimeError, match="HIP path only"):       # 2**20 itself passes the range check and gets as far as the device check
        ops.copymove_fwd(enc, mask, [(2 ** 20, -2 ** 20), (0, 0)])
    with pytest.raises(RuntimeError):
        ops.copymove_valid(torch.zeros(2, 4, dtype=torch.float64), 96)


def test_header_declares_the_entry_points():
    import ctypes
    from video_watermarking_forgery_detection_amd import _lib
    sigs = _lib.signatures()
    p, i = ctypes.c_void_p, ctypes.c_int
    assert sigs["wm_copymove_fwd"] == (i, [p] * 8 + [i] * 4 + [p])
    assert sigs["wm_copymove_valid"] == (i, [p, i, ctypes.c_double, p, p])


def test_options_parse_the_new_yml():
    from video_watermarking_forgery_detection_amd.options import options
    opt = options.parse(os.path.join(PKG, "options", "train", "train_hidden_c5_copymove.yml"), is_train=True)
    base = options.parse(os.path.join(PKG, "options", "train", "train_hidden_c5_unetd.yml"), is_train=True)
    t = opt["train"]
    assert t["tamper_cycle"] == ["splicing", "copymove", "splicing"] and t["copymove_shift_frac"] == 1.0 and t["copymove_per_clip"] is True
    extra = ("tamper_cycle", "copymove_shift_frac", "copymove_per_clip")
    assert {k: v for k, v in t.items() if k not in extra} == dict(base["train"]) and opt["datasets"] == base["datasets"]
    assert all(options.dict_to_nonedict(base)["train"][k] is None for k in extra)        # absent there: today's step
    assert _mod().tamper_cycle(t) == list(_mod().REFERENCE_TAMPER_CYCLE) and _mod().tamper_cycle(base["train"]) == ["splicing"]
