"""The block-by-block JPEG comparison (tests/jpeg_exact.py) with the float32 oracle standing in for the kernels: it passes on the case
list the GPU tests use, its conditions (skipped <= 0.5 %, strict >= 70 %) hold there with the reference alone, and it FAILS on each
planted defect of the kinds a kernel can have -- so a green tests/test_gpu_jpeg_exact.py means something."""
import pytest
import torch

import jpeg_exact as JX
from oracle import diffjpeg_ref, jpeg_ref


def _run(fam, specs):
    cases, tol = JX.build_cases(fam, specs)
    print(fam.label, tol.line())
    for c in cases:
        rep = c.compare(*c.oracle32(), tol)
        print("  ", rep.line())
        rep.assert_ok()
    return cases, tol


@pytest.mark.parametrize("mode,Q,sub", JX.BLOCK_CONFIGS, ids=lambda v: str(v))
def test_float32_oracle_passes_block_jpeg(mode, Q, sub):
    big = (mode, Q, sub) in (("round", 50, 0), ("ss", 100, 2))         # 16x3x256x256 on the CPU for two configurations
    cases, tol = _run(JX.BlockJpeg(mode, Q, sub), JX.block_specs(Q, big=big))
    if sub == 0:
        for c in cases:
            if "table multiples" in c.name:
                assert c.shares("y")["near"] == 0 and c.shares("gx")["near"] == 0, c.name


@pytest.mark.parametrize("quality", JX.DIFF_QUALITIES)
@pytest.mark.parametrize("rounding", [0, 1, 2])
def test_float32_oracle_passes_diffjpeg(rounding, quality):
    _run(JX.DiffJpeg(rounding, quality), JX.diff_specs(big=(rounding, quality) == (1, 75)))


@pytest.mark.parametrize("fam", [JX.BlockJpeg("ss", 50, 2), JX.BlockJpeg("mask", 50, 0), JX.DiffJpeg(1, 75), JX.DiffJpeg(2, 50)],
                         ids=lambda f: f.label)
def test_restatement_is_the_oracle_in_float64(fam):
    """the per-block composition equals the oracle's whole-image function, value and gradient, to float64 round-off"""
    name, make = JX.uniform_spec((2, 48, 80) if fam.bs == 16 else (2, 31, 33))
    x, gy = make(0)
    c = JX.Case(fam, x, gy)
    xd = x.double().requires_grad_(True)
    y = fam.oracle(xd)
    (gx,) = torch.autograd.grad(y, xd, gy.double())
    assert y.dtype == torch.float64
    assert float((y.detach() - c.y64).abs().max()) < 1e-13
    assert float((gx - c.gx64).abs().max()) < 1e-12 * c.gmax


def test_diffjpeg_oracle_follows_the_input_dtype():
    x, _ = JX.uniform_spec((1, 16, 32))[1](0)
    for rfn in (torch.round, diffjpeg_ref.round_only_at_0, diffjpeg_ref.diff_round):
        assert diffjpeg_ref.diffjpeg(x, 50, rfn).dtype == torch.float32
        assert diffjpeg_ref.diffjpeg(x.double(), 50, rfn).dtype == torch.float64


# ---------------------------------------------------------------------------------------------------------------- planted defects
@pytest.fixture(scope="module")
def planted():
    """Jpeg(50) on 2x3x61x75 (ragged last block in both directions) and 3x3x128x128: enough blocks for near ones to exist"""
    fam = JX.BlockJpeg("round", 50, 0)
    cases, tol = JX.build_cases(fam, [JX.uniform_spec((2, 61, 75)), JX.uniform_spec((3, 128, 128)), JX.uniform_spec((16, 256, 256))])
    return fam, cases, tol


def _first(mask):
    return int(mask.nonzero()[0])


def _fails(case, y, gx, tol, what):
    rep = case.compare(y, gx, tol)
    assert not rep.ok, "the comparison did not notice: " + what
    return rep


def test_two_wrong_pixels_in_a_strict_block_fail(planted):
    fam, cases, tol = planted
    c = cases[1]
    y, gx = (t.clone() for t in c.oracle32())
    assert c.compare(y, gx, tol).ok
    n = _first(c.strict("y"))
    br, bc = (n // c.nw) % c.nh, n % c.nw
    y[n // (c.nh * c.nw), 1, br * 8 + 2, bc * 8 + 5] += 1e-3
    y[n // (c.nh * c.nw), 1, br * 8 + 6, bc * 8 + 1] -= 1e-3
    rep = _fails(c, y, gx, tol, "two pixels of one strict block off by 1e-3")
    assert len(rep.failures) == 1 and "block row %d column %d" % (br, bc) in rep.failures[0] and "2 pixels" in rep.failures[0]


def test_a_wrong_table_entry_in_one_block_column_fails(planted):
    fam, cases, tol = planted
    c = cases[0]
    t = fam.t.clone().expand(c.N, 3, 8, 8).clone()
    col = torch.arange(c.N) % c.nw == 3
    t[col, 0, 2, 3] = fam.t[0, 2, 4]          # luminance entry [2][3] replaced by its neighbour [2][4] (24 -> 40) in block column 3
    wrong = JX.BlockJpeg("round", 50, 0, tables=t)
    yb, _, _, _ = JX.evaluate(wrong, JX.to_blocks(c.x.float(), 8))
    y = JX.from_blocks(yb, c.shape, 8)
    rep = _fails(c, y, torch.zeros_like(y), tol, "a wrong table entry")
    assert all("column 3:" in f for f in rep.failures)


def test_a_flipped_coefficient_in_a_strict_block_fails(planted):
    fam, cases, tol = planted
    c = cases[1]
    n = _first(c.strict("y"))
    flip = torch.zeros(1, 3, 8, 8, dtype=torch.bool)
    flip[0, 0, 1, 1] = True
    yb, _, _, _ = JX.evaluate(fam, c.xb[n:n + 1], None, flip)
    y = c.oracle32()[0].clone()
    blocks = JX.to_blocks(y, 8)
    blocks[n] = yb[0].float()
    y = JX.from_blocks(blocks, c.shape, 8)
    rep = _fails(c, y, torch.zeros_like(y), tol, "a strict block's coefficient rounded to the other integer")
    assert len(rep.failures) == 1 and "strict block" in rep.failures[0]


def test_an_unprocessed_last_partial_block_fails(planted):
    fam, cases, tol = planted
    c = cases[0]                               # W = 75: the last block of a row holds 3 pixels
    y = c.oracle32()[0].clone()
    y[0, :, 8:16, 72:] = c.x[0, :, 8:16, 72:]
    rep = _fails(c, y, torch.zeros_like(y), tol, "a partial block copied from the input")
    assert len(rep.failures) == 1 and "block row 1 column 9" in rep.failures[0]


def test_a_near_block_on_the_other_side_passes_and_a_mixture_fails(planted):
    fam, cases, tol = planted
    c = cases[2]
    near = ((c.k["y"] >= 1) & (c.k["y"] <= JX.KMAX)).nonzero().flatten()
    assert len(near) > 0
    n = near[:1]
    alts = {a: yb[0] for a, sel, yb, _ in c.alternates("y", n)}
    assert len(alts) == 2 ** int(c.k["y"][n])
    assert float((alts[0] - alts[1]).abs().max()) > 100 * tol.eps      # the two sides are far apart: the test below means something
    y0 = c.oracle32()[0]
    for a, blk in alts.items():                # every alternate is accepted, as a whole block
        blocks = JX.to_blocks(y0, 8).clone()
        blocks[n] = blk.float()
        rep = c.compare(JX.from_blocks(blocks, c.shape, 8), torch.zeros_like(y0), tol)
        assert rep.ok, rep.failures
    mix = alts[0].clone()
    mix[:, 4:] = alts[1][:, 4:]                # rows 0-3 from one alternate, rows 4-7 from the other
    blocks = JX.to_blocks(y0, 8).clone()
    blocks[n] = mix.float()
    rep = _fails(c, JX.from_blocks(blocks, c.shape, 8), torch.zeros_like(y0), tol, "a near block mixed from two alternates")
    assert len(rep.failures) == 1 and "near block" in rep.failures[0] and "alternate 1" in rep.failures[0]


def test_a_nonzero_gradient_through_hard_rounding_fails(planted):
    fam, cases, tol = planted
    c = cases[0]
    y, gx = c.oracle32()
    gx = gx.clone()
    gx[1, 2, 60, 74] = 1e-30
    _fails(c, y, gx, tol, "a gradient through torch.round")


def test_smooth_mode_defects_fail():
    """JpegSS / round_only_at_0: a colour constant wrong in its fifth digit (forward) and the derivative taken on the wrong side of
    |q| = 0.5 in a strict block (backward), both far below the 1e-4 the older tests resolve"""
    fam = JX.BlockJpeg("ss", 50, 0)
    cases, tol = JX.build_cases(fam, [JX.uniform_spec((3, 128, 128))])
    c = cases[0]
    y, gx = c.oracle32()
    assert c.compare(y, gx, tol).ok
    x = c.x.float()
    img = x * 255
    r, g, b = img[:, 0:1], img[:, 1:2], img[:, 2:3]
    yuv = torch.cat([0.299 * r + 0.587 * g + 0.114 * b, -0.1687 * r - 0.3313 * g + 0.5 * b, 0.5 * r - 0.41871 * g - 0.0813 * b], 1)   # 0.4187
    blk = JX.to_blocks(yuv, 8)
    cm = jpeg_ref.dct_matrix()
    q = torch.matmul(torch.matmul(cm, blk), cm.t()) / fam.table(torch.float32)
    yb = fam.synth(jpeg_ref.round_ss(q)) / 255
    rep = _fails(c, JX.from_blocks(yb, c.shape, 8), gx, tol, "0.41871 for 0.4187 in rgb2yuv")
    assert float((JX.from_blocks(yb, c.shape, 8) - y).abs().max()) < 1e-4           # invisible at the older tolerance
    n = _first(c.strict("gx"))
    flip = torch.zeros(1, 3, 8, 8, dtype=torch.bool)
    flip[0, 1, 7, 7] = True
    _, gxb, _, _ = JX.evaluate(fam, c.xb[n:n + 1], c.gyb[n:n + 1], flip)
    blocks = JX.to_blocks(gx, 8).clone()
    blocks[n] = gxb[0].float()
    rep = _fails(c, y, JX.from_blocks(blocks, c.shape, 8), tol, "round_ss' on the wrong side in a strict block")
    assert len(rep.failures) == 1 and " gx: strict block" in rep.failures[0]


def test_diffjpeg_clamp_pixels_are_near_items_of_the_backward():
    """DiffJPEG's gradient mask: a pixel within delta_F of 0 or 255 is a near item of the backward only, and taking it on the other
    side is an accepted alternate"""
    fam = JX.DiffJpeg(1, 90)          # high quality keeps the noise image's contrast: pixels at both ends of the range
    cases, tol = JX.build_cases(fam, [JX.uniform_spec((16, 256, 256))])
    c = cases[0]
    only_clamp = (c.k["gx"] > c.k["y"]) & (c.k["gx"] <= JX.KMAX) & (c.k["y"] == 0)
    assert only_clamp.any(), "no MCU whose only near items are clamp pixels: pick another input"
    n = only_clamp.nonzero().flatten()[:1]
    y, gx = c.oracle32()
    alts = {a: g[0] for a, sel, _, g in c.alternates("gx", n)}
    assert float((alts[0] - alts[1]).abs().max()) > 100 * tol.eps_g * c.gmax
    blocks = JX.to_blocks(gx, 16).clone()
    blocks[n] = alts[1].float()
    rep = c.compare(y, JX.from_blocks(blocks, c.shape, 16), tol)
    assert rep.ok, rep.failures
