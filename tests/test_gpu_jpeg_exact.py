"""GPU: the JPEG attack kernels (csrc/jpeg.hip) block by block against float64, ties included (tests/jpeg_exact.py).

Every pixel of every case is either within eps of the float64 restatement of the oracle (strict blocks), within eps of a named
alternate of its block -- a coefficient within delta_F of a jump of the rounding function taken on the other side -- or in a counted
skipped block (more than 4 such coefficients; at most 0.5 % of a case).  delta_F, eps, eps_g = 4 x the float32 oracle's own deviation
from float64 on these inputs, measured on the CPU at test time and printed with the kernels' own largest deviation (run with -s).
The shapes are chosen for the kernels' paths (jpeg_exact.BLOCK_SHAPES); tests/test_cpu_jpeg_exact.py shows that the comparison fails
on the defects it is there to catch."""
import pytest
import torch

import jpeg_exact as JX

pytestmark = pytest.mark.gpu


def _check(cases, tol, run, what):
    print("\n%s: %s" % (what, tol.line()))
    worst = {"y": 0.0, "gx": 0.0}
    for c in cases:
        y, gx = run(c)
        rep = c.compare(y, gx, tol)
        print("  ", rep.line())
        rep.assert_ok()
        worst["y"] = max(worst["y"], rep.stats["y"]["worst_strict"])
        worst["gx"] = max(worst["gx"], rep.stats["gx"]["worst_strict"] / c.gmax)
    print("   kernel, largest deviation on strict blocks: y %.3e (reference f32 %.3e), gx %.3e relative (reference f32 %.3e)"
          % (worst["y"], tol.y_dev, worst["gx"], tol.g_dev))


@pytest.mark.parametrize("mode,Q,sub", JX.BLOCK_CONFIGS, ids=lambda v: str(v))
def test_block_jpeg_kernels(mode, Q, sub):
    from video_watermarking_forgery_detection_amd import ops
    fam = JX.BlockJpeg(mode, Q, sub)
    cases, tol = JX.build_cases(fam, JX.block_specs(Q))
    tables = None if mode == "mask" else fam.host_tables
    mid = JX.BlockJpeg.MODE_ID[mode]

    def run(c):
        x, gy = c.x.cuda(), c.gy.cuda()
        return ops.jpeg_fwd(x, mid, tables, sub), ops.jpeg_bwd(x if mode == "ss" else None, gy, mid, tables, sub)
    _check(cases, tol, run, fam.label)
    if sub == 0 and mode != "mask":
        for c in cases:
            if "table multiples" in c.name:        # coefficients n t: no tie anywhere, and the attack is idempotent on its own output
                assert c.shares("y")["near"] == 0 and c.shares("gx")["near"] == 0, c.name
                y = ops.jpeg_fwd(c.x.cuda(), mid, tables, sub)
                c2 = JX.Case(fam, y.cpu(), c.gy).classify(tol.delta)
                assert c2.shares("y")["near"] == 0, c.name
                if mode == "round":
                    y2 = ops.jpeg_fwd(y, mid, tables, sub)
                    assert float((y2 - y).abs().max()) <= tol.eps, (c.name, float((y2 - y).abs().max()), tol.eps)


@pytest.mark.parametrize("quality", JX.DIFF_QUALITIES)
@pytest.mark.parametrize("rounding", [0, 1, 2])
def test_diffjpeg_kernels(rounding, quality):
    from video_watermarking_forgery_detection_amd import ops
    fam = JX.DiffJpeg(rounding, quality)
    cases, tol = JX.build_cases(fam, JX.diff_specs())

    def run(c):
        x, gy = c.x.cuda(), c.gy.cuda()
        return ops.diffjpeg_fwd(x, rounding, fam.factor), ops.diffjpeg_bwd(x, gy, rounding, fam.factor)
    _check(cases, tol, run, fam.label)


def _through_module(layer):
    def run(c):
        x = c.x.cuda().requires_grad_(True)
        y = layer(x)
        (y * c.gy.cuda()).sum().backward()
        return y.detach(), x.grad
    return run


@pytest.mark.parametrize("mode", ["round", "ss", "mask"])
def test_block_jpeg_modules(mode):
    """noise_layers.Jpeg / JpegSS / JpegMask: the module's own tables and its autograd wiring under the same comparison"""
    from video_watermarking_forgery_detection_amd import noise_layers as NL
    Q, sub = 50, 2
    fam = JX.BlockJpeg(mode, Q, sub)
    layer = {"round": NL.Jpeg, "ss": NL.JpegSS, "mask": NL.JpegMask}[mode](Q, subsample=sub)
    cases, tol = JX.build_cases(fam, [JX.uniform_spec(s) for s in ((2, 61, 75), (2, 40, 68), (3, 128, 128))])
    _check(cases, tol, _through_module(layer), "module " + layer.name)


@pytest.mark.parametrize("rounding", [0, 1, 2])
def test_diffjpeg_module(rounding):
    from video_watermarking_forgery_detection_amd.utils.JPEG import DiffJPEG, diff_round, round_only_at_0
    fam = JX.DiffJpeg(rounding, 60)
    layer = DiffJPEG(quality=60, rounding=(torch.round, round_only_at_0, diff_round)[rounding])
    cases, tol = JX.build_cases(fam, [JX.uniform_spec(s) for s in ((2, 48, 80), (3, 128, 128))])
    _check(cases, tol, _through_module(layer), "module " + layer.name)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32], ids=lambda d: str(d).split(".")[-1])
def test_act16_second_output_at_ragged_shapes(dt):
    """wm_jpeg_fwd_act's second output (the decoder's [B,H,W,16] input) where a wave's strip is ragged, a row has several strips or
    H < 8: channels 0-2 are y cast to the dtype, channels 3-15 exactly zero, byte for byte; y itself is the bytes of the plain call"""
    from video_watermarking_forgery_detection_amd import ops
    for i, (B, H, W) in enumerate(JX.RAGGED_SHAPES):
        mode, sub = i % 3, 2 * (i % 2)
        fam = JX.BlockJpeg(("round", "ss", "mask")[mode], 50, sub)
        x = JX.uniform_spec((B, H, W))[1](0)[0].cuda()
        tables = None if mode == 2 else fam.host_tables
        y0 = ops.jpeg_fwd(x, mode, tables, sub)
        y1, a16 = ops.jpeg_fwd(x, mode, tables, sub, act16_dtype=dt)
        assert a16.shape == (B, H, W, 16) and a16.dtype == dt
        assert torch.equal(y0, y1), (B, H, W)
        assert torch.equal(a16[..., :3], y0.permute(0, 2, 3, 1).to(dt)), (B, H, W)
        assert int((a16[..., 3:].view(torch.int16 if dt != torch.float32 else torch.int32) != 0).sum()) == 0, (B, H, W)
