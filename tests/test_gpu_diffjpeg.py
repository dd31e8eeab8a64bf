"""GPU parity of the fused DiffJPEG kernels against the golden vectors generated from the reference's
utils/JPEG.py (compress_jpeg + decompress_jpeg) and the oracle (oracle/diffjpeg_ref.py)."""
import numpy as np
import pytest
import torch

import detgen
import jpeg_exact
from oracle import diffjpeg_ref

pytestmark = pytest.mark.gpu


def test_diffjpeg_golden(golden):
    from video_watermarking_forgery_detection_amd import ops
    g = golden("diffjpeg")
    keys = sorted({k.split("/")[0] for k in g.files if k.startswith("DiffJPEG")})
    assert len(keys) == 18
    for key in keys:
        _, q, size, rname = key.split("_")
        q = int(q[1:])
        H, W = map(int, size.split("x"))
        seed = int(g[key + "/seed"])
        rid = 0 if rname == "round" else 1
        f = diffjpeg_ref.quality_to_factor(q)
        x = detgen.uniform((2, 3, H, W), seed).cuda()
        gy = detgen.normal((2, 3, H, W), seed + 5000).cuda()
        rec = ops.diffjpeg_fwd(x, rid, f)
        gx = ops.diffjpeg_bwd(x, gy, rid, f)
        err = np.abs(rec.cpu().numpy() - g[key + "/rec"])
        if rid == 0:
            # a coefficient within fp32 round-off of .5 may flip: only there may an MCU leave the fixture's side, and it is then held
            # to the float64 alternate of that side as a whole (tests/jpeg_exact.py)
            case, tol = jpeg_exact.fixed_case(jpeg_exact.DiffJpeg(0, q), x.cpu(), gy.cpu())
            jpeg_exact.assert_matches_fixture(case, tol, rec, g[key + "/rec"], 2e-4, gx)
            assert gx.abs().max().item() == 0.0          # torch.round: zero gradient
        else:
            assert err.max() < 1e-4, (key, err.max())
            np.testing.assert_allclose(gx.cpu().numpy(), g[key + "/gx"], rtol=1e-3, atol=3e-4, err_msg=key)


def test_diffjpeg_module_and_diff_round():
    from video_watermarking_forgery_detection_amd.utils.JPEG import DiffJPEG, diff_round, quality_to_factor, round_only_at_0
    assert quality_to_factor(50) == 1.0 and abs(quality_to_factor(90) - 0.2) < 1e-12 and quality_to_factor(10) == 5.0
    layer = DiffJPEG(90)                       # binds 90 to `differentiable` -> quality 75, like the reference (:502)
    assert layer.name == "DiffJPEG75" and layer.factor == quality_to_factor(75)
    for rounding, rfn in ((diff_round, diffjpeg_ref.diff_round), (round_only_at_0, diffjpeg_ref.round_only_at_0)):
        layer = DiffJPEG(quality=60, rounding=rounding)
        x = detgen.uniform((2, 3, 48, 80), 5)
        gy = detgen.normal((2, 3, 48, 80), 6)
        xr = x.clone().requires_grad_(True)
        yr = diffjpeg_ref.diffjpeg(xr, 60, rfn)
        (yr * gy).sum().backward()
        xg = x.cuda().requires_grad_(True)
        y = layer(xg)
        (y * gy.cuda()).sum().backward()
        if rounding is diff_round:
            # diff_round jumps at q = n + 0.5: MCU by MCU against float64 and its alternates (tests/jpeg_exact.py); MCUs without a
            # coefficient near a tie also against the float32 oracle at the older thresholds
            case, tol = jpeg_exact.fixed_case(jpeg_exact.DiffJpeg(2, 60), x, gy)
            jpeg_exact.assert_matches_fixture(case, tol, y, yr.detach(), 2e-4, xg.grad)
            eg = case.block_err(xg.grad.cpu() - xr.grad, torch.zeros_like(case.gxb))
            assert bool((eg[case.strict("gx")] <= 1e-3).all())
        else:
            torch.testing.assert_close(y.cpu(), yr.detach(), rtol=0, atol=1e-4)
            torch.testing.assert_close(xg.grad.cpu(), xr.grad, rtol=1e-3, atol=3e-4)
    with pytest.raises(RuntimeError, match="multiples of 16"):
        DiffJPEG()(torch.zeros(1, 3, 40, 40, device="cuda"))


def test_diffjpeg_full_size_block_independence():
    from video_watermarking_forgery_detection_amd import ops
    x = detgen.uniform((16, 3, 256, 256), 7).cuda()
    y0 = ops.diffjpeg_fwd(x, 1, 1.0)
    x2 = x.clone(); x2[5, :, 32:48, 208:224] += 0.2     # one 16x16 MCU
    d = (ops.diffjpeg_fwd(x2, 1, 1.0) - y0).abs()
    d[5, :, 32:48, 208:224] = 0
    assert d.max().item() == 0.0
    assert float(y0.min()) >= 0.0 and float(y0.max()) <= 1.0
