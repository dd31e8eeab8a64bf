#!/usr/bin/env python3
"""Generate tests/golden/metrics.npz from the REFERENCE's pytorch_ssim and metrics modules.

Runs only where the reference tree exists (both modules imported unmodified, torch alone suffices; PYTHONDONTWRITEBYTECODE=1), like
make_golden_noise.py.  The inputs of every case are remade from detgen seeds by tests/metrics_restate.py (case_inputs / case_masks), so
nothing large is stored.  Per case `s<shape>_<kind>_` (shapes and kinds: metrics_restate.SHAPES / KINDS):

    mean32, img32      the reference's SSIM at float32: batch mean (size_average=True) and per-image means (size_average=False)
    mean64, img64      the same from the reference's _ssim called on float64 tensors (its float32 window cast to float64)
    grad32             float32 autograd gradient of the batch mean wrt the first image: in full for the three small shapes; at 256 x 256
                       every GRAD_STRIDE-th element (grad32_sample) and sum |g| (grad32_abs)
    dev_mean, dev_img  |mean32 - mean64|, max |img32 - img64|: THE REFERENCE'S OWN float32-vs-float64 deviation of the value
    dev_grad           N * max |grad32 - grad64| with N = B C H W (the deviation of the gradient of the map's SUM, comparable across shapes)
    psnr1, psnr255     metrics.PSNR(1.0)(x, y), metrics.PSNR(255.0)(255 x, 255 y)
and per shape `m<shape>_`: prec, rec = metrics.EdgeAccuracy(0.5)(gt, pred) on the case's masks.  The deviations calibrate the tolerances
of tests/test_gpu_metrics.py (4 x the largest over the cases).

calculate_f1.py cannot be imported: it is a script that runs on import, with hard-coded paths and cv2.  Its TN / TP / FN / FP counts and
the scores derived from them are checked in the tests against a plain numpy count instead.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metrics.py REFERENCE_ROOT
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import metrics_restate as R  # noqa: E402


def main(ref):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    import metrics as ref_metrics
    import pytorch_ssim as ref_ssim

    torch.set_num_threads(1)   # one summation order, whatever the machine
    out = {}
    for si, shape in enumerate(R.SHAPES):
        n = int(np.prod(shape))
        for kind in R.KINDS:
            tag = "s%d_%s_" % (si, kind)
            x, y = R.case_inputs(si, kind)
            res = {}
            for name, dt in (("32", torch.float32), ("64", torch.float64)):
                a = x.to(dt).clone().requires_grad_(True)
                b = y.to(dt)
                win = ref_ssim.create_window(11, shape[1]).to(dt)
                mean = ref_ssim._ssim(a, b, win, 11, shape[1], True)
                (g,) = torch.autograd.grad(mean, a)
                with torch.no_grad():
                    img = ref_ssim._ssim(a, b, win, 11, shape[1], False)
                res[name] = (mean.detach(), img, g)
            with torch.no_grad():   # the module and the function are the same computation: hold them to it
                assert torch.equal(ref_ssim.SSIM()(x, y), res["32"][0]) and torch.equal(ref_ssim.ssim(x, y), res["32"][0])
            out[tag + "mean32"], out[tag + "img32"] = res["32"][0].numpy(), res["32"][1].numpy()
            out[tag + "mean64"], out[tag + "img64"] = res["64"][0].numpy(), res["64"][1].numpy()
            g32, g64 = res["32"][2], res["64"][2]
            if n <= 32768:
                out[tag + "grad32"] = g32.numpy()
            else:
                out[tag + "grad32_sample"] = g32.reshape(-1)[::R.GRAD_STRIDE].numpy().copy()
                out[tag + "grad32_abs"] = g32.double().abs().sum().numpy()
            out[tag + "dev_mean"] = (res["32"][0].double() - res["64"][0]).abs().numpy()
            out[tag + "dev_img"] = (res["32"][1].double() - res["64"][1]).abs().max().numpy()
            out[tag + "dev_grad"] = (n * (g32.double() - g64).abs().max()).numpy()
            out[tag + "psnr1"] = ref_metrics.PSNR(1.0)(x, y).numpy()
            out[tag + "psnr255"] = ref_metrics.PSNR(255.0)(255 * x, 255 * y).numpy()
        pred, gt = R.case_masks(si)
        prec, rec = ref_metrics.EdgeAccuracy(0.5)(gt, pred)
        out["m%d_prec" % si], out["m%d_rec" % si] = prec.numpy(), rec.numpy()
    z = torch.zeros(1, 1, 8, 8)
    prec, rec = ref_metrics.EdgeAccuracy(0.5)(z, z)
    out["empty_prec"], out["empty_rec"] = prec.numpy(), rec.numpy()
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_metrics.py REFERENCE_ROOT (the reference repository's checkout)")
    main(sys.argv[1])
