#!/usr/bin/env python3
"""Time the separable blur (ops.gauss_sep / gauss_sep_bwd, csrc/gauss_sep.hip) at k = 3, 7, 15 and both borders against the 3 x 3 stencil
path (ops.stencil3, what GaussianBlur(3) runs) at 16x3x256x256, and Cropout's two launches: device events around each call after warm-up,
the variants alternating in one process, median [p10, p90] microseconds per call, and the fraction of the HBM roof from the algorithmic
bytes -- 8 B per pixel and plane for the blurs (one read + one write), 12 for Cropout's forward (image, cover, result) and its backward with
the cover's gradient (one read, two writes).

    python tools/bench_blur.py [--iters 200] [--hbm-tbs 8.0] [--shape 16,3,256,256] [--out profiles/blur_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM roof in TB/s (MI355X: 8 TB/s peak)")
    ap.add_argument("--shape", default="16,3,256,256")
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    args = ap.parse_args()
    from video_watermarking_forgery_detection_amd import ops
    from video_watermarking_forgery_detection_amd.noise_layers.gaussian_blur import GaussianBlur, gaussian_taps
    shape = tuple(int(v) for v in args.shape.split(","))
    B, C, H, W = shape
    elems = B * C * H * W
    x = torch.rand(shape, device="cuda")
    c = torch.rand(shape, device="cuda")
    g = torch.randn(shape, device="cuda")
    w9 = GaussianBlur()._w9
    rect = (H // 4, H // 4 + H // 2, W // 4, W // 4 + W // 2)
    cases = [("stencil3 (GaussianBlur(3))", 8, lambda: ops.stencil3(x, w9))]
    for k in (3, 7, 15):
        t = gaussian_taps(k)
        for border, bname in ((ops.BORDER_ZERO, "zero"), (ops.BORDER_REFLECT, "reflect")):
            cases.append(("gauss_sep k=%d %s fwd" % (k, bname), 8, lambda t=t, b=border: ops.gauss_sep(x, t, b)))
            cases.append(("gauss_sep k=%d %s bwd" % (k, bname), 8, lambda t=t, b=border: ops.gauss_sep_bwd(g, t, b)))
    cases.append(("cropout fwd", 12, lambda: ops.cropout_fwd(x, c, rect)))
    cases.append(("cropout bwd (gx)", 8, lambda: ops.cropout_bwd(g, rect)))
    cases.append(("cropout bwd (gx, gcover)", 12, lambda: ops.cropout_bwd(g, rect, want_cover=True)))
    for _, _, fn in cases:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for _ in range(args.iters):
        for name, _, fn in cases:          # alternating: every variant sees the same clocks and neighbours
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3)
    rows = []
    for name, bpe, _ in cases:
        t = np.array(times[name])
        med = float(np.median(t))
        row = {"case": name, "us": round(med, 2), "p10": round(float(np.percentile(t, 10)), 2), "p90": round(float(np.percentile(t, 90)), 2),
               "roof": round(bpe * elems / (med * 1e-6) / (args.hbm_tbs * 1e12), 3)}
        rows.append(row)
        print(json.dumps(row))
    line = json.dumps({"shape": list(shape), "iters": args.iters, "hbm_tbs": args.hbm_tbs, "device": torch.cuda.get_device_name(0), "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
