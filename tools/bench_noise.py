#!/usr/bin/env python3
"""Time the forward and backward of each stochastic / JPEG-Drop attack layer at 16x3x256x256 (config C2's frames) with device events
after warm-up, and print microseconds per call and the fraction of the HBM roof from the algorithmic bytes: 24 B/px (3 channels f32, one
read + one write), 36 B/px when the cover is read too (forward of the two Dropouts) or a second gradient is written (their backward with
the cover's gradient); the Gaussian backward reads x and g and writes one gradient (36 B/px).

    python tools/bench_noise.py [--iters 200] [--hbm-tbs 8.0]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, iters, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM roof in TB/s (MI355X: 8 TB/s peak)")
    ap.add_argument("--shape", default="16,3,256,256")
    args = ap.parse_args()
    from video_watermarking_forgery_detection_amd import noise_layers as NL
    from video_watermarking_forgery_detection_amd.noise_layers.dropout import Dropout as KeepDropout
    shape = tuple(int(v) for v in args.shape.split(","))
    B, C, H, W = shape
    px = B * H * W
    x = torch.rand(shape, device="cuda")
    c = torch.rand(shape, device="cuda")
    g = torch.randn(shape, device="cuda")
    cases = [("dropout.Dropout", KeepDropout(), True, 36, 36), ("crop.Dropout", NL.Dropout(), True, 36, 36),
             ("Gaussian", NL.Gaussian(), False, 24, 36), ("GN", NL.GN(0.01), False, 24, None),
             ("SaltPepper", NL.SaltPepper(0.01), False, 24, 24), ("JpegCompression", NL.JpegCompression(), False, 24, 24)]
    rows = []
    for name, layer, cov, bf, bb in cases:
        fwd = (lambda l=layer: l.fwd(x, cover=c)) if cov else (lambda l=layer: l.fwd(x))
        _, ctx = fwd()
        us_f = timed(fwd, args.iters)
        row = {"layer": name, "fwd_us": round(us_f, 2), "fwd_roof": round(bf * px / (us_f * 1e-6) / (args.hbm_tbs * 1e12), 3)}
        if bb is not None:
            if cov:   # the cover's gradient too (the autograd path when the cover requires grad): both outputs written
                from video_watermarking_forgery_detection_amd import ops
                if isinstance(layer, KeepDropout):
                    bwd = lambda l=layer, k=ctx: ops.dropout_bwd(g, l.keep_min, l._span, k, want_cover=True)
                else:
                    bwd = lambda l=layer, k=ctx: ops.noise_bwd(ops.NOISE_DROP, g, l._prob, 0.0, k, want_cover=True)
            else:
                bwd = lambda l=layer, k=ctx: l.bwd(k, g)
            us_b = timed(bwd, args.iters)
            row.update(bwd_us=round(us_b, 2), bwd_roof=round(bb * px / (us_b * 1e-6) / (args.hbm_tbs * 1e12), 3))
        rows.append(row)
        print(json.dumps(row))
    print(json.dumps({"shape": list(shape), "hbm_tbs": args.hbm_tbs, "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
