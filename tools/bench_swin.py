#!/usr/bin/env python3
"""Time one SwinTransformerBlock (network/SUNet_detail.py) with the fused attention of csrc/swin.hip against the same block with its
attention composed from torch operators and the host partition helpers (fused=False), at the reference SUNet's four stage shapes
(training.yaml: window 8, embedding 96, qk_scale 8): 64x64 tokens x 96 channels / 3 heads, 32x32 x 192 / 6, 16x16 x 384 / 12,
8x8 x 768 / 24; shifted blocks (shift 4), except the last stage, which the window covers.

    python tools/bench_swin.py [--batch 2] [--iters 50] [--dtype bf16]

Device events around forward + backward of each variant on the token grid, the two alternating in one process, median [p10, p90] in
milliseconds; one JSON line per stage.  Needs an MI355X and the built library."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ((64, 96, 3), (32, 192, 6), (16, 384, 12), (8, 768, 24))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--dtype", default="bf16", choices=("f32", "bf16", "f16"))
    a = ap.parse_args()
    from video_watermarking_forgery_detection_amd.network import SUNet_detail as D
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
    for res, dim, heads in STAGES:
        torch.manual_seed(0)
        kw = dict(dim=dim, input_resolution=(res, res), num_heads=heads, window_size=8, shift_size=4, qk_scale=8, dtype=dtype)
        blocks = {True: D.SwinTransformerBlock(**kw, fused=True).cuda()}
        blocks[False] = D.SwinTransformerBlock(**kw, fused=False).cuda()
        blocks[False].load_state_dict(blocks[True].state_dict())
        x = D.tokens_to_grid(torch.randn(a.batch, res * res, dim, device="cuda"), res, res, dtype).requires_grad_(True)
        gy = torch.randn_like(x)
        times = {True: [], False: []}
        for it in range(a.iters + 5):
            for fused in (True, False):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = blocks[fused].forward_grid(x)
                out.backward(gy)
                e1.record()
                e1.synchronize()
                x.grad = None
                blocks[fused].zero_grad()
                if it >= 5:
                    times[fused].append(e0.elapsed_time(e1))
        q = {("fused" if f else "composed"): [round(float(np.percentile(t, p)), 4) for p in (50, 10, 90)] for f, t in times.items()}
        print(json.dumps({"stage": f"{res}x{res}x{dim}", "heads": heads, "shift": blocks[True].shift_size, "batch": a.batch, "dtype": a.dtype,
                          "ms_median_p10_p90": q}))


if __name__ == "__main__":
    main()
