#!/usr/bin/env python3
"""Time one InvBlockExp (models/modules/Inv_arch.py) with the fused couplings of csrc/invblock.hip against the same block composed from
chan_slice / add / coupling / chan_cat, at the two levels of the reference's x4 generator: 64x64x12 and 32x32x48 channels.

    python tools/bench_invblock.py [--batch 8] [--iters 50] [--dtype bf16]

Device events around forward + backward of each variant, the two alternating in one process, median [p10, p90] in milliseconds; one JSON
line per (level, direction).  Needs an MI355X and the built library."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--dtype", default="bf16", choices=("f32", "bf16", "f16"))
    a = ap.parse_args()
    from video_watermarking_forgery_detection_amd import glayers as G
    from video_watermarking_forgery_detection_amd.models.modules import Inv_arch as A
    from video_watermarking_forgery_detection_amd.models.modules import Subnet_constructor as S
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
    for hw, ch in ((64, 12), (32, 48)):
        torch.manual_seed(0)
        blocks = {True: A.InvBlockExp(S.DenseBlock, ch, 3, fused=True).cuda()}
        blocks[False] = A.InvBlockExp(S.DenseBlock, ch, 3, fused=False).cuda()
        blocks[False].load_state_dict(blocks[True].state_dict())
        x = G.to_nhwc(torch.randn(a.batch, ch, hw, hw, device="cuda"), dtype).requires_grad_(True)
        gy = torch.randn_like(x)
        for rev in (False, True):
            times = {True: [], False: []}
            for it in range(a.iters + 5):
                for fused in (True, False):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = blocks[fused](x, rev)
                    out.backward(gy)
                    e1.record()
                    e1.synchronize()
                    x.grad = None
                    blocks[fused].zero_grad()
                    if it >= 5:
                        times[fused].append(e0.elapsed_time(e1))
            q = {("fused" if f else "composed"): [round(float(np.percentile(t, p)), 4) for p in (50, 10, 90)] for f, t in times.items()}
            print(json.dumps({"level": f"{hw}x{hw}x{ch}", "batch": a.batch, "dtype": a.dtype, "rev": rev, "ms_median_p10_p90": q}))


if __name__ == "__main__":
    main()
