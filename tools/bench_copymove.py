"""The copy-move forgery (csrc/localise.hip copymove_kernel) beside the splice it alternates with, at configuration C5's shape -- a
16 x 3 x 256 x 256 f32 batch with `real` (the PSNR sums ride along), both through ops:

    copymove_dev    ops.copymove_fwd(enc, mask, shifts as a device int32 [B,2], real=real)      1 launch, 4*(2C+2) B per pixel
    copymove_host   the same with shifts as host pairs (adds the copy of B pairs into a fresh device tensor)
    splice          ops.splice_fwd(enc, real=real, prev=prev, mask=mask)                        1 launch, 4*(3C+1) B per pixel

Algorithmic bytes count each tensor once (enc, real read; tampered written; mask read, moved mask written once per pixel; the splice also
reads prev) and the gathers as cache hits.  Device events around each call, the three alternating in one process, median over --iters
rounds, the achieved GB/s and its share of the 8 TB/s HBM peak.  For the record only: no threshold.  One JSON line.

    python tools/bench_copymove.py [--iters 200] [--batch 16] [--size 256]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from video_watermarking_forgery_detection_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12


def _time(stages, iters, warm=10):
    for fn in stages.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in stages}
    for _ in range(iters):
        for k, fn in stages.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_copymove: needs the GPU (a timing taken anywhere else says nothing)")
    g = torch.Generator().manual_seed(1)
    B, C, S = a.batch, 3, a.size
    enc = (torch.rand(B, C, S, S, generator=g) * 1.2 - 0.1).cuda()
    real, prev = torch.rand(B, C, S, S, generator=g).cuda(), torch.rand(B, C, S, S, generator=g).cuda()
    mask = torch.zeros(B, 1, S, S)
    mask[..., S // 4:S // 2, S // 8:S // 2] = 1
    mask = mask.cuda()
    pairs = [(int(S * (float(torch.rand(1, generator=g)) - 0.5)), int(S * (float(torch.rand(1, generator=g)) - 0.5))) for _ in range(B)]
    shifts = torch.tensor(pairs, dtype=torch.int32, device="cuda")
    stages = {"copymove_dev": lambda: ops.copymove_fwd(enc, mask, shifts, real=real),
              "copymove_host": lambda: ops.copymove_fwd(enc, mask, pairs, real=real),
              "splice": lambda: ops.splice_fwd(enc, real=real, prev=prev, mask=mask)}
    times = _time(stages, a.iters)
    px = B * S * S
    nbytes = {"copymove_dev": 4 * (2 * C + 2) * px, "copymove_host": 4 * (2 * C + 2) * px, "splice": 4 * (3 * C + 1) * px}
    out = {"shape": [B, C, S, S], "iters": a.iters, "device": torch.cuda.get_device_name(0), "what": "device events, microseconds", "shifts": pairs}
    for k, v in times.items():
        v.sort()
        med = statistics.median(v)
        out[k + "_us_median"] = round(med, 2)
        out[k + "_us_p10_p90"] = [round(v[len(v) // 10], 2), round(v[(9 * len(v)) // 10], 2)]
        out[k + "_bytes"] = nbytes[k]
        out[k + "_GBps"] = round(nbytes[k] / (med * 1e-6) / 1e9, 1)
        out[k + "_share_of_hbm_peak"] = round(nbytes[k] / (med * 1e-6) / HBM_PEAK, 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
