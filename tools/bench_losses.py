"""The localiser's loss stage at configuration C5's shapes (prediction and mask 16 x 1 x 256 x 256, f32) with and without the Dice term:

    BCE only      ops.bce_logits_target(pred, mask, w, chain_sigmoid=True)                       2 launches  (the stage as it was)
    BCE + Dice    the same, then ops.dice_binary(..., chain_sigmoid=True, grad_out=g_logit)       + 3 launches (sums, finalise, backward-accumulate)

Device events around each stage, the two alternating in one process, median over --iters rounds; also the Dice launches alone and the
algorithmic bytes they move.  Prints one JSON line.

    python tools/bench_losses.py [--iters 300] [--batch 16] [--size 256]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_watermarking_forgery_detection_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_losses: needs the GPU (a timing taken anywhere else says nothing)")
    g = torch.Generator().manual_seed(1)
    shape = (a.batch, 1, a.size, a.size)
    pred = torch.sigmoid(2 * torch.randn(shape, generator=g)).cuda()
    mask = (torch.rand(shape, generator=g) < 0.15).float().cuda()
    scale = torch.full((1,), 65536.0, device="cuda")

    def bce():
        return ops.bce_logits_target(pred, mask, 1.0, chain_sigmoid=True, gscale_dev=scale)

    def bce_dice():
        loss, gl = ops.bce_logits_target(pred, mask, 1.0, chain_sigmoid=True, gscale_dev=scale)
        dice, _ = ops.dice_binary(pred, mask, 1.0, 2.0, "mean", want_grad=True, chain_sigmoid=True, gscale=1.0, gscale_dev=scale, grad_out=gl)
        return loss, dice, gl

    buf = torch.zeros_like(pred)

    def dice_only():
        return ops.dice_binary(pred, mask, 1.0, 2.0, "mean", want_grad=True, chain_sigmoid=True, gscale=1.0, gscale_dev=scale, grad_out=buf)

    stages = {"bce_only": bce, "bce_plus_dice": bce_dice, "dice_only": dice_only}
    for fn in stages.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in stages}
    for _ in range(a.iters):
        for k, fn in stages.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    n = pred.numel() * 4
    out = {"shape": list(shape), "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    for k, v in times.items():
        v.sort()
        out[k + "_us_median"] = round(statistics.median(v), 2)
        out[k + "_us_p10_p90"] = [round(v[len(v) // 10], 2), round(v[(9 * len(v)) // 10], 2)]
    out["dice_added_us"] = round(out["bce_plus_dice_us_median"] - out["bce_only_us_median"], 2)
    out["dice_algorithmic_bytes"] = 2 * n + 4 * n       # sums read pred + mask; backward reads pred, mask, the gradient and writes it
    print(json.dumps(out))


if __name__ == "__main__":
    main()
