"""The localiser's full-resolution tail (UNetDiscriminator: decoder_0(cat(e0, d1)) -> sigmoid -> NCHW f32) at configuration C5's shape --
16 frames of 256 x 256, dim = 16 -- in bfloat16 and float32:

    fused      glayers._Head2Fn (csrc/mask_head.hip): one launch forwards, one + the partial sums' finalise backwards; reads e0 and d1 in
               place: (2 dim) * sizeof(dtype) + 4 bytes per pixel forwards, 2 * (2 dim) * sizeof(dtype) + 8 backwards
    unfused    the separate launches of fused_head=False: chan_cat, the general 1x1 convolution padded to 16 output channels, the sigmoid pass,
               the layout pass (and their backward passes)

Each as forward alone (no autograd graph) and as forward + backward through autograd (the upstream gradient of the mask given).  Device events
around each call, the stages alternating in one process, median and p10 / p90 over --iters rounds.  One JSON line per dtype.

With --steps S (> 0): then the C5 step through the model surface, train.localizer_arch unet and unetd (options/train/train_hidden_c5.yml /
train_hidden_c5_unetd.yml), S steps each (the first 20 untimed), median per step: one more JSON line.  The two are different networks: the
line is information, not a comparison of implementations.

    python tools/bench_mask_head.py [--iters 200] [--batch 16] [--size 256] [--dim 16] [--steps 0]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from video_watermarking_forgery_detection_amd import glayers as G  # noqa: E402


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


def tail(a, dtype):
    gen = torch.Generator().manual_seed(1)
    B, S, dim = a.batch, a.size, a.dim
    cp = G.cpad(dim)
    e0 = torch.zeros(B, S, S, cp, dtype=dtype, device="cuda")
    d1 = torch.zeros(B, S, S, cp, dtype=dtype, device="cuda")
    e0[..., :dim] = torch.randn(B, S, S, dim, generator=gen).to("cuda", dtype)
    d1[..., :dim] = torch.randn(B, S, S, dim, generator=gen).to("cuda", dtype)
    head = G.Conv2d(2 * dim, 1, 1, 1, 0, bias_grad_f64=True).cuda()
    sig = G.Act("sigmoid")
    gy = torch.randn(B, 1, S, S, generator=gen).cuda()

    def fused(x, y):
        return G._Head2Fn.apply(x, dim, y, dim, head.weight, head.bias, 1)

    def unfused(x, y):
        return G.to_nchw(sig(head(G.chan_cat(x, dim, y, dim))), 1)

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(e0, d1)
        return run

    def fwd_bwd(fn):
        def run():
            x, y = e0.detach().requires_grad_(True), d1.detach().requires_grad_(True)
            head.weight.grad = head.bias.grad = None
            fn(x, y).backward(gy)
            return x.grad, y.grad, head.weight.grad, head.bias.grad
        return run

    stages = {"fused_fwd": fwd(fused), "unfused_fwd": fwd(unfused), "fused_fwd_bwd": fwd_bwd(fused), "unfused_fwd_bwd": fwd_bwd(unfused)}
    diff = float((stages["fused_fwd"]() - stages["unfused_fwd"]()).abs().max())
    gf, gu = stages["fused_fwd_bwd"](), stages["unfused_fwd_bwd"]()
    gdiff = [float((p.float() - q.float()).abs().max()) for p, q in zip(gf, gu)]
    times = _time(stages, a.iters)
    npix, sz = B * S * S, e0.element_size()
    out = {"dtype": str(dtype).replace("torch.", ""), "shape": [B, S, S, dim], "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "what": "device events, microseconds", "fwd_max_abs_diff": diff, "grad_max_abs_diff_ga_gb_dw_db": gdiff,
           "fused_fwd_bytes": npix * (2 * cp * sz + 4), "fused_bwd_bytes": npix * (4 * cp * sz + 8)}
    for k, v in times.items():
        v.sort()
        out[k + "_us_median"] = round(statistics.median(v), 2)
        out[k + "_us_p10_p90"] = [round(v[len(v) // 10], 2), round(v[(9 * len(v)) // 10], 2)]
    out["fused_fwd_GBps"] = round(out["fused_fwd_bytes"] / (out["fused_fwd_us_median"] * 1e-6) / 1e9, 1)
    out["unfused_over_fused_fwd"] = round(out["unfused_fwd_us_median"] / out["fused_fwd_us_median"], 3)
    out["unfused_over_fused_fwd_bwd"] = round(out["unfused_fwd_bwd_us_median"] / out["fused_fwd_bwd_us_median"], 3)
    return out


def steps(a):
    from video_watermarking_forgery_detection_amd.models.IRNrhi_model import IRNrhiModel
    from video_watermarking_forgery_detection_amd.options import options as option
    from video_watermarking_forgery_detection_amd.train import synthetic_batches
    out = {"steps": a.steps, "untimed": 20, "what": "device events around optimize_parameters, milliseconds"}
    for tag, name in (("unet", "train_hidden_c5.yml"), ("unetd", "train_hidden_c5_unetd.yml")):
        opt = option.parse(os.path.join(ROOT, "video_watermarking_forgery_detection_amd", "options", "train", name), is_train=True)
        opt['dist'] = False
        torch.manual_seed(10)
        model = IRNrhiModel(opt)
        B = opt['datasets']['train']['batch_size']
        batches = [tuple(t.pin_memory() for t in d) for d in synthetic_batches(opt, B, 0, a.steps)]
        ts = []
        for i, data in enumerate(batches):
            model.feed_data(data)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            logs, _ = model.optimize_parameters(i + 1, None)
            e1.record()
            torch.cuda.synchronize()
            if logs and i >= 20:
                ts.append(e0.elapsed_time(e1))
        ts.sort()
        out[tag + "_ms_median"] = round(statistics.median(ts), 3)
        out[tag + "_ms_p10_p90"] = [round(ts[len(ts) // 10], 3), round(ts[(9 * len(ts)) // 10], 3)]
        del model
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--steps", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mask_head: needs the GPU (a timing taken anywhere else says nothing)")
    for dtype in (torch.bfloat16, torch.float32):
        print(json.dumps(tail(a, dtype)), flush=True)
    if a.steps > 0:
        print(json.dumps({"c5_step": steps(a)}), flush=True)


if __name__ == "__main__":
    main()
