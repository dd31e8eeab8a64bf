#!/usr/bin/env python3
"""Time the fused SSIM forward and backward (csrc/ssim.hip) with device events, warm, median of --iters calls, at 16x3x256x256 (config C2's
frames) and 8x3x512x512 -- and beside them the SAME arithmetic through torch ops on the same GPU: five grouped F.conv2d with the 11 x 11
window plus the element-wise map, autograd backward (what a user would otherwise run).  Reports time, algorithmic bytes over time and the
fraction of the HBM roof.  Algorithmic bytes per pixel-channel, from the shapes: forward 8 (read x, y), forward that also writes the three
derivative planes 20, backward 24 (read three planes, x, y; write the gradient).

    python tools/bench_metrics.py [--iters 30] [--hbm-tbs 8.0] [--out FILE.json]
    python tools/bench_metrics.py --step     # also: the C2 step (256 x 256, batch 16, Jpeg(50), bf16, replayed from the graph) with
                                             # ssim_weight 0 and 0.1 in one process, and the difference
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def median_us(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def torch_ssim(a, b, w):
    ch = a.shape[1]
    mu_a, mu_b = F.conv2d(a, w, padding=5, groups=ch), F.conv2d(b, w, padding=5, groups=ch)
    mu_aa, mu_bb, mu_ab = mu_a.pow(2), mu_b.pow(2), mu_a * mu_b
    var_a = F.conv2d(a * a, w, padding=5, groups=ch) - mu_aa
    var_b = F.conv2d(b * b, w, padding=5, groups=ch) - mu_bb
    cov = F.conv2d(a * b, w, padding=5, groups=ch) - mu_ab
    return (((2 * mu_ab + 0.01 ** 2) * (2 * cov + 0.03 ** 2)) / ((mu_aa + mu_bb + 0.01 ** 2) * (var_a + var_b + 0.03 ** 2))).mean()


def step_ms(weight, steps, warm):
    from video_watermarking_forgery_detection_amd.hidden_models import Hidden
    from video_watermarking_forgery_detection_amd.noise_layers import Jpeg
    from video_watermarking_forgery_detection_amd.options import HiDDenConfiguration
    torch.manual_seed(0)
    h = Hidden(HiDDenConfiguration(H=256, W=256), torch.device("cuda"), Jpeg(50), None, compute_dtype=torch.bfloat16, ssim_weight=weight,
               keep_dead_discriminator_grads=False)
    h.two_streams = True
    h.enable_graph()
    images, messages = torch.rand(16, 3, 256, 256, device="cuda"), torch.randint(0, 2, (16, 30), device="cuda").float()
    for _ in range(warm):
        h.train_on_batch([images, messages])
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            h.train_on_batch([images, messages])
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / steps)
    g = next(iter(h._graphs.values()))
    return statistics.median(ts), g.graph is not None and g.failed is None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM roof in TB/s (MI355X: 8 TB/s peak)")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from video_watermarking_forgery_detection_amd import ops
    g = torch.tensor([math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    rows = []
    for shape in ((16, 3, 256, 256), (8, 3, 512, 512)):
        n = 1
        for v in shape:
            n *= v
        a = torch.rand(shape, device="cuda")
        b = (a + 0.02 * torch.randn(shape, device="cuda")).contiguous()
        w = g.mm(g.t()).expand(shape[1], 1, 11, 11).contiguous().cuda()
        _, planes = ops.ssim(a, b, True, want_grad=True)
        ar = a.clone().requires_grad_(True)

        def torch_bwd():
            v = torch_ssim(ar, b, w)
            torch.autograd.grad(v, ar)
        with torch.no_grad():
            t_fwd_torch = median_us(lambda: torch_ssim(a, b, w), args.iters)
        t_fb_torch = median_us(torch_bwd, args.iters)
        cases = (("fwd", lambda: ops.ssim(a, b, True), 8, t_fwd_torch),
                 ("fwd+planes", lambda: ops.ssim(a, b, True, want_grad=True), 20, t_fwd_torch),
                 ("bwd", lambda: ops.ssim_bwd(planes, a, b), 24, t_fb_torch - t_fwd_torch))
        for name, fn, bpp, t_torch in cases:
            us = median_us(fn, args.iters)
            tbs = n * bpp / us / 1e6
            rows.append({"shape": list(shape), "kernel": name, "us": round(us, 2), "bytes": n * bpp, "TB_s": round(tbs, 3),
                         "roof_fraction": round(tbs / args.hbm_tbs, 4), "torch_ops_us": round(t_torch, 2), "speedup": round(t_torch / us, 2)})
            print("%-16s %-11s %8.1f us  %6.3f TB/s (%4.1f %% of %.0f TB/s)  torch ops %8.1f us  x%.1f" % (
                "x".join(map(str, shape)), name, us, tbs, 100 * tbs / args.hbm_tbs, args.hbm_tbs, t_torch, t_torch / us))
    out = {"kernels": rows, "iters": args.iters, "device": torch.cuda.get_device_name(0)}
    if args.step:
        off, ok0 = step_ms(0.0, 40, 12)
        on, ok1 = step_ms(0.1, 40, 12)
        out["step_c2"] = {"ssim_weight_0_ms": round(off, 4), "ssim_weight_0.1_ms": round(on, 4), "difference_ms": round(on - off, 4),
                          "replayed_from_graph": bool(ok0 and ok1)}
        print("C2 step replayed: ssim_weight 0: %.3f ms, 0.1: %.3f ms, difference %.3f ms" % (off, on, on - off))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
