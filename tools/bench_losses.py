"""The localiser's loss stage at configuration C5's shapes (prediction and mask 16 x 1 x 256 x 256, f32) with and without the Dice term:

    BCE only      ops.bce_logits_target(pred, mask, w, chain_sigmoid=True)                       2 launches  (the stage as it was)
    BCE + Dice    the same, then ops.dice_binary(..., chain_sigmoid=True, grad_out=g_logit)       + 3 launches (sums, finalise, backward-accumulate)

Device events around each stage, the two alternating in one process, median over --iters rounds; also the Dice launches alone and the
algorithmic bytes they move.  Prints one JSON line.

Then the three image losses of csrc/imgloss.hip at 16 x 3 x 256 x 256 (forward + backward wrt every input), each against the same loss
composed from torch ops under autograd on the same GPU: a second JSON line, {"image_losses": ...}.

Then the GAN objectives of csrc/advloss.hip (loss + gradient, two launches each) at a discriminator map of batch x 1 x 30 x 30 and at
batch x 1 x size x size, the masked labels from a size x size mask, and the Carlini-Wagner margin at batch x 1000, each against the torch
composition under autograd: a third JSON line, {"gan_objectives": ...}.

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
    print(json.dumps({"image_losses": image_losses(a)}))
    print(json.dumps({"gan_objectives": gan_objectives(a)}))


def _torch_exclusion(x, y, level=3):
    """the exclusion loss from torch ops, as a trainer without the fused kernel would write it"""
    total = 0
    for _ in range(level):
        for dx, dy in ((x[:, :, 1:] - x[:, :, :-1], y[:, :, 1:] - y[:, :, :-1]), (x[..., 1:] - x[..., :-1], y[..., 1:] - y[..., :-1])):
            s1, s2 = 2 * torch.sigmoid(dx) - 1, 2 * torch.sigmoid(dy) - 1
            for i in range(x.shape[1]):
                for j in range(y.shape[1]):
                    total = total + (s1[:, i] ** 2 * s2[:, j] ** 2).mean() ** 0.25
        x, y = torch.nn.functional.avg_pool2d(x, 2), torch.nn.functional.avg_pool2d(y, 2)
    return total / (level * 9) / 2


def image_losses(a):
    g = torch.Generator().manual_seed(2)
    shape = (a.batch, 3, a.size, a.size)
    x, y = torch.rand(shape, generator=g).cuda(), torch.rand(shape, generator=g).cuda()
    xa, ya = x.clone().requires_grad_(True), y.clone().requires_grad_(True)

    def hip_excl():
        loss, _, coef = ops.exclusion_fwd(x, y, 3)
        return loss, ops.exclusion_bwd(x, y, coef, 3)

    def hip_recon():
        loss, gx = ops.recon_loss(x, y, "l_char", 1e-6, want_grad=True)
        return loss, gx, ops.recon_loss_bwd(x, y, "l_char", 1e-6, gscale=-1.0)

    def hip_gradl():
        return ops.gradient_loss(x), ops.gradient_loss_bwd(x)

    def torch_excl():
        return torch.autograd.grad(_torch_exclusion(xa, ya), (xa, ya))

    def torch_recon():
        d = xa - ya
        return torch.autograd.grad(torch.sqrt(d * d + 1e-6).sum((1, 2, 3)).mean(), (xa, ya))

    def torch_gradl():
        return torch.autograd.grad((xa[..., :-1] - xa[..., 1:]).abs().mean() + (xa[:, :, :-1] - xa[:, :, 1:]).abs().mean(), xa)

    stages = {"exclusion_hip": hip_excl, "exclusion_torch": torch_excl, "recon_l_char_hip": hip_recon, "recon_l_char_torch": torch_recon,
              "gradient_hip": hip_gradl, "gradient_torch": torch_gradl}
    for fn in stages.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    iters = max(10, a.iters // 6)
    times = {k: [] for k in stages}
    for _ in range(iters):
        for k, fn in stages.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    n = x.numel() * 4
    out = {"shape": list(shape), "iters": iters, "what": "forward + backward wrt every input, device events, microseconds"}
    for k, v in times.items():
        v.sort()
        out[k + "_us_median"] = round(statistics.median(v), 2)
        out[k + "_us_p10_p90"] = [round(v[len(v) // 10], 2), round(v[(9 * len(v)) // 10], 2)]
    # algorithmic bytes: the forward reads both images once; the backward reads them once more and writes the gradients
    out["algorithmic_bytes"] = {"exclusion": 2 * n + 2 * n + 2 * n, "recon": 2 * n + 2 * (2 * n + n), "gradient": n + n + n}
    return out


def gan_objectives(a):
    g = torch.Generator().manual_seed(3)
    F = torch.nn.functional
    maps = {"map30": torch.sigmoid(torch.randn((a.batch, 1, 30, 30), generator=g)).cuda(),
            "full": torch.sigmoid(torch.randn((a.batch, 1, a.size, a.size), generator=g)).cuda()}
    mask = (torch.rand((a.batch, 1, a.size, a.size), generator=g) < 0.15).float().cuda()
    logits, target = (3 * torch.randn((a.batch, 1000), generator=g)).cuda(), torch.randint(0, 1000, (a.batch,), generator=g).cuda()
    la = logits.clone().requires_grad_(True)
    stages = {}
    for name, x in maps.items():
        xa = x.clone().requires_grad_(True)
        ones = torch.ones_like(x)
        for obj, label, ref in (("bce_prob", 1.0, lambda v, o=ones: F.binary_cross_entropy(v, o)),
                                ("bce_logits", 0.9, lambda v, o=ones: F.binary_cross_entropy_with_logits(v, o * 0.9)),
                                ("mse", 1.0, lambda v, o=ones: F.mse_loss(v, o)),
                                ("hinge_disc", -1.0, lambda v: torch.relu(1 - v).mean()),
                                ("neg_mean", None, lambda v: (-v).mean())):
            stages["%s_%s_hip" % (obj, name)] = lambda x=x, obj=obj, label=label: ops.adv_loss(x, obj, label, want_grad=True)
            stages["%s_%s_torch" % (obj, name)] = lambda xa=xa, ref=ref: torch.autograd.grad(ref(xa), xa)
    x30, xa30 = maps["map30"], maps["map30"].clone().requires_grad_(True)
    stages["masked_bce_prob_map30_hip"] = lambda: ops.adv_loss(x30, "bce_prob", mask=mask, real_label=1.0, want_grad=True)
    stages["masked_bce_prob_map30_torch"] = lambda: torch.autograd.grad(
        F.binary_cross_entropy(xa30, 1.0 - F.interpolate(mask, size=(30, 30), mode="bilinear", align_corners=False)), xa30)
    stages["cw_margin_hip"] = lambda: ops.cw_margin(logits, target, True, 0.0, want_grad=True)

    def torch_cw():
        onehot = torch.eye(1000, device="cuda")[target]
        real = (onehot * la).sum(1)
        other = ((1 - onehot) * la - onehot * 10000).max(1)[0]
        return torch.autograd.grad(torch.max(other - real, torch.zeros_like(other)).sum(), la)
    stages["cw_margin_torch"] = torch_cw
    for fn in stages.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    iters = max(10, a.iters // 6)
    times = {k: [] for k in stages}
    for _ in range(iters):
        for k, fn in stages.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    out = {"shapes": {k: list(v.shape) for k, v in maps.items()}, "cw": list(logits.shape), "iters": iters,
           "what": "loss + gradient wrt the input, device events, microseconds (median)"}
    for k, v in times.items():
        out[k + "_us"] = round(statistics.median(v), 2)
    return out


if __name__ == "__main__":
    main()
