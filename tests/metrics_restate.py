"""Torch-CPU restatement of the image-quality and mask metrics the kernels of csrc/ssim.hip compute: windowed SSIM (value, autograd
gradient, and the closed-form backward the kernel implements), PSNR, the edge precision / recall pair and the confusion-count scores.
Dtype-generic: run at float32 it applies the same torch ops in the same order as the reference's pytorch_ssim / metrics modules do (the
CPU tests compare it with their recorded outputs in tests/golden/metrics.npz), run at float64 it is the yardstick of the GPU tests.
Also here: the deterministic inputs of the fixture cases (shared by the fixture generator and the tests, so nothing large is stored).
torch and numpy only."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import detgen

C1, C2 = 0.01 ** 2, 0.03 ** 2
SHAPES = ((2, 3, 16, 16), (1, 3, 30, 43), (2, 3, 64, 64), (16, 3, 256, 256))
KINDS = ("indep", "near", "equal", "smooth")
GRAD_STRIDE = 997      # the 256 x 256 case stores every 997th gradient element and sum |g|


def window11(dtype=torch.float32):
    """the 11 Gaussian taps (sigma 1.5) normalised to sum 1, EVALUATED IN FLOAT32 (a float32 vector divided by its float32 sum) and only
    then cast: a window built in float64 moves the mean SSIM by ~2e-7"""
    g = torch.tensor([math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    return (g / g.sum()).to(dtype)


def window2d(channels, dtype):
    """[channels,1,11,11]: the float32 outer product of the taps, cast to dtype"""
    w = window11().unsqueeze(1)
    return w.mm(w.t()).to(dtype).expand(channels, 1, 11, 11).contiguous()


def ssim_map(a, b):
    ch = a.shape[1]
    w = window2d(ch, a.dtype)
    mu_a = F.conv2d(a, w, padding=5, groups=ch)
    mu_b = F.conv2d(b, w, padding=5, groups=ch)
    mu_aa, mu_bb, mu_ab = mu_a.pow(2), mu_b.pow(2), mu_a * mu_b
    var_a = F.conv2d(a * a, w, padding=5, groups=ch) - mu_aa
    var_b = F.conv2d(b * b, w, padding=5, groups=ch) - mu_bb
    cov = F.conv2d(a * b, w, padding=5, groups=ch) - mu_ab
    return ((2 * mu_ab + C1) * (2 * cov + C2)) / ((mu_aa + mu_bb + C1) * (var_a + var_b + C2))


def ssim(a, b, size_average=True):
    m = ssim_map(a, b)
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def ssim_autograd(a, b, size_average=True, gout=None, wrt=0):
    """gradient of sum(gout * ssim(a, b)) wrt a (wrt=0) or b (wrt=1) through torch autograd; gout defaults to ones"""
    a = a.detach().clone().requires_grad_(wrt == 0)
    b = b.detach().clone().requires_grad_(wrt == 1)
    v = ssim(a, b, size_average)
    g = torch.ones_like(v) if gout is None else torch.as_tensor(gout, dtype=v.dtype).reshape(v.shape)
    (gr,) = torch.autograd.grad(v, a if wrt == 0 else b, g)
    return gr


def ssim_backward_formula(x, y, g):
    """the backward the kernel implements, written out: g [B,1,1,1] or [B,C,H,W] is the upstream weight per pixel of the map.
    p = w*x, m = w*y, q = w*x^2, q2 = w*y^2, r = w*xy;  grad_x = w*(g dS/dp) + 2x . w*(g dS/dq) + y . w*(g dS/dr)"""
    ch = x.shape[1]
    w = window2d(ch, x.dtype)

    def conv(t):
        return F.conv2d(t, w, padding=5, groups=ch)
    p, m, q, q2, r = conv(x), conv(y), conv(x * x), conv(y * y), conv(x * y)
    A1, A2 = 2 * p * m + C1, 2 * (r - p * m) + C2
    B1, B2 = p * p + m * m + C1, (q - p * p) + (q2 - m * m) + C2
    S = A1 * A2 / (B1 * B2)
    dp = 2 * m * (A2 - A1) / (B1 * B2) - 2 * p * S * (1 / B1 - 1 / B2)
    dq = -S / B2
    dr = 2 * A1 / (B1 * B2)
    g = g.expand_as(x)
    return conv(g * dp) + 2 * x * conv(g * dq) + y * conv(g * dr)


def psnr(a, b, max_val):
    """20 log(max_val) / log 10 - 10 log(mse) / log 10 in the dtype of a; 0 (an integer tensor, as the reference returns) when equal"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    mse = torch.mean((a - b) ** 2)
    if mse == 0:
        return torch.tensor(0)
    base10 = torch.log(torch.tensor(10.0, dtype=a.dtype))
    return 20 * torch.log(torch.tensor(max_val, dtype=a.dtype)) / base10 - 10 * torch.log(mse) / base10


def edge_accuracy(inputs, outputs, threshold=0.5):
    """(precision, recall) of outputs > threshold against inputs > threshold; (1, 1) when both are empty"""
    lab, out = inputs > threshold, outputs > threshold
    relevant, selected = lab.float().sum(), out.float().sum()
    if relevant == 0 and selected == 0:
        return torch.tensor(1), torch.tensor(1)
    tp = ((out == lab) * lab).float().sum()
    return tp / (selected + 1e-8), tp / (relevant + 1e-8)


def confusion(pred, gt, thr_pred, thr_gt):
    """numpy count -> (TN, TP, FN, FP) python ints"""
    p, g = np.asarray(pred).astype(np.float32) > np.float32(thr_pred), np.asarray(gt).astype(np.float32) > np.float32(thr_gt)
    return int((~p & ~g).sum()), int((p & g).sum()), int((~p & g).sum()), int((p & ~g).sum())


def mask_scores(TN, TP, FN, FP):
    """the scores of a confusion count in float64; a zero denominator gives nan"""
    def div(a, b):
        return float(a) / float(b) if b else float("nan")
    tpr, fpr = div(TP, TP + FN), div(FP, FP + TN)
    return {"F1": div(2 * TP, 2 * TP + FP + FN), "ACC": div(TP + TN, TP + FP + FN + TN), "BER": 0.5 * (fpr + div(FN, FN + TP)),
            "TPR": tpr, "FPR": fpr, "TN": TN, "TP": TP, "FN": FN, "FP": FP}


# ----------------------------------------------------------------------------- the fixture cases
def case_seed(si, ki):
    return 9300 + 40 * si + 10 * ki


def case_inputs(si, kind):
    """(x, y) float32 CPU tensors of shape SHAPES[si]"""
    shape = SHAPES[si]
    seed = case_seed(si, KINDS.index(kind))
    x = detgen.uniform(shape, seed)
    if kind == "indep":
        return x, detgen.uniform(shape, seed + 1)
    if kind == "near":
        return x, x + 0.02 * detgen.normal(shape, seed + 1)
    if kind == "equal":
        return x, x.clone()
    # smooth: a 7 x 7 box filter of x (zero padded) -- local variance near zero, the worst cancellation in q - p^2
    ch = shape[1]
    box = torch.full((ch, 1, 7, 7), 1.0 / 49.0)
    xs = F.conv2d(x, box, padding=3, groups=ch)
    return xs, xs + 0.01 * detgen.normal(shape, seed + 1)


def case_masks(si):
    """(pred, gt) float32 [B,1,H,W]: a soft prediction in [0,1] and a {0,1} ground truth"""
    B, _, H, W = SHAPES[si]
    seed = 9800 + 10 * si
    gt = (detgen.uniform((B, 1, H, W), seed) < 0.3).float()
    pred = (0.45 * gt + 0.7 * detgen.uniform((B, 1, H, W), seed + 1)).clamp(0, 1)   # all four outcomes occur at 0.5
    return pred, gt


def case_gout(si):
    """per-image upstream weights for the size_average=False gradient"""
    return detgen.uniform((SHAPES[si][0],), 9900 + si, 0.5, 1.5)
