"""metrics -- the reference's scoring helpers (metrics.py:5-46, calculate_f1.py:5-41) on the device: `PSNR(max_val)`,
`EdgeAccuracy(threshold=0.5)` with their return conventions, and `mask_scores(pred, gt, thresh)` = F1 / ACC / BER / TPR / FPR of a
thresholded mask from exact integer TN / TP / FN / FP counts (one pass, csrc/ssim.hip).  Every result is a device tensor: nothing here
synchronises with the host (the reference's `if mse == 0` / `if relevant == 0 and selected == 0` branches are selects on the device)."""
import torch
import torch.nn as nn

from . import ops
from .noise_layers._device_rng import need_cuda

TN, TP, FN, FP = 0, 1, 2, 3


class PSNR(nn.Module):
    """20 log10(max_val) - 10 log10(mean((a - b)^2)) as a 0-dim device tensor; 0 when the images are equal"""

    def __init__(self, max_val):
        super().__init__()
        self.max_val = float(max_val)

    def forward(self, a, b):
        need_cuda("PSNR", a, b)
        return ops.psnr(a, b, self.max_val)[0]


def _as_mask(t):
    return t if t.dtype in (torch.float32, torch.uint8) else t.to(torch.float32)


class EdgeAccuracy(nn.Module):
    """(precision, recall) of `outputs > threshold` against the labels `inputs > threshold`, with 1e-8 added to the denominators;
    (1, 1) when neither holds a pixel"""

    def __init__(self, threshold=0.5):
        super().__init__()
        self.threshold = threshold

    def forward(self, inputs, outputs):
        need_cuda("EdgeAccuracy", inputs, outputs)
        c = ops.confusion_counts(_as_mask(outputs), _as_mask(inputs), self.threshold, self.threshold)[0].to(torch.float32)
        relevant, selected = c[TP] + c[FN], c[TP] + c[FP]
        empty = (relevant == 0) & (selected == 0)
        one = torch.ones((), device=c.device)
        return torch.where(empty, one, c[TP] / (selected + 1e-8)), torch.where(empty, one, c[TP] / (relevant + 1e-8))


def mask_scores(pred, gt, thresh):
    """scores of `pred > thresh` against `gt > thresh` over the whole batch: a dict of 0-dim device tensors -- F1 = 2TP / (2TP + FP + FN),
    ACC = (TP + TN) / all, BER = (FPR + FN / (FN + TP)) / 2, TPR = TP / (TP + FN), FPR = FP / (FP + TN) in float64 (a zero denominator gives
    nan), and the int64 counts TN, TP, FN, FP"""
    need_cuda("mask_scores", pred, gt)
    c = ops.confusion_counts(_as_mask(pred), _as_mask(gt), thresh, thresh)[0]
    return scores_from_counts(c)


def scores_from_counts(c):
    """c: int64 [..., 4] (TN, TP, FN, FP) -> the dict of mask_scores"""
    f = c.to(torch.float64)
    tn, tp, fn, fp = f[..., TN], f[..., TP], f[..., FN], f[..., FP]
    fpr = fp / (fp + tn)
    return {"F1": 2 * tp / (2 * tp + fp + fn), "ACC": (tp + tn) / (tp + fp + fn + tn), "BER": 0.5 * (fpr + fn / (fn + tp)),
            "TPR": tp / (tp + fn), "FPR": fpr, "TN": c[..., TN], "TP": c[..., TP], "FN": c[..., FN], "FP": c[..., FP]}
