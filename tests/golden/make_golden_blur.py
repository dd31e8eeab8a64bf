#!/usr/bin/env python3
"""Generate tests/golden/blur.npz.  Runs only where the reference tree exists (REFERENCE_ROOT, default /root/reference); the tests read the
.npz.

GaussianBlur(k), k = 5 and 7, comes from the REFERENCE's own noise_layers/gaussian_blur.py, loaded unmodified as a module of its own
(the package's __init__ imports kornia, which is not installed where this runs; the file itself needs torch and math only).  Its forward
hard-codes .cuda() (gaussian_blur.py:55), so its own layer builder get_gaussian_kernel(channels=3) is taken and run on the CPU, as
make_golden.py does for the 3 x 3 blur.  Inputs: batch 2 of 3 x 12 x 10 planes, x ~ U[0, 1), and an upstream gradient gw ~ N(0, 1) (the loss is sum(out * gw)).

    x, gw                      the inputs, float32
    gb<k>/out, gb<k>/gx        the float64 run (the layer's float32 weights, cast): output and input gradient
    dev32/gb<k>/<q>            the reference's own max |float32 run - float64 run|;  amax/gb<k>/<q> = max |float64 value|
    w2d/<k>                    the reference's float32 2-D weights [k, k]
    wdev/<k>                   max relative |those weights - the same expression evaluated in float64| (the expression of
                               gaussian_blur.py:31-38 restated in numpy float64): the weights' own float32-vs-float64 deviation

GF is kornia's GaussianBlur2d in the reference (noise_layers/gaussian_filter.py) and kornia is not installed where this runs, so the GF entries
are a RESTATEMENT, not the reference's output: F.pad(mode='reflect') by k // 2 and a depthwise conv2d with outer(t, t), t =
blur_restate.kornia_taps(k, sigma) (float32 taps), run in float64.  They are labelled so:

    gf<k>/out, gf<k>/gx        restatement, float64, for (k, sigma) = (7, 2.0) and (5, 1.0);  gf<k>/taps = t;  gf/source = what they are

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_blur.py
"""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import blur_restate as BR  # noqa: E402

REFERENCE_ROOT = os.environ.get("REFERENCE_ROOT", "/root/reference")
SHAPE = (2, 3, 12, 10)
GB_KS = (5, 7)
GF_CASES = ((7, 2.0), (5, 1.0))


def inputs():
    rs = np.random.RandomState(20240)
    return rs.random_sample(SHAPE).astype(np.float32), rs.standard_normal(SHAPE).astype(np.float32)


def run(fn, x, gw, dtype):
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = fn(xt)
    (out * torch.from_numpy(gw).to(dtype)).sum().backward()
    return {"out": out.detach().double().numpy(), "gx": xt.grad.double().numpy()}


def weights64(k, sigma=2.0):
    """gaussian_blur.py:31-38 in numpy float64"""
    c = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    g = (1.0 / (2.0 * np.pi * sigma ** 2)) * np.exp(-(c[None, :] ** 2 + c[:, None] ** 2) / (2.0 * sigma ** 2))
    return g / g.sum()


def main():
    spec = importlib.util.spec_from_file_location("reference_gaussian_blur", os.path.join(REFERENCE_ROOT, "noise_layers", "gaussian_blur.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    GaussianBlur = mod.GaussianBlur

    x, gw = inputs()
    out = {"x": x, "gw": gw}

    def store(name, r64, r32):
        for q, v in r64.items():
            key = "%s/%s" % (name, q)
            out[key] = v
            out["amax/" + key] = np.float64(np.max(np.abs(v)))
            if r32 is not None:
                out["dev32/" + key] = np.float64(np.max(np.abs(r32[q] - v)))
                print("%-12s amax %.3e  float32 deviation %.3e" % (key, out["amax/" + key], out["dev32/" + key]))

    for k in GB_KS:
        conv = GaussianBlur(kernel_size=k).get_gaussian_kernel(channels=3)
        w = conv.weight.detach()
        assert w.dtype == torch.float32 and tuple(w.shape) == (3, 1, k, k) and torch.equal(w[0], w[1]) and torch.equal(w[0], w[2])
        out["w2d/%d" % k] = w[0, 0].numpy().copy()
        w64 = weights64(k)
        out["wdev/%d" % k] = np.float64(np.max(np.abs(w[0, 0].double().numpy() - w64) / w64))
        print("k = %d: weights' float32 deviation %.3e (relative)" % (k, out["wdev/%d" % k]))
        store("gb%d" % k, run(copy.deepcopy(conv).double(), x, gw, torch.float64), run(conv, x, gw, torch.float32))

    out["gf/source"] = np.array("restatement: F.pad(reflect) + depthwise conv2d with outer(kornia_taps, kornia_taps) in float64; kornia itself is not installed")
    for k, sigma in GF_CASES:
        t = BR.kornia_taps(k, sigma)
        w = torch.from_numpy(BR.outer64(t)).view(1, 1, k, k).repeat(3, 1, 1, 1)

        def gf(xt, w=w, k=k):
            return F.conv2d(F.pad(xt, (k // 2,) * 4, mode="reflect"), w.to(xt.dtype), groups=3)
        out["gf%d/taps" % k] = t
        out["gf%d/sigma" % k] = np.float64(sigma)
        store("gf%d" % k, run(gf, x, gw, torch.float64), None)
    path = os.path.join(HERE, "blur.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
