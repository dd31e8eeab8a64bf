#!/usr/bin/env python3
"""Generate tests/golden/ssim3.npz from the REFERENCE's loss.py, imported unmodified on the CPU (an empty stub module in sys.modules stands
in for torchvision, which loss.py imports and SSIM_Loss does not use).  Runs only where the reference tree exists; the tests read the .npz.

Cases and inputs: tests/ssim3_restate.py (CASES, case_inputs).  Per case, key `<case>_`:
    x, y, g                         the float32 inputs and the seeded upstream map g
    map32, map64, mean32, mean64    SSIM_Loss()(x, y) on float32 and on float64 tensors, and torch's .mean() of each
    gmean32_x, gmean32_y, gmean64_x, gmean64_y      torch.autograd gradients of map.mean()
    gmap32_x, gmap32_y, gmap64_x, gmap64_y          ... of (g * map).sum()
    dev_map, dev_mean, dev_gmean, dev_gmap          THE REFERENCE'S OWN float32-vs-float64 deviation on these inputs: map absolute; mean
        relative (torch's float32 map.mean() against the float64 one); the gradients max |g32 - g64| over the pixels kept by
        ssim3_restate.grad_keep / max |g64|, the larger of x's and y's
    kink_share                      share of the outputs within 1e-4 of a bound of the clamp in float64
Checked here, on the reference alone: every uniform case has kink_share 0, `low` stays under the 1 % cap.
`same_`: x = y (the tile case's x): map64 and the float32 map of the reference (both 0), and that its gradients are finite.

ExtendedL1Loss and GrayLoss call .cuda() in their constructors and cannot be instantiated on the CPU.  For them, and for NonBlurryLoss
alongside, the file holds float64 torch RESTATEMENTS of the cited lines (loss.py:369-376 L1Loss(mask*a, mask*b) / L1Loss(mask, 0); :388
1 - MSELoss(x, 0.5); :409-410 1 / L1Loss(x, 0.5)) with their autograd gradients, key `<shape>_<loss>[_<mask case>]_{val, ga, gb, gx}`;
NonBlurryLoss, which does construct, is also run itself and must agree with its restatement to 1e-15.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ssim3.py REFERENCE_ROOT
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ssim3_restate as R  # noqa: E402


def load(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run(mod, dt, x, y, g):
    """map, map.mean(), (d mean / dx, dy), (d (g * map).sum() / dx, dy)"""
    x, y = (torch.from_numpy(t).to(dt).requires_grad_(True) for t in (x, y))
    m = mod(x, y)
    gmean = torch.autograd.grad(m.mean(), (x, y), retain_graph=True)
    gmap = torch.autograd.grad((torch.from_numpy(g).to(dt) * m).sum(), (x, y))
    return m.detach().numpy(), float(m.detach().mean()), [t.numpy() for t in gmean], [t.numpy() for t in gmap]


def main(ref):
    sys.dont_write_bytecode = True
    for n in ("torchvision", "torchvision.models", "torchvision.transforms"):
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.path.insert(0, ref)
    ref_loss = load(ref, "loss.py", "ref_loss")
    torch.set_num_threads(1)   # one summation order, whatever the machine
    S = ref_loss.SSIM_Loss()
    out = {}
    for name in R.CASES:
        x, y, g = R.case_inputs(name)
        m32, mean32, gm32, gp32 = run(S, torch.float32, x, y, g)
        m64, mean64, gm64, gp64 = run(S, torch.float64, x, y, g)
        assert m32.dtype == np.float32 and m64.dtype == np.float64
        share = float(R.kink_outputs(x, y).mean())
        assert share == 0.0 if name != "low" else share <= R.KINK_SHARE, (name, share, "reseed ssim3_restate.case_inputs")
        keep = R.grad_keep(x, y)
        dev = {"map": R.abs_dev(m32, m64), "mean": abs(mean32 - mean64) / mean64,
               "gmean": max(R.grad_dev(a, b, keep) for a, b in zip(gm32, gm64)),
               "gmap": max(R.grad_dev(a, b, keep) for a, b in zip(gp32, gp64))}
        t = name + "_"
        out[t + "x"], out[t + "y"], out[t + "g"], out[t + "map32"], out[t + "map64"] = x, y, g, m32, m64
        out[t + "mean32"], out[t + "mean64"] = np.float32(mean32), np.float64(mean64)
        for k, v32, v64 in (("gmean", gm32, gm64), ("gmap", gp32, gp64)):
            for i, ax in enumerate("xy"):
                out[t + k + "32_" + ax], out[t + k + "64_" + ax] = v32[i], v64[i]
        out[t + "kink_share"] = np.float64(share)
        for q, v in dev.items():
            assert q == "mean" or v > 0, (name, q)
            out["%s_dev_%s" % (name, q)] = np.float64(v)
        print("%-6s dev map %.3e mean %.3e gmean %.3e gmap %.3e kink %.4f" % (name, dev["map"], dev["mean"], dev["gmean"], dev["gmap"], share))
    # x = y
    x = R.case_inputs("tile")[0]
    m32, _, gm32, _ = run(S, torch.float32, x, x.copy(), np.ones_like(x))
    m64, _, gm64, _ = run(S, torch.float64, x, x.copy(), np.ones_like(x))
    assert (m64 == 0).all() and all(np.isfinite(t).all() for t in gm32 + gm64)
    out["same_x"], out["same_map32"], out["same_map64"] = x, m32, m64
    print("x = y: reference float32 map max %.3e, float64 max %.3e" % (np.abs(m32).max(), np.abs(m64).max()))

    # the three reductions: float64 restatements of the cited lines (see the docstring), and NonBlurryLoss itself
    l1 = torch.nn.L1Loss()
    mse = torch.nn.MSELoss()
    for sname in R.RED_SHAPES:
        d = R.red_inputs(sname)
        for mcase in ("binary", "zeros", "zeromask"):
            a, b, m = (torch.from_numpy(t).double() for t in d[mcase])
            a.requires_grad_(True); b.requires_grad_(True)
            val = l1(m * a, m * b) / l1(m, torch.zeros(m.shape, dtype=m.dtype))
            ga, gb = torch.autograd.grad(val, (a, b))
            t = "%s_extl1_%s_" % (sname, mcase)
            out[t + "val"], out[t + "ga"], out[t + "gb"] = val.detach().numpy(), ga.numpy(), gb.numpy()
            assert bool(torch.isfinite(val)) == (mcase != "zeromask")
        x = torch.from_numpy(d["x"]).double().requires_grad_(True)
        val = 1 - mse(x, torch.ones_like(x) * 0.5)
        assert abs(float(val) - float(ref_loss.NonBlurryLoss()(x))) <= 1e-15
        out[sname + "_nonblurry_val"], out[sname + "_nonblurry_gx"] = val.detach().numpy(), torch.autograd.grad(val, x)[0].numpy()
        val = 1 / l1(x, torch.ones_like(x) / 2.)
        out[sname + "_gray_val"], out[sname + "_gray_gx"] = val.detach().numpy(), torch.autograd.grad(val, x)[0].numpy()
    path = os.path.join(HERE, "ssim3.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_ssim3.py REFERENCE_ROOT (the reference repository's checkout)")
    main(sys.argv[1])
