#!/usr/bin/env python3
"""Generate tests/golden/imgloss.npz from the REFERENCE's loss.py (ExclusionLoss, GradientLoss) and models/modules/loss.py
(ReconstructionLoss), both imported unmodified; loss.py imports torchvision, which an empty stub module in sys.modules stands in for.

Runs only where the reference tree exists, like make_golden_dice.py.  Inputs come from the seeded generators of tests/imgloss_restate.py
(uniform [0, 1) float32 images); the file stores those of seed 0 as `<case>_img1`, `<case>_img2`:

    e0  2 x 3 x 32 x 32      e1  1 x 3 x 30 x 43      e2  2 x 3 x 9 x 13      e3  1 x 3 x 70 x 91      e4  1 x 1 x 8 x 8 against 1 x 2 x 8 x 8
    e0_l1, e0_l2: e0's images at level 1 and 2 (every other exclusion case: level 3)

Exclusion, key `<case>_excl_`:   loss32, loss64 (ExclusionLoss(level)(img1, img2) at float32 and on float64 tensors), means64 [level, 2, C1*C2]
    (the means under the fourth roots, in the reference's list order), grad1_32, grad2_32 (the float32 autograd gradients), and THE
    REFERENCE'S OWN float32-vs-float64 deviation: dev_loss (relative), dev_mean (relative, the largest over the terms), dev_grad (of both
    gradients, relative to max |grad64|).  e4 is the exception: the reference's _all_comb indexes img1's differences with img2's channel
    counter and raises IndexError whenever C1 != C2, so e4 holds its inputs and `e4_excl_reference_raises` = 1 and the float64 restatement
    alone is its yardstick.
Reconstruction, key `<case>_recon_<kind>_<eps>_` for e0 .. e3, kind in {l2, l_char, l1}, eps in {1e-06, 0.001}: loss32, loss64, dev_loss,
    dev_grad (wrt x; the gradient wrt the target is its negative), grad32 for e2 only.  `quirk_*`: the constructor / call behaviour.
GradientLoss, key `<case>_gradl_` for e0 .. e3, of img1: loss32, loss64, dev_loss, dev_grad, grad32 for e1 and e2.
`dev_<quantity>_max_<excl|recon|gradl>`: the largest deviation over all cases and the seeds 0, 1, 2 -- the basis of the tolerances.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_imgloss.py REFERENCE_ROOT
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import imgloss_restate as R  # noqa: E402


def load(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run(fn, dt, *xs):
    xs = [x.to(dt).clone().requires_grad_(True) for x in xs]
    loss = fn(*xs)
    return loss.detach(), [g for g in torch.autograd.grad(loss, xs)]


def devs(l32, l64, g32, g64):
    dl = float((l32.double() - l64).abs() / l64.abs())
    dg = max(float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(g32, g64))
    return dl, dg


def main(ref):
    sys.dont_write_bytecode = True
    for n in ("torchvision", "torchvision.models", "torchvision.transforms"):
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.path.insert(0, ref)
    ref_loss = load(ref, "loss.py", "ref_loss")
    ref_mloss = load(ref, os.path.join("models", "modules", "loss.py"), "ref_mloss")

    torch.set_num_threads(1)   # one summation order, whatever the machine
    out = {}
    worst = {}

    def note(key, v):
        worst[key] = max(worst.get(key, 0.0), v)

    for seed in R.SEEDS:
        keep = seed == 0
        for name in R.CASES:
            a, b, level = R.gen_case(name, seed)
            tag = name + "_excl_"
            if keep and "_" not in name:
                out[name + "_img1"], out[name + "_img2"] = a.numpy(), b.numpy()
            E = ref_loss.ExclusionLoss(level=level)
            if a.shape[1] != b.shape[1]:
                try:
                    E(a, b)
                    raise SystemExit("the reference's ExclusionLoss ran with C1 != C2: the note in DESIGN.md section 7 is out of date")
                except IndexError:
                    if keep:
                        out[tag + "reference_raises"] = np.int64(1)
                continue
            terms = {}

            def fwd(x, y):
                gx, gy = E.get_gradients(x, y)
                terms[x.dtype] = torch.stack([torch.stack(gx).reshape(level, -1), torch.stack(gy).reshape(level, -1)], dim=1).detach() ** 4
                return E(x, y)
            l32, g32 = run(fwd, torch.float32, a, b)
            l64, g64 = run(fwd, torch.float64, a, b)
            assert l32.dtype == torch.float32 and l64.dtype == torch.float64
            dl, dg = devs(l32, l64, g32, g64)
            # the means themselves: the reference's expression before ** 0.25, taken again (the fourth power of a root is not the mean)
            m = {}
            for dt in (torch.float32, torch.float64):
                m[dt] = R.exclusion_means(a.to(dt), b.to(dt), level)
                assert torch.allclose(m[dt], terms[dt], rtol=1e-5 if dt == torch.float32 else 1e-12, atol=0)
            dm = float(((m[torch.float32].double() - m[torch.float64]).abs() / m[torch.float64].abs()).max())
            note("dev_loss_max_excl", dl); note("dev_mean_max_excl", dm); note("dev_grad_max_excl", dg)
            if keep:
                out[tag + "loss32"], out[tag + "loss64"], out[tag + "means64"] = l32.numpy(), l64.numpy(), m[torch.float64].numpy()
                out[tag + "grad1_32"], out[tag + "grad2_32"] = g32[0].numpy(), g32[1].numpy()
                out[tag + "dev_loss"], out[tag + "dev_mean"], out[tag + "dev_grad"] = np.float64(dl), np.float64(dm), np.float64(dg)
        for name in R.IMAGE_CASES:
            a, b, _ = R.gen_case(name, seed)
            for kind in R.KINDS:
                for eps in R.EPS:
                    mod = ref_mloss.ReconstructionLoss(eps=eps)
                    fn = lambda x, _t=None, _b=b: mod(x, _b.to(x.dtype), kind)  # noqa: E731
                    l32, g32 = run(fn, torch.float32, a)
                    l64, g64 = run(fn, torch.float64, a)
                    dl, dg = devs(l32, l64, g32, g64)
                    note("dev_loss_max_recon", dl); note("dev_grad_max_recon", dg)
                    if keep:
                        tag = "%s_recon_%s_%g_" % (name, kind, eps)
                        out[tag + "loss32"], out[tag + "loss64"] = l32.numpy(), l64.numpy()
                        out[tag + "dev_loss"], out[tag + "dev_grad"] = np.float64(dl), np.float64(dg)
                        if name == "e2":
                            out[tag + "grad32"] = g32[0].numpy()
            G = ref_loss.GradientLoss()
            l32, g32 = run(G, torch.float32, a)
            l64, g64 = run(G, torch.float64, a)
            dl, dg = devs(l32, l64, g32, g64)
            note("dev_loss_max_gradl", dl); note("dev_grad_max_gradl", dg)
            if keep:
                tag = name + "_gradl_"
                out[tag + "loss32"], out[tag + "loss64"] = l32.numpy(), l64.numpy()
                out[tag + "dev_loss"], out[tag + "dev_grad"] = np.float64(dl), np.float64(dg)
                if name in ("e1", "e2"):
                    out[tag + "grad32"] = g32[0].numpy()
    # the constructor / call quirks of ReconstructionLoss on e2: the call-time losstype decides, the constructor's is ignored
    a, b, _ = R.gen_case("e2")
    q = ref_mloss.ReconstructionLoss(losstype="l2", eps=1e-3)
    out["quirk_ctor_l2_default_call"] = q(a.double(), b.double()).numpy()            # = l_char at eps 1e-3
    out["quirk_ctor_l2_call_l1"] = q(a.double(), b.double(), "l1").numpy()
    assert q(a, b, "nonsense") == 0
    # the documented difference: a vanished term's gradient is NaN in the reference
    c = torch.full((1, 3, 16, 16), 0.5, requires_grad=True)
    l = ref_loss.ExclusionLoss()(c, R.gen_pair((1, 3, 16, 16), (1, 3, 16, 16), 5)[1])
    (g,) = torch.autograd.grad(l, c)
    out["const_image_loss"], out["const_image_grad_is_nan"] = l.detach().numpy(), np.int64(bool(torch.isnan(g).any()))
    assert float(l.detach()) == 0.0 and bool(torch.isnan(g).any())
    for k in sorted(worst):
        out[k] = np.float64(worst[k])
        print("%-22s %.3e" % (k, worst[k]))
    path = os.path.join(HERE, "imgloss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_imgloss.py REFERENCE_ROOT (the reference repository's checkout)")
    main(sys.argv[1])
