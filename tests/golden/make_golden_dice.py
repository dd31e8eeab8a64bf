#!/usr/bin/env python3
"""Generate tests/golden/dice.npz from the REFERENCE's dice_loss module (imported unmodified; torch and numpy suffice).

Runs only where the reference tree exists, like make_golden_metrics.py.  Cases (inputs from the seeded generators of tests/dice_restate.py,
stored with the results):

    b0  2 x 1 x 32 x 32     b1  3 x 1 x 30 x 43, sample 2 with an all-zero target          pred = sigmoid(2 randn), target = rand < 0.15
    m0  2 x 4 x 32 x 32     m1  4 x 3 x 64 x 64                                             logits = 2 randn, one-hot targets (stored as labels)

Binary, per case, p in {1, 2, 3} and reduction in {mean, sum, none} (smooth = 1), key `<case>_p<p>_<reduction>_`:
    loss32, loss64     BinaryDiceLoss(p=p, reduction=reduction)(pred, target) at float32 and on float64 tensors
    grad32             float32 autograd gradient of loss.sum() wrt pred
    dev_loss           max |loss32 - loss64| / |loss64|: THE REFERENCE'S OWN float32-vs-float64 deviation
    dev_grad           max |grad32 - grad64| / max |grad64|
Multi-class, per case, ignore_index in {None, 1} (`i-` / `i1`), p = 2, the three reductions, key `<case>_<ignore>_<reduction>_`: the same five
of DiceLoss(ignore_index=..., reduction=...)(logits, target), the gradient wrt the logits (grad32 kept for reduction mean only, and at 64 x 64
without ignore_index only: the file stays small; the deviations are of every combination).  The weighted path is absent: the reference raises
AttributeError there (it reads self.weights).  `dev_*_max_binary` / `dev_*_max_multi`: the largest deviations, the basis of the tolerances.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dice.py REFERENCE_ROOT
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dice_restate as R  # noqa: E402


def run(module, x, t, dt):
    a = x.to(dt).clone().requires_grad_(True)
    loss = module(a, t.to(dt))
    (g,) = torch.autograd.grad(loss.sum(), a)
    return loss.detach(), g


def record(out, tag, module, x, t, keep_grad=True):
    l32, g32 = run(module, x, t, torch.float32)
    l64, g64 = run(module, x, t, torch.float64)
    assert l32.dtype == torch.float32 and l64.dtype == torch.float64
    out[tag + "loss32"], out[tag + "loss64"] = l32.numpy(), l64.numpy()
    if keep_grad:
        out[tag + "grad32"] = g32.numpy()
    dl = float(((l32.double() - l64).abs() / l64.abs()).max())
    dg = float((g32.double() - g64).abs().max() / g64.abs().max())
    out[tag + "dev_loss"], out[tag + "dev_grad"] = np.float64(dl), np.float64(dg)
    return dl, dg


def main(ref):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    import dice_loss as ref_dice

    torch.set_num_threads(1)   # one summation order, whatever the machine
    out = {}
    worst = {"binary": [0.0, 0.0], "multi": [0.0, 0.0]}
    for i, shape in enumerate(R.BINARY_SHAPES):
        x, t = R.gen_binary(shape, 100 + i, empty=2 if i == 1 else None)
        out["b%d_x" % i], out["b%d_t" % i] = x.numpy(), t.numpy().astype(np.uint8)
        for p in R.POWERS:
            for red in R.REDUCTIONS:
                d = record(out, "b%d_p%d_%s_" % (i, p, red), ref_dice.BinaryDiceLoss(p=p, reduction=red), x, t)
                worst["binary"] = [max(a, b) for a, b in zip(worst["binary"], d)]
    for i, shape in enumerate(R.MULTI_SHAPES):
        x, t = R.gen_multi(shape, 200 + i)
        out["m%d_x" % i], out["m%d_labels" % i] = x.numpy(), t.argmax(1, keepdim=True).numpy().astype(np.uint8)
        for ig in (None, 1):
            for red in R.REDUCTIONS:
                d = record(out, "m%d_i%s_%s_" % (i, "-" if ig is None else ig, red), ref_dice.DiceLoss(ignore_index=ig, reduction=red), x, t,
                           keep_grad=red == "mean" and (i == 0 or ig is None))
                worst["multi"] = [max(a, b) for a, b in zip(worst["multi"], d)]
    try:   # the documented difference: the reference's weighted path raises
        ref_dice.DiceLoss(weight=torch.ones(4))(*R.gen_multi(R.MULTI_SHAPES[0], 200))
        raise SystemExit("the reference's weighted DiceLoss ran: the parity note in DESIGN.md section 7 is out of date")
    except AttributeError:
        pass
    for k, (dl, dg) in worst.items():
        out["dev_loss_max_" + k], out["dev_grad_max_" + k] = np.float64(dl), np.float64(dg)
        print(k, "reference float32 vs float64: loss %.3e (relative), gradient %.3e of max |grad|" % (dl, dg))
    path = os.path.join(HERE, "dice.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_dice.py REFERENCE_ROOT (the reference repository's checkout)")
    main(sys.argv[1])
