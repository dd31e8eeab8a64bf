#!/usr/bin/env python3
"""Generate tests/golden/advloss.npz from the REFERENCE's loss.py (AdversarialLoss) and models/modules/loss.py (GANLoss, CWLoss), both
imported unmodified; loss.py imports torchvision, which an empty stub module in sys.modules stands in for.

Runs only where the reference tree exists, like make_golden_imgloss.py.  Inputs come from the seeded generators of
tests/advloss_restate.py and are stored: `x_<family>_n<n>` for the element cases, `<case>_out` / `_mask` for the masked-label cases,
`<case>_logits` / `_target` for the Carlini-Wagner cases.  For every case of advloss_restate.CASES, MASK_CASES and CW_CASES, key `<case>_`:

    loss32, grad32   the reference's module on float32 tensors, and its autograd gradient wrt the discriminator output / the logits
    loss64, grad64   the same module on float64 tensors (buffers and label values: the float32 values, widened)
    dev_loss         |loss32 - the float64 RESTATEMENT's loss| on the same inputs: the reference's own float32 error, a scalar
    dev_grad         |grad32 - the restatement's gradient| per element
The GPU tests bound the kernels by 4 x these deviations with a floor of 2 float32 ulp (advloss_restate.bound).
`adv_state_dict_keys`: the keys of AdversarialLoss().state_dict().  `dev_*_max_<elem|mask|cw>`: the largest deviation RELATIVE to the value
(loss) or to max |grad64| (gradient) per family, printed for the record.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_advloss.py REFERENCE_ROOT
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import advloss_restate as R  # noqa: E402


def load(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run(fn, x, dt):
    x = torch.from_numpy(x).to(dt).requires_grad_(True)
    loss = fn(x)
    (g,) = torch.autograd.grad(loss, x)
    assert loss.dtype == dt and g.dtype == dt
    return loss.detach().numpy(), g.numpy()


def main(ref):
    sys.dont_write_bytecode = True
    warnings.filterwarnings("ignore", message=".*upsample.*")
    for n in ("torchvision", "torchvision.models", "torchvision.transforms"):
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.path.insert(0, ref)
    ref_loss = load(ref, "loss.py", "ref_loss")
    ref_mloss = load(ref, os.path.join("models", "modules", "loss.py"), "ref_mloss")
    torch.set_num_threads(1)   # one summation order, whatever the machine
    out, worst = {}, {}

    def record(case, family, l32, g32, l64, g64, want_loss, want_grad):
        out[case + "_loss32"], out[case + "_grad32"], out[case + "_loss64"], out[case + "_grad64"] = l32, g32, l64, g64
        dl, dg = abs(float(l32) - want_loss), np.abs(g32.astype(np.float64) - want_grad)
        out[case + "_dev_loss"], out[case + "_dev_grad"] = np.float64(dl), dg
        for k, v in (("dev_loss_max_" + family, dl / max(abs(want_loss), 1e-300)), ("dev_grad_max_" + family, float(dg.max() / max(np.abs(want_grad).max(), 1e-300)))):
            worst[k] = max(worst.get(k, 0.0), v)

    def module(how, dt):
        cls, typ, (real, fake), _ = how
        if cls == "adv":
            return ref_loss.AdversarialLoss(typ, real, fake).to(dt)      # (the label buffers: float32 values, widened for float64)
        return ref_mloss.GANLoss(typ, R.f32(real), R.f32(fake))

    for case, (variant, n) in R.CASES.items():
        objective, label, family, how = R.VARIANTS[variant]
        x = R.gen_input(family, n)
        out["x_%s_n%d" % (family, n)] = x
        res = [run(lambda v, _m=module(how, dt): _m(v, *how[3]), x, dt) for dt in (torch.float32, torch.float64)]
        want = R.adv_loss(objective, x, None if label is None else R.f32(label))
        record(case, "elem", *res[0], *res[1], *want)

    for case, (shape, kind, typ) in R.MASK_CASES.items():
        o, m = R.gen_mask_case(case)
        out[case + "_out"], out[case + "_mask"] = o, m
        res = []
        for dt in (torch.float32, torch.float64):
            mod = ref_loss.AdversarialLoss(typ, R.MASK_REAL_LABEL, 0.0).to(dt)
            res.append(run(lambda v, _m=mod, _k=torch.from_numpy(m).to(dt): _m(v, False, True, mask=_k), o, dt))
        want = R.adv_loss("bce_prob" if typ == "nsgan" else "mse", o, R.masked_labels(m, o.shape, R.MASK_REAL_LABEL))
        record(case, "mask", *res[0], *res[1], *want)

    cw = ref_mloss.CWLoss()
    for case, (B, K, targeted, kappa) in R.CW_CASES.items():
        z, t = R.gen_cw_case(case)
        out[case + "_logits"], out[case + "_target"] = z, t
        res = [run(lambda v: cw(v, torch.from_numpy(t), targeted, num_classes=K, kappa=kappa), z, dt) for dt in (torch.float32, torch.float64)]
        record(case, "cw", *res[0], *res[1], *R.cw_margin(z, t, targeted, kappa))

    out["adv_state_dict_keys"] = np.array(list(ref_loss.AdversarialLoss().state_dict().keys()))
    for k in sorted(worst):
        out[k] = np.float64(worst[k])
        print("%-22s %.3e" % (k, worst[k]))
    path = os.path.join(HERE, "advloss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_advloss.py REFERENCE_ROOT (the reference repository's checkout)")
    main(sys.argv[1])
