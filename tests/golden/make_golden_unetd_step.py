#!/usr/bin/env python3
"""Generate tests/golden/unetd_step.npz: TWO consecutive training steps of the REFERENCE's own models.networks.UNetDiscriminator as its
trainers run it as the tamper localiser (IRNcrop_model.py:125-126,376-378,391-393,407-416), on the CPU in float64 and float32.  The class
is imported unmodified the way make_golden_unetd.py does (install_shims; torch.load and .cuda() replaced inside this process only).  Runs
only where the reference tree exists; the tests read the .npz.

Case `srm` of tests/unetd_restate.py (detgen parameters by state_dict key, 2 x 3 x 20 x 28), the seeded image unetd_restate.step_inputs()
and its seeded {0,1} mask.  A step: forward in train mode (the spectral norms take their power-iteration step), nn.BCEWithLogitsLoss() on
the SIGMOID output against the mask, backward, torch.optim.Adam(lr 1e-3, default betas, no weight decay) over net.parameters() (the SRM
filters never receive a gradient, so Adam leaves them alone).  Step 2 starts from step 1's parameters, moments and u / v.

Stored (data only), n = 1, 2 the step:
    in, mask                     the image and the mask (float32)
    loss<n>                      the loss (float64)
    gx1                          the input gradient of step 1 (float64)
    p<n>, p<n>/names, /sizes     every 401st value of every parameter after step n (float64), concatenated in the order of `names`
    uv<n>, uv<n>/names, /sizes   weight_u / weight_v after step n (float64; every 17th value of those longer than 256), likewise
    qnames, dev32, amax          per quantity q (loss1, gx1, p1/<parameter>, uv1/<buffer>, ...): THE REFERENCE'S OWN max |float32 run - float64
                                 run| of q over the WHOLE tensor, and max |float64 value|
    has_f16, dev16/loss1         whether torch's CPU build runs the network in float16 and, if so, |float16 loss - float32 loss| of step 1 (the
                                 loss itself evaluated in float32 on the float16 output, as under autocast)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_unetd_step.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import detgen  # noqa: E402
import make_golden  # noqa: E402
import unetd_restate as R  # noqa: E402
import unetd_step_restate as S  # noqa: E402

NAME = S.NAME


def n64(t):
    return t.detach().to(torch.float64).clone().numpy()       # (a copy: parameters and u / v change in place at the next step)


def run(cls, dt, steps=2):
    """{quantity: float64 numpy array over the whole tensor} of `steps` steps in dtype dt"""
    net = R.fill_net(cls(**R.net_kwargs(NAME)), NAME).train().to(dt)
    opt = torch.optim.Adam(net.parameters(), lr=S.LR)
    x0, mask = S.step_inputs()
    q = {}
    for n in range(1, steps + 1):
        x = x0.to(dt).requires_grad_(True)
        opt.zero_grad()
        pred, _ = net(x)
        loss = nn.BCEWithLogitsLoss()(pred.float() if dt == torch.float16 else pred, mask.to(torch.float32 if dt == torch.float16 else dt))
        loss.backward()
        opt.step()
        q[f"loss{n}"] = n64(loss)
        if n == 1:
            q["gx1"] = n64(x.grad)
        for k, p in net.named_parameters():
            q[f"p{n}/{k}"] = n64(p)
        for k, v in net.state_dict().items():
            if k.endswith("weight_u") or k.endswith("weight_v"):
                q[f"uv{n}/{k}"] = n64(v)
    return q


def main():
    make_golden.install_shims()
    torch.set_num_threads(1)       # one summation order, whatever the machine
    srm = detgen.normal((9, 3, 5, 5), 9490, std=0.2)
    saved = torch.load, torch.Tensor.cuda, nn.Module.cuda
    torch.load = lambda *a, **k: {"SRMConv2D.weight": srm.clone()}
    torch.Tensor.cuda = lambda self, *a, **k: self
    nn.Module.cuda = lambda self, *a, **k: self
    out = {}
    try:
        from models.networks import UNetDiscriminator
        q64, q32 = run(UNetDiscriminator, torch.float64), run(UNetDiscriminator, torch.float32)
        x0, mask = S.step_inputs()
        out["in"], out["mask"] = x0.numpy(), mask.numpy()
        for k in ("loss1", "loss2", "gx1"):
            out[k] = q64[k]
        for grp in S.GROUPS:       # one concatenated vector per group (hundreds of tiny arrays would cost more in zip headers than in data)
            names = [k for k in q64 if k.startswith(grp + "/")]
            out[grp + "/names"] = np.array([k[len(grp) + 1:] for k in names])
            out[grp + "/sizes"] = np.array([S.stored(k, q64[k]).size for k in names], np.int64)
            out[grp] = np.concatenate([S.stored(k, q64[k]) for k in names])
        keys = list(q64)
        out["qnames"] = np.array(keys)
        out["amax"] = np.array([np.abs(q64[k]).max() for k in keys])
        out["dev32"] = np.array([np.abs(q32[k] - q64[k]).max() for k in keys])
        worst = max((d / max(a, 1e-30), k) for d, a, k in zip(out["dev32"], out["amax"], keys))
        print("reference float32 vs float64 over two steps: largest relative deviation %.3e (%s)" % worst)
        try:
            q16 = run(UNetDiscriminator, torch.float16, steps=1)
            assert np.isfinite(q16["loss1"]).all()
            out["has_f16"] = np.int64(1)
            out["dev16/loss1"] = np.float64(np.abs(q16["loss1"] - q32["loss1"]).max())
            print("reference float16 vs float32, loss of step 1: %.3e" % out["dev16/loss1"])
        except RuntimeError as e:      # an operator torch's CPU build lacks in float16
            print("the reference does not run in float16 on the CPU: " + str(e).splitlines()[0])
            out["has_f16"] = np.int64(0)
    finally:
        torch.load, torch.Tensor.cuda, nn.Module.cuda = saved
    path = os.path.join(HERE, "unetd_step.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
