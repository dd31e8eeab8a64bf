#!/usr/bin/env python3
"""Generate tests/golden/unetd.npz from the REFERENCE's own models.networks.UNetDiscriminator and ResnetBlock, imported unmodified on the
CPU with the import stubs of make_golden.py (install_shims).  Runs only where the reference tree exists; the tests read the .npz.

ROUTE TAKEN: the reference class itself is instantiated.  Its constructor calls torch.load('MantraNetv4.pt') (a file outside its tree) and
.cuda(); inside this process only, torch.load is replaced by a function returning {'SRMConv2D.weight': a random [9,3,5,5]} and
torch.Tensor.cuda / nn.Module.cuda return self.  The first block e0 is captured by a forward hook on net.activation (use_SRM) or on
net.init_conv (the plain first block).  The fall-back route of the issue (a literal restatement of the class) was not needed.

Cases, shapes, parameters and inputs: tests/unetd_restate.py.  The two network cases run in train mode (spectral norm takes its
power-iteration step).  A committed file may hold 1 MiB at most and the two state_dicts alone are 2.6 MB, so -- as tests/golden/f1.npz
does for the networks of the same family -- parameters are NOT stored: unetd_restate.fill_net regenerates them by state_dict key, and the
fixture holds every 101st value of each as a probe the tests compare; activations and large gradients are stored subsampled
(unetd_restate.stride_of), the deviations below are taken over the WHOLE tensors.  Per network case, key `<case>/`:
    keys                       "name:shape" of the reference's state_dict, in its order
    probe/<key>                every 101st value of the parameter / buffer before the forward (float32)
    in                         the image (float32); the upstream gradients come from unetd_restate.net_inputs
    e0, x, d2, d1, gx          net.double(): first block, the three outputs, the input gradient (float64)
    g/<parameter>              every parameter gradient (float64); nograd/<parameter> where the reference leaves .grad None (the SRM filters)
    after/<buffer>             weight_u / weight_v after the step, and after/BayarConv2D.weight, the constrained filter (float64)
    dev32/<q>, amax/<q>        THE REFERENCE'S OWN max |float32 run - float64 run| of quantity q on the same inputs, and max |float64 value|
    devbf16/<q>, devf16/<q>    the same with the reference run in bfloat16 / float16 on the CPU (absent if torch's CPU build lacks an
                               operator: has_bf16 / has_f16 say so)
    bayar_min_abs_sum          the smallest |plane sum| the constraint divided by
Kernel-level cases (inputs: the seeded unetd_restate.pad_inputs / conv_inputs / bayar_inputs): `pad/<case>/{y64, gx64}` (nn.ReflectionPad2d and
its autograd adjoint in float64), `conv/<case>/{y64, gx64, gw64, amax_*, dev32_y, dev32_gx, dev32_gw}` (F.conv2d with dilation 2 in float64,
large results subsampled by unetd_restate.conv_stride, and torch's own float32 run against it over the whole tensors),
`bayar/<case>/{w, out32, out64, sum32}` (the three statements of networks.py:1059-1061 executed by torch in float32 -- out32 is what the
kernel must reproduce BIT FOR BIT -- and in float64; sum32 = torch's float32 plane sums).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_unetd.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import detgen  # noqa: E402
import make_golden  # noqa: E402
import unetd_restate as R  # noqa: E402

DT = {"64": torch.float64, "32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def n64(t):
    return t.detach().to(torch.float64).numpy()


def run_net(cls, name, dt):
    """the reference network of case `name` in dtype dt: {quantity: float64 numpy array}, the state_dict keys, the parameter probes"""
    net = R.fill_net(cls(**R.net_kwargs(name)), name).train()
    keys = np.array([f"{k}:{tuple(v.shape)}" for k, v in net.state_dict().items()])
    probes = {k: v.detach().reshape(-1)[::101].numpy().copy() for k, v in net.state_dict().items()}
    min_sum = float(net.BayarConv2D.weight.detach().double().sum((2, 3)).abs().min()) if hasattr(net, "BayarConv2D") else None
    net = net.to(dt)
    cap = {}
    hook = (net.activation if hasattr(net, "activation") else net.init_conv).register_forward_hook(lambda m, i, o: cap.__setitem__("e0", o))
    x, gy, g2, g1 = (t.to(dt) for t in R.net_inputs(name))
    x.requires_grad_(True)
    y, (d2, d1) = net(x)
    ((y * gy).sum() + (d2 * g2).sum() + (d1 * g1).sum()).backward()
    hook.remove()
    q = {"e0": n64(cap["e0"]), "x": n64(y), "d2": n64(d2), "d1": n64(d1), "gx": n64(x.grad)}
    nograd = []
    for k, p in net.named_parameters():
        if p.grad is None:
            nograd.append(k)
        else:
            q["g/" + k] = n64(p.grad)
    for k, v in net.state_dict().items():
        if k.endswith("weight_u") or k.endswith("weight_v") or k == "BayarConv2D.weight":
            q["after/" + k] = n64(v)
    return q, keys, probes, nograd, min_sum


def gen_nets(out):
    from models.networks import UNetDiscriminator
    for name in R.NET_CASES:
        q64, keys, probes, nograd, min_sum = run_net(UNetDiscriminator, name, torch.float64)
        out[f"{name}/keys"] = keys
        out[f"{name}/in"] = R.net_inputs(name)[0].numpy()
        for k, v in probes.items():
            out[f"{name}/probe/{k}"] = v
        for k in nograd:
            out[f"{name}/nograd/{k}"] = np.int64(1)
        if min_sum is not None:
            out[f"{name}/bayar_min_abs_sum"] = np.float64(min_sum)
            assert min_sum > 0.5, min_sum
        for k, v in q64.items():
            out[f"{name}/{k}"] = R.sub(v, R.stride_of(k, v.size)).copy()
            out[f"{name}/amax/{k}"] = np.float64(np.abs(v).max())
        for tag in ("32", "bf16", "f16"):
            try:
                q = run_net(UNetDiscriminator, name, DT[tag])[0]
            except RuntimeError as e:      # an operator torch's CPU build lacks in that dtype
                if tag == "32":
                    raise
                print(f"[{name}] the reference does not run in {tag} on the CPU: {str(e).splitlines()[0]}")
                out[f"{name}/has_{tag}"] = np.int64(0)
                continue
            if tag != "32":
                out[f"{name}/has_{tag}"] = np.int64(1)
            for k, v in q.items():
                assert np.isfinite(v).all(), (name, tag, k)
                out[f"{name}/dev{tag}/{k}"] = np.float64(np.abs(v - q64[k]).max())
            worst = max((out[f"{name}/dev{tag}/{k}"] / max(out[f"{name}/amax/{k}"], 1e-30), k) for k in q)
            print(f"[{name}] reference {tag} vs float64: largest relative deviation {worst[0]:.3e} ({worst[1]})")


def gen_kernels(out):
    for name, (B, H, W, CP, p) in R.PAD_CASES.items():
        x, g = R.pad_inputs(name)
        xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
        y = nn.ReflectionPad2d(p)(xt)
        y.backward(torch.from_numpy(g).double().permute(0, 3, 1, 2))
        out[f"pad/{name}/y64"], out[f"pad/{name}/gx64"] = n64(y.permute(0, 2, 3, 1)), n64(xt.grad.permute(0, 2, 3, 1))
    for name, (B, Cin, Cout, IH, IW, pad, dil) in R.CONV_CASES.items():
        x, w, g = R.conv_inputs(name)
        res = {}
        for tag in ("64", "32"):
            xt, wt = (torch.from_numpy(a).to(DT[tag]).requires_grad_(True) for a in (x, w))
            y = F.conv2d(xt, wt, None, 1, pad, dil)
            y.backward(torch.from_numpy(g).to(DT[tag]))
            res[tag] = (n64(y), n64(xt.grad), n64(wt.grad))
        for i, q in enumerate(("y", "gx", "gw")):
            out[f"conv/{name}/{q}64"] = R.sub(res["64"][i], R.conv_stride(res["64"][i].size)).copy()
            out[f"conv/{name}/amax_{q}"] = np.float64(np.abs(res["64"][i]).max())
            out[f"conv/{name}/dev32_{q}"] = np.float64(np.abs(res["32"][i] - res["64"][i]).max())
    mask = torch.ones(5, 5, dtype=torch.float64)
    mask[2, 2] = 0
    final = torch.zeros(5, 5, dtype=torch.float64)
    final[2, 2] = -1
    for name in R.BAYAR_CASES:
        w = R.bayar_inputs(name)
        for tag in ("32", "64"):
            t = torch.from_numpy(w.copy()).to(DT[tag])
            t *= mask                                                    # networks.py:1059
            if tag == "32":
                out[f"bayar/{name}/sum32"] = t.sum(axis=(2, 3)).numpy()
            t *= torch.pow(t.sum(axis=(2, 3)).view(3, 3, 1, 1), -1)      # :1060
            t += final                                                   # :1061
            out[f"bayar/{name}/out{tag}"] = t.numpy()
        out[f"bayar/{name}/w"] = w


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
        gen_nets(out)
        gen_kernels(out)
    finally:
        torch.load, torch.Tensor.cuda, nn.Module.cuda = saved
    path = os.path.join(HERE, "unetd.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
