#!/usr/bin/env python3
"""Generate tests/golden/instnorm_resblock.npz from the REFERENCE's own models.modules.Subnet_constructor.ResBlock, imported unmodified
on the CPU with the import stubs of make_golden.py (install_shims).  Runs only where the reference tree exists; the tests read the .npz.

The reference's forward (Subnet_constructor.py:172-179) calls `self.relu1`, which the class never defines, so the module cannot be called.
Its submodules are called here in its order instead: conv5(cat(x, conv4(conv3(conv2(conv1(x)))))) -- each convN the reference's own
nn.Sequential(Conv2d, InstanceNorm2d, ReLU); the ReLU it intends to repeat is the identity on a ReLU's output.

One case: ResBlock(3, 9) on x [2,3,8,12], parameters as torch initialises them under seed 9100, loss = sum(out * gy).  Stored:
    keys                     "name:shape" of the reference's state_dict, in its order
    norm_keys                state_dict keys of nn.InstanceNorm2d(64): affine=False (none) and affine=True
    p/<key>                  every parameter (float32)
    x, gy                    the input and the upstream gradient (float32)
    out, gx                  output and input gradient of the float64 copy
    g/conv1.0.weight, g/conv5.bias      two parameter gradients of the float64 copy
    dev32/<q>, amax/<q>      the reference's own max |float32 run - float64 run| of each stored result q, and max |float64 value|

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_instnorm.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

CIN, COUT, SHAPE = 3, 9, (2, 3, 8, 12)
STORED_GRADS = ("conv1.0.weight", "conv5.bias")


def run(block, x, gy):
    x = x.clone().requires_grad_(True)
    r = block.conv4(block.conv3(block.conv2(block.conv1(x))))
    out = block.conv5(torch.cat((x, r), dim=1))
    (out * gy).sum().backward()
    q = {"out": out, "gx": x.grad}
    params = dict(block.named_parameters())
    q.update({"g/" + k: params[k].grad for k in STORED_GRADS})
    return {k: v.detach().double().numpy() for k, v in q.items()}


def main():
    make_golden.install_shims()
    from models.modules import Subnet_constructor as S

    torch.manual_seed(9100)
    b32 = S.ResBlock(CIN, COUT)
    b64 = copy.deepcopy(b32).double()
    x = torch.randn(*SHAPE)
    gy = torch.randn(SHAPE[0], COUT, SHAPE[2], SHAPE[3])
    q32, q64 = run(b32, x, gy), run(b64, x.double(), gy.double())
    out = {"keys": np.array([f"{k}:{tuple(v.shape)}" for k, v in b32.state_dict().items()]),
           "norm_keys": np.array([",".join(torch.nn.InstanceNorm2d(64).state_dict().keys()),
                                  ",".join(torch.nn.InstanceNorm2d(64, affine=True).state_dict().keys())]),
           "x": x.numpy(), "gy": gy.numpy()}
    for k, v in b32.state_dict().items():
        out["p/" + k] = v.detach().numpy()
    for k in q64:
        out[k] = q64[k]
        out["dev32/" + k] = np.float64(np.max(np.abs(q32[k] - q64[k])))
        out["amax/" + k] = np.float64(np.max(np.abs(q64[k])))
        print("%-18s amax %.3e  float32 deviation %.3e" % (k, out["amax/" + k], out["dev32/" + k]))
    path = os.path.join(HERE, "instnorm_resblock.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
