#!/usr/bin/env python3
"""Generate tests/golden/noise.npz from the REFERENCE's stochastic and JPEG-Drop attack layers.

Runs only where the reference tree exists (imported unmodified, PYTHONDONTWRITEBYTECODE=1), like make_golden.py.  The layers draw their
randomness from torch.rand, np.random.choice / np.random.uniform, np.random.normal and nn.init.normal_; each is patched for the duration of
one call to return a recorded array made by detgen (so the draws are known), and `.cuda()` to the identity.  Stored per case: the detgen
seed of the inputs, the draws and the reference's outputs; at 2x3x64x64 the per-element draws are left out (the file stays under 1 MiB):
draws(npz, tag) below remakes them from the seed, bit for bit.  JpegCompression is deterministic; only its forward is stored (its backward does
not run on current torch: an in-place unsqueeze_ on a view, jpeg_compression.py:109).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_noise.py REFERENCE_ROOT
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import detgen  # noqa: E402

SIZES = ((2, 3, 16, 16), (1, 3, 30, 43), (2, 3, 64, 64))   # 30 x 43: the padding path of JpegCompression


@contextlib.contextmanager
def patched(obj, name, fn):
    old = getattr(obj, name)
    setattr(obj, name, fn)
    try:
        yield
    finally:
        setattr(obj, name, old)


def draws(seed, shape):
    """the per-element draws of one case, from its seed (what the patched generators returned)"""
    return {"cdrop_u": detgen.uniform(shape, seed + 4).numpy(),
            "gauss_noise": (detgen.normal(shape, seed + 5) * 0.05 + 0.0).numpy(),
            "gn_noise": (0 + 0.1 * np.random.RandomState(seed + 6).standard_normal(shape)).astype(np.float32),
            "sp_u": detgen.uniform(shape, seed + 7).numpy()}


def install_shims():
    """kornia and torchvision are absent and only the layers this script does not run use them (middle_filter.py, gaussian_filter.py,
    jpeg.py): empty stand-ins let the reference's noise_layers package import"""
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    k = types.ModuleType("kornia")
    kf = types.ModuleType("kornia.filters")
    for name in ("MedianBlur", "GaussianBlur2d"):
        setattr(kf, name, type(name, (nn.Module,), {}))
    k.filters = kf
    sys.modules.setdefault("kornia", k)
    sys.modules.setdefault("kornia.filters", kf)


def main(ref):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    install_shims()
    from noise_layers.crop import Dropout as CropDropout
    from noise_layers.dropout import Dropout
    from noise_layers.gaussian import Gaussian
    from noise_layers.gaussian_noise import GN
    from noise_layers.jpeg_compression import JpegCompression
    from noise_layers.salt_pepper_noise import SaltPepper

    out = {}
    with patched(torch.Tensor, "cuda", lambda self, *a, **k: self), patched(nn.Module, "cuda", lambda self, *a, **k: self):
        for ci, shape in enumerate(SIZES):
            B, C, H, W = shape
            tag = "s%d_" % ci
            seed = 9100 + 10 * ci
            x = detgen.uniform(shape, seed)
            cover = detgen.uniform(shape, seed + 1)
            out[tag + "shape"] = np.array(shape)
            out[tag + "seed"] = np.array(seed)

            # dropout.Dropout: np.random.uniform -> the keep ratio, np.random.choice -> the H x W {0,1} mask
            ratio = float(0.5 + 0.5 * detgen.uniform((1,), seed + 2).item())
            mask = (detgen.uniform((H, W), seed + 3).numpy() < ratio).astype(np.float64)
            with patched(np.random, "uniform", lambda lo, hi: ratio), \
                    patched(np.random, "choice", lambda a, size, p=None: mask.copy()):
                y = Dropout()(x, cover)
            out[tag + "dropout_ratio"], out[tag + "dropout_mask"] = np.array(ratio), mask.astype(np.uint8)
            out[tag + "dropout_y"] = y.numpy()

            # crop.Dropout(prob=0.5): torch.rand
            u = detgen.uniform(shape, seed + 4)
            with patched(torch, "rand", lambda *s, **k: u.clone()):
                y = CropDropout(0.5)([x, cover])
            out[tag + "cdrop_u"], out[tag + "cdrop_y"] = u.numpy(), y.numpy()
            assert np.array_equal(u.numpy(), draws(seed, shape)["cdrop_u"])

            # Gaussian(): nn.init.normal_(t, mean, stddev) fills t with N(mean, stddev)
            z = detgen.normal(shape, seed + 5)
            rec = []

            def normal_(t, mean=0.0, std=1.0):
                rec.append(z * std + mean)
                return t.copy_(rec[-1])
            with patched(nn.init, "normal_", normal_):
                y = Gaussian()(x)
            out[tag + "gauss_noise"], out[tag + "gauss_y"] = rec[-1].numpy(), y.numpy()
            assert np.array_equal(rec[-1].numpy(), draws(seed, shape)["gauss_noise"])

            # GN(var=0.01): np.random.normal(mean, sd, shape), float64, cast to f32 by torch.Tensor
            zz = np.random.RandomState(seed + 6).standard_normal(shape)
            rec = []
            with patched(np.random, "normal", lambda mean, sd, size: rec.append(mean + sd * zz) or rec[-1]):
                y = GN(0.01)([x, cover])
            out[tag + "gn_noise"] = rec[-1].astype(np.float32)
            out[tag + "gn_y"] = y.numpy()
            assert np.array_equal(out[tag + "gn_noise"], draws(seed, shape)["gn_noise"])

            # SaltPepper(prob=0.1): torch.rand (a larger prob than the trainers' 0.01, so that both replacements occur at 2x3x16x16)
            u = detgen.uniform(shape, seed + 7)
            with patched(torch, "rand", lambda *s, **k: u.clone()):
                y = SaltPepper(0.1)(x)
            out[tag + "sp_u"], out[tag + "sp_y"] = u.numpy(), y.numpy()
            assert np.array_equal(u.numpy(), draws(seed, shape)["sp_u"])
            if B * H * W > 4096:
                for k in ("cdrop_u", "gauss_noise", "gn_noise", "sp_u"):
                    del out[tag + k]

            # JpegCompression: deterministic, forward only
            with torch.no_grad():
                y = JpegCompression("cpu")(x.clone())
            out[tag + "jpegc_y"] = y.numpy()
    path = os.path.join(HERE, "noise.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_noise.py REFERENCE_ROOT (the reference repository's checkout)")
    main(sys.argv[1])
