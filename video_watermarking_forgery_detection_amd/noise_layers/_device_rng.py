"""The device-side generator of the stochastic attack layers (csrc/noise.hip: Philox4x32-10, state in device memory).

A layer draws its 64-bit seed from torch's default CPU generator when it is constructed -- torch.manual_seed(s) before building the layers
makes a run reproducible, and train.py's per-rank seed gives each rank its own noise -- and keeps a small device tensor {seed, offset} that
its kernels read through a pointer and advance in stream order, so an eager step and a replayed (hipGraph) step draw the same fresh numbers.
"""
import inspect

import torch

from .. import ops


class DeviceRng:
    def __init__(self):
        self.seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        self.state = None

    def state_on(self, device):
        """the state tensor on `device` (made at the first call there, offset 0)"""
        if self.state is None or self.state.device != device:
            self.state = ops.rng_state(self.seed, device)
        return self.state


def need_cuda(name, *ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(name + " runs on the HIP path only: move the input to cuda")


_ACCEPTS_COVER = {}


def accepts_cover(fn):
    """does fn(image, cover=...) exist?  Looked up from the signature (cached per function), not by catching TypeError around the call"""
    key = getattr(fn, "__func__", fn)
    hit = _ACCEPTS_COVER.get(key)
    if hit is None:
        try:
            hit = "cover" in inspect.signature(fn).parameters
        except (TypeError, ValueError):
            hit = False
        _ACCEPTS_COVER[key] = hit
    return hit


def call_fwd(layer, image, cover, **kw):
    """layer.fwd(image, **kw), with the cover when the layer's fwd takes one"""
    if accepts_cover(layer.fwd):
        return layer.fwd(image, cover=cover, **kw)
    return layer.fwd(image, **kw)
