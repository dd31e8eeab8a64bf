#!/usr/bin/env python3
"""Generate tests/golden/swin.npz from the REFERENCE's own network/SUNet_detail.py, imported unmodified on the CPU.  Runs only where the
reference tree exists (REFERENCE_ROOT, default /root/reference); the tests read the .npz.

The reference module imports timm and thop, which the generator does not need to be installed: it puts stubs into sys.modules before the
import -- timm.models.layers.to_2tuple, trunc_normal_ (= torch.nn.init.trunc_normal_), DropPath (identity at rate 0) and thop.profile.

Parameters are NOT stored: both sides fill their modules with tests/swin_restate.fill_swin (detgen.fill_module by state_dict key, the index
and mask buffers kept; the bias table becomes N(0, 1), far from the reference's std .02 that shows nothing).  The procedure is
tests/swin_restate.run_cases, the same one the tests run on the other implementations, over swin_restate.CASES (batch 2):

    blk1   SwinTransformerBlock(dim=24, (8, 8), heads 2, window 4, shift 2, qk_scale=8)
    blk2   SwinTransformerBlock(dim=24, (14, 7), heads 2, window 7, shift 3): N = 49, not square
    blk3   SwinTransformerBlock(dim=16, (4, 4), heads 2, window 8, shift 3): collapses to window 4, shift 0
    layer  BasicLayer(dim=24, (8, 8), depth 2, heads 2, window 4)

Stored: <case>/out, <case>/gx and four parameter gradients of the float64 run; `dev32/<q>`, `devbf16/<q>` = the reference's own max
|float32 / bfloat16 CPU run - float64 run|, `amax/<q>` = max |float64 value|; `keys/<case>` = "name:shape" of the state_dicts in order;
`buf/<case>/relative_position_index`, `buf/<case>/attn_mask` = the reference's buffers of the three blocks; and for blk1 and blk2 the raw
attention core of the float64 run on the token grid: `core/<case>/qkv` [B,H,W,3C] (the qkv Linear's output, un-partitioned),
`core/<case>/table`, `core/<case>/out` [B,H,W,C] (the input of proj, windows reversed and rolled back).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_swin.py
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import swin_restate as SR  # noqa: E402

REFERENCE_ROOT = os.environ.get("REFERENCE_ROOT", "/root/reference")


def install_stubs():
    class DropPath(torch.nn.Module):
        def __init__(self, drop_prob=0.):
            super().__init__()
            assert not drop_prob

        def forward(self, x):
            return x

    timm, models, layers, thop = (types.ModuleType(n) for n in ("timm", "timm.models", "timm.models.layers", "thop"))
    layers.to_2tuple = lambda x: tuple(x) if isinstance(x, (tuple, list)) else (x, x)
    layers.trunc_normal_ = torch.nn.init.trunc_normal_
    layers.DropPath = DropPath
    thop.profile = lambda *a, **kw: (0, 0)
    timm.models, models.layers = models, layers
    sys.modules.update({"timm": timm, "timm.models": models, "timm.models.layers": layers, "thop": thop})


def core_of(block, x):
    """(qkv, out) of the block's attention core on the token grid, float64: the qkv Linear's output and proj's input, windows reversed and
    rolled back"""
    from network.SUNet_detail import window_reverse
    got = {}
    hooks = [block.attn.qkv.register_forward_hook(lambda m, i, o: got.__setitem__("qkv", o.detach())),
             block.attn.proj.register_forward_hook(lambda m, i, o: got.__setitem__("out", i[0].detach()))]
    with torch.no_grad():
        block(x)
    for h in hooks:
        h.remove()
    H, W = block.input_resolution
    ws, s = block.window_size, block.shift_size
    res = []
    for t in (got["qkv"], got["out"]):
        g = window_reverse(t.view(-1, ws, ws, t.shape[-1]), ws, H, W)
        res.append(torch.roll(g, shifts=(s, s), dims=(1, 2)) if s else g)
    return res


def main():
    install_stubs()
    sys.path.insert(0, REFERENCE_ROOT)
    from network import SUNet_detail as D

    mods = SR.build((D.SwinTransformerBlock, D.BasicLayer), torch.float32)
    inp = SR.case_inputs()
    runs = {}
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32), ("bf16", torch.bfloat16)):
        runs[tag] = SR.run_cases({k: copy.deepcopy(m).to(dtype) for k, m in mods.items()}, inp, lambda t: t.to(dtype).clone())
    out = {}
    for name, m in mods.items():
        out["keys/" + name] = np.array(SR.keys_of(m))
        if SR.CASES[name][0] == "block":
            out["buf/%s/relative_position_index" % name] = m.attn.relative_position_index.numpy()
            if m.attn_mask is not None:
                out["buf/%s/attn_mask" % name] = m.attn_mask.numpy()
    for name in SR.CORE_CASES:
        m = copy.deepcopy(mods[name]).double()
        qkv, o = core_of(m, inp[name + "/x"].double())
        out["core/%s/qkv" % name], out["core/%s/out" % name] = qkv.numpy(), o.numpy()
        out["core/%s/table" % name] = m.attn.relative_position_bias_table.detach().numpy()
    for k, v in runs["f64"].items():
        out[k] = v
        out["amax/" + k] = np.float64(np.max(np.abs(v)))
        out["dev32/" + k] = np.float64(np.max(np.abs(runs["f32"][k] - v)))
        out["devbf16/" + k] = np.float64(np.max(np.abs(runs["bf16"][k] - v)))
        print("%-58s amax %.3e  float32 deviation %.3e  bfloat16 deviation %.3e" % (k, out["amax/" + k], out["dev32/" + k], out["devbf16/" + k]))
    path = os.path.join(HERE, "swin.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
