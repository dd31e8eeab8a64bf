#!/usr/bin/env python3
"""Generate tests/golden/copymove.npz from the REFERENCE's own copy_move() (models/IRNp_model.py:1007-1037).

Runs only where the reference tree exists.  The class around the method cannot be imported without its training stack, so the method alone is
taken: the file is parsed with `ast`, the FunctionDef named copy_move is compiled as it stands and called with a stand-in `self` that carries
real_H (the method reads only its shape).  Its two surroundings are replaced: torch.Tensor.cuda is the identity for the run (no GPU is
needed), and the `np` the method sees has a scripted random.rand (tests/copymove_restate.scripted), so the two draws -- rows first, columns
second -- are the recorded ones.  Nothing of the reference's text is stored: it is read when this runs.

Cases, key `<shape index>_<mask kind>_<shift name>_`: shapes 2 x 3 x 10 x 14 and 1 x 1 x 8 x 8; masks binary and fractional in [0, 1]; shifts
positive, negative, zero, mixed in sign, and one that leaves only a corner.  copy_move() draws within a quarter of the frame
(int(H / 4 * (rand - 0.5)): at most 1 pixel at these sizes), so the draws of the larger shifts lie outside [0, 1): the construction under
test -- pad by 2|s|, write at |s|+s, read at |s| -- is the same, and the draws are recorded.  Stored per shape and mask kind
(`<shape index>_<mask kind>_src`, `_mask`): the clamped and quantised image handed in and the mask; per case: draws [2], shifts [2] (the
method's formula applied to the draws), tampered, mask_shifted.

The trainer's inline form (:561-598) differs from the method in two places only: the range factor (H instead of H / 4: frac = 1.0 of
draw_copymove_shifts) and a clamp of the moved mask to [0, 1], the identity on masks that are already there.  It is covered by the
restatement (tests/copymove_restate.py, which clamps) and by frac = 1.0 in tests/test_cpu_copymove.py, not by a second recording.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_copymove.py REFERENCE_ROOT
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import copymove_restate as R  # noqa: E402

SHIFTS = (("pos", (1, 3)), ("neg", (-2, -1)), ("zero", (0, 0)), ("mixed", (3, -4)), ("mixed2", (-1, 2)), ("corner", (-7, 7)))
FRAC = 0.25       # copy_move()'s range as draw_copymove_shifts states it


def load_method(ref):
    path = os.path.join(ref, "models", "IRNp_model.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    fns = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "copy_move"]
    assert len(fns) == 1, "expected exactly one copy_move in " + path
    mod = ast.Module(body=[fns[0]], type_ignores=[])
    env = {"torch": torch, "np": types.SimpleNamespace(random=types.SimpleNamespace(rand=None))}
    exec(compile(mod, path, "exec"), env)
    return env["copy_move"], env["np"].random


def main(ref):
    sys.dont_write_bytecode = True
    torch.set_num_threads(1)
    method, rnd = load_method(ref)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    out, n = {}, 0
    try:
        for si, shape in enumerate(R.GOLDEN_SHAPES):
            B, C, H, W = shape
            for mk in ("binary", "fractional"):
                enc, mask = R.gen_inputs(shape, 10 * si + (mk == "fractional"), mk)
                src = R.clamp_quant32(enc)
                out["%d_%s_src" % (si, mk)], out["%d_%s_mask" % (si, mk)] = src, mask
                for name, (sx, sy) in SHIFTS:
                    draws = R.draws_for(sx, sy, H, W, FRAC)
                    rnd.rand = R.scripted(draws)
                    me = types.SimpleNamespace(real_H=torch.zeros(shape))
                    tam, ms = method(me, torch.from_numpy(src.copy()), torch.from_numpy(mask.copy()))
                    assert rnd.rand.left() == 0 and tam.dtype == torch.float32 and ms.dtype == torch.float32
                    got = (int(H / 4 * (draws[0] - 0.5)), int(W / 4 * (draws[1] - 0.5)))
                    assert got == (sx, sy), (got, sx, sy)
                    tag = "%d_%s_%s_" % (si, mk, name)
                    out[tag + "draws"], out[tag + "shifts"] = np.asarray(draws, np.float64), np.asarray(got, np.int32)
                    out[tag + "tampered"], out[tag + "mask_shifted"] = tam.numpy().copy(), ms.numpy().copy()
                    n += 1
    finally:
        torch.Tensor.cuda = cuda
    path = os.path.join(HERE, "copymove.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", n, "cases")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_copymove.py REFERENCE_ROOT (the reference repository's checkout)")
    main(sys.argv[1])
