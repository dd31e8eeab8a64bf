"""Restatement of the copy-move forgery csrc/localise.hip's copymove_kernel computes (the reference's models/IRNp_model.py:561-598 inline form
and :1007-1037 copy_move()).  Per frame b with the integer shift (sx, sy) -- rows, columns:

    ms[b,0,i,j] = clamp01(m[b,0,i-sx,j-sy])      t[b,c,i,j] = q[b,c,i-sx,j-sy]      (0 where the source index lies outside the frame)
    tampered    = q*(1-ms) + t*ms                valid = mean(ms)                   q = Q(clamp(enc)) = rint(255 clip(enc,0,1)) / 255

Two statements of it:
  * copymove(): numpy, by the index identity above, dtype-generic.  At float32 every operation is the kernel's own, one rounding each, in
    its order (the CPU tests compare it bit for bit with tests/golden/copymove.npz, recorded from the reference's method); at float64 it is
    the GPU tests' yardstick.  q is ALWAYS formed in float32 (the kernel's q is exact against that; the float64 run widens it), so the
    float64 result differs from the kernel's by the combine alone: one subtraction, two products, one sum.
  * copymove_pad_torch(): torch, the reference's own construction restated -- pad by 2|s|, write at offset |s|+s, read back at |s| -- one
    frame at a time.  The CPU tests hold the two against each other.
Also: the shift-draw helpers (a scripted np.random.rand, draws that produce a wanted shift) and the seeded inputs.  torch and numpy only."""
import numpy as np
import torch

GOLDEN_SHAPES = ((2, 3, 10, 14), (1, 1, 8, 8))
F32 = np.float32


def clamp_quant32(x):
    """wm_clamp_quant in float32: clip, one product, rint (half to even), one true division"""
    c = np.clip(np.asarray(x, F32), F32(0), F32(1))
    return (np.rint(c * F32(255)) / F32(255)).astype(F32)


def shift2d(a, sx, sy):
    """out[..., i, j] = a[..., i-sx, j-sy] where that index exists, else 0"""
    H, W = a.shape[-2:]
    out = np.zeros_like(a)
    if abs(sx) >= H or abs(sy) >= W:
        return out
    i0, i1, j0, j1 = max(sx, 0), min(H + sx, H), max(sy, 0), min(W + sy, W)
    out[..., i0:i1, j0:j1] = a[..., i0 - sx:i1 - sx, j0 - sy:j1 - sy]
    return out


def copymove(enc, mask, shifts, dtype=np.float32, quantise=True):
    """-> (q, tampered, mask_shifted) as `dtype` arrays.  enc [B,C,H,W], mask [B,1,H,W], shifts: B pairs (sx, sy).  quantise=False takes
    enc as q (the reference's method is handed an already clamped image)."""
    q = clamp_quant32(enc) if quantise else np.asarray(enc, F32)
    q = q.astype(dtype)
    m = np.clip(np.asarray(mask, F32), F32(0), F32(1)).astype(dtype)
    B = q.shape[0]
    assert len(shifts) == B and m.shape == (B, 1) + q.shape[2:]
    t, ms = np.empty_like(q), np.empty_like(m)
    for b, (sx, sy) in enumerate(shifts):
        t[b], ms[b] = shift2d(q[b], int(sx), int(sy)), shift2d(m[b], int(sx), int(sy))
    one = np.asarray(1, dtype)
    tampered = q * (one - ms) + t * ms          # numpy rounds each of the four operations: no contraction
    return q, tampered, ms


def copymove_pad_torch(q, mask, shifts):
    """the reference's construction on torch tensors (any float dtype), frame by frame: -> (tampered, mask_shifted)"""
    B, C, H, W = q.shape
    out, outm = torch.empty_like(q), torch.empty_like(mask)
    for b, (sx, sy) in enumerate(shifts):
        sx, sy = int(sx), int(sy)
        ms = torch.zeros(1, H + abs(2 * sx), W + abs(2 * sy), dtype=mask.dtype)
        ts = torch.zeros(C, H + abs(2 * sx), W + abs(2 * sy), dtype=q.dtype)
        ms[:, abs(sx) + sx:abs(sx) + sx + H, abs(sy) + sy:abs(sy) + sy + W] = mask[b]
        ts[:, abs(sx) + sx:abs(sx) + sx + H, abs(sy) + sy:abs(sy) + sy + W] = q[b]
        ms = torch.clamp(ms[:, abs(sx):abs(sx) + H, abs(sy):abs(sy) + W], 0, 1)
        ts = ts[:, abs(sx):abs(sx) + H, abs(sy):abs(sy) + W]
        out[b] = q[b] * (1 - ms) + ts * ms
        outm[b] = ms
    return out, outm


# ----------------------------------------------------------------------------- draws
def scripted(draws):
    """a stand-in for np.random.rand that hands out `draws` in order and fails when asked for more; .left() says how many remain"""
    pending = list(draws)

    def rand():
        assert pending, "more draws asked for than scripted"
        return pending.pop(0)
    rand.left = lambda: len(pending)
    return rand


def draws_for(sx, sy, H, W, frac=1.0):
    """two draws r with int(H*frac*(r-0.5)) == sx and int(W*frac*(r-0.5)) == sy: the middle of the interval that truncates to the shift.
    (They leave [0, 1) where |s| >= H*frac/2: a scripted sequence may, np.random.rand would not.)"""
    def one(s, n):
        return 0.5 + (s + (0.5 if s > 0 else -0.5 if s < 0 else 0.0)) / (n * frac)
    return [one(sx, H), one(sy, W)]


# ----------------------------------------------------------------------------- inputs
def gen_inputs(shape, seed, mask_kind):
    """(enc, mask): enc float32 uniform in [-0.1, 1.1) (so the clamp works on both sides); mask [B,1,H,W] 'binary' (a block and a few single
    pixels, different per frame) or 'fractional' (uniform in [0, 1], exact 0 and 1 among them)"""
    B, C, H, W = shape
    r = np.random.RandomState(seed)
    enc = (r.rand(*shape) * 1.2 - 0.1).astype(F32)
    if mask_kind == "binary":
        mask = np.zeros((B, 1, H, W), F32)
        for b in range(B):
            i0, j0 = r.randint(0, max(H // 2, 1)), r.randint(0, max(W // 2, 1))
            mask[b, 0, i0:i0 + max(H // 3, 1), j0:j0 + max(W // 2, 1)] = 1
            for _ in range(4):
                mask[b, 0, r.randint(0, H), r.randint(0, W)] = 1
            mask[b, 0, 0, 0] = mask[b, 0, H - 1, W - 1] = 1        # the corners: what a shift moves out of, or into, the frame first
    else:
        assert mask_kind == "fractional"
        mask = r.rand(B, 1, H, W).astype(F32)
        mask[:, :, 0, 0], mask[:, :, H - 1, W - 1] = 1, 0
    return enc, mask
