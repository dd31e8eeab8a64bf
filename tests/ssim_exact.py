"""Float64 restatements of the image-quality and mask metrics of csrc/ssim.hip -- the windowed SSIM of pytorch_ssim/__init__.py:7-40 (its
five zero-padded window sums, S, the three derivative planes dS/dp, dS/dq, dS/dr, the batch mean, the per-image means, the gradient with
respect to either image), metrics.PSNR(max_val) (metrics.py:30-46) and the confusion counts of calculate_f1.py:5-20 with their totals row
-- written from include/wm_hip.h, the header of csrc/ssim.hip and the reference's modules, with the case tables and the per-element
comparisons built on them.  A plain helper module (CPU only, never imports the HIP package): tests/test_cpu_ssim_exact.py runs float32
imitations -- faithful and defective -- through these comparisons, tests/test_gpu_ssim_exact.py runs the kernels through them.

Bounds follow the rule of tests/steploss_exact.py and tests/norm_exact.py: a float32 value made with k roundings is accepted within
FACTOR * k * 2**-24 * (the sum of the absolute values of its terms) + TINY32 (R = FACTOR * 2**-24 below); a sum kept in double from float32
terms costs D53 per addition in any order, so no bound depends on the tile grid; the float32 made from a double sum is allowed one ulp32
of the reference.  The roundings are counted from the arithmetic the header of csrc/ssim.hip lists, operation by operation:

  window sum    11 fmas along the row, 11 down the column: 22 on w*|t| (the taps are positive: the absolute terms of the column pass
                are the row sums of the absolute terms).  The reference's window is the FLOAT32 outer product of the taps
                (pytorch_ssim/__init__.py:11-15), which is what wsum() sums with; the separable kernel multiplies by w_i and by w_j in
                turn and never forms fl(w_i w_j): one more rounding per term, k = 23.  x^2, y^2 and xy are rounded once before the
                window: k = 24 for q, q2 and r.
  S, planes     the errors of p, m, q, q2, r go to first order through every intermediate (pm, pp, mm, s1, s2, s12, A1, A2, B1, B2, the
                two products, the quotient, the three reciprocals, the differences A2 - A1 and 1/B1 - 1/B2) with the absolute value of each
                float64 partial derivative, and every operation adds its own rounding on the sum of its absolute terms (mul, add, recip).
                The cancellation in q - p^2 is part of it: s1 carries the whole of 24 R w*x^2 while it may itself be near 0, which is why
                smooth and constant planes get wide bounds.  C1 and C2 are float32 constants: one more rounding on them where they enter.
  values        mean = (sum of the float32 S) / n in double: the mean of the per-pixel bounds, D53 per addition and for the division, one
                ulp32 of the reference.
  gradient      wm_ssim_bwd is compared with float64 of ITS OWN inputs: planes that are float32 data (k = 23 per plane sum, 3 for
                (a0 + 2x a1) + y a2 with its two products, 1 to 3 for g, 1 for the product with g, 1 for accumulate), and, chained behind
                the forward, with the forward's bounds passed through the same window.
  PSNR          the model of steploss_exact.psnr_ref with log(max_val) for log(255): the float32 difference squared (2), the double sums
                (D53 each), mse = fl(sum / n) (1), logf U["log"] ulps each, two products, two quotients, the difference.

Exact, with no tolerance: SENTINEL around every destination, the bits of two runs, the bits of the element-by-element staging against the
float4 staging on the same values, accumulate with power-of-two scales (g 2**k: g * inner is exact, so fused or not the sum is
fl(old + plain)), every confusion count, PSNR of equal images == 0.  SSIM has no branch on a computed value: no comparison leaves an
element out.

The uint8 threshold: for an integer v and thr >= 0, v > thr holds exactly when v > trunc(thr), so no non-negative threshold can tell a
threshold truncated to an integer from the float comparison; the table therefore adds thr = -0.5 (every uint8 is above it, 0 is not above
trunc(-0.5) = 0) to the thresholds 127.0 and 127.5.
"""
import functools
import math

import numpy as np
import torch

import detgen  # noqa: F401
from norm_exact import D53, R
from steploss_exact import EPS32, FACTOR, LN10, SENTINEL, TINY32, U, ECmp, all_ok, f64, fl, normal, nxt, r32, store, uni, ulp32, worst  # noqa: F401

C1, C2 = 0.01 ** 2, 0.03 ** 2
NT, RAD = 11, 5
TW, TH = 64, 16                                           # csrc/ssim.hip: "a workgroup owns a 64 x 16 tile of one plane"
WIN_K = 2 * NT + 1                                        # roundings of one window sum: 11 + 11 fmas, and the 2-D tap the kernel never forms
NAN = float("nan")


def taps():
    """the 11 taps as ops.ssim_window forms them (pytorch_ssim/__init__.py:7-9): a float32 vector divided by its float32 sum, then exact"""
    g = torch.tensor([math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(NT)], dtype=torch.float32)
    return (g / g.sum()).double().numpy()


WIN = taps()
WIN2 = r32(np.outer(WIN, WIN))                            # pytorch_ssim/__init__.py:11-15: the FLOAT32 outer product of the taps is the window


def wsum(t):
    """the zero-padded 11 x 11 window sum of every pixel of [..., H, W] in float64, tap by tap of the 2-D window"""
    H, W = t.shape[-2:]
    pad = np.zeros(t.shape[:-2] + (H + 2 * RAD, W + 2 * RAD))
    pad[..., RAD:RAD + H, RAD:RAD + W] = t
    out = np.zeros(t.shape)
    for i in range(NT):
        for j in range(NT):
            out += WIN2[i, j] * pad[..., i:i + H, j:j + W]
    return out


# ----------------------------------------------------------------------------------------------------------------- first-order propagation
def mul(a, da, b, db):
    v = a * b
    return v, np.abs(b) * da + np.abs(a) * db + R * np.abs(v)


def add(a, da, b, db, sign=1.0):
    """a + sign b: one rounding on |a| + |b|"""
    return a + sign * b, da + db + R * (np.abs(a) + np.abs(b))


def recip(a, da):
    v = 1.0 / a
    return v, da / (a * a) + R * np.abs(v)


def forward_ref(x, y):
    """x, y [..., H, W] float64 holding float32 values -> dict of the five sums, S, the planes [3, ...] and the bound of each"""
    p, m, q, q2, r = wsum(x), wsum(y), wsum(x * x), wsum(y * y), wsum(x * y)
    ep, em = WIN_K * R * wsum(np.abs(x)), WIN_K * R * wsum(np.abs(y))
    eq, eq2, er = (WIN_K + 1) * R * q, (WIN_K + 1) * R * q2, (WIN_K + 1) * R * wsum(np.abs(x * y))
    pm, dpm = mul(p, ep, m, em)
    pp, dpp = mul(p, ep, p, ep)
    mm, dmm = mul(m, em, m, em)
    s1, ds1 = add(q, eq, pp, dpp, -1.0)
    s2, ds2 = add(q2, eq2, mm, dmm, -1.0)
    s12, ds12 = add(r, er, pm, dpm, -1.0)
    A1, dA1 = add(2 * pm, 2 * dpm, C1, R * C1)
    A2, dA2 = add(2 * s12, 2 * ds12, C2, R * C2)
    t, dt = add(pp, dpp, mm, dmm)
    B1, dB1 = add(t, dt, C1, R * C1)
    t, dt = add(s1, ds1, s2, ds2)
    B2, dB2 = add(t, dt, C2, R * C2)
    N, dN = mul(A1, dA1, A2, dA2)
    D, dD = mul(B1, dB1, B2, dB2)
    S = N / D
    dS = dN / np.abs(D) + np.abs(N) * dD / (D * D) + R * np.abs(S)
    inv, dinv = recip(D, dD)
    i1, di1 = recip(B1, dB1)
    i2, di2 = recip(B2, dB2)
    t1, dt1 = add(A2, dA2, A1, dA1, -1.0)
    u1, du1 = mul(2 * m, 2 * em, t1, dt1)
    v1, dv1 = mul(u1, du1, inv, dinv)
    t2, dt2 = add(i1, di1, i2, di2, -1.0)
    u2, du2 = mul(2 * p, 2 * ep, S, dS)
    v2, dv2 = mul(u2, du2, t2, dt2)
    Dp, dDp = add(v1, dv1, v2, dv2, -1.0)
    Dq, dDq = mul(-S, dS, i2, di2)
    Dr, dDr = mul(2 * A1, 2 * dA1, inv, dinv)
    return {"sums": (p, m, q, q2, r), "S": S, "bS": dS + TINY32, "planes": np.stack([Dp, Dq, Dr]), "bplanes": np.stack([dDp, dDq, dDr]) + TINY32}


def means_ref(S, bS):
    """S [B, C, H, W] -> (mean, bound, per-image means [B], bounds)"""
    B, n = S.shape[0], S[0].size
    flat, bflat = S.reshape(B, n), bS.reshape(B, n)
    img = flat.mean(1)
    bimg = bflat.mean(1) + D53 * (n + 1) * np.abs(flat).mean(1)
    mean = flat.mean()
    bmean = bflat.mean() + D53 * (B * n + 1) * np.abs(flat).mean()
    return mean, bmean + ulp32(mean), img, bimg + ulp32(img)


def upstream(B, C, H, W, per_image=False, gscale=1.0, gdev=None, gout=None):
    """(g [B] in float64, its roundings): float32(gscale) / (C H W [B]) rounded once, times gscale_dev[0], times gout[per_image ? b : 0]"""
    g = np.full(B, float(np.float32(gscale)) / (float(C) * H * W * (1.0 if per_image else float(B))))
    k = 1
    if gdev is not None:
        g, k = g * float(np.float32(gdev)), k + 1
    if gout is not None:
        go = r32(np.asarray(gout, dtype=np.float64)).reshape(-1)
        assert go.size == (B if per_image else 1)
        g, k = g * (go if per_image else go[0]), k + 1
    return g, k


def plane_sums(planes, bplanes=None):
    """the window sums of the three planes and their bounds: k = WIN_K on w*|D|, and what the planes themselves may be off by"""
    a = [wsum(planes[i]) for i in range(3)]
    return a, [WIN_K * R * wsum(np.abs(planes[i])) + (0.0 if bplanes is None else wsum(bplanes[i])) for i in range(3)]


def grad_ref(planes, x, y, bplanes=None, old=None, sums=None, **up):
    """the gradient wrt x from the three planes [3, B, C, H, W] (float32 data unless bplanes says how far they may be off):
    g * (w*Dp + 2x . w*Dq + y . w*Dr), + old with accumulate -> (value, bound)"""
    B, C, H, W = x.shape
    a, da = plane_sums(planes, bplanes) if sums is None else sums
    t1, t2 = 2 * x * a[1], y * a[2]
    inner = a[0] + t1 + t2
    dinner = da[0] + 2 * np.abs(x) * da[1] + np.abs(y) * da[2] + 3 * R * (np.abs(a[0]) + np.abs(t1) + np.abs(t2))
    g, k = upstream(B, C, H, W, **up)
    g = g.reshape(B, 1, 1, 1)
    v = g * inner
    dv = np.abs(g) * dinner + (k + 1) * R * np.abs(v)
    if old is not None:
        dv = dv + R * (np.abs(old) + np.abs(v))
        v = v + old
    return v, dv + TINY32


# ----------------------------------------------------------------------------------------------------------------- SSIM cases
HEIGHTS = (1, 3, 6, 11, 16, 17, 21, 32, 33)
WIDTHS = (1, 5, 6, 11, 43, 64, 65, 68, 70, 72, 128, 132)
SHAPES = (      # every height with a width <= 11 and one >= 43, every width with a height <= 11 and one >= 16
    (1, 1), (1, 70), (1, 128),          # one row: every row of the window but one is padding
    (3, 5), (3, 68), (3, 72),           # a plane smaller than the window radius; with a second tile column of one and of two float4s
    (6, 6), (6, 43), (6, 65), (6, 132),  # the first plane whose far edge is out of a corner pixel's reach; one scalar column past the seam
    (11, 11), (11, 64),                 # the window's own size; exactly one tile column
    (16, 5), (16, 64), (16, 132),       # exactly one tile row: its lower halo is all padding; three tile columns, the last of one float4
    (17, 1), (17, 65), (17, 68),        # a second tile row one row deep, with one column, one scalar column and one float4 past the seam
    (21, 6), (21, 43), (21, 128),       # the second tile row as deep as the halo; two whole tile columns
    (32, 5), (32, 11), (32, 72),        # two whole tile rows
    (33, 1), (33, 70), (33, 132))       # three tile rows; W % 4 == 2 past the seam; the largest plane: 3 x 3 tiles
BCS = ((1, 1), (1, 3), (3, 1), (2, 3), (3, 4))
KINDS = ("indep", "near", "equal", "smooth", "const", "impulse")
CONST_X, CONST_Y = float(np.float32(0.3)), float(np.float32(0.7))
GRAD_MODES = (      # how wm_ssim_bwd is driven: the mean's weight and the per-image weight, host scale, device scale, accumulate
    dict(),
    dict(per_image=True, gout="per_image"),
    dict(gout="one", gscale=0.7, gdev=1.5),
    dict(accumulate=True),
    dict(per_image=True, gout="per_image", gscale=-0.25, gdev=0.5, accumulate=True))


def box7(x):
    """the 7 x 7 zero-padded box mean metrics_restate's `smooth` kind filters with"""
    H, W = x.shape[-2:]
    pad = np.zeros(x.shape[:-2] + (H + 6, W + 6))
    pad[..., 3:3 + H, 3:3 + W] = x
    h = sum(pad[..., :, k:k + W] for k in range(7))
    return sum(h[..., k:k + H, :] for k in range(7)) / 49.0


def impulse_positions(H, W):
    """where an impulse names a tap pair that a wrong halo would move: the four corners, both sides of every tile seam, and 5 and 6 pixels
    (the window radius and one more) from a seam or an edge"""
    rows = {0, H - 1, RAD, RAD + 1, H - 1 - RAD, H - 2 - RAD}
    cols = {0, W - 1, RAD, RAD + 1, W - 1 - RAD, W - 2 - RAD}
    for s in range(TH, H, TH):
        rows |= {s - 1, s, s - RAD, s - RAD - 1, s + RAD, s + RAD - 1, s + RAD + 1}
    for s in range(TW, W, TW):
        cols |= {s - 1, s, s - RAD, s - RAD - 1, s + RAD, s + RAD - 1, s + RAD + 1}
    rows, cols = sorted(r for r in rows if 0 <= r < H), sorted(c for c in cols if 0 <= c < W)
    n = max(len(rows), len(cols))
    pos = [(rows[i % len(rows)], cols[i % len(cols)]) for i in range(n)]                       # every listed row and column once
    pos += [(rows[i % len(rows)], cols[(i * 5 + 3) % len(cols)]) for i in range(n)]            # and crossed
    fixed = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)] + [(r, c) for r, c in ((15, 63), (16, 64), (15, 64), (16, 63)) if r < H and c < W]
    return list(dict.fromkeys(fixed + pos))


def make_inputs(kind, shape, seed, first=0):
    """(x, y) float64 arrays of float32 values; the first four kinds are metrics_restate's"""
    x = uni(shape, seed)
    if kind == "indep":
        return x, uni(shape, seed + 1)
    if kind == "near":
        return x, r32(x + 0.02 * normal(shape, seed + 1))
    if kind == "equal":
        return x, x.copy()
    if kind == "smooth":
        xs = r32(box7(x))
        return xs, r32(xs + 0.01 * normal(shape, seed + 1))
    if kind == "const":
        return np.full(shape, CONST_X), np.full(shape, CONST_Y)
    B, C, H, W = shape
    pos = impulse_positions(H, W)
    x, y = np.zeros(shape), np.zeros(shape)
    for n in range(B * C):
        a = pos[(first + n) % len(pos)]
        b = a if n % 2 == 0 else pos[(first + n + 1) % len(pos)]                               # the same pixel, or elsewhere
        x[n // C, n % C][a] = 1.0
        y[n // C, n % C][b] = 1.0
    return x, y


class SsimCase:
    """one shape, batch and input kind of wm_ssim_fwd / _finalize / _bwd; side 0 is (x, y), side 1 the swapped call that gives y's gradient"""

    def __init__(self, H, W, B, C, kind, first=0):
        self.H, self.W, self.B, self.C, self.kind = H, W, B, C, kind
        self.shape = (B, C, H, W)
        self.label = "ssim %dx%d B=%d C=%d %s%s" % (H, W, B, C, kind, "@%d" % first if kind == "impulse" else "")
        seed = 31000 + 131 * H + 7 * W + 17 * B + 3 * C + 1000 * KINDS.index(kind)
        self.x, self.y = make_inputs(kind, self.shape, seed, first)
        self.gout = r32(0.5 + 0.375 * np.arange(B))                                            # distinct per image: n / C indexing shows
        self.gone = r32(np.array([0.75]))
        self.old = r32(1e-3 * normal(self.shape, seed + 5))
        self.nparts = C * (-(-H // TH)) * (-(-W // TW))
        self.vec_ok = W % 4 == 0

    def xy(self, side):
        return (self.x, self.y) if side == 0 else (self.y, self.x)

    @functools.lru_cache(maxsize=None)
    def fwd(self, side=0):
        a, b = self.xy(side)
        f = forward_ref(a, b)
        f["mean"], f["bmean"], f["img"], f["bimg"] = means_ref(f["S"], f["bS"])
        f["planes32"] = r32(f["planes"])                                                         # what the backward is fed on its own
        return f

    def check_planes(self, dplanes, side=0, tag=""):
        f, got = self.fwd(side), f64(dplanes).reshape((3,) + self.shape)
        return [ECmp("%s side %d%s %s" % (self.label, side, tag, n), got[i], f["planes"][i], f["bplanes"][i]) for i, n in enumerate(("dS/dp", "dS/dq", "dS/dr"))]

    def check_values(self, out, side=0, tag=""):
        f, o = self.fwd(side), f64(out).reshape(1 + self.B)
        return [ECmp("%s side %d%s mean" % (self.label, side, tag), o[:1], [f["mean"]], [f["bmean"]]),
                ECmp("%s side %d%s per-image means" % (self.label, side, tag), o[1:], f["img"], f["bimg"])]

    def check_partials(self, partials, side=0):
        """the per-workgroup doubles: their sum per image against the float64 sum of S"""
        f, q = self.fwd(side), f64(partials).reshape(self.B, self.nparts)
        n = self.C * self.H * self.W
        tot = f["S"].reshape(self.B, n)
        return [ECmp("%s side %d partial sums per image" % (self.label, side), q.sum(1), tot.sum(1),
                     f["bS"].reshape(self.B, n).sum(1) + D53 * (n + 1) * np.abs(tot).sum(1))]

    @functools.lru_cache(maxsize=None)
    def sums(self, side, chain):
        f = self.fwd(side)
        return plane_sums(f["planes"], f["bplanes"]) if chain else plane_sums(f["planes32"])

    def mode(self, m):
        """a GRAD_MODES entry resolved: (the keywords of upstream(), accumulate)"""
        up = {k: v for k, v in m.items() if k != "accumulate"}
        if up.get("gout") == "per_image":
            up["gout"] = self.gout
        elif up.get("gout") == "one":
            up["gout"] = self.gone
        return up, bool(m.get("accumulate"))

    def grad(self, m, side=0, chain=False):
        a, b = self.xy(side)
        up, acc = self.mode(m)
        return grad_ref(None, a, b, old=self.old if acc else None, sums=self.sums(side, chain), **up)

    def check_grad(self, grad, m, side=0, chain=False, tag=""):
        v, bv = self.grad(m, side, chain)
        name = " ".join("%s=%s" % (k, w) for k, w in sorted(m.items())) or "mean"
        return [ECmp("%s side %d%s grad%s [%s]" % (self.label, side, tag, " chained" if chain else "", name), f64(grad).reshape(self.shape), v, bv)]

    def pow2_scales(self):
        """upstream keywords that make g = 2**-3 exactly: gscale = C H W B / 4 (an integer below 2**24: the host quotient is exact), device
        scale 1/4, mean's upstream 2"""
        return dict(gscale=float(self.C * self.H * self.W * self.B) / 4.0, gdev=0.25, gout=np.array([2.0]))


@functools.lru_cache(maxsize=None)
def ssim_case(*key):
    return SsimCase(*key)


def ssim_keys():
    """(H, W, B, C, kind, first): every shape with (B, C) and the five dense kinds taking turns; the five kinds and the five (B, C) at the
    two-tile shapes the issue names; impulse pairs, twelve planes at a time, over every listed position of the 3 x 3-tile plane and of
    the two-tile planes 17 x 65 and 17 x 68"""
    keys = []
    for i, (H, W) in enumerate(SHAPES):
        B, C = BCS[i % 5]
        keys.append((H, W, B, C, KINDS[(i // 5 + i) % 5], 0))
    for j, kind in enumerate(KINDS[:5]):
        keys.append((17, 68, BCS[(j + 3) % 5][0], BCS[(j + 3) % 5][1], kind, 0))
        keys.append((33, 70, BCS[(j + 1) % 5][0], BCS[(j + 1) % 5][1], kind, 0))
        keys.append((16, 132, BCS[j][0], BCS[j][1], kind, 0))
    for H, W in ((33, 132), (17, 65), (17, 68), (3, 5), (1, 1)):
        n = len(impulse_positions(H, W))
        keys += [(H, W, 3, 4, "impulse", first) for first in range(0, n, 12)]
    return tuple(dict.fromkeys(keys))


SSIM_GROUPS = ("small", "one-tile-row", "two-tile-rows", "impulse")


def ssim_group(key):
    H, kind = key[0], key[4]
    return "impulse" if kind == "impulse" else "small" if H <= 11 else "one-tile-row" if H <= 16 else "two-tile-rows"


def ssim_group_keys(group):
    return tuple(k for k in ssim_keys() if ssim_group(k) == group)


# ----------------------------------------------------------------------------------------------------------------- PSNR
PSNR_CAP = 1024                                           # ops._nparts: one partial per 4096 elements, at most 1024
PSNR_N = (1, 255, 256, 257, 4097, PSNR_CAP * 4096 + 4097)  # 4097: two partials, nine trips; the last: past the capped grid's one-per-4096 reach
PSNR_MAX = (1.0, 255.0)
PSNR_KINDS = ("noisy", "equal", "one")


def psnr_nparts(n):
    return max(1, min(PSNR_CAP, -(-n // 4096)))


def psnr_model(sumsq, n, max_val, rel=0.0):
    """steploss_exact.psnr_ref for any max_val: 20 log(max_val) / log(10) - 10 log(mse) / log(10); sum == 0 -> 0.  (value, bound).
    rel: what the double sum the kernel forms may be off by, relative.  mse = fl(sum / n): 1 rounding; base = logf(10), logf(max_val),
    logf(mse): U log ulps each, the base's error relative on both quotients; 20 * and 10 *, the two divisions, the subtraction: k = 2 + 2 + 1"""
    if sumsq == 0.0:
        return 0.0, 0.0
    mse = sumsq / n
    db = U["log"] * float(ulp32(LN10)) / LN10
    lmax, lm = float(np.log(float(np.float32(max_val)))), float(np.log(mse))
    maxv, t = 20.0 * lmax / LN10, 10.0 * lm / LN10
    dmax = (20.0 * U["log"] * float(ulp32(lmax)) / LN10 if lmax != 0.0 else 0.0) + abs(maxv) * db + 2 * R * abs(maxv)
    dt = 10.0 * (rel + R + U["log"] * float(ulp32(lm))) / LN10 + abs(t) * db + 2 * R * abs(t)
    return maxv - t, dmax + dt + R * (abs(maxv) + abs(t)) + TINY32


def psnr_of(a, b, max_val):
    """metrics.PSNR(max_val)(a, b) of float32 images in float64 and its bound: d = fl(a - b) (1 rounding: 2 on its square), the squares and
    the n - 1 additions in double (D53 each)"""
    d = np.asarray(a, dtype=np.float64).reshape(-1) - np.asarray(b, dtype=np.float64).reshape(-1)
    n = d.size
    return psnr_model(float((d * d).sum()), float(n), max_val, rel=2 * R + D53 * (n + 1))


class PsnrCase:
    """wm_psnr_partials + wm_psnr_finalize on n elements in [0, max_val]: noisy (b = a + N(0, 0.02 max_val)), equal, or equal but for
    one element (the last: the ragged trip) that differs by max_val / 4"""

    def __init__(self, n, max_val, kind):
        self.n, self.max_val, self.kind = n, max_val, kind
        self.label = "psnr n=%d max_val=%g %s" % (n, max_val, kind)
        if n > 1 << 20:                                    # index-made data for the large case
            self.a = r32(max_val * ((np.arange(n, dtype=np.int64) * 37) % 251).astype(np.float64) / 251.0)
            noise = max_val * (((np.arange(n, dtype=np.int64) * 41) % 33) - 16).astype(np.float64) / 512.0
        else:
            self.a = r32(max_val * uni((n,), 32000 + n % 9973))
            noise = 0.02 * max_val * normal((n,), 32001 + n % 9973)
        self.b = self.a.copy()
        if kind == "noisy":
            self.b = r32(self.a + noise)
            if n == 1 and self.b[0] == self.a[0]:
                self.b[0] = fl(self.a[0] + 0.25 * max_val)
        if kind == "one":
            self.b[-1] = fl(self.a[-1] + 0.25 * max_val)
        self.ref, self.bound = psnr_of(self.a, self.b, max_val)
        assert (self.ref == 0.0) == (kind == "equal"), self.label

    def check(self, out):
        return [ECmp(self.label, f64(out).reshape(1), [self.ref], [self.bound])]


@functools.lru_cache(maxsize=4)
def psnr_case(n, max_val, kind):
    return PsnrCase(n, max_val, kind)


PSNR_KEYS = tuple((n, mv, k) for n in PSNR_N for mv in PSNR_MAX for k in PSNR_KINDS if n < 1 << 20 or k != "equal")


# ----------------------------------------------------------------------------------------------------------------- confusion counts
CONF_PER = (1, 63, 64, 65, 255, 257, 4096, 4097, 64 * 4096 + 1)   # the last: the second trip of the grid-stride loop at the 64-partial cap
CONF_B = (1, 3)
CONF_DT = (("f32", "f32"), ("f32", "u8"), ("u8", "f32"), ("u8", "u8"))
CONF_THR = {"f32": (0.5,), "u8": (127.0, 127.5, -0.5)}
CONF_FILL = ("mixed", "blocks")
NP_DT = {"f32": np.float32, "u8": np.uint8}


def conf_nparts(per):
    return max(1, min(64, -(-per // 4096))) if per > 0 else 0


def conf_values(dt, thr, pred):
    """what a mask holds: values exactly on the threshold and next to it on either side, far ones, and for a float prediction a NaN"""
    if dt == "u8":
        return [127, 128, 0, 255, 127, 128]
    v = [thr, nxt(thr, True), nxt(thr, False), 0.0, 1.0, nxt(thr, True)]
    return v + [NAN] if pred else v


def confusion_ref(pred, gt, thr_pred, thr_gt):
    """pred, gt [B, per] (float32 or uint8) -> int64 [1 + B, 4] = {TN, TP, FN, FP} in total, then per image; P = float(pred) > float32(thr)
    (a NaN is not above anything, as in numpy), G likewise"""
    with np.errstate(invalid="ignore"):
        p, g = pred.astype(np.float32) > np.float32(thr_pred), gt.astype(np.float32) > np.float32(thr_gt)
    per = np.stack([(~p & ~g).sum(1), (p & g).sum(1), (~p & g).sum(1), (p & ~g).sum(1)], 1).astype(np.int64)
    return np.concatenate([per.sum(0, keepdims=True), per], 0)


class ConfCase:
    """wm_confusion_counts on B images of `per` elements.  fill `mixed`: every element drawn from conf_values; `blocks`: image 0 all
    negative, image 1 all positive (both masks), the last image mixed -- so a count taken from a neighbouring image's elements differs"""

    def __init__(self, per, B, pdt, gdt, thr_pred, thr_gt, fill):
        self.per, self.B, self.pdt, self.gdt, self.thr_pred, self.thr_gt, self.fill = per, B, pdt, gdt, thr_pred, thr_gt, fill
        self.label = "confusion per=%d B=%d pred %s > %g gt %s > %g %s" % (per, B, pdt, thr_pred, gdt, thr_gt, fill)
        seed = 33000 + per % 9973 + 7 * B + 3 * len(fill)
        out = []
        for dt, thr, is_pred, s in ((pdt, thr_pred, True, seed), (gdt, thr_gt, False, seed + 1)):
            vals = np.array(conf_values(dt, 0.5 if dt == "f32" else thr, is_pred), dtype=np.float64)
            k = np.minimum(np.floor(uni((B, per), s) * len(vals)), len(vals) - 1).astype(np.int64)
            a = vals[k]
            if fill == "blocks":
                a[0] = 0.0
                if B > 1:
                    a[1] = 255.0 if dt == "u8" else 1.0
            with np.errstate(invalid="ignore"):
                out.append(a.astype(NP_DT[dt]))
        self.pred, self.gt = out
        self.ref = confusion_ref(self.pred, self.gt, thr_pred, thr_gt)

    def check(self, counts):
        c = np.asarray(counts.cpu().numpy() if torch.is_tensor(counts) else counts)
        assert c.dtype == np.int64 and c.shape == self.ref.shape, (self.label, c.dtype, c.shape)
        return [ECmp(self.label + " counts per image", c[1:].astype(np.float64), self.ref[1:].astype(np.float64)),
                ECmp(self.label + " totals", c[:1].astype(np.float64), self.ref[:1].astype(np.float64))]


@functools.lru_cache(maxsize=4)
def conf_case(*key):
    return ConfCase(*key)


def conf_keys():
    """(per, B, pred dtype, gt dtype, thr_pred, thr_gt, fill): the four dtype pairs at every length and both B, the uint8 thresholds and
    the two fills taking turns; every uint8 threshold on either side at the lengths 65 and 4097 with B = 3"""
    keys, i = [], 0
    for pdt, gdt in CONF_DT:
        for per in CONF_PER:
            for B in CONF_B:
                tp, tg = CONF_THR[pdt][i % len(CONF_THR[pdt])], CONF_THR[gdt][(i // 2) % len(CONF_THR[gdt])]
                keys.append((per, B, pdt, gdt, tp, tg, CONF_FILL[(i // 3) % 2]))
                i += 1
        for per in (65, 4097):
            keys += [(per, 3, pdt, gdt, tp, tg, fill) for tp in CONF_THR[pdt] for tg in CONF_THR[gdt] for fill in CONF_FILL]
    return tuple(dict.fromkeys(keys))
