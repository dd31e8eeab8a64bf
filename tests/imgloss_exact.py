"""Float64 restatements of the image losses of csrc/imgloss.hip (ReconstructionLoss l2 / l_char / l1, GradientLoss, ExclusionLoss) and of
csrc/ssim3.hip (SSIM_Loss map and mean, ExtendedL1 / NonBlurry / Gray), written from include/wm_hip.h and the headers of the two files, with
the case tables and the per-element comparisons built on them.  A plain helper module (CPU only, no fixtures, never imports the HIP
package): tests/test_cpu_imgloss_exact.py runs float32 imitations -- faithful and defective -- through these comparisons,
tests/test_gpu_imgloss_exact.py runs the kernels through them.

Gradients are written in another form than the kernels': the kernels gather (a pixel collects the differences or windows it is part of),
the references SCATTER (every difference or window adds onto the pixels it reads; the reflection is an index map the additions go
through; a pooled pixel hands a quarter of its gradient to each of its four sources).

Bounds.  None comes from a run.  One counted float32 rounding is R = FACTOR * 2**-24 of the absolute terms of the operation (FACTOR = 4,
the project's margin, tests/layers_exact.py); an operation in double costs D53 = 2**-53 of its absolute terms; a double rounded to
float32 costs EPS32 = 2**-24 of itself (round32).  Errors go to first order through mul / add / recip of tests/ssim_exact.py.  The counts:

  K_BOX = 9     a nine-tap mean of ssim3.hip: the taps added row by row from 0 (the first addition is exact: 8) and one division by 9.
  K_BOX2 = 10   the same of a product plane (x^2, y^2, xy): each product is rounded before it is added (+1).
  K_W_MAP = 4   the weight of one SSIM_Loss output in the map's backward: k = (float) of the double upstream product (1), g[p] * k (1),
                / 9 (1; * -0.5 is exact), the product with the coefficient (1).
  K_W_MEAN = 5  the mean's: (float) upstream (1), 1.f / count (1), their product (1), / 9 (1), the product with the coefficient (1).
  K_GATHER = 9  the nine additions of one gather; a multiplicity 1, 2 or 4 times a coefficient is exact.
  K_OUT = 3     ax + 2 x q + y r: two products (2 x is exact) on their own terms through mul(), then two additions charged on the three terms.
  K_POOL = 3    AvgPool2d(2): three additions; * 0.25 is exact.
  K_SIG         s = (1 / (1 + expf(-d))) * 2 - 1: expf U["exp"] = 3 ulps of e (the OpenCL full-profile requirement: no table of HIP's
                math accuracy is installed under the ROCm tree; the same source tests/gelem_exact.py names), 1 + e (1) and the reciprocal
                (1) on q = 1 / (1 + e), * 2 exact, - 1 one rounding of the result |s| (for q in [1/4, 1] the subtraction is exact).
                The division counts as correctly rounded because build.py's FLAGS pass hipcc no option that turns its default
                (-fhip-fp32-correctly-rounded-divide-sqrt) off; that is what K_BOX, recip() and this count rely on.
  K_LINK = 4    the four fmas that add a pixel's links (first / second of a row link, of a column link) into its gradient.
  K_LEVELS = 2  g0 + up1 + up2; the scalings by 1/4 and 1/16 are exact.
  K_CF = 1      cf = (float)(coef * upstream): the double product is D53, the conversion one float32 rounding.

Exact, with no tolerance.  SENTINEL around every destination.  On GRID data (multiples of 1/8 in [-2, 2], masks from {0, 1/2, 1, 2}) every
term and every sum of the streaming kernels is exact in double, so each workgroup's partial, predicted from the model of split16 /
stream16 / wm_groups below (owners()), coef and the loss (ONE float32 rounding of the same double expression) are compared bit for bit.
The l2 and l1 gradients, the pixel-loss gradients on GRID data and the GradientLoss backward are one float32 rounding of a double
expression with one inexact operation, restated here operation by operation: bit for bit.  GradientLoss planes (grid, quarters,
checkerboard, monotone, float32-subnormal steps) make every difference and sum exact.  COUNT images for ExclusionLoss: pixels from {0, 100}
with the number of 100s in every aligned 4 x 4 block made a multiple of 4, so that every difference of every level is a multiple of 25
(without that the level-2 pixels are multiples of 6.25 and s(6.25) = 0.996 is not saturated); then s is exactly 0 or +-1 in float32, every
product 0 or 1, and a tile's partial of a slot is the integer count of the differences whose FIRST pixel lies in the tile.

Either way (no element is left out).  l_char: a value whose float64 reference lies within 4 * 2**-53 relative of a float32 rounding
boundary may round to either neighbour (d*d, + eps, sqrt and the division in double: either(), lo == hi elsewhere).  SSIM_Loss: an output
whose float64 unclamped value lies within its own derived bound of 0 or 1 may pass or cut its gradient: the whole coefficient of such an
output is added to the bound of every input pixel it feeds (`ambiguous`, as tests/cbr_bwd_exact.py).  An output whose two windows are
equal is NOT ambiguous: n == d bit for bit there, the unclamped value is exactly 0 and the bound passes (>=).  The gradient is 0 at such a
point (S = 1 is its maximum), so passing shows only as the rounding residue of the cancelling terms 2 x q + y r: the `equal` kind also
asserts that residue is there (a kernel that cuts at the bound writes exact zeros).  Shares are capped at EITHER_CAP = 1 % per case.
"""
import functools

import numpy as np

import detgen  # noqa: F401
from layers_exact import EPS32, SENTINEL, half_ulp
from norm_exact import D53
from ssim_exact import add, mul, recip
from steploss_exact import FACTOR, R, TINY32, U, ECmp, all_ok, f64, fl, grid, normal, pick, r32, store, uni, ulp32, worst  # noqa: F401

K_BOX, K_BOX2, K_W_MAP, K_W_MEAN, K_GATHER, K_OUT, K_POOL, K_LINK, K_LEVELS, K_CF = 9, 10, 4, 5, 9, 3, 3, 4, 2, 1
LCHAR_D53 = 4.0                                           # d*d, + eps (halved by the root: 1 together), sqrt, /, * k
EITHER_CAP = 0.01
f32 = np.float32


def round32(v, dt="f32"):
    """what one conversion of a double to the stored type may move it by"""
    v = np.asarray(v, dtype=np.float64)
    return EPS32 * np.abs(v) + TINY32 if dt == "f32" else half_ulp(v, dt)


def either(what, got, lo, hi):
    """got must be lo or hi, bit for bit; .either = how many elements have two answers"""
    got, lo, hi = f64(got), np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    c = ECmp(what, got, np.where(got == hi, hi, lo))
    c.either = int((lo != hi).sum())
    return c


def near32(v, rel):
    """the float32 roundings of v (1 - rel) and v (1 + rel), ordered: equal unless v is within rel of a rounding boundary"""
    a, b = r32(v - rel * np.abs(v)), r32(v + rel * np.abs(v))
    return np.minimum(a, b), np.maximum(a, b)


# ----------------------------------------------------------------------------------------------------------------- split16 / stream16 / wm_groups
def groups(n, unit, cap):
    """wm_reduce.h: ceil(n / unit) within [1, cap]"""
    return int(min(cap, max(1, -(-n // unit))))


def split16(n, offs):
    """offs: the element offset (0..3) past a 16-byte boundary of every pointer of the split, the first being the one the head is taken
    from -> (head, nv, tail0): a scalar head up to the first pointer's boundary, nv float4s, the tail from tail0; the others share the
    split only when they reach a boundary at the same element, otherwise nv = 0 and everything is scalar (head = 0)"""
    head = min((4 - offs[0]) % 4, n)
    nv = (n - head) // 4 if all(o % 4 == offs[0] % 4 for o in offs) else 0
    if nv == 0:
        head = 0
    return head, nv, head + 4 * nv


def owners(n, offs, G):
    """the workgroup (of G, 256 threads each, grid-stride) that handles each of the n elements"""
    head, nv, tail0 = split16(n, offs)
    own = np.empty(n, dtype=np.int64)
    v = np.arange(nv)
    own[head:tail0] = np.repeat((v // 256) % G, 4)
    i = np.arange(head + n - tail0)
    own[np.where(i < head, i, tail0 + (i - head))] = (i // 256) % G
    return own


def trips(n, offs, G):
    """(float4 trips, scalar trips) of the busiest thread"""
    head, nv, tail0 = split16(n, offs)
    return -(-nv // (256 * G)), -(-(head + n - tail0) // (256 * G))


def by_owner(terms, own, G):
    return np.bincount(own, weights=terms, minlength=G)


def upstream(gscale=1.0, gdev=None, gout=None):
    """wm_reduce.h: g = (double)gscale, *= (double)gscale_dev[0], *= (double)gout[0] -- each product one double operation"""
    g = np.float64(f32(gscale))
    if gdev is not None:
        g = g * np.float64(f32(gdev))
    if gout is not None:
        g = g * np.float64(f32(gout))
    return g


MODES = (dict(), dict(gscale=0.7, gdev=1.5, gout=0.75), dict(gscale=-0.5, gdev=4.0, gout=3.0, accumulate=True),
         dict(gscale=0.3, gdev=1.1, gout=0.9, accumulate=True))


def up_of(m):
    return upstream(m.get("gscale", 1.0), m.get("gdev"), m.get("gout"))


def mode_name(m):
    return " ".join("%s=%s" % kv for kv in sorted(m.items())) or "plain"


def accumulate32(v32, old):
    """the store with accumulate: fl(fl(v) + old) in float32"""
    return (np.asarray(v32, dtype=np.float64).astype(f32) + np.asarray(old, dtype=np.float64).astype(f32)).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------- streaming: reconstruction
RECON_KINDS = {"l2": 0, "l_char": 1, "l1": 2}
LENGTHS = (1, 3, 4, 5, 7, 1023, 1024, 1027, 4096, 4097, 8193)
RECON_CAP = 64 * 4096 + 5                                 # = 256 * 1024 + 5: past the 64 parts of the sums and the 256 groups of the backward
RECON_ALIGN = ((0, 0, 0), (1, 1, 1), (3, 3, 3), (1, 0, 0), (0, 2, 0), (0, 0, 3), (1, 2, 3))     # x, t, grad
RECON_DATA = ("grid", "uniform", "zerosum")


class ReconCase:
    """wm_recon_sums / _finalize / _bwd on x, t [B, per] placed `offs` elements past a 16-byte boundary"""

    def __init__(self, kind, per, B, offs, data, eps=1e-6):
        self.kind, self.per, self.B, self.offs, self.data = kind, per, B, offs, data
        self.eps = float(f32(eps))                        # the entry point takes a float and widens it
        self.label = "recon %s per=%d B=%d offs=%s %s eps=%g" % (kind, per, B, offs, data, eps)
        seed = 41000 + per % 9973 + 7 * B + 13 * sum(offs)
        if data == "uniform":
            self.x, self.t = r32(uni((B, per), seed)), r32(uni((B, per), seed + 1))
        else:
            self.x, self.t = grid((B, per), seed, 0.125, -2.0, 2.0), grid((B, per), seed + 1, 0.125, -2.0, 2.0)
            if data == "zerosum":
                self.t = self.x[:, ::-1].copy()
        self.old = grid((B, per), seed + 2, 0.125, -2.0, 2.0)
        self.exact = data != "uniform" and kind != "l_char"
        self.P, self.G = groups(per, 4096, 64), groups(per, 1024, 256)
        d = self.x - self.t
        self.d = d
        self.terms = d * d if kind == "l2" else np.sqrt(d * d + self.eps) if kind == "l_char" else d

    def sample_offs(self, b, which):
        """where sample b's pointers stand: the base offsets moved on by b * per elements"""
        return tuple((o + b * self.per) % 4 for o in which)

    def check_partials(self, partials):
        q = f64(partials).reshape(self.B, self.P)
        ref, bound = np.zeros((self.B, self.P)), np.zeros((self.B, self.P))
        for b in range(self.B):
            own = owners(self.per, self.sample_offs(b, self.offs[:2]), self.P)
            ref[b] = by_owner(self.terms[b], own, self.P)
            if not self.exact:
                n = np.bincount(own, minlength=self.P)
                bound[b] = (n + (LCHAR_D53 if self.kind == "l_char" else 1.0)) * D53 * by_owner(np.abs(self.terms[b]), own, self.P)
        return [ECmp(self.label + " partials", q, ref, bound)]

    def check_loss(self, loss):
        scale = 1.0 / self.B
        if self.exact:
            return [ECmp(self.label + " loss", f64(loss).reshape(1), [fl(self.terms.sum() * scale)])]
        a = np.abs(self.terms).sum()
        n = self.per + self.P + (LCHAR_D53 if self.kind == "l_char" else 1.0)
        ref = self.terms.sum() * scale
        return [ECmp(self.label + " loss", f64(loss).reshape(1), [ref], [(n + self.B) * D53 * a * scale + round32(ref)])]

    def grad_ref(self, m):
        """(lo, hi): the two float32 values an element may take (equal but for l_char near a rounding boundary)"""
        k = up_of(m) / np.float64(self.B)
        if self.kind == "l2":
            v = r32((2.0 * self.d) * k)
            lo, hi = v, v
        elif self.kind == "l1":
            v = np.full(self.d.shape, fl(k))
            lo, hi = v, v
        else:
            lo, hi = near32(self.d / np.sqrt(self.d * self.d + self.eps) * k, LCHAR_D53 * D53)
        if m.get("accumulate"):
            lo, hi = accumulate32(lo, self.old), accumulate32(hi, self.old)
        return lo, hi

    def check_grad(self, grad, m):
        lo, hi = self.grad_ref(m)
        return [either("%s grad [%s]" % (self.label, mode_name(m)), f64(grad).reshape(self.B, self.per), lo, hi)]

    def either_share(self):
        lo, hi = self.grad_ref({})
        return float((lo != hi).mean())


@functools.lru_cache(maxsize=8)
def recon_case(*key):
    return ReconCase(*key)


def recon_keys():
    """(kind, per, B, offs, data, eps): every length with every kind, B and the alignments taking turns, grid and uniform data; the
    zero-sum l1 case; past the caps the float4 path and the scalar fallback, each kind"""
    keys, i = [], 0
    for kind in RECON_KINDS:
        for per in LENGTHS:
            for data in ("grid", "uniform"):
                keys.append((kind, per, (1, 3)[i % 2], RECON_ALIGN[i % len(RECON_ALIGN)], data, (1e-6, 1e-3)[(i // 3) % 2]))
                i += 1
        keys.append((kind, RECON_CAP, 1, (1, 1, 1), "grid", 1e-6))     # head + float4 + tail
        keys.append((kind, RECON_CAP, 1, (0, 0, 0), "grid", 1e-6))     # no head: one float4 more, the backward's second float4 trip
        keys.append((kind, RECON_CAP, 1, (0, 2, 0), "grid", 1e-6))
        keys.append((kind, RECON_CAP, 3, (3, 3, 3), "uniform", 1e-6))
    keys += [("l1", 1027, 3, (1, 1, 1), "zerosum", 1e-6), ("l1", 8193, 1, (0, 2, 0), "zerosum", 1e-6)]
    return tuple(dict.fromkeys(keys))


# ----------------------------------------------------------------------------------------------------------------- streaming: the three pixel losses
PIX_KINDS = {"maskl1": 0, "nonblurry": 1, "gray": 2}
PIX_SUMS_CAP, PIX_BWD_CAP = 256 * 4096 + 5, 2048 * 1024 + 5
PIX_ALIGN = ((0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (3, 3, 3, 3, 3), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0),
             (0, 0, 0, 0, 1), (0, 1, 2, 3, 1))         # a, b, mask, ga, gb
PIX_WANT = ("both", "ga", "gb")


class PixCase:
    """wm_pixloss_sums / _finalize / _bwd on n elements; offs = (a, b, mask, ga, gb); want: which gradients are asked for (MASKL1)"""

    def __init__(self, kind, n, offs, data, want="both"):
        self.kind, self.n, self.offs, self.data = kind, n, offs, data
        self.want = want if kind == "maskl1" else "ga"
        self.label = "pixloss %s n=%d offs=%s %s want=%s" % (kind, n, offs, data, self.want)
        seed = 42000 + n % 9973 + 13 * sum(offs) + 3 * len(kind)
        if data == "grid":
            self.a, self.b = grid((n,), seed, 0.125, -2.0, 2.0), grid((n,), seed + 1, 0.125, -2.0, 2.0)
            self.m = pick((n,), seed + 2, (0.0, 0.5, 1.0, 2.0))
            self.m[0] = 2.0                               # never a zero mask: that case is the existing test's
            if n > 2 and kind != "maskl1":
                self.a[n // 2] = 0.5                      # x exactly 1/2: sign(0) = 0
        else:
            self.a, self.b, self.m = r32(uni((n,), seed)), r32(uni((n,), seed + 1)), r32(uni((n,), seed + 2) + 0.25)
        eq = uni((n,), seed + 3) < 1.0 / 3.0              # a third of a == b: sign(0) = 0
        self.b = np.where(eq, self.a, self.b)
        self.old_a, self.old_b = grid((n,), seed + 4, 0.125, -2.0, 2.0), grid((n,), seed + 5, 0.125, -2.0, 2.0)
        self.exact = data == "grid"
        self.P, self.G = groups(n, 4096, 256), groups(n, 1024, 2048)
        if kind == "maskl1":
            self.dm = self.m * self.a - self.m * self.b   # the products are exact in double, the difference rounded once
            self.t0, self.t1 = np.abs(self.dm), np.abs(self.m)
        else:
            self.dm = self.a - 0.5
            self.t0, self.t1 = (self.dm * self.dm if kind == "nonblurry" else np.abs(self.dm)), np.zeros(n)
        self.c0, self.c1 = self.t0.sum() / np.float64(n), self.t1.sum() / np.float64(n)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.loss = self.c0 / self.c1 if kind == "maskl1" else 1.0 - self.c0 if kind == "nonblurry" else 1.0 / self.c0
        self.brel = 0.0 if self.exact else (n + self.P + 3) * D53      # of a sum of same-signed terms and of the coef made from it

    def sums_offs(self):
        return self.offs[:3] if self.kind == "maskl1" else self.offs[:1]

    def bwd_offs(self):
        if self.kind != "maskl1":
            return (self.offs[0], self.offs[3])
        return self.offs[:3] + tuple(o for o, w in zip(self.offs[3:], ("ga", "gb")) if self.want in ("both", w))

    def check_partials(self, partials):
        q = f64(partials).reshape(self.P, 2)
        own = owners(self.n, self.sums_offs(), self.P)
        ref = np.stack([by_owner(self.t0, own, self.P), by_owner(self.t1, own, self.P)], 1)
        return [ECmp(self.label + " partials", q, ref, self.brel * ref)]

    def check_coef_loss(self, coef, loss):
        ref = np.array([self.c0, self.c1])
        bl = 0.0 if self.exact else (2 * self.brel + D53) * abs(self.loss) + round32(self.loss)
        if self.kind == "nonblurry" and not self.exact:
            bl = self.brel * self.c0 + D53 + round32(self.loss)
        return [ECmp(self.label + " coef", f64(coef).reshape(2), ref, self.brel * ref),
                ECmp(self.label + " loss", f64(loss).reshape(1), [fl(self.loss) if self.exact else self.loss], [bl])]

    def grad_ref(self, m):
        """ga (gb = -ga before the accumulate) and the bound of either: 0 on GRID data; else one float32 rounding and coef's bound"""
        g, n = up_of(m), np.float64(self.n)
        if self.kind == "maskl1":
            k, rel = g / (n * self.c1), self.brel + 2 * D53
            v = k * (np.sign(self.dm) * self.m)
        elif self.kind == "nonblurry":
            k, rel = (-2.0 * g) / n, 0.0
            v = k * self.dm
        else:
            k, rel = (-g) / ((n * self.c0) * self.c0), 2 * self.brel + 3 * D53
            v = k * np.sign(self.dm)
        if self.exact or self.kind == "nonblurry":
            return r32(v), np.zeros(self.n)
        return v, rel * np.abs(v) + round32(v)

    def check_grads(self, ga, gb, m):
        v, bv = self.grad_ref(m)
        out = []
        for name, got, sign, old in (("ga", ga, 1.0, self.old_a), ("gb", gb, -1.0, self.old_b)):
            if got is None:
                continue
            ref, b = sign * v, bv
            if m.get("accumulate"):
                if b.any():
                    ref, b = ref + old, b + EPS32 * (np.abs(ref) + np.abs(old)) + TINY32
                else:
                    ref = accumulate32(ref, old)
            out.append(ECmp("%s %s [%s]" % (self.label, name, mode_name(m)), f64(got).reshape(self.n), ref, b))
        return out


@functools.lru_cache(maxsize=4)
def pix_case(*key):
    return PixCase(*key)


def pix_keys():
    """(kind, n, offs, data, want)"""
    keys, i = [], 0
    for kind in PIX_KINDS:
        for n in LENGTHS:
            for data in ("grid", "uniform"):
                keys.append((kind, n, PIX_ALIGN[i % len(PIX_ALIGN)], data, PIX_WANT[i % 3]))
                i += 1
        for n in (PIX_SUMS_CAP, PIX_BWD_CAP):
            keys.append((kind, n, (1, 1, 1, 1, 1), "grid", "both"))     # head + float4 + tail
            keys.append((kind, n, (0, 0, 0, 0, 0), "grid", "both"))     # no head: one float4 more, the backward's second float4 trip
            keys.append((kind, n, (0, 0, 0, 1, 0), "grid", "both"))     # ga apart: the backward falls back, the sums (a, b, mask) do not
        keys.append((kind, PIX_SUMS_CAP, (0, 1, 0, 0, 0) if kind == "maskl1" else (2, 2, 2, 2, 2), "uniform", "both"))
    for j, offs in enumerate(PIX_ALIGN):                  # every alignment with ExtendedL1 at a head + float4 + tail length, every `want`
        keys += [("maskl1", 1027, offs, "grid", PIX_WANT[(j + k) % 3]) for k in range(2)]
    return tuple(dict.fromkeys(keys))


# ----------------------------------------------------------------------------------------------------------------- GradientLoss
GRADL_SHAPES = ((2, 2), (2, 9), (9, 2), (3, 257), (17, 241), (513, 512))
GRADL_N = (1, 6)
GRADL_DATA = ("grid", "quarters", "checker", "monotone", "subnormal")


class GradlCase:
    """wm_gradloss_sums / _finalize / _bwd on N planes of H x W; every kind of data makes every difference and every sum exact"""

    def __init__(self, N, H, W, data):
        self.N, self.H, self.W, self.data = N, H, W, data
        self.label = "gradloss N=%d %dx%d %s" % (N, H, W, data)
        seed = 43000 + 31 * H + 7 * W + N
        shape = (N, H, W)
        yy, xx = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
        if data == "grid":
            a = grid(shape, seed, 0.125, -2.0, 2.0)
        elif data == "quarters":
            a = np.floor(grid(shape, seed, 0.125, -2.0, 2.0) * 4.0) / 4.0
        elif data == "checker":
            a = ((yy + xx + np.arange(N)[:, None, None]) % 2).astype(np.float64)
        elif data == "monotone":
            a = (yy * W + xx + np.arange(N)[:, None, None]) * 0.125
        else:                                             # normal float32 values whose neighbours differ by float32 subnormals, both signs
            a = 2.0 ** -126 + np.floor(uni(shape, seed) * 64.0) * 2.0 ** -149
        self.a = a
        assert np.array_equal(r32(a), a)
        self.old = grid(shape, seed + 1, 0.125, -2.0, 2.0)
        self.P = groups(H * W, 4096, 64)
        self.cx, self.cy = np.float64(N) * H * (W - 1.0), np.float64(N) * (H - 1.0) * W
        self.dx, self.dy = a[:, :, :-1] - a[:, :, 1:], a[:, :-1, :] - a[:, 1:, :]

    def check_sums(self, partials, loss):
        """partials [n][P][2]: pixel (y, x) owns the differences to its right and lower neighbours"""
        N, H, W = self.N, self.H, self.W
        tx, ty = np.zeros((N, H, W)), np.zeros((N, H, W))
        tx[:, :, :-1], ty[:, :-1, :] = np.abs(self.dx), np.abs(self.dy)
        own = (np.arange(H * W) // 256) % self.P
        ref = np.stack([np.stack([by_owner(t[n].reshape(-1), own, self.P) for t in (tx, ty)], 1) for n in range(N)])
        want = fl(tx.sum() / self.cx + ty.sum() / self.cy)
        return [ECmp(self.label + " partials", f64(partials).reshape(N, self.P, 2), ref), ECmp(self.label + " loss", f64(loss).reshape(1), [want])]

    def check_grad(self, grad, m):
        """scatter form: every difference hands its sign to its first pixel and the opposite to its second"""
        g = up_of(m)
        gx, gy = g / self.cx, g / self.cy
        nx, ny = np.zeros(self.a.shape), np.zeros(self.a.shape)
        sx, sy = np.sign(self.dx), np.sign(self.dy)
        nx[:, :, :-1] += sx
        nx[:, :, 1:] -= sx
        ny[:, :-1, :] += sy
        ny[:, 1:, :] -= sy
        ref = r32(nx * gx + ny * gy)                      # n * g is exact (n in -2 .. 2): one rounding in double, fused or not
        if m.get("accumulate"):
            ref = accumulate32(ref, self.old)
        return [ECmp("%s grad [%s]" % (self.label, mode_name(m)), f64(grad).reshape(self.a.shape), ref)]


@functools.lru_cache(maxsize=4)
def gradl_case(*key):
    return GradlCase(*key)


def gradl_keys():
    keys = [(N, H, W, d) for (H, W) in GRADL_SHAPES[:5] for N in GRADL_N for d in GRADL_DATA]
    keys += [(1, 513, 512, d) for d in GRADL_DATA] + [(6, 513, 512, "quarters")]
    return tuple(keys)


# ----------------------------------------------------------------------------------------------------------------- ExclusionLoss
ETH, ETW = 16, 32                                         # imgloss.hip: "a workgroup owns a 16 x 32 tile of level-0 pixels of one sample"
EXCL_H = (2, 3, 4, 5, 8, 9, 15, 16, 17, 18, 20, 33)
EXCL_W = (2, 3, 4, 5, 8, 31, 32, 33, 36, 37, 64, 65, 70)
EXCL_PAIRS = ((1, 1), (3, 3), (2, 4), (4, 1), (1, 4), (4, 4))
EXCL_SEAM_H, EXCL_SEAM_W = (17, 18, 20, 33), (33, 36, 37, 65)
EXCL_TABLE = (      # H, W, levels, C1, C2, B
    (2, 2, 1, 1, 1, 1), (3, 3, 1, 3, 3, 2), (4, 4, 2, 2, 4, 1), (5, 5, 2, 4, 1, 1), (2, 31, 1, 1, 4, 2), (3, 64, 1, 4, 4, 1),
    (8, 8, 3, 4, 4, 1), (9, 32, 3, 3, 3, 1), (15, 33, 3, 1, 1, 2), (16, 36, 3, 2, 4, 1), (17, 37, 3, 4, 1, 1), (18, 64, 3, 1, 4, 1),
    (20, 65, 3, 4, 4, 1), (33, 70, 3, 3, 3, 1), (17, 33, 3, 3, 3, 2), (18, 36, 3, 1, 1, 1), (20, 37, 3, 2, 4, 1), (33, 65, 3, 4, 1, 1),
    (16, 32, 1, 3, 3, 1), (17, 64, 2, 1, 4, 2), (33, 36, 2, 4, 4, 1), (8, 4, 2, 3, 3, 1), (4, 8, 1, 2, 4, 2), (5, 2, 1, 4, 1, 1),
    (2, 3, 1, 1, 1, 1), (33, 5, 2, 1, 1, 1), (20, 8, 3, 3, 3, 1))
EXCL_DATA = ("count", "uniform", "low")
EXCL_WANT = ((True, True), (True, False), (False, True))


def pool2(a):
    h, w = a.shape[-2] // 2, a.shape[-1] // 2
    a = a[..., :2 * h, :2 * w]
    return (a[..., 0::2, 0::2] + a[..., 0::2, 1::2] + a[..., 1::2, 0::2] + a[..., 1::2, 1::2]) * 0.25


def unpool(g, H, W):
    """the adjoint of pool2 onto an H x W plane: a quarter to each of the four sources, nothing to an odd last row / column"""
    out = np.zeros(g.shape[:-2] + (H, W))
    h, w = g.shape[-2:]
    out[..., :2 * h, :2 * w] = np.repeat(np.repeat(g, 2, -2), 2, -1) * 0.25
    return out


def sig2m1_ref(d, dd):
    """s = 2 sigmoid(d) - 1 = tanh(d / 2) and the bound of (1 / (1 + expf(-d))) * 2 - 1 (K_SIG) given the bound dd of d"""
    with np.errstate(over="ignore"):
        s, e = np.tanh(d / 2.0), np.exp(-d)
        q = 1.0 / (1.0 + e)
        de = np.where(np.isfinite(e), e * dd + U["exp"] * ulp32(e), 0.0)
        dq = np.where(np.isfinite(e), de * q * q, 0.0) + 2 * R * q
    return s, 2.0 * dq + R * np.abs(s) + TINY32


def count_image(shape, seed):
    """pixels from {0, 100}; in every aligned 4 x 4 block that lies inside the image the number of 100s is made a multiple of 4 by clearing
    its first set pixels, so that the level-2 pixels are multiples of 25 like the level-1 ones"""
    a = (uni(shape, seed) < 0.5).astype(np.float64)
    H, W = shape[-2:]
    flat = a.reshape(-1, H, W)
    for p in flat:
        for y in range(0, H - 3, 4):
            for x in range(0, W - 3, 4):
                blk = p[y:y + 4, x:x + 4]
                on = np.argwhere(blk > 0)
                for r, c in on[:len(on) % 4]:
                    blk[r, c] = 0.0
    return a * 100.0


class ExclCase:
    """wm_excl_fwd / _finalize / _bwd on img1 [B, C1, H, W], img2 [B, C2, H, W]"""

    def __init__(self, H, W, levels, C1, C2, B, data):
        self.H, self.W, self.levels, self.C1, self.C2, self.B, self.data = H, W, levels, C1, C2, B, data
        self.label = "excl %dx%d levels=%d C=(%d,%d) B=%d %s" % (H, W, levels, C1, C2, B, data)
        seed = 44000 + 131 * H + 7 * W + 17 * levels + 3 * C1 + C2 + B
        s1, s2 = (B, C1, H, W), (B, C2, H, W)
        if data == "count":
            self.img1, self.img2 = count_image(s1, seed), count_image(s2, seed + 1)
        elif data == "uniform":
            self.img1, self.img2 = r32(uni(s1, seed)), r32(uni(s2, seed + 1))
        else:                                             # low contrast: s is about d / 2 and the cancellation in 2 sigma - 1 dominates
            self.img1, self.img2 = r32(0.5 + 0.01 * normal(s1, seed)), r32(0.5 + 0.01 * normal(s2, seed + 1))
        self.old1, self.old2 = grid(s1, seed + 2, 2.0 ** -10, -2.0 ** -6, 2.0 ** -6), grid(s2, seed + 3, 2.0 ** -10, -2.0 ** -6, 2.0 ** -6)
        self.ty, self.tx = -(-H // ETH), -(-W // ETW)
        self.nwg = B * self.ty * self.tx
        self.CC = C1 * C2
        self.nslots = levels * 2 * self.CC
        self.norm = np.float64(levels) * 18.0
        self.vec_ok = W % 4 == 0

    def count(self, l, d):
        Hl, Wl = np.float64(self.H >> l), np.float64(self.W >> l)
        return np.float64(self.B) * ((Hl - 1.0) * Wl if d == 0 else Hl * (Wl - 1.0))

    @functools.lru_cache(maxsize=None)
    def links(self):
        """per level and direction (0: rows, img[y+1] - img[y]; 1: columns): (s1, ds1, s2, ds2), s [B, C, h, w] of the differences
        indexed by their FIRST pixel"""
        out = []
        a, da = [self.img1, self.img2], [np.zeros(self.img1.shape), np.zeros(self.img2.shape)]
        for l in range(self.levels):
            row = []
            for d in range(2):
                sd = []
                for v, dv in zip(a, da):
                    hi, lo = (v[..., 1:, :], v[..., :-1, :]) if d == 0 else (v[..., :, 1:], v[..., :, :-1])
                    dhi, dlo = (dv[..., 1:, :], dv[..., :-1, :]) if d == 0 else (dv[..., :, 1:], dv[..., :, :-1])
                    sd += list(sig2m1_ref(hi - lo, dhi + dlo + R * np.abs(hi - lo)))
                row.append(tuple(sd))
            out.append(row)
            da = [pool2(dv) + K_POOL * R * pool2(np.abs(v)) for v, dv in zip(a, da)]
            a = [pool2(v) for v in a]
        return out

    @functools.lru_cache(maxsize=None)
    def products(self):
        """per level and direction (P, dP) [B, C2, C1, h, w] = (s1^2)(s2^2) and its bound"""
        out = []
        for row in self.links():
            r = []
            for s1, ds1, s2, ds2 in row:
                q1, dq1 = mul(s1, ds1, s1, ds1)
                q2, dq2 = mul(s2, ds2, s2, ds2)
                r.append(mul(q1[:, None], dq1[:, None], q2[:, :, None], dq2[:, :, None]))
            out.append(r)
        return out

    @functools.lru_cache(maxsize=None)
    def fwd(self):
        """means, coef, loss in float64 with their bounds (intervals through the fourth root, which has no slope at 0)"""
        means, bm = np.zeros(self.nslots), np.zeros(self.nslots)
        for l, row in enumerate(self.products()):
            for d, (P, dP) in enumerate(row):
                cnt = self.count(l, d)
                s = slice((l * 2 + d) * self.CC, (l * 2 + d + 1) * self.CC)
                means[s] = (P.sum((0, 3, 4)) / cnt).reshape(-1)
                bm[s] = (dP.sum((0, 3, 4)) / cnt).reshape(-1) + (P[0, 0, 0].size * self.B + self.nwg + 2) * D53 * means[s]
        lo, hi = np.maximum(means - bm, 0.0), means + bm
        root = lambda m: np.sqrt(np.sqrt(m))  # noqa: E731
        cnts = np.repeat([self.count(l, d) for l in range(self.levels) for d in range(2)], self.CC)
        with np.errstate(divide="ignore", invalid="ignore"):
            cf = lambda m: np.where(m > 0, 0.25 / root(m) ** 3 / self.norm / cnts, 0.0)  # noqa: E731
            coef = cf(means)
            bcoef = np.maximum(np.abs(cf(lo) - coef), np.abs(cf(hi) - coef)) + 8 * D53 * coef
            bcoef = np.where((lo <= 0) & (means > 0), np.inf, bcoef)
        r, br = root(means), np.maximum(root(hi) - root(means), root(means) - root(lo)) + 3 * D53 * root(means)
        loss = r.sum() / self.norm
        return dict(means=means, bmeans=bm, coef=coef, bcoef=bcoef, loss=loss, bloss=(br.sum() + (self.nslots + 1) * D53 * r.sum()) / self.norm + round32(loss))

    def check_fwd(self, means, coef, loss):
        f = self.fwd()
        return [ECmp(self.label + " means", f64(means).reshape(-1), f["means"], f["bmeans"]),
                ECmp(self.label + " coef", f64(coef).reshape(-1), f["coef"], f["bcoef"]),
                ECmp(self.label + " loss", f64(loss).reshape(1), [f["loss"]], [f["bloss"]])]

    # COUNT data: ownership, bit for bit
    def tile_counts(self):
        """[nslots, nwg]: per slot and tile the number of differences whose first pixel lies in the tile and whose s1 and s2 are both +-1"""
        out = np.zeros((self.nslots, self.nwg))
        a = [self.img1, self.img2]
        for l in range(self.levels):
            for d in range(2):
                on = [(v[..., 1:, :] != v[..., :-1, :]) if d == 0 else (v[..., :, 1:] != v[..., :, :-1]) for v in a]
                h, w = on[0].shape[-2:]
                ty, tx = (np.arange(h) << l) // ETH, (np.arange(w) << l) // ETW      # the tile of the first pixel: its level-0 origin
                for i2 in range(self.C2):
                    for i1 in range(self.C1):
                        both = (on[0][:, i1] & on[1][:, i2]).astype(np.float64)
                        slot = (l * 2 + d) * self.CC + i2 * self.C1 + i1
                        for b in range(self.B):
                            wg = ((b * self.ty + ty[:, None]) * self.tx + tx[None, :]).reshape(-1)
                            out[slot] += np.bincount(wg, weights=both[b].reshape(-1), minlength=self.nwg)
            a = [pool2(v) for v in a]
        return out

    def check_counts(self, partials, means, coef, loss):
        cnt = self.tile_counts()
        cnts = np.repeat([self.count(l, d) for l in range(self.levels) for d in range(2)], self.CC)
        m = cnt.sum(1) / cnts
        r = np.sqrt(np.sqrt(m))
        with np.errstate(divide="ignore", invalid="ignore"):
            cf = np.where(m > 0, 0.25 / (r * r * r) / self.norm / cnts, 0.0)
        loss_ref = r.sum() / self.norm
        return [ECmp(self.label + " partials = counts per tile", f64(partials).reshape(self.nslots, self.nwg), cnt),
                ECmp(self.label + " means = count / divisor", f64(means).reshape(-1), m),
                ECmp(self.label + " coef", f64(coef).reshape(-1), cf, 8 * D53 * cf),
                ECmp(self.label + " loss", f64(loss).reshape(1), [loss_ref], [(self.nslots + 4) * D53 * loss_ref + round32(loss_ref)])]

    def saturated(self):
        """float32 numpy: every difference of every level of a COUNT image is 0 or at least 25 in size, and s is exactly 0 or +-1 there"""
        for v in (self.img1, self.img2):
            a = v.astype(f32)
            for l in range(self.levels):
                for d in (a[..., 1:, :] - a[..., :-1, :], a[..., :, 1:] - a[..., :, :-1]):
                    with np.errstate(over="ignore"):
                        s = (f32(1) / (f32(1) + np.exp(-d))) * f32(2) - f32(1)
                    if not (((d == 0) | (np.abs(d) >= 25)).all() and np.array_equal(s, np.sign(d))):
                        return False
                a = (((a[..., 0:2 * (a.shape[-2] // 2):2, 0:2 * (a.shape[-1] // 2):2] + a[..., 0:2 * (a.shape[-2] // 2):2, 1:2 * (a.shape[-1] // 2):2])
                      + a[..., 1:2 * (a.shape[-2] // 2):2, 0:2 * (a.shape[-1] // 2):2]) + a[..., 1:2 * (a.shape[-2] // 2):2, 1:2 * (a.shape[-1] // 2):2]) * f32(0.25)
        return True

    @functools.lru_cache(maxsize=None)
    def unit_grads(self):
        """per unit upstream weight: (g1, b1, a1, g2, b2, a2) -- the gradient, the part of its bound that scales with |upstream| (coef's
        own bound included: the backward is fed the coef the forward made), and the absolute terms"""
        f = self.fwd()
        H, W = self.H, self.W
        tot = [[np.zeros(s) for _ in range(3)] for s in (self.img1.shape, self.img2.shape)]
        for l, row in enumerate(self.links()):
            hl, wl = H >> l, W >> l
            lev = [[np.zeros(s[:2] + (hl, wl)) for _ in range(3)] for s in (self.img1.shape, self.img2.shape)]
            for d, (s1, ds1, s2, ds2) in enumerate(row):
                base = (l * 2 + d) * self.CC
                c = f["coef"][base:base + self.CC].reshape(self.C2, self.C1)
                dc = np.where(np.isfinite(f["bcoef"][base:base + self.CC]), f["bcoef"][base:base + self.CC], 0.0).reshape(self.C2, self.C1) \
                    + (K_CF * R + D53) * np.abs(c)
                q = [mul(s, ds, s, ds) for s, ds in ((s1, ds1), (s2, ds2))]
                A = []
                for (s, ds), (sq, dsq) in zip(((s1, ds1), (s2, ds2)), q):
                    om, dom = add(1.0, 0.0, sq, dsq, -1.0)
                    A.append(mul(s, ds, om, dom))
                # T of img1's channel i1 = sum_i2 c[i2, i1] s2[i2]^2 (C2 fmas), of img2's channel i2 = sum_i1 c[i2, i1] s1[i1]^2 (C1 fmas)
                T1 = np.einsum("ji,bjhw->bihw", c, q[1][0])
                aT1 = np.einsum("ji,bjhw->bihw", np.abs(c), q[1][0])
                dT1 = np.einsum("ji,bjhw->bihw", np.abs(c), q[1][1]) + np.einsum("ji,bjhw->bihw", dc, q[1][0]) + self.C2 * R * aT1
                T2 = np.einsum("ji,bihw->bjhw", c, q[0][0])
                aT2 = np.einsum("ji,bihw->bjhw", np.abs(c), q[0][0])
                dT2 = np.einsum("ji,bihw->bjhw", np.abs(c), q[0][1]) + np.einsum("ji,bihw->bjhw", dc, q[0][0]) + self.C1 * R * aT2
                for k, ((Av, dA), T, aT, dT) in enumerate(((A[0], T1, aT1, dT1), (A[1], T2, aT2, dT2))):
                    V = Av * T
                    dV = np.abs(T) * dA + np.abs(Av) * dT
                    second = (Ellipsis, slice(1, None), slice(None)) if d == 0 else (Ellipsis, slice(None), slice(1, None))
                    first = (Ellipsis, slice(None, -1), slice(None)) if d == 0 else (Ellipsis, slice(None), slice(None, -1))
                    lev[k][0][second] += V
                    lev[k][0][first] -= V
                    for j, t in ((1, dV), (2, np.abs(V))):
                        lev[k][j][second] += t
                        lev[k][j][first] += t
            for k in range(2):
                g, b, a = lev[k]
                b = b + K_LINK * R * a
                for hh, ww in [(H >> j, W >> j) for j in range(l)][::-1]:      # down through the levels: 4**-l in all
                    g, b, a = unpool(g, hh, ww), unpool(b, hh, ww), unpool(a, hh, ww)
                tot[k][0] += g
                tot[k][1] += b
                tot[k][2] += a
        out = []
        for k in range(2):
            g, b, a = tot[k]
            out += [g, b + K_LEVELS * R * a, a]
        return tuple(out)

    def check_grads(self, g1, g2, m):
        u1, b1, a1, u2, b2, a2 = self.unit_grads()
        up = up_of(m)
        out = []
        for name, got, u, b, old in (("grad1", g1, u1, b1, self.old1), ("grad2", g2, u2, b2, self.old2)):
            if got is None:
                continue
            ref, bound = up * u, abs(up) * b + TINY32
            if m.get("accumulate"):
                bound = bound + R * (np.abs(ref) + np.abs(old))
                ref = ref + old
            out.append(ECmp("%s %s [%s]" % (self.label, name, mode_name(m)), f64(got).reshape(u.shape), ref, bound))
        return out


@functools.lru_cache(maxsize=None)
def excl_case(*key):
    return ExclCase(*key)


def excl_keys():
    """every table row with COUNT data and with one of the two generic kinds, taking turns"""
    keys = []
    for i, row in enumerate(EXCL_TABLE):
        keys += [row + ("count",), row + (EXCL_DATA[1 + i % 2],)]
    return tuple(keys)


# ----------------------------------------------------------------------------------------------------------------- SSIM_Loss
STW, STH = 64, 16                                         # ssim3.hip: "a workgroup owns a 16 x 64 tile of one plane"
C1F, C2F = 0.01 ** 2, 0.03 ** 2
SSIM3_H = (2, 3, 4, 15, 16, 17, 18, 33)
SSIM3_W = (2, 3, 4, 63, 64, 65, 66, 129)
SSIM3_SHAPES = ((2, 2, 3), (2, 65, 1), (3, 3, 2), (3, 129, 1), (4, 4, 1), (4, 63, 2), (15, 2, 1), (15, 64, 1), (16, 3, 2), (16, 66, 1),
                (17, 4, 1), (17, 65, 2), (18, 63, 1), (18, 129, 1), (33, 64, 1), (33, 66, 1), (33, 129, 1), (2, 129, 1))     # H, W, N
SSIM3_KINDS = ("indep", "near", "equal", "const", "grid", "impulse")
SSIM3_FULL = ((2, 2, 3), (17, 65, 2), (33, 129, 1))       # every kind, the impulse pairs over every listed position, the one-hot upstreams


def refl(n):
    """ReflectionPad2d(1) as an index map: padded index 0 .. n+1 -> image index (-1 -> 1, n -> n - 2)"""
    i = np.arange(-1, n + 1)
    return np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def box9(a):
    """the nine-tap sum of the reflect-padded planes [..., H, W], / 9"""
    H, W = a.shape[-2:]
    p = a[..., refl(H)[:, None], refl(W)[None, :]]
    return sum(p[..., i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0


def scatter9(c):
    """the adjoint of box9: every output adds c / 9 onto the nine pixels its window reads, through the reflection's index map"""
    H, W = c.shape[-2:]
    out = np.zeros(c.shape)
    ry, rx = refl(H), refl(W)
    flat, cf = out.reshape(-1, H, W), c.reshape(-1, H, W)
    for i in range(3):
        for j in range(3):
            for n in range(flat.shape[0]):
                np.add.at(flat[n], (ry[i:i + H][:, None], rx[j:j + W][None, :]), cf[n] / 9.0)
    return out


def marks(H, W):
    """where an impulse or a one-hot upstream is placed: the corners, rows and columns 1 and n - 2 (the reflection's double taps), both
    sides of the 15|16 and 63|64 seams"""
    rows = sorted({r for r in (0, 1, H - 2, H - 1, 15, 16, 31, 32) if 0 <= r < H})
    cols = sorted({c for c in (0, 1, W - 2, W - 1, 63, 64, 127, 128) if 0 <= c < W})
    n = max(len(rows), len(cols))
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)] + [(rows[i % len(rows)], cols[i % len(cols)]) for i in range(n)]
    pos += [(rows[i % len(rows)], cols[(3 * i + 1) % len(cols)]) for i in range(n)]
    return list(dict.fromkeys(pos))


class Ssim3Case:
    """wm_ssim3_fwd / _finalize / _bwd on N planes of H x W"""

    def __init__(self, H, W, N, kind, first=0):
        self.H, self.W, self.N, self.kind, self.first = H, W, N, kind, first
        self.shape = (N, H, W)
        self.label = "ssim3 %dx%d N=%d %s%s" % (H, W, N, kind, "@%d" % first if kind == "impulse" else "")
        seed = 45000 + 131 * H + 7 * W + 17 * N + 1000 * SSIM3_KINDS.index(kind)
        x = r32(uni(self.shape, seed))
        if kind == "indep":
            y = r32(uni(self.shape, seed + 1))
        elif kind == "near":
            y = r32(x + 0.02 * normal(self.shape, seed + 1))
        elif kind == "equal":
            y = x.copy()
        elif kind == "const":
            x, y = np.full(self.shape, fl(0.3)), np.full(self.shape, fl(0.7))
        elif kind == "grid":
            x, y = grid(self.shape, seed, 0.125, 0.0, 2.0), grid(self.shape, seed + 1, 0.125, 0.0, 2.0)
        else:
            pos = marks(H, W)
            x, y = np.zeros(self.shape), np.zeros(self.shape)
            for n in range(N):
                a = pos[(first + n) % len(pos)]
                x[n][a] = 1.0
                y[n][a if n % 2 == 0 else pos[(first + n + 1) % len(pos)]] = 1.0
        self.x, self.y = x, y
        self.g = r32(uni(self.shape, seed + 2, -1.0, 1.0))
        self.old = grid(self.shape, seed + 3, 2.0 ** -10, -2.0 ** -4, 2.0 ** -4)
        self.tiles_y, self.tiles_x = -(-H // STH), -(-W // STW)
        self.nparts = N * self.tiles_y * self.tiles_x
        self.count = fl(float(N) * H * W)

    @functools.lru_cache(maxsize=None)
    def ref(self):
        x, y = self.x, self.y
        mx, my, ex2, ey2, exy = box9(x), box9(y), box9(x * x), box9(y * y), box9(x * y)
        dmx, dmy = K_BOX * R * box9(np.abs(x)), K_BOX * R * box9(np.abs(y))
        dex2, dey2, dexy = K_BOX2 * R * ex2, K_BOX2 * R * ey2, K_BOX2 * R * box9(np.abs(x * y))
        mxy, dmxy = mul(mx, dmx, my, dmy)
        mxx, dmxx = mul(mx, dmx, mx, dmx)
        myy, dmyy = mul(my, dmy, my, dmy)
        sgx, dsgx = add(ex2, dex2, mxx, dmxx, -1.0)
        sgy, dsgy = add(ey2, dey2, myy, dmyy, -1.0)
        sgxy, dsgxy = add(exy, dexy, mxy, dmxy, -1.0)
        A1, dA1 = add(2 * mxy, 2 * dmxy, C1F, R * C1F)
        A2, dA2 = add(2 * sgxy, 2 * dsgxy, C2F, R * C2F)
        t, dt = add(mxx, dmxx, myy, dmyy)
        B1, dB1 = add(t, dt, C1F, R * C1F)
        t, dt = add(sgx, dsgx, sgy, dsgy)
        B2, dB2 = add(t, dt, C2F, R * C2F)
        Nn, dN = mul(A1, dA1, A2, dA2)
        D, dD = mul(B1, dB1, B2, dB2)
        S = Nn / D
        dSq = dN / np.abs(D) + np.abs(Nn) * dD / (D * D) + R * np.abs(S)           # the forward's quotient
        v, dv = add(1.0, 0.0, S, dSq, -1.0)
        v, dv = v / 2.0, dv / 2.0 + TINY32
        # the backward's own way to S and the coefficients, per unit of w = gp * -0.5 / 9
        inv, dinv = recip(D, dD)
        i1, di1 = recip(B1, dB1)
        i2, di2 = recip(B2, dB2)
        Sb, dSb = mul(Nn, dN, inv, dinv)
        t, dt = add(A2, dA2, A1, dA1, -1.0)
        da, dda = mul(2 * t, 2 * dt, inv, dinv)
        t, dt = add(i1, di1, i2, di2, -1.0)
        db, ddb = mul(2 * Sb, 2 * dSb, t, dt)
        p1, q1 = mul(my, dmy, da, dda), mul(mx, dmx, db, ddb)
        p2, q2 = mul(mx, dmx, da, dda), mul(my, dmy, db, ddb)
        cmx, cmy = add(p1[0], p1[1], q1[0], q1[1], -1.0), add(p2[0], p2[1], q2[0], q2[1], -1.0)
        cq = mul(-Sb, dSb, i2, di2)
        cr = mul(2 * A1, 2 * dA1, inv, dinv)
        same = box9((x != y).astype(np.float64)) == 0                                # both windows equal: exactly 0, passes
        near = ((np.abs(v) <= dv) | (np.abs(v - 1.0) <= dv)) & ~same
        return dict(v=v, dv=dv, map=np.clip(v, 0.0, 1.0), coefs=(cmx, cmy, cq, cr), passes=(v >= 0) & (v <= 1), ambiguous=near, same=same)

    def either_share(self):
        return float(self.ref()["ambiguous"].mean())

    def check_map(self, out):
        f = self.ref()
        cm = [ECmp(self.label + " map", f64(out).reshape(self.shape), f["map"], f["dv"])]
        if f["same"].any():
            cm.append(ECmp(self.label + " map where both windows are equal: exactly 0", f64(out).reshape(self.shape)[f["same"]], np.zeros(int(f["same"].sum()))))
        return cm

    def check_partials(self, partials, out, mean):
        """each tile's partial against the float64 sum of the map the same call stored; the mean against fl(sum * 1 / (N H W))"""
        o = f64(out).reshape(self.shape)
        q = f64(partials).reshape(self.N, self.tiles_y, self.tiles_x)
        ref = np.zeros(q.shape)
        for ty in range(self.tiles_y):
            for tx in range(self.tiles_x):
                ref[:, ty, tx] = o[:, ty * STH:(ty + 1) * STH, tx * STW:(tx + 1) * STW].sum((1, 2))
        scale = 1.0 / (np.float64(self.N) * self.H * self.W)
        m = o.sum() * scale
        return [ECmp(self.label + " partials", q, ref, (STH * STW + 1) * D53 * ref),
                ECmp(self.label + " mean", f64(mean).reshape(1), [m], [(self.H * self.W * self.N + self.nparts + 2) * D53 * m + round32(m)])]

    def weights(self, g, m):
        """(gp [N, H, W] in float64, its roundings): the map's backward g[p] * k, or with g None the mean's k * (1 / count)"""
        k = up_of(m)
        if g is None:
            return np.full(self.shape, k / self.count), K_W_MEAN
        return np.asarray(g, dtype=np.float64) * k, K_W_MAP

    def grads(self, g, m):
        """-> ((gx, bound), (gy, bound)) for the upstream map g (None: the mean)"""
        f = self.ref()
        gp, kw = self.weights(g, m)
        w = gp * (-0.5)
        live = np.where(f["passes"], 1.0, 0.0)
        amb = np.where(f["ambiguous"], 1.0, 0.0)
        sc = {}
        for name, (c, dc) in zip(("mx", "my", "q", "r"), f["coefs"]):
            val, a = w * c, np.abs(w * c)
            err = np.abs(w) * dc + kw * R * a
            sc[name] = (scatter9(val * live), scatter9(err * live) + K_GATHER * R * scatter9(a * live) + scatter9(a * amb), scatter9(a * np.maximum(live, amb)))
        out = []
        for own, a, b, old in (("mx", self.x, self.y, self.old), ("my", self.y, self.x, self.old)):
            (ax, dax, aax), (q, dq, aq), (r, dr, ar) = sc[own], sc["q"], sc["r"]
            t1, dt1 = mul(2 * a, 0.0, q, dq)
            t2, dt2 = mul(b, 0.0, r, dr)
            v = ax + t1 + t2
            bv = dax + dt1 + dt2 + (K_OUT - 1) * R * (aax + np.abs(2 * a) * aq + np.abs(b) * ar) + TINY32
            if m.get("accumulate"):
                bv = bv + R * (np.abs(v) + np.abs(old))
                v = v + old
            out.append((v, bv))
        return tuple(out)

    def check_grads(self, gx, gy, g, m, tag=""):
        (vx, bx), (vy, by) = self.grads(g, m)
        what = "%s %s [%s]%s" % (self.label, "mean's backward" if g is None else "map's backward", mode_name(m), tag)
        out = []
        if gx is not None:
            out.append(ECmp(what + " gx", f64(gx).reshape(self.shape), vx, bx))
        if gy is not None:
            out.append(ECmp(what + " gy", f64(gy).reshape(self.shape), vy, by))
        return out

    def onehots(self):
        """upstream maps that are 1 at one marked output per plane and 0 elsewhere, N positions at a time"""
        pos = marks(self.H, self.W)
        out = []
        for s in range(0, len(pos), self.N):
            g = np.zeros(self.shape)
            for n in range(self.N):
                g[n][pos[(s + n) % len(pos)]] = 1.0
            out.append(g)
        return out


@functools.lru_cache(maxsize=None)
def ssim3_case(*key):
    return Ssim3Case(*key)


def ssim3_keys():
    """(H, W, N, kind, first): every shape with the five dense kinds taking turns; every kind at SSIM3_FULL, the impulse pairs there N
    planes at a time over every marked position"""
    keys = []
    for i, (H, W, N) in enumerate(SSIM3_SHAPES):
        keys.append((H, W, N, SSIM3_KINDS[i % 5], 0))
        keys.append((H, W, N, SSIM3_KINDS[(i + 2) % 5], 0))
    for H, W, N in SSIM3_FULL:
        keys += [(H, W, N, k, 0) for k in SSIM3_KINDS[:5]]
        keys += [(H, W, N, "impulse", s) for s in range(0, len(marks(H, W)), N)]
    return tuple(dict.fromkeys(keys))


# ----------------------------------------------------------------------------------------------------------------- what is compared, per family
# An engine runs a case's entry points (the kernels on the GPU, a float32 imitation on the CPU) and hands back the buffers; it collects
# the comparisons of its own guard elements in .guards.  Both test files go through these drivers, so they make the same comparisons.
def _guards(eng):
    g, eng.guards = list(getattr(eng, "guards", [])), []
    return g


def run_recon(c, eng):
    partials, loss = eng.recon_fwd(c)
    cm = {"partials": c.check_partials(partials), "loss": c.check_loss(loss), "grad": []}
    for m in MODES[:3]:
        cm["grad"] += c.check_grad(eng.recon_bwd(c, m), m)
    cm["exact"] = _guards(eng)
    return cm


def run_pix(c, eng):
    partials, coef, loss = eng.pix_fwd(c)
    cl = c.check_coef_loss(coef, loss)
    cm = {"partials": c.check_partials(partials), "coef": cl[:1], "loss": cl[1:], "grad": []}
    for m in MODES[:3]:
        ga, gb = eng.pix_bwd(c, coef, m)
        cm["grad"] += c.check_grads(ga, gb, m)
    cm["exact"] = _guards(eng)
    return cm


def run_gradl(c, eng):
    partials, loss = eng.gradl_fwd(c)
    cm = {"sums": c.check_sums(partials, loss), "grad": []}
    for m in MODES[:3]:
        cm["grad"] += c.check_grad(eng.gradl_bwd(c, m), m)
    cm["exact"] = _guards(eng)
    return cm


def same_bits(what, a, b):
    return [ECmp(what + ", same bits", f64(a), f64(b))]


def run_excl(c, eng):
    partials, means, coef, loss = eng.excl_fwd(c, 0)
    cm = {"counts": [], "means": [], "coef": [], "loss": [], "grad": [], "exact": []}
    if c.data == "count":
        cm["counts"] = c.check_counts(partials, means, coef, loss)
    else:
        f = c.check_fwd(means, coef, loss)
        cm["means"], cm["coef"], cm["loss"] = f[:1], f[1:2], f[2:]
    runs = [(EXCL_WANT[0], MODES[0]), (EXCL_WANT[1], MODES[1]), (EXCL_WANT[2], MODES[1]), (EXCL_WANT[0], MODES[2])]
    got = []
    for want, m in runs:
        g1, g2 = eng.excl_bwd(c, coef, want, m, 0)
        got.append((g1, g2))
        cm["grad"] += c.check_grads(g1, g2, m)
    if c.vec_ok:                                          # the scalar staging: the same tensors one element past a 16-byte boundary
        p1, m1, c1, l1 = eng.excl_fwd(c, 1)
        cm["exact"] += same_bits(c.label + " misaligned partials", p1, partials) + same_bits(c.label + " misaligned means", m1, means) \
            + same_bits(c.label + " misaligned coef", c1, coef) + same_bits(c.label + " misaligned loss", l1, loss)
        for (want, m), (g1, g2) in zip(runs[::3], got[::3]):
            h1, h2 = eng.excl_bwd(c, coef, want, m, 1)
            cm["exact"] += same_bits(c.label + " misaligned grad1 [%s]" % mode_name(m), h1, g1) + same_bits(c.label + " misaligned grad2 [%s]" % mode_name(m), h2, g2)
    cm["exact"] += _guards(eng)
    return cm


def run_ssim3(c, eng):
    out, partials, mean = eng.ssim3_fwd(c)
    pm = c.check_partials(partials, out, mean)
    cm = {"map": c.check_map(out), "partials": pm[:1], "mean": pm[1:], "grad": [], "grad one-hot": [], "exact": []}
    for i, m in enumerate(MODES[:3]):
        gx, gy = eng.ssim3_bwd(c, c.g, (True, True), m)
        cm["grad"] += c.check_grads(gx, gy, c.g, m)
    gx, _ = eng.ssim3_bwd(c, c.g, (True, False), MODES[1])
    _, gy = eng.ssim3_bwd(c, c.g, (False, True), MODES[1])
    cm["grad"] += c.check_grads(gx, None, c.g, MODES[1], " gx alone") + c.check_grads(None, gy, c.g, MODES[1], " gy alone")
    for m in MODES[1:3]:
        mx, my = eng.ssim3_bwd(c, None, (True, True), m)
        cm["grad"] += c.check_grads(mx, my, None, m)
        if not m.get("accumulate"):                       # a map backward with the mean's weight: the same bits
            k = f32(up_of(m)) * (f32(1) / f32(c.count))
            wx, wy = eng.ssim3_bwd(c, np.full(c.shape, float(k)), (True, True), {})
            cm["exact"] += same_bits(c.label + " mean's backward = map's backward with the mean's weight, gx", wx, mx) \
                + same_bits(c.label + " mean's backward = map's backward with the mean's weight, gy", wy, my)
    if c.kind == "equal":                                 # module docstring: the bounds pass, which shows as a rounding residue
        gx, gy = eng.ssim3_bwd(c, c.g, (True, True), {})
        cm["exact"] += [ECmp(c.label + " the gradient passes at exactly 0: a rounding residue is there", [float(f64(gx).any() or f64(gy).any())], [1.0])]
    if (c.H, c.W, c.N) in SSIM3_FULL and c.kind in ("indep", "near"):
        for j, g in enumerate(c.onehots()):
            gx, gy = eng.ssim3_bwd(c, g, (True, True), {})
            cm["grad one-hot"] += c.check_grads(gx, gy, g, {}, " one-hot %d" % j)
    cm["exact"] += _guards(eng)
    return cm


def flat(res):
    return [x for v in res.values() for x in v]
