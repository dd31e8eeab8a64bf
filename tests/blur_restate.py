"""Float64 restatement and bound model of the separable blur (csrc/gauss_sep.hip: wm_gauss_sep_fwd / wm_gauss_sep_bwd), shared by
tests/test_cpu_blur_cropout.py, tests/test_gpu_blur_cropout.py and tests/golden/make_golden_blur.py.  numpy only.

The operator.  With r = k // 2 and xpad = x padded by r pixels (zeros, or reflected without repeating the border pixel, as F.pad(mode='reflect')),
    y[h, w] = sum_i tc[i] * (sum_j tr[j] * xpad[h + i, w + j]).
The kernel takes ONE tap vector (tc = tr = taps); the restatement keeps the row taps tr and the column taps tc apart, so that a swap of the two
passes can be stated (below).  `fwd64` / `bwd64` evaluate the operator and its exact transpose in float64 FROM THE SAME float32 TAPS the kernel
gets: the transpose is written in scatter form (every output's gradient is spread over the padded window, then the halo is folded back onto the
pixels it copies: i <- -i and i <- 2(n-1) - i per axis), the opposite of the kernel's gather form.

The bound model follows the kernel's summation order (the inner, row, sum first; each sum a chain of k fmaf from 0, left to right):
  * forward, and the zero-border backward (the forward with reversed taps): k fused multiply-adds per pass, each one rounding of a partial sum, and
    the intermediate is itself such a rounded sum -> |got - ref64| <= (2k + 2) 2^-24 sum_ij |tc_i| |tr_j| |xpad_ij|, plus one float32 subnormal;
  * reflected-border backward: the same bound, (2k + 2) 2^-24 (|A|^T |g|) plus one subnormal.  Per axis the result is Z(q) + Z(-q) +
    Z(2(n-1)-q), each Z a chain of k fmaf; a tap that reads the zero extension adds nothing and rounds nothing, so within r of a border the
    chains are short and a term passes k + 1 roundings per pass at most (its chain and the fold's addition), 2k + 2 in all.
Nothing here is measured from the kernel.

`imitate_fwd` / `imitate_bwd` replay the kernel's order in float32 on the host (an fmaf is formed as float32(float64(a) * b + c): the product is
exact in float64, the sum is rounded to 53 bits before the 24 -- a double rounding far below the bound); their `defect` argument builds the
mistakes the CPU tests require the bound model to catch:
    "no_reverse"   zero-border backward with the taps not reversed
    "no_fold"      reflected-border backward without the fold (the halo's gradient is dropped)
    "halo_shift"   the staged window starts one pixel late (halo off by one)
    "swap_passes"  the column pass done before the row pass, i.e. tr applied along columns and tc along rows.  With a single tap vector the two
                   orders are the same operator in exact arithmetic (only the rounding differs, inside the bound), so this defect can only show
                   -- and is tested -- with distinct row and column taps, which is what an unsymmetric 2-D kernel outer(tc, tr) means."""
import numpy as np

EPS = 2.0 ** -24
SUBNORMAL = 2.0 ** -149
ZERO, REFLECT = 0, 1
KS = (3, 5, 7, 9, 15)
MIN_K, MAX_K = 3, 15


def gaussian_taps(k, sigma=2.0):
    """GaussianBlur(k)'s 1-D taps: g_i = exp(-(i - (k-1)/2)^2 / (2 sigma^2)), t = g / sum(g), in float64, rounded once to float32"""
    d = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    g = np.exp(-d * d / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def kornia_taps(k, sigma):
    """GF's taps, kornia's get_gaussian_kernel1d restated for odd k: exp(-x^2 / (2 sigma^2)) on x = arange(k) - k // 2, normalised"""
    x = np.arange(k, dtype=np.float64) - k // 2
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def unsym_taps(k, seed=0):
    """signed, unsymmetric float32 taps (t[i] != t[k-1-i] for every i but the centre), so that neither a reversal nor a transposition can hide"""
    t = np.random.RandomState(7000 + 10 * k + seed).uniform(0.25, 1.0, k) * np.where(np.arange(k) % 3 == 1, -1.0, 1.0)
    t[: k // 2] *= 0.5
    return t.astype(np.float32)


def outer64(tc, tr=None):
    tr = tc if tr is None else tr
    return np.outer(np.asarray(tc, np.float64), np.asarray(tr, np.float64))


def pad64(x, r, border):
    x = np.asarray(x, np.float64)
    width = [(0, 0)] * (x.ndim - 2) + [(r, r), (r, r)]
    if border == REFLECT:
        assert r < x.shape[-2] and r < x.shape[-1], "reflect padding needs r < H and r < W"
        return np.pad(x, width, mode="reflect")
    return np.pad(x, width, mode="constant")


def _corr(xp, tc, tr, H, W):
    k = len(tc)
    row = sum(float(tr[j]) * xp[..., :, j:j + W] for j in range(k))
    return sum(float(tc[i]) * row[..., i:i + H, :] for i in range(k))


def fwd64(x, taps, border, taps_col=None):
    """float64 forward from float32 taps; taps = row taps, taps_col = column taps (default: the same)"""
    tr = np.asarray(taps, np.float32).astype(np.float64)
    tc = tr if taps_col is None else np.asarray(taps_col, np.float32).astype(np.float64)
    H, W = np.shape(x)[-2:]
    return _corr(pad64(x, len(tr) // 2, border), tc, tr, H, W)


def fwd_abs64(x, taps, border, taps_col=None):
    """sum_ij |tc_i| |tr_j| |xpad_ij|"""
    return fwd64(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(taps, np.float32)), border,
                 None if taps_col is None else np.abs(np.asarray(taps_col, np.float32)))


def _fold(gp, r, n, axis):
    """fold the padded gradient gp (n + 2r along `axis`) back: padded position p (image coordinate) is a copy of pixel -p (p < 0) or
    2(n-1) - p (p >= n)"""
    gp = np.moveaxis(gp, axis, 0)
    out = gp[r:r + n].copy()
    for p in range(-r, 0):
        out[-p] += gp[p + r]
    for p in range(n, n + r):
        out[2 * (n - 1) - p] += gp[p + r]
    return np.moveaxis(out, 0, axis)


def bwd64(g, taps, border, taps_col=None):
    """the exact transpose of fwd64 in float64, scatter form"""
    tr = np.asarray(taps, np.float32).astype(np.float64)
    tc = tr if taps_col is None else np.asarray(taps_col, np.float32).astype(np.float64)
    g = np.asarray(g, np.float64)
    k, r = len(tr), len(tr) // 2
    H, W = g.shape[-2:]
    gp = np.zeros(g.shape[:-2] + (H + 2 * r, W + 2 * r))
    for i in range(k):
        for j in range(k):
            gp[..., i:i + H, j:j + W] += tc[i] * tr[j] * g
    if border == REFLECT:
        assert r < H and r < W
        return _fold(_fold(gp, r, H, -2), r, W, -1)
    return gp[..., r:r + H, r:r + W]


def bwd_abs64(g, taps, border, taps_col=None):
    return bwd64(np.abs(np.asarray(g, np.float64)), np.abs(np.asarray(taps, np.float32)), border,
                 None if taps_col is None else np.abs(np.asarray(taps_col, np.float32)))


def fwd_factor(k):
    return (2 * k + 2) * EPS


def bwd_factor(k, border):
    return (2 * k + 2) * EPS       # one bound model, both borders


def bound_fwd(x, taps, border, taps_col=None):
    return fwd_factor(len(taps)) * fwd_abs64(x, taps, border, taps_col) + SUBNORMAL


def bound_bwd(g, taps, border, taps_col=None):
    return bwd_factor(len(taps), border) * bwd_abs64(g, taps, border, taps_col) + SUBNORMAL


class Cmp:
    """one per-element comparison: worst error as a fraction of its bound, printed before it is asserted"""

    def __init__(self, label, got, ref, bound):
        got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
        assert got.shape == ref.shape == bound.shape, (label, got.shape, ref.shape, bound.shape)
        assert np.isfinite(got).all(), label
        self.label = label
        self.frac = float(np.max(np.abs(got - ref) / bound)) if got.size else 0.0
        self.err = float(np.max(np.abs(got - ref))) if got.size else 0.0

    @property
    def ok(self):
        return self.frac <= 1.0

    def assert_ok(self):
        print("%-64s max error %.3e = %.3f of its bound" % (self.label, self.err, self.frac))
        assert self.ok, (self.label, self.err, self.frac)
        return self


# ----------------------------------------------------------------------------- float32 imitation of the kernel's order
def _fma32(a, b, c):
    return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _chain(window, taps):
    """sum_i taps[i] * window(i): a chain of fmaf from 0, left to right, in float32"""
    acc = np.zeros(window(0).shape, np.float32)
    for i, t in enumerate(taps):
        acc = _fma32(np.float32(t), window(i), acc)
    return acc


def imitate_fwd(x, taps, border, taps_col=None, defect=None):
    tr = np.asarray(taps, np.float32)
    tc = tr if taps_col is None else np.asarray(taps_col, np.float32)
    if defect == "swap_passes":
        tr, tc = tc, tr
    x = np.asarray(x, np.float32)
    k, r = len(tr), len(tr) // 2
    H, W = x.shape[-2:]
    xp = pad64(x, r, border).astype(np.float32)
    if defect == "halo_shift":          # the staged window starts one pixel late
        xp = np.concatenate([xp[..., 1:, :], np.zeros_like(xp[..., :1, :])], axis=-2)
        xp = np.concatenate([xp[..., :, 1:], np.zeros_like(xp[..., :, :1])], axis=-1)
    row = _chain(lambda j: xp[..., :, j:j + W], tr)
    return _chain(lambda i: row[..., i:i + H, :], tc)


def _z32(gz, rev, r, n, axis, fold):
    """one axis of the kernel's backward: Z(p) = sum_i rev[i] * G[p + i - r] on the zero-extended G, gx[q] = Z(q) (+ the two fold terms)"""
    gz = np.moveaxis(gz, axis, 0)
    ext = np.concatenate([np.zeros((2 * r,) + gz.shape[1:], np.float32), gz, np.zeros((2 * r,) + gz.shape[1:], np.float32)], axis=0)
    # Z at padded positions p = -r .. n + r - 1: Z[p + r] = sum_i rev[i] * ext[p + i + r]  (ext[m] = G[m - 2r])
    Z = _chain(lambda i: ext[i:i + n + 2 * r], rev)
    out = Z[r:r + n].copy()
    if fold:
        for q in range(n):
            acc = out[q]
            if 1 <= q <= r:
                acc = (acc + Z[-q + r]).astype(np.float32)
            if n - 1 - r <= q <= n - 2:
                acc = (acc + Z[2 * (n - 1) - q + r]).astype(np.float32)
            out[q] = acc
    return np.moveaxis(out, 0, axis)


def imitate_bwd(g, taps, border, taps_col=None, defect=None):
    tr = np.asarray(taps, np.float32)
    tc = tr if taps_col is None else np.asarray(taps_col, np.float32)
    g = np.asarray(g, np.float32)
    r = len(tr) // 2
    H, W = g.shape[-2:]
    rev_r, rev_c = (tr, tc) if defect == "no_reverse" else (tr[::-1], tc[::-1])
    fold = border == REFLECT and defect != "no_fold"
    rowp = _z32(g, rev_r, r, W, -1, fold)
    return _z32(rowp, rev_c, r, H, -2, fold)
