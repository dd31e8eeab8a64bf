"""Float64 restatements of the BatchNorm, pooling, up-convolution and layout operations (csrc/bn.hip, csrc/unet.hip, csrc/layout.hip),
written from the definitions in include/wm_hip.h and the reference's modules (nn.BatchNorm2d + nn.ReLU, nn.AdaptiveAvgPool2d,
nn.MaxPool2d(2, 2), nn.ConvTranspose2d(k=2, s=2), torch.cat), with the case tables and the per-element comparisons built on them.  A plain
helper module (no fixtures, CPU only, never imports the HIP package): tests/test_cpu_layers_exact.py runs float32 imitations -- faithful
and defective -- through these comparisons, tests/test_gpu_layers_exact.py runs the kernels through them.

Inputs.  The fused relu(scale*y + shift) and its mask z > 0 are where float64 and float32 may disagree legitimately, so the data removes
the ambiguity: GRID cases draw y, g, scale, shift, mean, invstd and coef from dyadic grids (y, g: multiples of 1/8 in [-2, 2]; scale,
invstd, coef[0]: {0.5, 1, 2}; shift, mean: multiples of 1/4 in [-1, 1]; coef[1], coef[2]: multiples of 1/8 in [-1, 1]), so that
z = scale*y + shift is a multiple of 1/16 with |z| <= 5 -- exact in float32, bf16 and f16, and either 0 or >= 1/16.  One GENERIC case
per kernel uses normal data; there an element is `ambiguous` when |z64| <= 4 * 2**-24 * (|scale*y| + |shift|): it is left out of the
elementwise comparisons and its largest possible contribution is added to the bound of every sum it enters.

Bounds.  None is picked and none comes from a kernel's output: a float32 result that takes k roundings to form from exact inputs is
accepted within FACTOR * k * 2**-24 * (the sum of the absolute values of its terms), FACTOR = 4 being this project's margin for "same
arithmetic, another order" (tests/jpeg_exact.py); a sum of n terms takes at most n - 1 inexact additions in ANY order (adding an exact
zero is exact), so k never depends on how a kernel splits its loops beyond the number of terms a workgroup owns; a value stored as bf16 /
f16 adds half an ulp, 2**-8 / 2**-11 of |reference|; sums a kernel forms in double add DBL = 2**-48 of their absolute terms.  Every k is
derived next to its use.  Counts, pooling values and routing, copies, zero padding and the sentinel bytes around every strided
destination are exact.
"""
import functools
import math

import numpy as np
import torch

import detgen

EPS32 = 2.0 ** -24
DBL = 2.0 ** -48
FACTOR = 4.0
DTYPES = ("f32", "bf16", "f16")
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
VE = {"f32": 4, "bf16": 8, "f16": 8}                      # elements of a 16-byte vector: every channel count and stride is a multiple
HALF_ULP = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
MIN_HALF_ULP = {"f32": 0.0, "bf16": 2.0 ** -134, "f16": 2.0 ** -25}    # half the spacing of the format's subnormals
CPS = {"f32": (4, 32, 64), "bf16": (8, 64, 512), "f16": (8, 64, 512)}
SENTINEL = 768.0                                          # exact in every dtype; no result of any case comes near it
GAP = 16                                                  # the strided run of a case: ld = C + 16


# ----------------------------------------------------------------------------------------------------------------- plumbing
def rnd(a, dt):
    """float64 array -> the same values rounded to dtype dt (round to nearest even, what the kernels' conversions do), as float64"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return torch.from_numpy(a).to(TORCH[dt]).double().numpy()


def half_ulp(ref, dt):
    """the rounding of a stored value: 2**-8 (bf16) / 2**-11 (f16) of |ref|, and never less than half the subnormal spacing"""
    return np.maximum(HALF_ULP[dt] * np.abs(ref), MIN_HALF_ULP[dt]) if dt != "f32" else np.zeros(np.shape(ref))


def store(a, dt):
    """float64 array -> torch tensor of dtype dt (the operand as a kernel reads it)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(TORCH[dt])


def f64(t):
    if torch.is_tensor(t):
        return t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def grid(shape, seed, step, lo, hi):
    """multiples of `step` in [lo, hi], uniformly, as float64"""
    n = int(round((hi - lo) / step)) + 1
    k = np.minimum(np.floor(detgen.uniform(shape, seed).double().numpy() * n), n - 1)
    return lo + k * step


def pick(shape, seed, values):
    v = np.asarray(values, dtype=np.float64)
    k = np.minimum(np.floor(detgen.uniform(shape, seed).double().numpy() * len(v)), len(v) - 1).astype(np.int64)
    return v[k]


def normal(shape, seed, std=1.0, mean=0.0):
    return detgen.normal(shape, seed, std=std, mean=mean).double().numpy()


def strided(a, ld, dt, c0=0):
    """[npix, C] values -> a [npix, ld] tensor of dtype dt holding them at channels [c0, c0 + C) and SENTINEL everywhere else"""
    a = np.asarray(a, dtype=np.float64)
    buf = np.full((a.shape[0], ld), SENTINEL, dtype=np.float64)
    buf[:, c0:c0 + a.shape[1]] = a
    return store(buf, dt)


def sentinel_dest(npix, ld, dt):
    return torch.full((npix, ld), SENTINEL, dtype=TORCH[dt])


class Cmp:
    """one per-element comparison: got within `bound` of `ref` wherever `skip` is not set; bound 0 = exact.  A NaN fails."""

    def __init__(self, what, got, ref, bound=0.0, skip=None):
        got, ref = f64(got), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
        err = np.abs(got - ref)
        bad = ~(err <= bound)
        if skip is not None:
            bad &= ~skip
            err = np.where(skip, 0.0, err)
        self.what, self.n, self.nbad = what, ref.size, int(bad.sum())
        self.skipped = 0 if skip is None else int(np.sum(skip))
        self.err = float(np.nanmax(err)) if err.size else 0.0
        self.bound = float(bound.max()) if bound.size else 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        self.worst = float(np.nanmax(ratio)) if ratio.size else 0.0
        self.exact = not bool(bound.any())

    @property
    def ok(self):
        return self.nbad == 0

    def line(self):
        if self.exact:
            return "%-58s exact over %d values: %d differ" % (self.what, self.n, self.nbad)
        return "%-58s largest error %.3e = %.3f of its bound (largest bound %.3e)%s%s" % (
            self.what, self.err, self.worst, self.bound, ", %d ambiguous left out" % self.skipped if self.skipped else "",
            "" if self.ok else "  -- %d of %d beyond the bound" % (self.nbad, self.n))

    def assert_ok(self):
        assert self.ok, self.line()
        return self


def all_ok(cmps):
    return all(c.ok for c in cmps)


def first_bad(cmps):
    return next((c.line() for c in cmps if not c.ok), "all within bounds")


def gap_cmps(what, buf, c0, C):
    """the SENTINEL bytes of a strided destination [npix, ld] outside channels [c0, c0 + C) must be untouched"""
    b = f64(buf)
    keep = np.ones(b.shape[1], dtype=bool)
    keep[c0:c0 + C] = False
    if not keep.any():
        return []
    return [Cmp(what + " stride gap", b[:, keep], np.full((b.shape[0], int(keep.sum())), SENTINEL))]


# ----------------------------------------------------------------------------------------------------------------- partial-row sums
FOLD_ABOVE = 256                                          # wm_hip.h: "with more than 256 rows it first folds them in place to 64 rows"
FOLD_ROWS = 64


def fold_adds(nparts):
    """inexact float32 additions behind one folded row: above FOLD_ABOVE rows the call sums rows j, j + 64, ... in float32 -- at most
    ceil(n / 64) terms, so ceil(n / 64) - 1 additions in any order; up to FOLD_ABOVE rows everything is summed in double: none"""
    return 0 if nparts <= FOLD_ABOVE else -(-nparts // FOLD_ROWS) - 1


def colsum64(rows):
    r = np.asarray(rows, dtype=np.float64)
    return r.sum(0), np.abs(r).sum(0)


def sum_bound(nparts, absum, extra_roundings=0):
    """error of a column sum of float32 rows as the finalisation kernels form it (fold in float32 above 256 rows, then double)"""
    return FACTOR * (fold_adds(nparts) + extra_roundings) * EPS32 * absum + DBL * absum


NPARTS = (1, 33, 256, 257, 1000)
BN_CCP = ((64, 64), (30, 32), (3, 16))
MOMENTUM = float(np.float32(0.1))
BN_EPS = float(np.float32(1e-5))
CONSTANTS = (0.1, 0.3, 0.7, 1.1)                           # float32(c) in every row of a constant channel: sumsq/count - m*m is rounding noise


class BnFinalizeCase:
    """wm_bn_finalize on synthetic partial rows [nparts][2][CP] (sum, sum of squares of n_per values per row).  Channel 1 (and 2..4 where
    C allows) is constant, so its biased variance is rounding noise around 0; the last real channel is a cancellation channel: row 0 holds
    +2**24, row 1 -2**24 and every other row 1.0, which a float32 fold of <= 256 rows (nothing may fold there) would destroy.  Padded
    channels hold junk and must come out as exact zeros."""

    def __init__(self, nparts, C, CP, count_one=False):
        self.nparts, self.C, self.CP = nparts, C, CP
        n_per = 1 if count_one else 3
        self.count = float(nparts * n_per)
        seed = 5000 + 7 * nparts + C
        x = normal((nparts, n_per, CP), seed, std=1.0) + 0.25 * np.arange(CP)[None, None, :] % 3
        x = rnd(x, "f32")
        self.const = tuple(range(1, 1 + min(len(CONSTANTS), max(C - 2, 0))))
        for k, c in enumerate(self.const):
            x[:, :, c] = float(np.float32(CONSTANTS[k]))
        rows = np.stack([x.sum(1), (x * x).sum(1)], axis=1)                # [nparts, 2, CP]
        self.cancel = C - 1 if (C >= 3 and nparts >= 2 and not count_one) else None
        if self.cancel is not None:
            rows[:, 0, self.cancel] = 1.0
            rows[:, 1, self.cancel] = 1.0
            rows[0, :, self.cancel] = (2.0 ** 24, 2.0 ** 48)
            rows[1, :, self.cancel] = (-2.0 ** 24, 2.0 ** 48)
        self.rows = rnd(rows, "f32")
        self.gamma = rnd(normal((C,), seed + 1, std=0.1, mean=1.0), "f32")
        self.beta = rnd(normal((C,), seed + 2, std=0.1), "f32")
        self.rmean = rnd(normal((C,), seed + 3, std=0.5), "f32")
        self.rvar = rnd(1.0 + np.abs(normal((C,), seed + 4, std=0.5)), "f32")
        self.label = "bn_finalize nparts=%d C=%d CP=%d count=%g" % (nparts, C, CP, self.count)
        self._ref()

    def _ref(self):
        C, n = self.C, self.count
        s1, a1 = colsum64(self.rows[:, 0, :C])
        s2, a2 = colsum64(self.rows[:, 1, :C])
        m = s1 / n
        self.raw_var = s2 / n - m * m
        var = np.maximum(self.raw_var, 0.0)                                # a biased variance is not negative
        invstd = 1.0 / np.sqrt(var + BN_EPS)
        scale = self.gamma * invstd
        shift = self.beta - m * scale
        unbiased = var * n / (n - 1.0) if n > 1 else var                   # one value per channel: torch refuses; the project keeps var
        self.ref = {"mean": m, "invstd": invstd, "scale": scale, "shift": shift,
                    "running_mean": (1.0 - MOMENTUM) * self.rmean + MOMENTUM * m,
                    "running_var": (1.0 - MOMENTUM) * self.rvar + MOMENTUM * unbiased}
        # error propagation, each line the roundings of that output:
        d1, d2 = sum_bound(self.nparts, a1), sum_bound(self.nparts, a2)
        dm_exact = d1 / n                                                  # the mean before its cast
        dm = dm_exact + FACTOR * EPS32 * np.abs(m)                         # 1 rounding: the cast to float32
        dvar = d2 / n + 2.0 * np.abs(m) * dm_exact + dm_exact ** 2 + DBL * (a2 / n + m * m)
        lo = 1.0 / np.sqrt(var + dvar + BN_EPS)                            # invstd is monotone in var: the interval is exact, not first order
        hi = 1.0 / np.sqrt(np.maximum(var - dvar, 0.0) + BN_EPS)
        dis = np.maximum(hi - invstd, invstd - lo) + FACTOR * EPS32 * invstd          # + the cast
        dsc = np.abs(self.gamma) * dis + FACTOR * EPS32 * np.abs(scale)               # + one multiplication
        dsh = np.abs(m) * dsc + np.abs(scale) * dm + FACTOR * 2 * EPS32 * (np.abs(self.beta) + np.abs(m * scale))   # + product, difference
        drm = MOMENTUM * dm + FACTOR * 4 * EPS32 * (np.abs(self.rmean) + MOMENTUM * np.abs(m))     # 1 - momentum, two products, one sum
        dun = dvar * (n / (n - 1.0) if n > 1 else 1.0)
        drv = MOMENTUM * dun + FACTOR * 5 * EPS32 * (np.abs(self.rvar) + MOMENTUM * np.abs(unbiased))   # ... and the cast of the variance
        self.bound = {"mean": dm, "invstd": dis, "scale": dsc, "shift": dsh, "running_mean": drm, "running_var": drv}

    def check(self, out, running=True):
        """out: scale, shift, mean, invstd [CP] and (running) running_mean, running_var [C]"""
        cm = []
        for k in ("mean", "invstd", "scale", "shift"):
            got = f64(out[k])
            assert got.shape == (self.CP,), (k, got.shape)
            cm.append(Cmp("%s %s" % (self.label, k), got[:self.C], self.ref[k], self.bound[k]))
            if self.CP > self.C:
                cm.append(Cmp("%s %s padded channels" % (self.label, k), got[self.C:], np.zeros(self.CP - self.C)))
        if running:
            for k in ("running_mean", "running_var"):
                cm.append(Cmp("%s %s" % (self.label, k), f64(out[k]), self.ref[k], self.bound[k]))
        return cm


@functools.lru_cache(maxsize=16)
def bn_finalize_case(nparts, C, CP, count_one=False):
    return BnFinalizeCase(nparts, C, CP, count_one)


BN_FINALIZE_CASES = tuple((n, C, CP, False) for n in NPARTS for C, CP in BN_CCP) + ((1, 64, 64, True), (1, 3, 16, True))

BWD_FIN_KINDS = ("xhat", "raw", "pooled")
POOLED_B = (1, 17)


class BnBwdFinalizeCase:
    """wm_bn_bwd_finalize (rows hold sum gz, sum gz*xhat), _finalize_raw (sum gz, sum gz*y: xhat = (y - mean) * invstd applied to the sums)
    and _finalize_pooled / wm_pooled_bn_bwd_rows (row b = gvec[b] * N+[b], gvec[b] * S+[b], formed in float32)."""

    def __init__(self, kind, n, C, CP, accumulate):
        self.kind, self.n, self.C, self.CP, self.accumulate = kind, n, C, CP, accumulate
        seed = 5200 + 11 * n + C + 1000 * BWD_FIN_KINDS.index(kind)
        self.gamma = rnd(normal((C,), seed, std=0.1, mean=1.0), "f32")
        self.mean = rnd(normal((C,), seed + 1, std=0.5), "f32")
        self.invstd = rnd(0.5 + 1.5 * detgen.uniform((C,), seed + 2).double().numpy(), "f32")
        self.dgamma0 = rnd(normal((C,), seed + 3), "f32")
        self.dbeta0 = rnd(normal((C,), seed + 4), "f32")
        if kind == "pooled":
            hw = 37
            self.count = float(n * hw)
            self.gvec = rnd(normal((n, CP), seed + 5, std=0.1), "f32")
            self.npos = np.floor(detgen.uniform((n, CP), seed + 6).double().numpy() * (hw + 1))
            self.ysum = rnd(normal((n, CP), seed + 7, std=6.0), "f32")
            self.rows_ref = np.stack([self.gvec * self.npos, self.gvec * self.ysum], axis=1)
            self.rows = None
            rows, mul = self.rows_ref, 1                                   # 1 rounding per term: the product, in float32
        else:
            self.count = float(n * 7)
            self.rows = rnd(normal((n, 2, CP), seed + 5, std=3.0), "f32")
            rows, mul = self.rows, 0
        self.label = "bn_bwd_finalize %s n=%d C=%d CP=%d acc=%d" % (kind, n, C, CP, accumulate)
        s1, a1 = colsum64(rows[:, 0, :C])
        s2, a2 = colsum64(rows[:, 1, :C])
        nrows = n if kind != "pooled" else 1                               # the pooled form never folds: its B rows are summed in double
        d1, d2 = sum_bound(nrows, a1, mul), sum_bound(nrows, a2, mul)
        if kind != "xhat":
            d2 = (d2 + np.abs(self.mean) * d1) * self.invstd + DBL * (a2 + np.abs(self.mean) * a1) * self.invstd
            s2 = (s2 - self.mean * s1) * self.invstd
        old_b = self.dbeta0 if accumulate else np.zeros(C)
        old_g = self.dgamma0 if accumulate else np.zeros(C)
        coef = np.zeros((3, CP))
        coef[0, :C], coef[1, :C], coef[2, :C] = self.gamma * self.invstd, s1 / self.count, s2 / self.count
        self.ref = {"dbeta": old_b + s1, "dgamma": old_g + s2, "coef": coef}
        dcoef = np.zeros((3, CP))
        dcoef[0, :C] = FACTOR * EPS32 * np.abs(coef[0, :C])                # one product
        dcoef[1, :C] = d1 / self.count + FACTOR * EPS32 * np.abs(coef[1, :C])         # the sum, then the cast
        dcoef[2, :C] = d2 / self.count + FACTOR * EPS32 * np.abs(coef[2, :C])
        self.bound = {"dbeta": d1 + FACTOR * 2 * EPS32 * (np.abs(old_b) + np.abs(s1)),        # the cast and the accumulation
                      "dgamma": d2 + FACTOR * 2 * EPS32 * (np.abs(old_g) + np.abs(s2)), "coef": dcoef}

    def check(self, out):
        """out: dgamma, dbeta [C], coef [3, CP] (padded channels exactly 0: their bound is 0)"""
        return [Cmp("%s %s" % (self.label, k), out[k], self.ref[k], self.bound[k]) for k in ("dbeta", "dgamma", "coef")]

    def check_rows(self, rows):
        """wm_pooled_bn_bwd_rows: one float32 product per element"""
        return [Cmp("pooled_bn_bwd_rows B=%d CP=%d" % (self.n, self.CP), rows, self.rows_ref, FACTOR * EPS32 * np.abs(self.rows_ref))]


@functools.lru_cache(maxsize=16)
def bn_bwd_finalize_case(kind, n, C, CP, accumulate):
    return BnBwdFinalizeCase(kind, n, C, CP, accumulate)


BN_BWD_FINALIZE_CASES = tuple((k, n, C, CP, a) for k in ("xhat", "raw") for n in NPARTS for C, CP in BN_CCP for a in (0, 1)) + \
    tuple(("pooled", B, C, CP, a) for B in POOLED_B for C, CP in BN_CCP for a in (0, 1))

COLSUM_CASES = tuple((n, C, ldp, a) for n in (256, 257, 1000) for C, ldp in ((195, 195), (100, 128)) for a in (0, 1))


class ColsumCase:
    """wm_colsum_finalize: out[c] (+)= sum_p partials[p][c]; ldp = 195 is no multiple of 4 (one column per thread), ldp = 128 is"""

    def __init__(self, n, C, ldp, accumulate):
        self.n, self.C, self.ldp, self.accumulate = n, C, ldp, accumulate
        seed = 5400 + n + ldp
        self.rows = rnd(normal((n, ldp), seed, std=2.0), "f32")
        self.out0 = rnd(normal((C,), seed + 1), "f32")
        s, a = colsum64(self.rows[:, :C])
        old = self.out0 if accumulate else np.zeros(C)
        self.ref = old + s
        self.bound = sum_bound(n, a) + FACTOR * 2 * EPS32 * (np.abs(old) + np.abs(s))          # the cast and the accumulation
        self.label = "colsum_finalize n=%d C=%d ldp=%d acc=%d" % (n, C, ldp, accumulate)

    def check(self, out):
        return [Cmp(self.label, out, self.ref, self.bound)]


@functools.lru_cache(maxsize=16)
def colsum_case(n, C, ldp, accumulate):
    return ColsumCase(n, C, ldp, accumulate)


# ----------------------------------------------------------------------------------------------------------------- BN + ReLU data
def bnrelu_params(CP, seed, data):
    """scale, shift, mean, invstd [CP] and coef [3, CP] as float64 (float32-exact)"""
    if data == "grid":
        sc, sh = pick((CP,), seed, (0.5, 1.0, 2.0)), grid((CP,), seed + 1, 0.25, -1.0, 1.0)
        mu, isd = grid((CP,), seed + 2, 0.25, -1.0, 1.0), pick((CP,), seed + 3, (0.5, 1.0, 2.0))
        coef = np.stack([pick((CP,), seed + 4, (0.5, 1.0, 2.0)), grid((CP,), seed + 5, 0.125, -1.0, 1.0), grid((CP,), seed + 6, 0.125, -1.0, 1.0)])
    else:
        sc, sh = rnd(normal((CP,), seed, std=0.3, mean=1.0), "f32"), rnd(normal((CP,), seed + 1, std=0.5), "f32")
        mu, isd = rnd(normal((CP,), seed + 2, std=0.5), "f32"), rnd(0.5 + 1.5 * detgen.uniform((CP,), seed + 3).double().numpy(), "f32")
        coef = rnd(np.stack([normal((CP,), seed + 4, std=0.3, mean=1.0), normal((CP,), seed + 5, std=0.3), normal((CP,), seed + 6, std=0.3)]), "f32")
    return sc, sh, mu, isd, coef


def activations(shape, seed, data, dt):
    """raw conv outputs / gradients as the kernel reads them (values of dtype dt, as float64)"""
    return grid(shape, seed, 0.125, -2.0, 2.0) if data == "grid" else rnd(normal(shape, seed), dt)


def ambiguous(z, sc, y, sh):
    return np.abs(z) <= 4 * EPS32 * (np.abs(sc * y) + np.abs(sh))


def z_is_exact(z, dt):
    """the grid condition: z equals its own rounding to the storage dtype, and is 0 or at least a grid step (1/16) from 0"""
    return bool(np.array_equal(rnd(z, dt), z)) and bool(np.all((z == 0) | (np.abs(z) >= 1.0 / 16)))


# ----------------------------------------------------------------------------------------------------------------- BN backward passes
BWD_BT = 1024                                             # wm_bn_bwd_nparts: one partial row per 1024 pixels, at most 256 rows
BWD_SHAPES = ((1, 1), (3, 43), (2, 1025), (5, 480))
BWD_LARGE = ("bf16", 32, 2, 147456)                       # above the 256-row cap: every workgroup sweeps several trips


def bn_bwd_nparts(npix):
    return min(max(-(-npix // BWD_BT), 1), 256)


class BnBwdCase:
    """wm_bn_bwd_reduce and wm_bn_bwd_apply on one (dtype, CP, B, hw): g a tensor or one vector per sample, dense or strided operands.
        gz = g * [scale*y + shift > 0],  xhat = (y - mean) * invstd
        reduce: rows of sum gz | sum gz*xhat (checked after a float64 sum over the rows)
        apply : dy = coef0 * (gz - coef1 - xhat * coef2), stored as dt; rows of the column sums of dy (the conv's bias gradient)"""

    def __init__(self, dt, CP, B, hw, gform, gap, data="grid"):
        self.dt, self.CP, self.B, self.hw, self.gform, self.gap, self.data = dt, CP, B, hw, gform, gap, data
        self.npix = npix = B * hw
        seed = 5600 + 13 * CP + 7 * B + hw % 1000 + (500 if data != "grid" else 0)
        self.sc, self.sh, self.mu, self.isd, self.coef = bnrelu_params(CP, seed, data)
        self.y = activations((npix, CP), seed + 10, data, dt)
        if gform == "gvec":
            self.gvec = grid((B, CP), seed + 11, 0.125, -2.0, 2.0) if data == "grid" else rnd(normal((B, CP), seed + 11), "f32")
            g = np.repeat(self.gvec, hw, axis=0)                          # sample b owns pixels [b*hw, (b+1)*hw)
        else:
            self.gvec = None
            g = activations((npix, CP), seed + 11, data, dt)
        self.g = g
        self.ld = CP + gap
        self.label = "bn_bwd %s CP=%d B=%d hw=%d %s%s%s" % (dt, CP, B, hw, gform, " strided" if gap else "", "" if data == "grid" else " generic")
        self.z = self.sc * self.y + self.sh
        self.amb = ambiguous(self.z, self.sc, self.y, self.sh) if data != "grid" else np.zeros(self.z.shape, dtype=bool)
        gz = np.where(self.z > 0, g, 0.0)
        xh = (self.y - self.mu) * self.isd
        ca, c1, c2 = self.coef
        self.dy = ca * (gz - c1 - xh * c2)
        # a workgroup owns at most ceil(npix / rows) pixels per channel: that many terms, one fewer inexact additions, in any order
        nadd = -(-npix // bn_bwd_nparts(npix))
        t1, t2 = np.abs(gz), np.abs(gz * xh)
        amb1, amb2 = np.where(self.amb, np.abs(g), 0.0).sum(0), np.where(self.amb, np.abs(g * xh), 0.0).sum(0)
        self.s1, self.s2 = gz.sum(0), (gz * xh).sum(0)
        self.b1 = FACTOR * nadd * EPS32 * t1.sum(0) + amb1                                  # gz is a selection: no rounding of its own
        self.b2 = FACTOR * (nadd + 3) * EPS32 * t2.sum(0) + amb2                            # + y - mean, * invstd, * gz
        # dy: six roundings whichever way it is grouped (unfolded: y - mean, * invstd, * c2, gz - c1, the difference, * coef0; folded:
        # invstd*c2, * coef0, the product with mean, its sum with coef0*c1, and two fused multiply-adds), on the terms of the expanded sum
        terms = np.abs(ca) * (np.abs(gz) + np.abs(c1) + np.abs(self.isd * c2) * (np.abs(self.y) + np.abs(self.mu)))
        self.dy_bound = FACTOR * 6 * EPS32 * terms + half_ulp(self.dy, dt)
        self.dbias = self.dy.sum(0)
        self.dbias_bound = FACTOR * (nadd + 6) * EPS32 * terms.sum(0) + np.where(self.amb, np.abs(ca * g), 0.0).sum(0)

    def operands(self):
        """(g or None, gvec or None, y) as tensors [npix, ld] of dtype dt / [B, CP] float32"""
        gt = None if self.gform == "gvec" else strided(self.g, self.ld, self.dt)
        gv = None if self.gform != "gvec" else store(self.gvec, "f32")
        return gt, gv, strided(self.y, self.ld, self.dt)

    def check_reduce(self, rows):
        r = f64(rows)
        assert r.ndim == 3 and r.shape[1:] == (2, self.CP), r.shape
        return [Cmp(self.label + " sum gz", r[:, 0].sum(0), self.s1, self.b1), Cmp(self.label + " sum gz*xhat", r[:, 1].sum(0), self.s2, self.b2)]

    def check_apply(self, dy_buf, bias_rows, form):
        d = f64(dy_buf)
        assert d.shape == (self.npix, self.ld), d.shape
        cm = [Cmp("%s dy (%s)" % (self.label, form), d[:, :self.CP], self.dy, self.dy_bound, self.amb if self.amb.any() else None)]
        cm += gap_cmps("%s dy (%s)" % (self.label, form), d, 0, self.CP)
        if bias_rows is not None:
            cm.append(Cmp("%s dbias (%s)" % (self.label, form), f64(bias_rows).sum(0), self.dbias, self.dbias_bound))
        return cm


@functools.lru_cache(maxsize=8)
def bn_bwd_case(dt, CP, B, hw, gform, gap, data="grid"):
    return BnBwdCase(dt, CP, B, hw, gform, gap, data)


def bn_bwd_cases(dt):
    """(CP, B, hw, gform, gap, data) of one dtype: every CP x shape for both gradient forms dense, the strided run and the generic case once"""
    rows = [(CP, B, hw, gf, 0, "grid") for CP in CPS[dt] for B, hw in BWD_SHAPES for gf in ("g", "gvec")]
    rows += [(CPS[dt][1], B, hw, gf, GAP, "grid") for B, hw in BWD_SHAPES for gf in ("g", "gvec")]
    rows += [(CPS[dt][1], 3, 43, gf, 0, "normal") for gf in ("g", "gvec")]
    return rows


# ----------------------------------------------------------------------------------------------------------------- average pool
POOL_B = 2
POOL_HW = (1, 31, 1024, 1025, 70000)                      # 70000: above the 64-slice cap of wm_avgpool_slices
POOL_MAX_BYTES = 20 << 20


def avgpool_slices(hw):
    return min(max(-(-hw // 1024), 1), 64)


class AvgpoolCase:
    """wm_bnrelu_avgpool (out [B, CP] = mean of relu(z)) and wm_bnrelu_avgpool_stats (also N+ = #[z > 0], exact, and S+ = sum of y there)"""

    def __init__(self, dt, CP, hw, gap, data="grid"):
        self.dt, self.CP, self.hw, self.gap, self.data, self.B = dt, CP, hw, gap, data, POOL_B
        seed = 5800 + CP + hw % 997 + (500 if data != "grid" else 0)
        self.sc, self.sh, _, _, _ = bnrelu_params(CP, seed, data)
        self.y = activations((POOL_B * hw, CP), seed + 10, data, dt)
        self.ld = CP + gap
        self.label = "avgpool %s CP=%d hw=%d%s%s" % (dt, CP, hw, " strided" if gap else "", "" if data == "grid" else " generic")
        y3 = self.y.reshape(POOL_B, hw, CP)
        self.z = self.sc * y3 + self.sh
        self.amb = ambiguous(self.z, self.sc, y3, self.sh) if data != "grid" else np.zeros(self.z.shape, dtype=bool)
        pos = self.z > 0
        a = np.where(pos, self.z, 0.0)
        self.mean, self.npos, self.ysum = a.sum(1) / hw, pos.sum(1).astype(np.float64), np.where(pos, y3, 0.0).sum(1)
        # a workgroup owns at most ceil(hw / slices) pixels of a sample; the slices are summed in double.  mean: + the product and the sum
        # that form z, the float32 1/hw and the cast; S+: + the cast
        nadd = -(-hw // avgpool_slices(hw))
        self.mean_bound = (FACTOR * (nadd + 4) * EPS32 * np.abs(a).sum(1) + np.where(self.amb, np.abs(self.z), 0.0).sum(1)) / hw
        self.npos_bound = self.amb.sum(1).astype(np.float64)                # exact unless an ambiguous element may count either way
        self.ysum_bound = FACTOR * (nadd + 1) * EPS32 * np.where(pos, np.abs(y3), 0.0).sum(1) + np.where(self.amb, np.abs(y3), 0.0).sum(1)

    def operand(self):
        return strided(self.y, self.ld, self.dt)

    def check(self, mean, npos=None, ysum=None, form="plain"):
        cm = [Cmp("%s mean (%s)" % (self.label, form), mean, self.mean, self.mean_bound)]
        if npos is not None:
            cm.append(Cmp("%s N+" % self.label, npos, self.npos, self.npos_bound))
            cm.append(Cmp("%s S+" % self.label, ysum, self.ysum, self.ysum_bound))
        return cm


@functools.lru_cache(maxsize=4)
def avgpool_case(dt, CP, hw, gap, data="grid"):
    return AvgpoolCase(dt, CP, hw, gap, data)


def avgpool_cases(dt):
    esz = 4 if dt == "f32" else 2
    rows = [(CP, hw, 0, "grid") for CP in CPS[dt] for hw in POOL_HW if POOL_B * hw * CP * esz <= POOL_MAX_BYTES]
    rows += [(CPS[dt][1], hw, GAP, "grid") for hw in (31, 1025)]
    rows += [(CPS[dt][1], 1025, 0, "normal")]
    return rows


# ----------------------------------------------------------------------------------------------------------------- BN + ReLU copy
class CopyCase:
    """wm_bnrelu_copy: y[p, c0 + c] = relu(scale*x + shift) (or x when scale is NULL) for c < C; grid data: exact in every dtype"""

    def __init__(self, dt, C, c0, with_scale, npix=77):
        self.dt, self.C, self.c0, self.with_scale, self.npix = dt, C, c0, with_scale, npix
        seed = 5900 + C + c0
        self.sc, self.sh, _, _, _ = bnrelu_params(C, seed, "grid")
        self.x = activations((npix, C), seed + 10, "grid", dt)
        self.ldx, self.ldy = C + GAP, c0 + C + GAP
        self.z = self.sc * self.x + self.sh
        self.ref = np.maximum(self.z, 0.0) if with_scale else self.x
        self.label = "bnrelu_copy %s C=%d c0=%d %s" % (dt, C, c0, "scale" if with_scale else "plain")

    def operand(self):
        return strided(self.x, self.ldx, self.dt)

    def dest(self):
        return sentinel_dest(self.npix, self.ldy, self.dt)

    def check(self, buf):
        b = f64(buf)
        return [Cmp(self.label, b[:, self.c0:self.c0 + self.C], self.ref)] + gap_cmps(self.label, b, self.c0, self.C)


def copy_cases(dt):
    return [(CPS[dt][1], c0, s) for c0 in (0, 64) for s in (False, True)] + [(CPS[dt][0], 64, True)]


# ----------------------------------------------------------------------------------------------------------------- max pool 2x2
POOL2_SHAPES = ((1, 2, 2), (2, 6, 10), (1, 2, 130))
POOL2_C = {"f32": (4, 64), "bf16": (8, 64), "f16": (8, 64)}


class MaxpoolCase:
    """wm_bnrelu_maxpool2 / wm_maxpool2_bwd on grid data: a = relu(scale*y + shift) exactly; pooled = the window's maximum; the backward
    hands gpooled to the FIRST maximum of the window in row-major order (nn.MaxPool2d) and adds g_skip.  Everything exact: the sums
    g_skip + gpooled are multiples of 1/8 within [-4, 4]."""

    def __init__(self, dt, B, H, W, C):
        self.dt, self.B, self.H, self.W, self.C = dt, B, H, W, C
        seed = 6000 + C + 3 * H + W
        self.sc, self.sh, _, _, _ = bnrelu_params(C, seed, "grid")
        self.y = grid((B, H, W, C), seed + 10, 0.25, -2.0, 2.0)             # coarser than the other cases: more ties
        self.gp = activations((B, H // 2, W // 2, C), seed + 11, "grid", dt)
        self.gs = activations((B, H, W, C), seed + 12, "grid", dt)
        self.z = self.sc * self.y + self.sh
        self.a = np.maximum(self.z, 0.0)
        win = self.a.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4, C)   # window taps, row-major
        self.pooled = win.max(3)
        first = win.argmax(3)                                              # numpy: the first maximum
        self.tie_share = float(np.mean((win.max(3) > 0) & ((win == win.max(3, keepdims=True)).sum(3) > 1)))
        route = np.zeros_like(win)
        np.put_along_axis(route, first[:, :, :, None, :], self.gp[:, :, :, None, :], axis=3)
        self.routed = route.reshape(B, H // 2, W // 2, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
        self.label = "maxpool %s %dx%dx%d C=%d" % (dt, B, H, W, C)

    def check_fwd(self, pooled, act_buf, c0a):
        cm = [Cmp(self.label + " pooled", f64(pooled).reshape(self.pooled.shape), self.pooled)]
        if act_buf is not None:
            b = f64(act_buf).reshape(-1, act_buf.shape[-1])
            cm.append(Cmp("%s act_out c0=%d" % (self.label, c0a), b[:, c0a:c0a + self.C], self.a.reshape(-1, self.C)))
            cm += gap_cmps("%s act_out c0=%d" % (self.label, c0a), b, c0a, self.C)
        return cm

    def check_bwd(self, g, with_skip):
        ref = self.routed + (self.gs if with_skip else 0.0)
        return [Cmp("%s bwd %s" % (self.label, "g_skip" if with_skip else "no skip"), f64(g).reshape(ref.shape), ref)]


@functools.lru_cache(maxsize=16)
def maxpool_case(dt, B, H, W, C):
    return MaxpoolCase(dt, B, H, W, C)


# ----------------------------------------------------------------------------------------------------------------- up-convolution 2x2
UPCONV_CH = ((5, 3), (20, 8), (48, 24), (64, 3))          # shapes the MFMA form refuses (Cin % 64 or Cout % 16): the scalar kernels
UPCONV_SHAPES = ((1, 1, 1), (2, 3, 5), (1, 4, 17), (3, 9, 8))
UPCONV_MANY_CHUNKS = (1, 33, 32)                          # 1056 pixels: wm_upconv2x2_dw_chunks > 1
MFMA_CH = ((64, 16), (128, 64), (64, 48))
MFMA_SHAPES = ((1, 1, 1), (1, 8, 16), (1, 3, 43), (2, 11, 13))


def upconv_dw_chunks(npix):
    return min(max(-(-npix // 1024), 1), 64)


class UpconvCase:
    """ConvTranspose2d(k = 2, s = 2) on a = relu(scale*x + shift) (or a = x), from the header's definition:
        y[b, 2h+i, 2w+j, c0+co] = bias[co] + sum_ci a[b,h,w,ci] * w[ci,co,i,j]
        gx[b,h,w,ci] = sum_(i,j,co) gy[b,2h+i,2w+j,c0+co] * w[ci,co,i,j]
        dw[ci,co,i,j] (+)= sum_(b,h,w) a * gy,   dbias[co] (+)= sum gy
    w16: the MFMA form reads the weight rounded to the activation dtype (wm_upconv2x2_pack) -- the restatement rounds at the same place;
    a is exact on its grid in every dtype."""

    def __init__(self, dt, Cin, Cout, B, H, W, c0, gap, with_scale, w16=False):
        self.dt, self.Cin, self.Cout, self.B, self.H, self.W, self.c0, self.gap, self.with_scale, self.w16 = dt, Cin, Cout, B, H, W, c0, gap, with_scale, w16
        seed = 6200 + 5 * Cin + Cout + 11 * H + W
        self.npix = npix = B * H * W
        self.sc, self.sh, _, _, _ = bnrelu_params(Cin, seed, "grid")
        self.x = activations((npix, Cin), seed + 10, "grid", dt)
        self.z = self.sc * self.x + self.sh
        self.a = np.maximum(self.z, 0.0) if with_scale else self.x
        self.w = rnd(normal((Cin, Cout, 2, 2), seed + 11, std=math.sqrt(2.0 / Cin)), "f32")
        self.bias = rnd(normal((Cout,), seed + 12, std=0.1), "f32")
        self.gy = activations((B, 2 * H, 2 * W, Cout), seed + 13, "grid", dt)
        self.dw0 = rnd(normal((Cin, Cout, 2, 2), seed + 14), "f32")
        self.db0 = rnd(normal((Cout,), seed + 15), "f32")
        self.ldx, self.ldy = Cin + gap, c0 + Cout + gap
        self.label = "upconv%s %s %d->%d %dx%dx%d c0=%d%s%s" % (" mfma" if w16 else "", dt, Cin, Cout, B, H, W, c0, " strided" if gap else "",
                                                                " scale" if with_scale else "")
        wk = rnd(self.w, dt) if w16 else self.w
        self.w_used = wk
        a4 = self.a.reshape(B, H, W, Cin)
        taps = np.einsum("bhwc,coij->bhiwjo", a4, wk).reshape(B, 2 * H, 2 * W, Cout)
        self.y = taps + self.bias
        absy = np.einsum("bhwc,coij->bhiwjo", np.abs(a4), np.abs(wk)).reshape(B, 2 * H, 2 * W, Cout) + np.abs(self.bias)
        # y: a product, Cin - 1 additions of products and the bias: Cin + 1 roundings on the longest path (+ 1: a sum kept in two halves)
        self.y_bound = FACTOR * (Cin + 2) * EPS32 * absy + half_ulp(self.y, dt)
        g6 = self.gy.reshape(B, H, 2, W, 2, Cout)
        self.gx = np.einsum("bhiwjo,coij->bhwc", g6, wk).reshape(npix, Cin)
        absgx = np.einsum("bhiwjo,coij->bhwc", np.abs(g6), np.abs(wk)).reshape(npix, Cin)
        self.gx_bound = FACTOR * (4 * Cout + 1) * EPS32 * absgx + half_ulp(self.gx, dt)     # 4 Cout terms, as above
        self.dw = np.einsum("bhwc,bhiwjo->coij", a4, g6)
        absdw = np.einsum("bhwc,bhiwjo->coij", np.abs(a4), np.abs(g6))
        self.db = g6.sum((0, 1, 2, 3, 4))
        absdb = np.abs(g6).sum((0, 1, 2, 3, 4))
        # dw, dbias: one partial per chunk of at most ceil(npix / chunks) pixels rounded up to 64 -- `terms` terms: a product (dw) and
        # terms - 1 additions -- the chunks summed in double; then the cast, (dbias) three additions over the taps, and the accumulation:
        # terms + 2 roundings for dw, terms + 4 for dbias.  The MFMA form sums its per-split partials in float32 too: all npix terms of
        # dw (4 npix of dbias) may lie on one path: npix + 1 and 4 npix + 1 with the accumulation.
        terms = min(npix, -(-(-(-npix // upconv_dw_chunks(npix))) // 64) * 64)
        tw, tb = (npix, 4 * npix) if w16 else (terms + 1, terms + 3)
        self.dw_bound = {a: FACTOR * (tw + 1) * EPS32 * (absdw + a * np.abs(self.dw0)) for a in (0, 1)}
        self.db_bound = {a: FACTOR * (tb + 1) * EPS32 * (absdb + a * np.abs(self.db0)) for a in (0, 1)}

    def operands(self):
        return strided(self.x, self.ldx, self.dt), strided(self.gy.reshape(-1, self.Cout), self.ldy, self.dt, self.c0)

    def dest(self):
        return sentinel_dest(4 * self.npix, self.ldy, self.dt)

    def check_fwd(self, ybuf):
        b = f64(ybuf).reshape(-1, self.ldy)
        what = self.label + " y"
        return [Cmp(what, b[:, self.c0:self.c0 + self.Cout], self.y.reshape(-1, self.Cout), self.y_bound.reshape(-1, self.Cout))] + \
            gap_cmps(what, b, self.c0, self.Cout)

    def check_bwd(self, gx, dw, db, accumulate):
        a = 1 if accumulate else 0
        return [Cmp(self.label + " gx", f64(gx).reshape(self.npix, self.Cin), self.gx, self.gx_bound),
                Cmp("%s dw acc=%d" % (self.label, a), dw, self.dw + a * self.dw0, self.dw_bound[a]),
                Cmp("%s dbias acc=%d" % (self.label, a), db, self.db + a * self.db0, self.db_bound[a])]

    def check_pack(self, wf, wb):
        """wf [(ij, co)][Cin], wb [Cin][(ij, co)]: the 16-bit roundings of the float32 weight, exactly"""
        w16 = rnd(self.w, self.dt)
        ref_f = w16.transpose(2, 3, 1, 0).reshape(4 * self.Cout, self.Cin)
        return [Cmp(self.label + " pack wf", wf, ref_f), Cmp(self.label + " pack wb", wb, ref_f.T)]


@functools.lru_cache(maxsize=8)
def upconv_case(dt, Cin, Cout, B, H, W, c0, gap, with_scale, w16=False):
    return UpconvCase(dt, Cin, Cout, B, H, W, c0, gap, with_scale, w16)


def upconv_cases(mfma=False):
    """(Cin, Cout, B, H, W, c0, gap, with_scale).  MFMA form: every channel pair x shape x c0 in {0, Cout} x dense / strided x scale NULL /
    given.  Scalar form: every channel pair x shape, alternating the three so that each value meets each channel pair and each shape"""
    ch, shapes = (MFMA_CH, MFMA_SHAPES) if mfma else (UPCONV_CH, UPCONV_SHAPES + (UPCONV_MANY_CHUNKS,))
    if mfma:          # small cases: the full cross
        return [(Cin, Cout, B, H, W, c0, gap, s) for Cin, Cout in ch for B, H, W in shapes for c0 in (0, Cout) for gap in (0, GAP) for s in (False, True)]
    rows = []
    for i, (Cin, Cout) in enumerate(ch):
        for j, (B, H, W) in enumerate(shapes):
            k = i + j
            rows.append((Cin, Cout, B, H, W, Cout if k % 2 else 0, GAP if (k // 2) % 2 else 0, bool((i + k // 2) % 2 == 0)))
    return rows


# ----------------------------------------------------------------------------------------------------------------- layout
LAYOUT_SHAPES = ((1, 1, 1), (2, 9, 13))


class LayoutCase:
    """the copies of csrc/layout.hip, all exact: values are grid data (exact in every dtype); destinations start as SENTINEL"""

    def __init__(self, dt, B, H, W):
        self.dt, self.B, self.H, self.W = dt, B, H, W
        seed = 6400 + H + W
        self.hw = H * W
        self.img = grid((B, 3, H, W), seed, 0.125, 0.0, 1.0)
        self.planes = grid((B, 5, H, W), seed + 1, 0.125, -2.0, 2.0)
        self.msg = pick((B, 30), seed + 2, (0.0, 1.0))
        self.C = 8 if dt != "f32" else 4                                     # feature channels of concat_full
        self.sc, self.sh, _, _, _ = bnrelu_params(self.C, seed + 3, "grid")
        self.x = activations((B * H * W, self.C), seed + 4, "grid", dt)
        self.z = self.sc * self.x + self.sh
        self.label = "layout %s %dx%dx%d" % (dt, B, H, W)

    def to_nhwc(self, planes):
        B, C = planes.shape[:2]
        return planes.reshape(B, C, self.hw).transpose(0, 2, 1).reshape(B * self.hw, C)

    def check_nchw_to_nhwc(self, buf, planes, c0, zero_tail, what):
        b = f64(buf).reshape(-1, buf.shape[-1])
        C = planes.shape[1]
        ref = np.concatenate([self.to_nhwc(planes), np.zeros((b.shape[0], zero_tail))], axis=1)
        return [Cmp("%s nchw_to_nhwc %s" % (self.label, what), b[:, c0:c0 + C + zero_tail], ref)] + \
            gap_cmps("%s nchw_to_nhwc %s" % (self.label, what), b, c0, C + zero_tail)

    def check_nhwc_to_nchw(self, out, vals, what):
        """vals [npix, C]: the channels the call was asked for"""
        C = vals.shape[1]
        ref = vals.reshape(self.B, self.hw, C).transpose(0, 2, 1).reshape(self.B, C, self.H, self.W)
        return [Cmp("%s nhwc_to_nchw %s" % (self.label, what), out, ref)]

    def tail_ref(self, tail):
        t = np.zeros((self.B * self.hw, tail))
        t[:, :30] = np.repeat(self.msg, self.hw, axis=0)
        t[:, 30:33] = self.to_nhwc(self.img)
        return t

    def check_broadcast(self, buf, c0):
        b = f64(buf).reshape(-1, buf.shape[-1])
        what = "%s broadcast c0=%d" % (self.label, c0)
        return [Cmp(what, b[:, c0:c0 + 30], np.repeat(self.msg, self.hw, axis=0))] + gap_cmps(what, b, c0, 30)

    def check_concat_tail(self, buf, c0, tail):
        b = f64(buf).reshape(-1, buf.shape[-1])
        what = "%s concat_tail c0=%d" % (self.label, c0)
        return [Cmp(what, b[:, c0:c0 + tail], self.tail_ref(tail))] + gap_cmps(what, b, c0, tail)

    def check_concat_full(self, buf):
        b = f64(buf).reshape(-1, buf.shape[-1])
        ref = np.concatenate([np.maximum(self.z, 0.0), self.tail_ref(b.shape[1] - self.C)], axis=1)
        return [Cmp("%s concat_full ld=%d" % (self.label, b.shape[1]), b, ref)]


@functools.lru_cache(maxsize=16)
def layout_case(dt, B, H, W):
    return LayoutCase(dt, B, H, W)


# ----------------------------------------------------------------------------------------------------------------- 1x1 heads
HEAD_CIN = {"f32": (4, 64, 256), "bf16": (8, 64, 512), "f16": (8, 64, 512)}       # 1 and 64 vectors per pixel, and the usual one
HEAD_BWD_NPIX = (1, 513, 150000)                          # 150000: 293 rows of pitch 3 * (Cin + 1), the scalar row fold (Cin = 16)


def head_ppb(Cin, dt):
    return 256 // (Cin // VE[dt])                         # pixels a 256-thread workgroup covers per trip


def head_fwd_shapes(Cin, dt):
    p = head_ppb(Cin, dt)
    return ((1, 1), (3, 77), (1, 4 * p - 1), (1, 4 * p + 1))                     # the four-pixel trip: one short of it, one past it


def head_nparts(npix):
    return min(max(-(-npix // 512), 1), 1024)


class HeadCase:
    """nn.Conv2d(Cin, Cout, 1) on a = relu(scale*y + shift) (a = y without scale), out NCHW float32, optionally through a sigmoid:
        fwd : out[b, co, q] = act(bias[co] + sum_c a[b, q, c] * w[co, c]);  act16 [npix, 16] = out rounded to dt, channels >= Cout zero
        bwd : g[p, c] = sum_co gout[b, co, q] * w[co, c] (stored as dt);  dw[co, c] = sum_p gout * a;  db[co] = sum_p gout;
              bn rows: sum gz | sum gz * y with gz = g AS STORED * [z > 0]"""

    def __init__(self, dt, Cin, Cout, B, hw, gap, with_scale):
        self.dt, self.Cin, self.Cout, self.B, self.hw, self.gap, self.with_scale = dt, Cin, Cout, B, hw, gap, with_scale
        self.npix = npix = B * hw
        seed = 6600 + Cin + 3 * Cout + hw % 1009
        self.sc, self.sh, _, _, _ = bnrelu_params(Cin, seed, "grid")
        self.y = activations((npix, Cin), seed + 10, "grid", dt)
        self.z = self.sc * self.y + self.sh
        self.a = np.maximum(self.z, 0.0) if with_scale else self.y
        self.w = rnd(normal((Cout, Cin), seed + 11, std=math.sqrt(2.0 / Cin)), "f32")
        self.bias = rnd(normal((Cout,), seed + 12, std=0.1), "f32")
        self.gout = grid((B, Cout, hw), seed + 13, 0.125, -2.0, 2.0)
        self.dw0 = rnd(normal((Cout, Cin), seed + 14), "f32")
        self.db0 = rnd(normal((Cout,), seed + 15), "f32")
        self.ld = Cin + gap
        self.label = "head %s %d->%d B=%d hw=%d%s%s" % (dt, Cin, Cout, B, hw, " strided" if gap else "", " scale" if with_scale else "")
        self.pre = self.a @ self.w.T + self.bias                                           # [npix, Cout]
        # a product, Cin - 1 additions and the bias: Cin + 1 roundings on the longest path
        self.pre_bound = FACTOR * (Cin + 1) * EPS32 * (np.abs(self.a) @ np.abs(self.w).T + np.abs(self.bias))
        go = self.gout.transpose(0, 2, 1).reshape(npix, Cout)                              # [npix, Cout]
        self.go = go
        self.g = go @ self.w
        self.g_bound = FACTOR * Cout * EPS32 * (np.abs(go) @ np.abs(self.w)) + half_ulp(self.g, dt)    # Cout products, Cout - 1 sums
        self.dw, self.db = go.T @ self.a, go.sum(0)
        # a workgroup owns head_ppb pixels per trip and ceil(npix / (rows * ppb)) trips: that many terms (a product each for dw) and
        # one fewer additions; wm_colsum_finalize then folds above 256 rows in float32, sums in double, casts and accumulates (2)
        rows, p = head_nparts(npix), head_ppb(Cin, dt)
        self.nterms = min(npix, p * -(-npix // (rows * p)))
        k = self.nterms + fold_adds(rows) + 2
        self.dw_bound = {a: FACTOR * k * EPS32 * (np.abs(go).T @ np.abs(self.a) + a * np.abs(self.dw0)) for a in (0, 1)}
        self.db_bound = {a: FACTOR * k * EPS32 * (np.abs(go).sum(0) + a * np.abs(self.db0)) for a in (0, 1)}

    def operand(self):
        return strided(self.y, self.ld, self.dt)

    def nchw(self, v):
        return v.reshape(self.B, self.hw, self.Cout).transpose(0, 2, 1)

    def check_fwd(self, out, act, act16=None):
        what = "%s act=%d" % (self.label, act)
        got = f64(out).reshape(self.B, self.Cout, self.hw)
        if act == 0:
            cm = [Cmp(what + " out", got, self.nchw(self.pre), self.nchw(self.pre_bound))]
        else:
            # the sigmoid (__expf on the device): 4 x the largest deviation of torch's float32 CPU head + sigmoid from float64 on this
            # case, measured here and never on the kernel, floor 8 * 2**-24
            ref = 1.0 / (1.0 + np.exp(-self.pre))
            t32 = torch.sigmoid(store(self.a, "f32") @ store(self.w, "f32").t() + store(self.bias, "f32")).double().numpy()
            dev32 = float(np.abs(t32 - ref).max())
            self.sigmoid_tol, self.sigmoid_dev32 = max(FACTOR * dev32, 8 * EPS32), dev32
            c = Cmp(what + " sigmoid out", got, self.nchw(ref), self.sigmoid_tol)
            c.what += " (torch f32 %.3e)" % dev32
            cm = [c]
        if act16 is not None:
            b = f64(act16).reshape(self.npix, 16)
            ref16 = np.zeros((self.npix, 16))
            ref16[:, :self.Cout] = rnd(got.transpose(0, 2, 1).reshape(self.npix, self.Cout), self.dt)
            cm.append(Cmp(what + " act16 = out rounded, zero tail", b, ref16))
        return cm

    def check_bwd(self, gbuf, dw, db, accumulate, bn_rows=None):
        a = 1 if accumulate else 0
        gb = f64(gbuf).reshape(self.npix, self.ld)
        gs = gb[:, :self.Cin]
        cm = [Cmp(self.label + " g", gs, self.g, self.g_bound)] + gap_cmps(self.label + " g", gb, 0, self.Cin)
        cm.append(Cmp("%s dw acc=%d" % (self.label, a), dw, self.dw + a * self.dw0, self.dw_bound[a]))
        cm.append(Cmp("%s db acc=%d" % (self.label, a), db, self.db + a * self.db0, self.db_bound[a]))
        if bn_rows is not None:
            r = f64(bn_rows)
            assert r.ndim == 3 and r.shape[1:] == (2, self.Cin), r.shape
            gz = np.where(self.z > 0, gs, 0.0)                                             # from g as the kernel stored it
            k = self.nterms
            cm.append(Cmp(self.label + " bn rows sum gz", r[:, 0].sum(0), gz.sum(0), FACTOR * k * EPS32 * np.abs(gz).sum(0)))
            cm.append(Cmp(self.label + " bn rows sum gz*y", r[:, 1].sum(0), (gz * self.y).sum(0), FACTOR * (k + 1) * EPS32 * np.abs(gz * self.y).sum(0)))
        return cm


def head_fwd_cases(dt):
    """(Cin, Cout, B, hw, gap, with_scale): every Cin x shape x Cout x scale dense, the middle Cin strided as well"""
    rows = [(Cin, Cout, B, hw, 0, s) for Cin in HEAD_CIN[dt] for B, hw in head_fwd_shapes(Cin, dt) for Cout in (1, 3) for s in (False, True)]
    Cin = HEAD_CIN[dt][1]
    rows += [(Cin, Cout, B, hw, GAP, True) for B, hw in head_fwd_shapes(Cin, dt) for Cout in (1, 3)]
    return rows


def head_bwd_cases(dt):
    rows = [(Cin, Cout, 1, n, 0, s) for Cin in HEAD_CIN[dt] for n in HEAD_BWD_NPIX[:2] for Cout in (1, 3) for s in (False, True)]
    rows += [(HEAD_CIN[dt][1], 3, 1, 513, GAP, True), (16, 3, 1, 150000, 0, True), (16, 1, 1, 150000, 0, True)]
    return rows


# ----------------------------------------------------------------------------------------------------------------- linear / pooled heads
LINEAR_BIO = ((1, 1, 1), (3, 7, 5), (16, 30, 30), (34, 32, 30))
INV_HW = float(np.float32(1.0 / 37.0))
G_ROUNDINGS = 6                                           # the loss gradient of one logit: exp, 1 + e, 1 / s, - target, * gscale, / n (at most)


class LinearCase:
    """nn.Linear after the global pool: out = pooled[:, :I] @ w.T + bias;  dw (+)= g.T @ pooled, db (+)= sum_b g,
    gvec[b, :CP] = (g @ w) * inv_hw with a zero tail -- and wm_pooled_head, which runs forward, loss, backward and the pooled layer's
    BatchNorm-backward finalisation in one launch; each of its stages is held to the float64 restatement of that stage evaluated on the
    values the launch itself stored for the stage before (logits -> loss and gradient -> dw, db, gvec -> dgamma, dbeta, coef)."""

    def __init__(self, B, I, O, accumulate):
        self.B, self.I, self.O, self.accumulate = B, I, O, accumulate
        self.ldp = self.CP = -(-(I + 5) // 8) * 8                         # ldp > I and CP > I
        self.C = I
        seed = 6800 + 31 * B + I + O
        self.out3 = rnd(np.stack([np.abs(normal((B, self.CP), seed)), np.floor(detgen.uniform((B, self.CP), seed + 1).double().numpy() * 38),
                                  normal((B, self.CP), seed + 2, std=6.0)]), "f32")
        self.pooled = self.out3[0]
        self.w = rnd(normal((O, I), seed + 3, std=math.sqrt(2.0 / I)), "f32")
        self.bias = rnd(normal((O,), seed + 4, std=0.1), "f32")
        self.gout = rnd(normal((B, O), seed + 5, std=0.1), "f32")
        self.msg = pick((B, O), seed + 6, (0.0, 1.0))
        self.dw0, self.db0 = rnd(normal((O, I), seed + 7), "f32"), rnd(normal((O,), seed + 8), "f32")
        self.gamma = rnd(normal((I,), seed + 9, std=0.1, mean=1.0), "f32")
        self.mean = rnd(normal((I,), seed + 10, std=0.5), "f32")
        self.invstd = rnd(0.5 + 1.5 * detgen.uniform((I,), seed + 11).double().numpy(), "f32")
        self.dgamma0, self.dbeta0 = rnd(normal((I,), seed + 12), "f32"), rnd(normal((I,), seed + 13), "f32")
        self.count = float(B * 37)
        self.target, self.gscale = 1.0, 0.5
        self.label = "linear head B=%d I=%d O=%d acc=%d" % (B, I, O, accumulate)
        p = self.pooled[:, :I]
        self.logits = p @ self.w.T + self.bias
        self.logits_bound = FACTOR * (I + 1) * EPS32 * (np.abs(p) @ np.abs(self.w).T + np.abs(self.bias))     # I fused multiply-adds from the bias

    def _bwd(self, g, gabs, extra):
        """dw, db, gvec and their bounds from a gradient g [B, O] known to gabs * extra roundings (gabs: the absolute terms of g)"""
        a, p, I = (1 if self.accumulate else 0), self.pooled[:, :self.I], self.I
        ref = {"dw": g.T @ p + a * self.dw0, "db": g.sum(0) + a * self.db0, "gvec": np.zeros((self.B, self.CP))}
        ref["gvec"][:, :I] = (g @ self.w) * INV_HW
        bound = {"dw": FACTOR * (self.B + 1 + extra) * EPS32 * (gabs.T @ np.abs(p) + a * np.abs(self.dw0)),        # B fmas, the accumulation
                 "db": FACTOR * (self.B + extra) * EPS32 * (gabs.sum(0) + a * np.abs(self.db0)),
                 "gvec": np.zeros((self.B, self.CP))}
        bound["gvec"][:, :I] = FACTOR * (self.O + 1 + extra) * EPS32 * (gabs @ np.abs(self.w)) * INV_HW            # O fmas, * inv_hw
        return ref, bound

    def check_fwd(self, out):
        return [Cmp(self.label + " out", out, self.logits, self.logits_bound)]

    def check_bwd(self, dw, db, gvec):
        ref, bound = self._bwd(self.gout, np.abs(self.gout), 0)
        return [Cmp("%s %s" % (self.label, k), v, ref[k], bound[k]) for k, v in (("dw", dw), ("db", db), ("gvec", gvec))]

    def check_pooled_head(self, kind, logits, loss, dw, db, gvec, dgamma, dbeta, coef):
        what = "pooled head kind=%d B=%d I=%d O=%d acc=%d" % (kind, self.B, self.I, self.O, self.accumulate)
        cm = [Cmp(what + " logits", logits, self.logits, self.logits_bound)]
        v = f64(logits)
        n = v.size
        if kind == 0:
            t = self.target
            terms = np.maximum(v, 0.0) - v * t + np.log1p(np.exp(-np.abs(v)))
            tabs = np.maximum(v, 0.0) + np.abs(v * t) + np.log1p(np.exp(-np.abs(v)))
            sig = 1.0 / (1.0 + np.exp(-v))
            g, gabs = (sig - t) * self.gscale / n, (sig + abs(t)) * self.gscale / n
            lref, labs = [terms.sum() / n], [tabs.sum() / n]
        else:
            d = v - self.msg
            g, gabs = d * self.gscale, (np.abs(v) + self.msg) * self.gscale
            hard = np.abs(np.clip(np.rint(v), 0.0, 1.0) - self.msg)
            lref, labs = [(d * d).sum() / n, hard.sum() / n], [(d * d).sum() / n, 0.0]       # the bit errors are small integers: exact sum
        # loss: per term at most 6 roundings (exp, log1p, two products, two sums), n - 1 additions, the division
        lb = [FACTOR * (n + 6) * EPS32 * a for a in labs]
        lb[-1] = lb[-1] if kind == 0 else FACTOR * EPS32 * lref[1]                          # ... the division only
        cm.append(Cmp(what + " loss", loss, np.array(lref), np.array(lb)))
        ref, bound = self._bwd(g, gabs, G_ROUNDINGS)
        cm += [Cmp("%s %s" % (what, k), x, ref[k], bound[k]) for k, x in (("dw", dw), ("db", db), ("gvec", gvec))]
        # the finalisation, from the gvec the launch stored: rows gv * N+, gv * S+ (one float32 product each), summed in double
        gv, C, CP = f64(gvec), self.C, self.CP
        r1, r2 = gv * self.out3[1], gv * self.out3[2]
        s1, a1, s2, a2 = r1[:, :C].sum(0), np.abs(r1[:, :C]).sum(0), r2[:, :C].sum(0), np.abs(r2[:, :C]).sum(0)
        d1, d2 = sum_bound(1, a1, 1), sum_bound(1, a2, 1)
        d2 = (d2 + np.abs(self.mean) * d1) * self.invstd + DBL * (a2 + np.abs(self.mean) * a1) * self.invstd
        s2 = (s2 - self.mean * s1) * self.invstd
        acc = 1 if self.accumulate else 0
        cref, cb = np.zeros((3, CP)), np.zeros((3, CP))
        cref[0, :C], cref[1, :C], cref[2, :C] = self.gamma * self.invstd, s1 / self.count, s2 / self.count
        cb[0, :C] = FACTOR * EPS32 * np.abs(cref[0, :C])
        cb[1, :C], cb[2, :C] = d1 / self.count + FACTOR * EPS32 * np.abs(cref[1, :C]), d2 / self.count + FACTOR * EPS32 * np.abs(cref[2, :C])
        cm.append(Cmp(what + " dbeta", dbeta, acc * self.dbeta0 + s1, d1 + FACTOR * 2 * EPS32 * (acc * np.abs(self.dbeta0) + np.abs(s1))))
        cm.append(Cmp(what + " dgamma", dgamma, acc * self.dgamma0 + s2, d2 + FACTOR * 2 * EPS32 * (acc * np.abs(self.dgamma0) + np.abs(s2))))
        cm.append(Cmp(what + " coef", coef, cref, cb))
        return cm


@functools.lru_cache(maxsize=8)
def linear_case(B, I, O, accumulate):
    return LinearCase(B, I, O, accumulate)


LINEAR_CASES = tuple((B, I, O, a) for B, I, O in LINEAR_BIO for a in (0, 1))
