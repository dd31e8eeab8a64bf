"""Float64 restatements of the instance normalisation (csrc/instnorm.hip: nn.InstanceNorm2d + nn.ReLU), of the Dice losses (csrc/dice.hip:
BinaryDiceLoss, DiceLoss over a softmax, tests/dice_restate.py) and of the two-source mask head (csrc/mask_head.hip: conv2d(cat(a, b)) with
a 1x1 filter, + sigmoid), written from include/wm_hip.h and the torch definitions it cites, with the case tables and the per-element
comparisons built on them.  A plain helper module (CPU only, never imports the HIP package): tests/test_cpu_norm_exact.py runs float32
imitations -- faithful and defective -- through these comparisons, tests/test_gpu_norm_exact.py runs the kernels through them.  Every
entry point is compared with float64 of ITS OWN inputs: apply and bwd_apply get float32 mean / rstd / mg / mgx that no stats call would give.

Bounds follow the rule of tests/steploss_exact.py: a float32 result formed with k roundings from the kernel's inputs is accepted within
FACTOR * k * 2**-24 * (the sum of the absolute values of its terms) + TINY32 (R = FACTOR * 2**-24 below); a 16-bit store adds half an ulp of
that type at the value (half_ulp); expf takes U["exp"] ulps of its float32 result, powf POW_ULP, both propagated through each expression's
conditioning.  A sum a kernel accumulates in double from float32 terms is charged D53 = 2**-53 per addition -- n - 1 additions for n terms
in ANY order, so no bound depends on how a kernel splits a plane -- and the float32 value made from it one float32 ulp of the reference
(ulp32): the correctly rounded value, give or take a reference that sits next to a rounding boundary.  rstd adds the conditioning of
E[x^2] - mean^2 in double: that difference is wrong by D53 * (n + 2) * (E[x^2] + mean^2), which 1 / sqrt(var + eps) passes on as
0.5 * rstd / (var + eps) of it; the reference variance itself is formed from the centred values, where nothing cancels.

Exact, with no tolerance: the zeros written to padding channels (whose inputs hold NaN in float32 and +inf in 16 bits), SENTINEL around
every destination, the ReLU select, and the bits of two runs.

A branch decided by a computed value -- the ReLU mask z > 0 on the value AS STORED -- must not depend on which side of its bound z falls:
mask_of() evaluates the stored sign at z - bound and at z + bound and the case generator moves every input where the two differ by a fixed
step (NUDGE) until none is left; InCase asserts that (self.ambiguous == 0) from the float64 values alone.  So no comparison leaves an
element out.  The softmax's max is a value, not a branch: a tie gives the same maximum whichever plane supplies it.

What the issue's text says about "one class dominating by 80" is only half true: exp(-80) = 1.8e-35 is a normal float32, so s is NOT 0
there; the cases keep the 80 and add a margin of 120, where expf does underflow (exp(-120) < 2**-150) and s is exactly 0.  Both are held
to the same formula (the spacing of the float32 subnormals covers the second).
"""
import functools

import numpy as np

import detgen  # noqa: F401
from gelem_exact import MIN_NORMAL, pattern, sigmoid_ref, ulp32
from layers_exact import half_ulp
from steploss_exact import EPS32, FACTOR, SENTINEL, TINY32, TORCH, U, ECmp, all_ok, f64, fl, normal, pick, r32, rnd, store, uni, worst  # noqa: F401

R = FACTOR * EPS32                                        # one counted rounding, relative
D53 = 2.0 ** -53                                          # one addition or multiplication in double
# OpenCL C specification, "Relative Error as ULPs", single precision, full profile: pow <= 16 ulp -- gelem_exact.U has no powf entry, and
# this is the table its other entries come from
POW_ULP = 16.0
INF, NAN = float("inf"), float("nan")
WM_OK, WM_E_BADARG, WM_E_SHAPE = 0, -1, -2                # include/wm_hip.h
WM_DT = {"f32": 0, "bf16": 1, "f16": 2}
VE = {"f32": 4, "bf16": 8, "f16": 8}                      # values of a 16-byte vector
PAD_FILL = {"f32": NAN, "bf16": INF, "f16": INF}          # what the padding channels of every activation input hold
DTYPES = ("f32", "bf16", "f16")


def nhwc(v, CP, dt, fill=None):
    """[B, C, n] float64 -> NHWC tensor [B, n, CP] of dtype dt, channels >= C holding `fill` (default PAD_FILL[dt])"""
    B, C, n = v.shape
    buf = np.full((B, n, CP), PAD_FILL[dt] if fill is None else fill, dtype=np.float64)
    buf[:, :, :C] = v.transpose(0, 2, 1)
    return store(buf, dt)


def nchw(t, C):
    """NHWC tensor [B, n, CP] -> ([B, C, n] float64 of the real channels, [B, n, CP - C] of the padding)"""
    a = f64(t)
    return a[:, :, :C].transpose(0, 2, 1), a[:, :, C:]


def rows(v, CP, fill=NAN):
    """[B, C] float64 -> float32 tensor [B, CP], entries >= C holding `fill` (the kernels must not read them)"""
    buf = np.full((v.shape[0], CP), fill, dtype=np.float64)
    buf[:, :v.shape[1]] = v
    return store(buf, "f32")


def pad_cmp(what, pad):
    return [ECmp(what + " padding channels", pad, np.zeros(pad.shape))] if pad.size else []


# ----------------------------------------------------------------------------------------------------------------- instance normalisation
IN_WG = 256                                               # wm_hip.h: "A plane of more than 256 pixels is summed by wm_instnorm_splits(hw)
IN_MAX_SPLITS = 64                                        # workgroups (<= 64)"
NUDGE = 0.125                                             # a value of every storage type


def in_chunk(hw):
    """pixels of a plane per workgroup: 256, or ceil(hw / 64) once that is more"""
    return max(IN_WG, -(-hw // IN_MAX_SPLITS))


def in_splits(hw):
    return -(-hw // in_chunk(hw)) if hw > 0 else 0


def in_scratch_doubles(B, hw, CP):
    return B * in_splits(hw) * 2 * CP


IN_SPLIT_SIZES = (1, 2, 255, 256, 257, 513, 16384, 16385, 16448, 16449)
IN_LAYOUTS = {"f32": ((16, 13), (48, 41), (1024, 1009)), "bf16": ((16, 13), (48, 41), (2048, 2033)), "f16": ((16, 13), (48, 41), (2048, 2033))}
IN_REFUSED_CP = {"f32": 1040, "bf16": 2064, "f16": 2064}
IN_HW = (1, 2, 255, 256, 257, 513)
IN_EPS = (1e-5, 1e-3, 0.0)
CONST_A, CONST_B = 2.5, float(np.float32(1000.1))
PLANT = 2.0 ** -30                                        # z of the planted elements: positive in float32 and bf16, 0 once stored as f16


def xhat_b(x, mean, rstd, dmean=0.0, drstd=0.0):
    """xhat = (x - mean) * rstd, the difference and the product in double, rounded once: k = 1; dmean, drstd: what the inputs are off by"""
    xh = (x - mean) * rstd
    return xh, np.abs(rstd) * dmean + np.abs(x - mean) * drstd + R * np.abs(xh)


def z_b(xh, dxh, gamma, beta):
    """z = xhat * gamma + beta: one fma, k = 1 on |xhat gamma| + |beta| (the product and the sum apart: 2 on the product -- the larger count
    is charged), xhat's own error through gamma; without gamma z = xhat"""
    if gamma is None:
        return xh, dxh
    return xh * gamma + beta, np.abs(gamma) * dxh + R * (2 * np.abs(xh * gamma) + np.abs(beta))


def mask_of(z, bz, dt):
    """(the ReLU mask on the value as stored, where it is ambiguous): the stored sign at both ends of z's bound"""
    lo, hi = rnd(z - bz, dt) > 0, rnd(z + bz, dt) > 0
    return hi, lo != hi


class InCase:
    """one shape of the four instance-norm entry points.  x, dy [B, C, hw] hold values of dtype dt; gamma, beta float32 [C] (affine);
    smean, srstd, smg, smgx float32 [B, C]: the synthetic statistics apply, bwd_sums and bwd_apply are fed.
    kind `const`: plane (0, 1) is 2.5 and plane (B - 1, 2) float32(1000.1) (beta is negative there: the ReLU masks the whole plane);
    kind `cancel`: plane (0, 3) is 1000 + N(0, 1).  Every case plants x = 0 in plane (0, 0) with smean = -2**-30, srstd = gamma = 1,
    beta = 0: z = 2**-30 there, which float16 stores as 0 (mask off) and bfloat16 / float32 as itself (mask on)."""

    def __init__(self, dt, CP, C, hw, B, affine, act, eps, kind="normal"):
        self.dt, self.CP, self.C, self.hw, self.B, self.affine, self.act, self.eps, self.kind = dt, CP, C, hw, B, affine, act, eps, kind
        self.label = "instnorm %s CP=%d C=%d hw=%d B=%d affine=%d act=%d eps=%g %s" % (dt, CP, C, hw, B, affine, act, eps, kind)
        seed = 20000 + 97 * CP + 13 * hw % 5000 + 7 * B + 3 * affine + act
        ch = np.arange(C)[None, :, None]
        x = normal((B, C, hw), seed, std=1.5) + 0.5 * (ch % 5) - 1.0
        if kind == "const":
            x[0, 1], x[B - 1, 2] = CONST_A, CONST_B
        if kind == "cancel":
            x[0, 3] = 1000.0 + normal((hw,), seed + 9)
        self.dy = rnd(normal((B, C, hw), seed + 1), dt)
        self.gamma = self.beta = None
        if affine:
            self.gamma, self.beta = r32(1.0 + 0.5 * normal((C,), seed + 2)), r32(0.3 * normal((C,), seed + 3))
            self.gamma[0], self.beta[0] = 1.0, 0.0
            self.beta[1:3] = -0.5
        self.smean, self.srstd = r32(0.2 * normal((B, C), seed + 4)), r32(uni((B, C), seed + 5, 0.5, 2.0))
        self.smg, self.smgx = r32(0.1 * normal((B, C), seed + 6)), r32(0.1 * normal((B, C), seed + 7))
        self.smean[0, 0], self.srstd[0, 0] = -PLANT, 1.0
        x = rnd(x, dt)
        x[0, 0, ::3] = 0.0
        self.planted = np.zeros((B, C, hw), dtype=bool)
        self.planted[0, 0, ::3] = True
        self.g3 = None if self.gamma is None else self.gamma[None, :, None]
        self.b3 = None if self.beta is None else self.beta[None, :, None]
        # no mask may hang on a rounding: move the inputs where it would, by a fixed step, for the synthetic and for the true statistics
        for _ in range(8):
            self.x = x
            self._stats()
            amb = self._masks()
            if not amb.any():
                break
            x = rnd(np.where(amb, x + NUDGE, x), dt)
        self.ambiguous = int(amb.sum())
        assert self.ambiguous == 0, (self.label, self.ambiguous)
        self._apply()
        self._sums()
        self._bwd_apply()
        self._chain()

    # -- wm_instnorm_stats
    def _stats(self):
        x, n, eps = self.x, self.hw, self.eps
        self.mean = x.mean(2)
        cen = x - self.mean[:, :, None]
        self.var = (cen * cen).mean(2)
        ex2 = (x * x).mean(2)
        self.rstd = 1.0 / np.sqrt(self.var + eps) if (self.var + eps > 0).all() else None
        assert self.rstd is not None, self.label + ": eps = 0 on a constant plane"
        self.bmean = ulp32(self.mean) + D53 * n * np.abs(x).mean(2)
        dvar = D53 * (n + 2) * (ex2 + self.mean ** 2)
        self.brstd = ulp32(self.rstd) + 0.5 * self.rstd / (self.var + eps) * dvar
        self.isconst = self.var == 0
        self.bmean = np.where(self.isconst, 0.0, self.bmean)      # n copies of one float32 value: their double sum and its quotient are exact

    def _z(self, mean, rstd, dmean=0.0, drstd=0.0):
        xh, dxh = xhat_b(self.x, mean[:, :, None], rstd[:, :, None], np.asarray(dmean)[..., None] if np.ndim(dmean) else dmean,
                         np.asarray(drstd)[..., None] if np.ndim(drstd) else drstd)
        z, bz = z_b(xh, dxh, self.g3, self.b3)
        return xh, dxh, z, bz

    def _masks(self):
        amb = np.zeros(self.x.shape, dtype=bool)
        if self.act:
            _, _, z, bz = self._z(self.smean, self.srstd)
            self.smask, a1 = mask_of(z, bz, self.dt)
            _, _, z, bz = self._z(self.mean, self.rstd, self.bmean, self.brstd)
            self.cmask, a2 = mask_of(z, bz, self.dt)
            amb = a1 | a2
        else:
            self.smask = self.cmask = np.ones(self.x.shape, dtype=bool)
        return amb

    def check_stats(self, mean, rstd):
        m, r = f64(mean), f64(rstd)
        C, lab = self.C, self.label + " stats"
        cm = [ECmp(lab + " mean", m[:, :C], self.mean, self.bmean), ECmp(lab + " rstd", r[:, :C], self.rstd, self.brstd)]
        return cm + pad_cmp(lab + " mean", m[:, C:]) + pad_cmp(lab + " rstd", r[:, C:])

    # -- wm_instnorm_apply on the synthetic statistics
    def _store_b(self, v, bv):
        return bv + half_ulp(v, self.dt) + TINY32

    def _apply(self):
        _, _, z, bz = self._z(self.smean, self.srstd)
        self.y = np.where(self.smask, z, 0.0) if self.act else z
        self.by = np.where(self.smask, self._store_b(z, bz), 0.0)

    def check_apply(self, y):
        real, pad = nchw(y, self.C)
        return [ECmp(self.label + " apply y", real, self.y, self.by)] + pad_cmp(self.label + " apply y", pad)

    # -- wm_instnorm_bwd_sums on the synthetic statistics
    def _sums(self):
        n = self.hw
        xh, dxh, _, _ = self._z(self.smean, self.srstd)
        g = np.where(self.smask, self.dy, 0.0)
        self.mg, self.mgx = g.mean(2), (g * xh).mean(2)
        ag, agx = np.abs(g).mean(2), np.abs(g * xh).mean(2)
        self.bmg = ulp32(self.mg) + D53 * n * ag
        self.bmgx = ulp32(self.mgx) + (np.abs(g) * dxh).mean(2) + D53 * (n + 1) * agx
        self.dbeta, self.dgamma = g.sum((0, 2)), (g * xh).sum((0, 2))
        tot = self.B * n
        self.bdbeta = ulp32(self.dbeta) + D53 * tot * np.abs(g).sum((0, 2))
        self.bdgamma = ulp32(self.dgamma) + (np.abs(g) * dxh).sum((0, 2)) + D53 * (tot + 1) * np.abs(g * xh).sum((0, 2))

    def check_sums(self, mg, mgx, dgamma=None, dbeta=None):
        a, b = f64(mg), f64(mgx)
        C, lab = self.C, self.label + " bwd_sums"
        cm = [ECmp(lab + " mg", a[:, :C], self.mg, self.bmg), ECmp(lab + " mgx", b[:, :C], self.mgx, self.bmgx)]
        cm += pad_cmp(lab + " mg", a[:, C:]) + pad_cmp(lab + " mgx", b[:, C:])
        if dgamma is not None:
            cm += [ECmp(lab + " dgamma", f64(dgamma).reshape(-1), self.dgamma, self.bdgamma), ECmp(lab + " dbeta", f64(dbeta).reshape(-1), self.dbeta, self.bdbeta)]
        return cm

    # -- wm_instnorm_bwd_apply on the synthetic statistics and means
    def _dx(self, xh, dxh, g, rstd, drstd, mg, dmg, mgx, dmgx):
        """dx = a * fma(-xhat, mgx, g - mg), a = gamma * rstd: g - mg: 1 on |g| + |mg|; the fma: 1 on |xhat mgx| + |g - mg| (apart: 2 on the
        product); a: 1; the product with a: 1"""
        inner = g - mg - xh * mgx
        binner = dmg + np.abs(mgx) * dxh + np.abs(xh) * dmgx + R * (2 * (np.abs(g) + np.abs(mg)) + 2 * np.abs(xh * mgx))
        a = rstd if self.g3 is None else self.g3 * rstd
        da = drstd * (1.0 if self.g3 is None else np.abs(self.g3)) + (0.0 if self.g3 is None else R * np.abs(a))
        dx = a * inner
        return dx, self._store_b(dx, np.abs(a) * binner + np.abs(inner) * da + R * np.abs(dx) + TINY32)

    def _bwd_apply(self):
        xh, dxh, _, _ = self._z(self.smean, self.srstd)
        g = np.where(self.smask, self.dy, 0.0)
        e = lambda v: v[:, :, None]
        self.dx, self.bdx = self._dx(xh, dxh, g, e(self.srstd), 0.0, e(self.smg), 0.0, e(self.smgx), 0.0)

    def check_bwd_apply(self, dx):
        real, pad = nchw(dx, self.C)
        return [ECmp(self.label + " bwd_apply dx", real, self.dx, self.bdx)] + pad_cmp(self.label + " bwd_apply dx", pad)

    # -- the four calls in a row (glayers.InstanceNorm2d): every error of a stage enters the next one's bound
    def _chain(self):
        e = lambda v: v[:, :, None]
        xh, dxh, z, bz = self._z(self.mean, self.rstd, self.bmean, self.brstd)
        const = e(self.isconst)
        self.cy = np.where(self.cmask, np.where(const, rnd(z, self.dt), z), 0.0)  # a constant plane: xhat = 0 and y = beta as stored, exactly
        self.bcy = np.where(self.cmask & ~const, self._store_b(z, bz), 0.0)
        g = np.where(self.cmask, self.dy, 0.0)
        mg, mgx = g.mean(2), (g * xh).mean(2)
        bmg = ulp32(mg) + D53 * self.hw * np.abs(g).mean(2)
        bmgx = ulp32(mgx) + (np.abs(g) * dxh).mean(2) + D53 * (self.hw + 1) * np.abs(g * xh).mean(2)
        self.cdx, self.bcdx = self._dx(xh, dxh, g, e(self.rstd), e(self.brstd), e(mg), e(bmg), e(mgx), e(bmgx))
        dead = const & ~self.cmask.any(2, keepdims=True)                          # ... and behind a ReLU that masks all of it dx = 0
        self.bcdx = np.where(dead, 0.0, self.bcdx)
        self.cdbeta, self.cdgamma = g.sum((0, 2)), (g * xh).sum((0, 2))
        tot = self.B * self.hw
        self.bcdbeta = ulp32(self.cdbeta) + D53 * tot * np.abs(g).sum((0, 2))
        self.bcdgamma = ulp32(self.cdgamma) + (np.abs(g) * dxh).sum((0, 2)) + D53 * (tot + 1) * np.abs(g * xh).sum((0, 2))

    def check_chain(self, y, dx, dgamma=None, dbeta=None):
        lab = self.label + " chain"
        yr, yp = nchw(y, self.C)
        dr, dp = nchw(dx, self.C)
        cm = [ECmp(lab + " y", yr, self.cy, self.bcy), ECmp(lab + " dx", dr, self.cdx, self.bcdx)] + pad_cmp(lab + " y", yp) + pad_cmp(lab + " dx", dp)
        if dgamma is not None:
            cm += [ECmp(lab + " dgamma", f64(dgamma).reshape(-1), self.cdgamma, self.bcdgamma), ECmp(lab + " dbeta", f64(dbeta).reshape(-1), self.cdbeta, self.bcdbeta)]
        return cm

    # -- operands as the kernels read them
    def t_x(self):
        return nhwc(self.x, self.CP, self.dt)

    def t_dy(self):
        return nhwc(self.dy, self.CP, self.dt)

    def t_rows(self, name):
        return rows(getattr(self, name), self.CP)

    def t_gamma(self):
        return None if self.gamma is None else store(self.gamma, "f32")

    def t_beta(self):
        return None if self.beta is None else store(self.beta, "f32")


@functools.lru_cache(maxsize=4)
def in_case(*key):
    return InCase(*key)


def in_keys(dt):
    """(dt, CP, C, hw, B, affine, act, eps, kind): every plane size at strides 16 and 48 with B, affine, act and eps taking turns (both
    values of each at every size), the four affine x act paths at hw = 257 with B = 3, the constant and the cancellation planes, 64 splits
    and the first size whose chunk grows (stride 16, B = 1), and the one-slot layout over one and over two splits"""
    keys, i = [], 0
    (s16, s48, s1) = IN_LAYOUTS[dt]
    for CP, C in (s16, s48):
        for hw in IN_HW:
            for B in (1, 3):
                eps = IN_EPS[i % 3]
                keys.append((dt, CP, C, hw, B, (i // 2 + i) % 2, (i // 2) % 2, IN_EPS[0] if hw == 1 and eps == 0 else eps, "normal"))
                i += 1
        keys += [(dt, CP, C, 257, 3, a, r, IN_EPS[1], "normal") for a in (0, 1) for r in (0, 1)]
        keys += [(dt, CP, C, 257, 3, 1, 1, IN_EPS[0], "const"), (dt, CP, C, 513, 1, 1, 0, IN_EPS[0], "cancel")]
    keys += [(dt, s16[0], s16[1], hw, 1, 1, 1, IN_EPS[0], "normal") for hw in (16384, 16385)]
    keys += [(dt, s1[0], s1[1], hw, 1, a, 1, IN_EPS[0], "normal") for hw, a in ((2, 0), (257, 1))]
    return tuple(dict.fromkeys(keys))


# ----------------------------------------------------------------------------------------------------------------- Dice
DICE_WG, DICE_MAX_PARTS = 4096, 64                        # one partial per 4096 elements of a sample, at most 64
DICE_PER = (1, 3, 4, 5, 255, 1027, 4097, 64 * 4096 + 5)
DICE_PW = (1.0, 2.0, 3.0, 1.5)
DICE_B = (1, 5)
DICE_OFFSETS = ((0, 0), (1, 1), (1, 2))                   # elements past a 16-byte boundary of p and of target: aligned, head + tail, all scalar
REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}
SMOOTH = 1.0
SOFT_C = (1, 2, 5, 32)
SOFT_TILE = 1024


def dice_nparts(per):
    return max(1, min(DICE_MAX_PARTS, -(-per // DICE_WG))) if per > 0 else 0


SOFT_HW = (1, 4, 255, 1024, 1028, 1029, 2 * SOFT_TILE * dice_nparts(2 * SOFT_TILE + 7) + 7)
SOFT_BWD_GROUPS = 256                                     # the backward's grid cap: one tile per workgroup up to here
SOFT_BWD_TWO_TILES = 2 * SOFT_TILE * SOFT_BWD_GROUPS + 7


def pow_b(v, dv, pw):
    """(v^pw, bound) as the kernels form it: pw = 1 the value itself, pw = 2 one product, otherwise powf"""
    if pw == 1.0:
        return v, dv
    if pw == 2.0:
        return v * v, 2 * np.abs(v) * dv + R * v * v
    y = np.power(v, pw)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = np.where(v > 0, pw * np.power(v, pw - 1.0), 0.0)
    return y, slope * dv + POW_ULP * ulp32(y)


def powm1_b(v, dv, pw):
    """(v^(pw-1), bound): 1, v, or powf(v, pw - 1)"""
    if pw == 1.0:
        return np.ones_like(v), np.zeros_like(v)
    if pw == 2.0:
        return v, dv + np.zeros_like(v)
    return pow_b(v, dv, pw - 1.0)


def unit_sums(s, ds, t, pw, n_axis):
    """{sum s t, sum s^pw, sum t^pw} over the last axis and their bounds: the products in float32 (k = 1), the additions in double"""
    st, bst = s * t, ds * np.abs(t) + R * np.abs(s * t)
    sp, bsp = pow_b(s, ds, pw)
    tp, btp = pow_b(t, 0.0 * t, pw)
    S = np.stack([st.sum(-1), sp.sum(-1), tp.sum(-1)], -1)
    bS = np.stack([bst.sum(-1), bsp.sum(-1), btp.sum(-1)], -1) + D53 * n_axis * np.stack([np.abs(st).sum(-1), np.abs(sp).sum(-1), np.abs(tp).sum(-1)], -1)
    return S, bS + TINY32


def finalize_ref(partials, B, C, smooth, reduction, ignore_index=-1, weight=None):
    """wm_dice_finalize of the partials it is GIVEN [B*C, P, 3] (doubles): coef [B*C, 2] = {num, den} in double, and the loss -- every
    operation in double (D53 each), one rounding to float32 at the end.  -> (coef, bcoef, loss, bloss)"""
    q = np.asarray(partials, dtype=np.float64).reshape(B * C, -1, 3)
    P = q.shape[1]
    num, den = q[:, :, 0].sum(1) + smooth, (q[:, :, 1].sum(1) + q[:, :, 2].sum(1)) + smooth
    anum, aden = np.abs(q[:, :, 0]).sum(1) + abs(smooth), np.abs(q[:, :, 1:]).sum((1, 2)) + abs(smooth)
    coef, bcoef = np.stack([num, den], 1), D53 * (2 * P + 2) * np.stack([anum, aden], 1)
    w = np.ones(C) if weight is None else np.asarray(weight, dtype=np.float64).copy()
    if 0 <= ignore_index < C:
        w[ignore_index] = 0.0
    w = np.tile(w / C, B)
    l = 1.0 - num / den
    dl = bcoef[:, 0] / np.abs(den) + np.abs(num) * bcoef[:, 1] / den ** 2 + 2 * D53 * (1.0 + np.abs(num / den))
    per_b, bper_b = (w * l).reshape(B, C).sum(1), (np.abs(w) * dl + D53 * (C + 2) * np.abs(w * l)).reshape(B, C).sum(1)
    if reduction == "none":
        loss, bloss = per_b, bper_b
    else:
        k = 1.0 / B if reduction == "mean" else 1.0
        loss = np.array([per_b.sum() * k])
        bloss = np.array([(bper_b.sum() + D53 * (B + 2) * np.abs((w * l)).sum()) * k])
    return coef, bcoef, loss, bloss + ulp32(loss)


def check_finalize(label, coef, loss, partials, B, C, smooth, reduction, ignore_index=-1, weight=None):
    rc, bc, rl, bl = finalize_ref(partials, B, C, smooth, reduction, ignore_index, weight)
    lab = "%s finalize %s" % (label, reduction)
    return [ECmp(lab + " coef", f64(coef).reshape(rc.shape), rc, bc), ECmp(lab + " loss", f64(loss).reshape(rl.shape), rl, bl)]


def upstream(B, reduction, gscale, gdev, gout):
    """[B]: gscale * gscale_dev[0] * gout[none ? b : 0], / B for the mean: float32 factors multiplied in double"""
    g = np.full(B, float(np.float32(gscale)))
    if gdev is not None:
        g = g * float(np.float32(gdev))
    if gout is not None:
        go = r32(np.asarray(gout, dtype=np.float64)).reshape(-1)
        g = g * (go if reduction == "none" else go[0])
    return g / B if reduction == "mean" else g


def dloss_b(s, ds, t, kp, kt, pw):
    """g = kp s^(pw-1) - kt t, kp and kt (here exact) rounded to float32 from double (1 each): the two products (1 each) and the difference (1) --
    k = 3 on each term whether or not the compiler contracts the difference into an fma (then 2)"""
    pm, dpm = powm1_b(s, ds, pw)
    t1, t2 = kp * pm, kt * t
    return t1 - t2, np.abs(kp) * dpm + 3 * R * (np.abs(t1) + np.abs(t2))


class DiceBinCase:
    """wm_dice_sums / wm_dice_finalize / wm_dice_bwd on p in (0, 1), target in {0, 1, 0.5}, [B, per] float32"""

    def __init__(self, per, B, pw):
        self.per, self.B, self.pw = per, B, float(pw)
        seed = 21000 + per % 9973 + 31 * B + int(8 * pw)
        self.p, self.t = r32(uni((B, per), seed, 0.02, 0.98)), pick((B, per), seed + 1, (0.0, 0.0, 0.0, 1.0, 1.0, 0.5))
        self.old = r32(normal((B, per), seed + 2, std=0.01))
        self.label = "dice_binary per=%d B=%d pw=%g" % (per, B, pw)
        self.S, self.bS = unit_sums(self.p, 0.0 * self.p, self.t, self.pw, per)
        self.coef = np.stack([self.S[:, 0] + SMOOTH, self.S[:, 1] + self.S[:, 2] + SMOOTH], 1)      # what the backward is fed: any doubles do

    def check_sums(self, partials):
        q = f64(partials).reshape(self.B, -1, 3)
        assert q.shape[1] == dice_nparts(self.per), (self.label, q.shape)
        return [ECmp(self.label + " sums per unit", q.sum(1), self.S, self.bS)]

    def grad_ref(self, reduction="mean", gscale=1.0, gdev=None, gout=None, chain=False, accumulate=False):
        g = upstream(self.B, reduction, gscale, gdev, gout)[:, None]
        num, den = self.coef[:, :1], self.coef[:, 1:]
        kt, kp = g / den, g * num * self.pw / (den * den)
        v, bv = dloss_b(self.p, 0.0, self.t, kp, kt, self.pw)
        if chain:                                                                                    # v * (x (1 - x)): 1 - x: 1, the two products
            x = self.p
            v2 = v * x * (1.0 - x)
            bv = bv * np.abs(x * (1.0 - x)) + np.abs(v * x) * R * (1.0 + np.abs(x)) + 2 * R * np.abs(v2)
            v = v2
        if accumulate:
            bv = bv + R * (np.abs(self.old) + np.abs(v))
            v = v + self.old
        return v, bv + TINY32

    def check_grad(self, grad, **kw):
        v, bv = self.grad_ref(**kw)
        tag = " ".join("%s=%s" % (k, ("dev" if k in ("gdev", "gout") and w is not None else w)) for k, w in sorted(kw.items()))
        return [ECmp("%s bwd %s" % (self.label, tag), f64(grad).reshape(v.shape), v, bv)]


@functools.lru_cache(maxsize=4)
def dice_bin_case(per, B, pw):
    return DiceBinCase(per, B, pw)


DICE_BIN_KEYS = tuple((per, B, pw) for per in DICE_PER[:-1] for B in DICE_B for pw in DICE_PW) + tuple((DICE_PER[-1], 1, pw) for pw in DICE_PW)
BIN_GRAD_MODES = (dict(), dict(chain=True), dict(accumulate=True), dict(gscale=0.7, gdev=1.5), dict(reduction="none", gout="per_sample"),
                  dict(reduction="sum", chain=True, accumulate=True, gscale=0.7))


def softmax_b(z):
    """softmax over axis 1 of [B, C, HW] as float32 forms it, and its bound: x = z - max (1), e = expf(x) (the rounding of x through exp,
    U exp ulps), d = the sum of the C e's in turn (C - 1), inv = 1 / d (1), s = e inv (1)"""
    C = z.shape[1]
    x = z - z.max(1, keepdims=True)
    e = np.exp(x)
    de = e * R * np.abs(x) + U["exp"] * ulp32(e)
    d, dd = e.sum(1, keepdims=True), de.sum(1, keepdims=True)
    dd = dd + R * (C - 1) * d
    inv = 1.0 / d
    dinv = dd / d ** 2 + R * inv
    s = e * inv
    return s, de * inv + e * dinv + R * s + TINY32


class DiceSoftCase:
    """wm_dice_softmax_sums / _finalize / _softmax_bwd on logits [B, C, HW] and one-hot targets; `dominate`: in every third pixel class 0
    leads by 80 (the others' exponentials are tiny normals), in the next by 120 (expf underflows: s is exactly 0)"""

    def __init__(self, B, C, HW, pw, dominate=False, cheap=False):
        self.B, self.C, self.HW, self.pw, self.dominate = B, C, HW, float(pw), dominate
        seed = 22000 + 7 * B + 31 * C + HW % 9973 + int(8 * pw)
        if cheap:
            self.z = 2.0 * pattern(B * C * HW).reshape(B, C, HW)
            lab = (np.arange(B * HW, dtype=np.int64) * 7 % 5 % C).reshape(B, 1, HW)
        else:
            self.z = r32(2.0 * normal((B, C, HW), seed))
            lab = np.minimum(np.floor(uni((B, 1, HW), seed + 1) * C), C - 1).astype(np.int64)
        if dominate and C > 1:
            self.z[:, 0, 0::3] = r32(self.z[:, 1:, 0::3].max(1) + 80.0)
            self.z[:, 0, 1::3] = r32(self.z[:, 1:, 1::3].max(1) + 120.0)
        self.t = (np.arange(C)[None, :, None] == lab).astype(np.float64)
        self.old = r32(0.01 * pattern(B * C * HW, 41).reshape(B, C, HW))
        self.weight = r32(uni((C,), seed + 3, 0.5, 1.5))
        self.label = "dice_softmax B=%d C=%d HW=%d pw=%g%s" % (B, C, HW, pw, " dominate" if dominate else "")
        self.s, self.ds = softmax_b(self.z)
        self.S, self.bS = unit_sums(self.s, self.ds, self.t, self.pw, HW)                          # [B, C, 3]
        self.coef = np.stack([self.S[..., 0] + SMOOTH, self.S[..., 1] + self.S[..., 2] + SMOOTH], -1).reshape(B * C, 2)

    def check_sums(self, partials):
        q = f64(partials).reshape(self.B, self.C, -1, 3)
        assert q.shape[2] == dice_nparts(self.HW), (self.label, q.shape)
        return [ECmp(self.label + " sums per unit", q.sum(2), self.S, self.bS)]

    def grad_ref(self, reduction="mean", ignore_index=-1, weighted=False, gscale=1.0, gdev=None, gout=None, accumulate=False):
        """dz_c = s_c (g_c - sum_k g_k s_k): the dot product's C fmas (C + 1 with the products apart) against sum |g_k s_k|, g_k's and
        s_k's own bounds through it; the difference: 1; the product with s_c: 1"""
        B, C = self.B, self.C
        w = self.weight.copy() if weighted else np.ones(C)
        if 0 <= ignore_index < C:
            w[ignore_index] = 0.0                           # g_c = 0 there; the class still gets -s_c * dot
        g = upstream(B, reduction, gscale, gdev, gout)[:, None] * (w / C)[None, :]                # [B, C], in double
        num, den = self.coef[:, 0].reshape(B, C), self.coef[:, 1].reshape(B, C)
        kt, kp = (g / den)[..., None], (g * num * self.pw / (den * den))[..., None]
        gc, bgc = dloss_b(self.s, self.ds, self.t, kp, kt, self.pw)
        dot = (gc * self.s).sum(1, keepdims=True)
        bdot = (bgc * self.s + np.abs(gc) * self.ds).sum(1, keepdims=True) + R * (C + 1) * np.abs(gc * self.s).sum(1, keepdims=True)
        diff = gc - dot
        bdiff = bgc + bdot + R * (np.abs(gc) + np.abs(dot))
        dz = self.s * diff
        bdz = self.ds * np.abs(diff) + self.s * bdiff + R * np.abs(dz)
        if accumulate:
            bdz = bdz + R * (np.abs(self.old) + np.abs(dz))
            dz = dz + self.old
        return dz, bdz + TINY32

    def check_grad(self, grad, **kw):
        v, bv = self.grad_ref(**kw)
        tag = " ".join("%s=%s" % (k, ("dev" if k in ("gdev", "gout") and w is not None else w)) for k, w in sorted(kw.items()))
        return [ECmp("%s bwd %s" % (self.label, tag), f64(grad).reshape(v.shape), v, bv)]


@functools.lru_cache(maxsize=4)
def dice_soft_case(B, C, HW, pw, dominate=False, cheap=False):
    return DiceSoftCase(B, C, HW, pw, dominate, cheap)


def dice_soft_keys():
    """(B, C, HW, pw, dominate, cheap): every C at every HW with pw and B taking turns, the dominated logits at a VEC and at a strided
    size, and the one size at which a workgroup of the BACKWARD takes two tiles (C = 2, index-made data)"""
    keys, i = [], 0
    for C in SOFT_C:
        for HW in SOFT_HW:
            keys.append((DICE_B[i % 2] if C < 32 else 1, C, HW, DICE_PW[i % 4], False, False))
            i += 1
    keys += [(2, 5, HW, pw, True, False) for HW in (1028, 1029) for pw in (2.0, 1.5)]
    keys.append((1, 2, SOFT_BWD_TWO_TILES, 2.0, False, True))
    return tuple(keys)


SOFT_GRAD_MODES = (dict(), dict(ignore_index=0), dict(ignore_index="last", weighted=True), dict(weighted=True, accumulate=True, gscale=0.7, gdev=1.5),
                   dict(reduction="none", gout="per_sample"), dict(reduction="sum", accumulate=True))


def resolve_mode(mode, B, C=1):
    """a grad mode of the tables above with its placeholders filled in: gout `per_sample` -> B float32 factors, ignore_index `last` -> C - 1"""
    m = dict(mode)
    if m.get("gout") == "per_sample":
        m["gout"] = r32(0.5 + 0.25 * np.arange(B)) if m.get("reduction") == "none" else r32(np.array([0.75]))
    if m.get("ignore_index") == "last":
        m["ignore_index"] = C - 1
    return m


# ----------------------------------------------------------------------------------------------------------------- two-source mask head
HEAD_MAXG, HEAD_PARTS_UNIT, HEAD_PARTS_CAP = 16, 128, 1024
HEAD_FWD_UNROLL, HEAD_FWD_CAP = 4, 2048                   # the forward: 4 pixels per lane group and trip, at most 2048 workgroups


def head_G(lda, ldb, dt):
    """lanes that share a pixel: the larger source's 16-byte vectors per pixel, rounded up to a power of two; 0: refused"""
    ve = VE[dt]
    if lda <= 0 or ldb <= 0 or lda % ve or ldb % ve:
        return 0
    g = 1
    while g < max(lda, ldb) // ve:
        g *= 2
    return g if g <= HEAD_MAXG else 0


def head_nparts(npix):
    return max(1, min(HEAD_PARTS_CAP, -(-npix // HEAD_PARTS_UNIT))) if npix > 0 else 0


def head_fwd_grid(npix, G):
    return max(1, min(HEAD_FWD_CAP, -(-npix // ((256 // G) * HEAD_FWD_UNROLL))))


def head_second_trip(G):
    """the first pixel count at which the forward's capped grid must go round again"""
    return HEAD_FWD_CAP * (256 // G) * HEAD_FWD_UNROLL + 1


class HeadCase:
    """out = act(bias + w[:, :na] a + w[:, na:] b) as NCHW float32 from two NHWC sources of dtype dt; its backward.  B x hw = npix."""

    def __init__(self, dt, lda, na, ldb, nb, Cout, B, hw, act, bias, chain, cheap=False):
        self.dt, self.lda, self.na, self.ldb, self.nb, self.Cout, self.B, self.hw = dt, lda, na, ldb, nb, Cout, B, hw
        self.act, self.has_bias, self.chain = act, bias, chain and act == 1
        npix = self.npix = B * hw
        self.G = head_G(lda, ldb, dt)
        self.PPB = 256 // self.G
        seed = 23000 + 3 * lda + 5 * na + 7 * ldb + 11 * nb + 13 * Cout + npix % 9973
        self.label = "head2 %s a %d/%d b %d/%d Cout=%d B=%d hw=%d act=%d bias=%d chain=%d" % (dt, na, lda, nb, ldb, Cout, B, hw, act, bias, self.chain)
        if cheap:
            self.a, self.b = pattern(npix * na).reshape(npix, na), pattern(npix * nb, 41).reshape(npix, nb)
            self.gout = pattern(npix * Cout, 43).reshape(B, Cout, hw)
        else:
            self.a, self.b = rnd(normal((npix, na), seed), dt), rnd(normal((npix, nb), seed + 1), dt)
            self.gout = r32(normal((B, Cout, hw), seed + 2))
        self.w = r32(0.3 * normal((Cout, na + nb), seed + 3))
        self.bias = r32(0.5 * normal((Cout,), seed + 4)) if bias else None
        self.old_w, self.old_b = r32(normal((Cout, na + nb), seed + 5)), r32(normal((Cout,), seed + 6))
        wa, wb = self.w[:, :na], self.w[:, na:]
        bs = self.bias if bias else np.zeros(Cout)
        # out: every product (1, were it not fused) and the na + nb additions of the chain, the tree and the bias, in any order
        v = self.a @ wa.T + self.b @ wb.T + bs
        av = np.abs(self.a) @ np.abs(wa).T + np.abs(self.b) @ np.abs(wb).T + np.abs(bs)
        bv = R * (na + nb + 2) * av + TINY32
        if act:
            s, ds = sigmoid_ref(v)
            v, bv = s, s * (1.0 - s) * bv + ds + TINY32
        self.out, self.bout = self._planes(v), self._planes(bv)
        # backward.  The saved sigmoid output is an INPUT: float32 of the reference
        self.saved = r32(self.out) if self.chain else None
        gz, bgz = self._pix(self.gout), 0.0
        if self.chain:                                     # go * (s * (1 - s)): 1 - s: 1 on 1 + s; the two products
            s = self._pix(self.saved)
            gz0 = gz
            gz = gz0 * s * (1.0 - s)
            bgz = np.abs(gz0 * s) * R * (1.0 + s) + 2 * R * np.abs(gz)
        self.gz = gz
        bgz = bgz + np.zeros_like(gz)
        self.ga, self.bga = self._gsrc(gz, bgz, wa)
        self.gb, self.bgb = self._gsrc(gz, bgz, wb)
        # dw, db: a lane adds its own pixels in float32 (T of them: one fma each), everything after that in double, one rounding
        self.nparts = head_nparts(npix)
        T = -(-npix // (self.nparts * self.PPB))
        x = np.concatenate([self.a, self.b], 1)
        self.dw = gz.T @ x
        self.bdw_sum = R * (T + 1) * (np.abs(gz).T @ np.abs(x)) + bgz.T @ np.abs(x) + D53 * npix * (np.abs(gz).T @ np.abs(x)) + TINY32
        self.db = gz.sum(0)
        self.bdb_sum = R * T * np.abs(gz).sum(0) + bgz.sum(0) + D53 * npix * np.abs(gz).sum(0) + TINY32

    def _planes(self, v):
        return v.reshape(self.B, self.hw, self.Cout).transpose(0, 2, 1)

    def _pix(self, planes):
        return planes.transpose(0, 2, 1).reshape(self.npix, self.Cout)

    def _gsrc(self, gz, bgz, ws):
        """ga[p, c] = sum_co gz[p, co] w[co, c]: Cout fmas (Cout + 1 with the products apart), stored in dt"""
        g = gz @ ws
        return g, bgz @ np.abs(ws) + R * (self.Cout + 1) * (np.abs(gz) @ np.abs(ws)) + TINY32 + half_ulp(g, self.dt)

    def t_a(self):
        return nhwc(self.a.T[None], self.lda, self.dt)[0]

    def t_b(self):
        return nhwc(self.b.T[None], self.ldb, self.dt)[0]

    def check_fwd(self, out):
        return [ECmp(self.label + " out", f64(out).reshape(self.out.shape), self.out, self.bout)]

    def check_bwd(self, ga, gb):
        lab, cm = self.label + " bwd", []
        for name, t, n, ref, bound in (("ga", ga, self.na, self.ga, self.bga), ("gb", gb, self.nb, self.gb, self.bgb)):
            real, pad = nchw(f64(t)[None], n)
            cm += [ECmp("%s %s" % (lab, name), real[0].T, ref, bound)] + pad_cmp("%s %s" % (lab, name), pad)
        return cm

    def check_partials(self, partials):
        q = f64(partials).reshape(self.nparts, -1).sum(0)
        n = self.Cout * (self.na + self.nb)
        return [ECmp(self.label + " bwd partials dw", q[:n].reshape(self.dw.shape), self.dw, self.bdw_sum),
                ECmp(self.label + " bwd partials db", q[n:], self.db, self.bdb_sum)]

    def check_params(self, dw, db, accumulate=False):
        rw, rb = (self.dw + self.old_w, self.db + self.old_b) if accumulate else (self.dw, self.db)
        lab = self.label + (" finalize accumulate" if accumulate else " finalize")
        return [ECmp(lab + " dw", f64(dw).reshape(rw.shape), rw, self.bdw_sum + ulp32(rw)), ECmp(lab + " db", f64(db).reshape(rb.shape), rb, self.bdb_sum + ulp32(rb))]


@functools.lru_cache(maxsize=4)
def head_case(*key):
    return HeadCase(*key)


HEAD_SOURCES = {     # (lda, na, ldb, nb): 16 lanes per pixel, the smallest stride, and the two unequal pairs (one source's lanes idle)
    "f32": ((64, 60, 16, 16), (16, 13, 16, 5), (16, 9, 48, 41), (48, 41, 16, 9)),
    "bf16": ((128, 120, 16, 13), (16, 13, 16, 5), (16, 9, 48, 41), (48, 41, 16, 9)),
    "f16": ((128, 120, 16, 13), (16, 13, 16, 5), (16, 9, 48, 41), (48, 41, 16, 9)),
}


def head_keys(dt):
    """(dt, lda, na, ldb, nb, Cout, B, hw, act, bias, chain, cheap): per source pair npix in {1, 4 PPB - 1, 4 PPB, 4 PPB + 1} (4 PPB as
    two samples), Cout, act, bias and the chain taking turns; Cout 1..4 x act at the 16-lane pair"""
    keys, i = [], 0
    for lda, na, ldb, nb in HEAD_SOURCES[dt]:
        n4 = (256 // head_G(lda, ldb, dt)) * HEAD_FWD_UNROLL
        for B, hw in ((1, 1), (1, n4 - 1), (2, n4 // 2), (1, n4 + 1)):
            keys.append((dt, lda, na, ldb, nb, 1 + i % 4, B, hw, (i // 2) % 2, (i + 1) % 2, (i // 4) % 2 == 0, False))
            i += 1
    lda, na, ldb, nb = HEAD_SOURCES[dt][0]
    n4 = (256 // head_G(lda, ldb, dt)) * HEAD_FWD_UNROLL
    keys += [(dt, lda, na, ldb, nb, co, 1, n4 + 1, act, 1, True, False) for co in (1, 2, 3, 4) for act in (0, 1)]
    return tuple(dict.fromkeys(keys))


def head_big_key():
    """the forward's second trip: float32, 16 lanes per pixel, one pixel past the capped grid's reach; index-made data"""
    lda, na, ldb, nb = 64, 60, 4, 3
    return ("f32", lda, na, ldb, nb, 2, 1, head_second_trip(head_G(lda, ldb, "f32")), 1, 1, False, True)
