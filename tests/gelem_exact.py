"""Float64 restatements of the general elementwise kernels (csrc/gelem.hip) and the invertible embedder's pieces (csrc/inn.hip), written from
the definitions in include/wm_hip.h, the kernels' comments and the reference modules they cite (nn.ReLU, nn.LeakyReLU(0.2), nn.GELU, nn.ELU,
nn.Sigmoid, nn.Tanh; x + gamma*res + beta; nn.AdaptiveAvgPool2d((1, 1)); symm_pad / nn.ReplicationPad2d; torch.nn.utils.spectral_norm with
one power iteration; HaarDownsampling / HaarUpsampling with order_by_wavelet; RNVPCouplingBlock's affine), with the case tables and the
per-element comparisons built on them.  A plain helper module (CPU only, never imports the HIP package): tests/test_cpu_gelem_exact.py runs
float32 imitations -- faithful and defective -- through these comparisons, tests/test_gpu_gelem_exact.py runs the kernels through them.

Bounds follow the rule of tests/layers_exact.py: a float32 result formed with k roundings from exact inputs is accepted within
FACTOR * k * 2**-24 * (the sum of the absolute values of its terms); a sum of n terms takes n - 1 roundings in any order, and adding an exact
zero is exact; a value stored as bf16 / f16 adds half_ulp(ref, dt); inputs are values of the storage type.  a + alpha*b is counted as two
roundings (the contracted fma has one).  Division and sqrtf are correctly rounded (no fast-math in build.py): one rounding each.  TINY32,
the spacing of the float32 subnormals, is added to every inexact bound: below 2**-126 the format's absolute spacing replaces its relative
one.

The device math functions cannot be bounded from the project.  U holds their allowance in ulps of the float32 result, taken from the
OpenCL C specification's table of minimum accuracy for single precision in the full profile ("Relative Error as ULPs": exp <= 3 ulp,
expm1 <= 3 ulp, erf <= 16 ulp, tanh <= 5 ulp), which the ROCm device library's math functions are written to meet.  No tighter documented
figure ships with the ROCm installation this was written against.  U is used as U * ulp32(result), once, with no margin of its own (FACTOR
multiplies only the counted roundings), and is propagated through each expression's conditioning next to its use.

Exact, bit for bit: copies, zero fills, padding gathers, routing, the untouched SENTINEL values around every destination, every piecewise
branch whose value is one correctly rounded float32 operation on exact inputs (relu, 0.2f * x, g * 0.2f, g * (out + 1): float64 holds the
exact product or sum, so rounding it to float32 IS the kernel's float32 result; stored as 16 bits it is exact where that result is a
value of the type and correctly rounded otherwise, see finish()), Haar with fac = 0.5 on multiples
of 1/8, gpool_bwd with hw a power of two.  The derivative at x = 0 follows the kernels' `x > 0` test: relu' 0, lrelu' 0.2, elu' 1
(exp(0)), ELU_OUT 1 (0 + 1) at out = 0.  No comparison leaves an element out: every branch is decided by an input value, never by a
computed one.
"""
import functools
import math

import numpy as np
import torch

from layers_exact import EPS32, FACTOR, SENTINEL, Cmp, grid, half_ulp, normal, pick, rnd, store  # noqa: F401  (re-exported to the two test files)
from layers_exact import DTYPES, TORCH, VE, all_ok, f64, first_bad  # noqa: F401

# OpenCL C specification, "Relative Error as ULPs", single precision, full profile
U = {"exp": 3.0, "expm1": 3.0, "erf": 16.0, "tanh": 5.0, "log": 3.0, "log1p": 2.0}      # log, log1p: tests/steploss_exact.py
F32_MAX = float(np.finfo(np.float32).max)
TINY32 = 2.0 ** -149
MIN_NORMAL = {"f32": 2.0 ** -126, "bf16": 2.0 ** -126, "f16": 2.0 ** -14}
MAX_FINITE = {"f32": F32_MAX, "bf16": float(torch.finfo(torch.bfloat16).max), "f16": 65504.0}
SLOPE = float(np.float32(0.2))                            # nn.LeakyReLU(0.2) on float32 tensors
INV_SQRT2 = float(np.float32(0.70710678118654752))
INV_SQRT2PI = float(np.float32(0.3989422804014327))
RELU, LRELU, GELU, ELU, SIGMOID, TANH, ELU_OUT = range(7)
KIND_NAMES = ("relu", "lrelu", "gelu", "elu", "sigmoid", "tanh", "elu_out")
R = FACTOR * EPS32                                        # one counted rounding, relative


def ulp32(v):
    """the spacing of float32 at |v| (at least that of the subnormals), as float64"""
    a = np.minimum(np.abs(np.asarray(v, dtype=np.float64)), F32_MAX)
    e = np.where(a > 0, np.frexp(a)[1] - 1, -126)
    return np.ldexp(1.0, np.maximum(e, -126) - 23)


def erf64(a):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).numpy()


def r32(a):
    return rnd(a, "f32")


def specials(dt):
    return np.array([0.0, MIN_NORMAL[dt], -MIN_NORMAL[dt], 20.0, -20.0, MAX_FINITE[dt], -MAX_FINITE[dt]])


def pattern(n, mul=37, mod=33):
    """cheap grid data for the large cases: multiples of 1/8 in [-2, 2] from the index"""
    return ((np.arange(n, dtype=np.int64) * mul) % mod - 16).astype(np.float64) / 8.0


def finish(y, b, dt):
    """(value before storage, its float32 bound; 0 = the value is the exact float32 result) -> (reference, bound) of the stored value"""
    y, b = np.asarray(y, dtype=np.float64), np.broadcast_to(np.asarray(b, dtype=np.float64), np.shape(y))
    exact = b == 0
    if dt != "f32":
        # a 16-bit store of an exact float32 result y = fl32(v): the compiler may fuse the operation with the conversion (one rounding of v
        # to dt, the mixed-precision multiply-add of this chip) or keep the two roundings; |v - y| <= 2**-24 |y|, so either way the stored
        # value lies within half a dt ulp + 2**-24 |y| of y -- they differ only where y sits next to a dt midpoint.  Where y is a dt value
        # already, both give y: exact.
        fits = rnd(y, dt) == y
        return np.where(exact & fits, rnd(y, dt), y), np.where(exact & fits, 0.0, np.where(exact, EPS32 * np.abs(y), b) + half_ulp(y, dt) + TINY32)
    return np.where(exact, rnd(y, dt), y), np.where(exact, 0.0, b + TINY32)


# ----------------------------------------------------------------------------------------------------------------- activations
def sigmoid_ref(x):
    """s = 1 / (1 + exp(-x)): the exponential's U ulp through d s / d e = -s**2, then the sum and the division: 2 roundings of s"""
    with np.errstate(over="ignore"):
        e = np.exp(-x)
    s = 1.0 / (1.0 + e)
    return s, U["exp"] * ulp32(e) * s * s + 2 * R * s


def act_ref(kind, x):
    """(y, bound): the activation in float64 and the bound of its float32 value; bound 0 where that value is exact"""
    x = np.asarray(x, dtype=np.float64)
    zero = np.zeros(x.shape)
    if kind == RELU:
        return np.maximum(x, 0.0), zero
    if kind == LRELU:
        return np.where(x > 0, x, r32(SLOPE * x)), zero                      # one product: exact in float64, rounded once
    if kind == ELU:
        y = np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
        return y, np.where(x > 0, 0.0, U["expm1"] * ulp32(y))
    if kind == SIGMOID:
        return sigmoid_ref(x)
    if kind == TANH:
        y = np.tanh(x)
        return y, U["tanh"] * ulp32(y)
    assert kind == GELU
    # y = (0.5 x) * (1 + erf(a)), a = x * float32(1/sqrt 2): a carries 2 roundings (the constant, the product), which erf passes on as
    # erf'(a) = 2/sqrt(pi) exp(-a*a); erf itself U ulp; 1 + erf: 1 rounding on 1 + |erf|; 0.5 x exact; the product: 1 rounding
    a = x / math.sqrt(2.0)
    er = erf64(a)
    inner = 2.0 / math.sqrt(math.pi) * np.exp(-a * a) * 2 * R * np.abs(a) + U["erf"] * ulp32(er) + R * (1.0 + np.abs(er))
    y = 0.5 * x * (1.0 + er)
    return y, np.abs(0.5 * x) * inner + R * np.abs(y)


def act_dref(kind, x):
    """(d, bound) of the derivative the backward kernels multiply by; kind ELU_OUT reads the layer's OUTPUT"""
    x = np.asarray(x, dtype=np.float64)
    zero = np.zeros(x.shape)
    if kind == RELU:
        return np.where(x > 0, 1.0, 0.0), zero
    if kind == LRELU:
        return np.where(x > 0, 1.0, SLOPE), zero
    if kind == ELU:
        d = np.where(x > 0, 1.0, np.exp(np.minimum(x, 0.0)))
        return d, np.where(x > 0, 0.0, U["exp"] * ulp32(d))
    if kind == ELU_OUT:
        return np.where(x > 0, 1.0, r32(x + 1.0)), zero                      # one sum, rounded once
    if kind == SIGMOID:
        # s (1 - s): d/ds = 1 - 2 s; 1 - s: 1 rounding on 1 + s -- an absolute error near saturation --; the product: 1 rounding
        s, ds = sigmoid_ref(x)
        d = s * (1.0 - s)
        return d, ds * np.abs(1.0 - 2.0 * s) + ds * ds + s * R * (1.0 + s) + R * d
    if kind == TANH:
        # 1 - t*t: t U ulp, t*t 1 rounding, the difference 1 rounding on 1 + t*t (absolute near saturation)
        t = np.tanh(x)
        dt_ = U["tanh"] * ulp32(t)
        return 1.0 - t * t, 2.0 * np.abs(t) * dt_ + dt_ * dt_ + R * t * t + R * (1.0 + t * t)
    assert kind == GELU
    # d = 0.5 (1 + erf(a)) + (x k) exp(h), k = float32(1/sqrt(2 pi)), h = -0.5 x x
    a = x / math.sqrt(2.0)
    er = erf64(a)
    t1 = 0.5 * (1.0 + er)
    b1 = 0.5 * (2.0 / math.sqrt(math.pi) * np.exp(-a * a) * 2 * R * np.abs(a) + U["erf"] * ulp32(er) + R * (1.0 + np.abs(er)))
    h = -0.5 * x * x                                                          # 1 rounding (x*x; the factor 0.5 is exact)
    eh = np.exp(h)
    xk = x / math.sqrt(2.0 * math.pi)
    t2 = xk * eh
    b2 = np.abs(xk) * (eh * R * np.abs(h) + U["exp"] * ulp32(eh)) + 3 * R * np.abs(t2)      # the constant, x k, the product with exp
    return t1 + t2, b1 + b2 + R * (np.abs(t1) + np.abs(t2))                   # and the sum


def bwd_ref(kind, x, g):
    """gx = g * act'(x) before storage: exact derivative -> one product, rounded once; otherwise |g| * its bound + 1 rounding"""
    d, bd = act_dref(kind, x)
    p = g * d
    return np.where(bd == 0, r32(p), p), np.where(bd == 0, 0.0, np.abs(g) * bd + R * np.abs(p))


UNARY_CAP = 4096 * 256                                    # gelem.hip's grid1: at most 4096 workgroups of 256 threads
UNARY_OPS = ("fwd", "bwd", "add")
ALPHAS = (1.0, 0.5, -0.3)


def unary_shapes(dt):
    """(n, offset in elements, data): one vector; four vectors (specials on the vector path); the scalar path by length; by alignment"""
    ve = VE[dt]
    return ((ve, 0, "grid"), (4 * ve, 0, "normal"), (3 * ve + 1, 0, "normal"), (4 * ve, 1, "normal"))


def unary_caps(dt):
    ve = VE[dt]
    return ((UNARY_CAP * ve + 5 * ve, 0, "pattern"), (UNARY_CAP + 3, 0, "pattern"))       # vector path, scalar path: a second pass each


class UnaryCase:
    """wm_unary_fwd (op fwd), wm_unary_bwd (bwd), wm_add_scaled (add; `kind` indexes ALPHAS) on n elements that start `off` elements
    into a 16-byte aligned buffer of n + off + VE elements; the destination starts as SENTINEL and only [off, off + n) may change"""

    def __init__(self, dt, op, kind, n, off, data):
        self.dt, self.op, self.kind, self.n, self.off, self.data = dt, op, kind, n, off, data
        seed = 7000 + 31 * kind + n % 1000 + 500 * off
        self.pad = VE[dt]

        def draw(sd, special):
            if data == "pattern":
                return pattern(n, 37 + sd % 5)
            if data == "grid":
                return grid((n,), sd, 0.125, -2.0, 2.0)
            a = rnd(normal((n,), sd, std=2.0), dt)
            if special:
                sp = specials(dt)
                m = min(n, len(sp))
                a[n - m:] = sp[:m]                                            # at the end: the tail elements of the vector kernels
            return a
        if op == "add":
            self.alpha = float(np.float32(ALPHAS[kind]))
            self.x, self.g = draw(seed, False), draw(seed + 1, False)
            y = self.x + self.alpha * self.g
            b = 2 * R * (np.abs(self.x) + np.abs(self.alpha * self.g))        # the product and the sum (one fma: fewer)
            name = "add_scaled alpha=%g" % ALPHAS[kind]
        elif op == "fwd":
            self.x, self.g = draw(seed, True), None
            y, b = act_ref(kind, self.x)
            name = "unary_fwd " + KIND_NAMES[kind]
        else:
            self.x, self.g = draw(seed, True), draw(seed + 1, False)
            if kind == ELU_OUT:                                               # the operand is an ELU's output: never below -1
                self.x = np.where(self.x < 0, rnd(np.expm1(np.minimum(self.x, 0.0)), dt), self.x)
            y, b = bwd_ref(kind, self.x, self.g)
            name = "unary_bwd " + KIND_NAMES[kind]
        self.y32, self.b32 = y, b
        self.ref, self.bound = finish(y, b, dt)
        self.label = "%s %s n=%d%s %s" % (name, dt, n, " +%d" % off if off else "", data)

    def buffer(self, a):
        """values -> the tensor a kernel is handed: [off + n + VE], SENTINEL outside [off, off + n)"""
        buf = np.full(self.off + self.n + self.pad, SENTINEL)
        if a is not None:
            buf[self.off:self.off + self.n] = a
        return store(buf, self.dt)

    def check(self, buf):
        b = f64(buf)
        lo, hi = self.off, self.off + self.n
        rest = np.concatenate([b[:lo], b[hi:]])
        return [Cmp(self.label, b[lo:hi], self.ref, self.bound), Cmp(self.label + " outside", rest, np.full(rest.shape, SENTINEL))]


@functools.lru_cache(maxsize=4)
def unary_case(dt, op, kind, n, off, data):
    return UnaryCase(dt, op, kind, n, off, data)


def unary_kinds(op):
    return range(6) if op == "fwd" else (range(7) if op == "bwd" else range(len(ALPHAS)))


def unary_keys(dt, op):
    return [(dt, op, k, n, off, data) for k in unary_kinds(op) for n, off, data in unary_shapes(dt)]


def unary_cap_keys(op):
    """the caps once each, bf16, the cheapest kind"""
    return [("bf16", op, 1 if op == "add" else RELU, n, off, data) for n, off, data in unary_caps("bf16")]


# ----------------------------------------------------------------------------------------------------------------- backward + column sums
def ubc_nsplit(npix):
    """gelem.hip: >= 128 pixels per split, at most 512 splits"""
    return min(max(-(-npix // 128), 1), 512)


def lanes(cw, dt):
    """pixel lanes of a block of cw channels: 256 threads / (cw / VE) vectors -- 21 for 48 channels in f32, four threads idle"""
    return 256 // (cw // VE[dt])


def ubc_roundings(npix, C, dt, accumulate):
    """per column: a lane adds ceil(per / PL) stored values, min(PL, per) lanes that hold anything are added, a reduce lane adds
    ceil(ns / 16) partials, min(16, ns) reduce lanes that hold anything are added, then the prior value: additions on the longest path
    (the first of each chain starts from an exact zero, so this counts one too many per stage -- an upper bound)"""
    ns = ubc_nsplit(npix)
    per = -(-npix // ns)
    k = np.zeros(C)
    for c0 in range(0, C, 64):
        cw = min(64, C - c0)
        PL = lanes(cw, dt)
        k[c0:c0 + cw] = -(-per // PL) + min(PL, per) + -(-ns // 16) + min(16, ns) + (1 if accumulate else 0)
    return k


UBC_C = (16, 48, 64, 112)
UBC_NPIX = (1, 127, 129, 1025)
UBC_LARGE = 128 * 512 + 1                                 # above the 512-split cap, C = 16 only


def ubc_keys(dt):
    rows, i = [], 0
    for C in UBC_C:
        for npix in UBC_NPIX + ((UBC_LARGE,) if C == 16 else ()):
            for Creal in (C, C - 3):
                for acc in (0, 1):
                    rows.append((dt, i % 7, C, Creal, acc, npix, "grid"))
                    i += 1
    rows += [(dt, k, 64, 64, 0, 1025, "normal") for k in (GELU, TANH)] + [(dt, SIGMOID, 112, 109, 1, 1025, "normal")]
    return rows


class UbcCase:
    """wm_unary_bwd_colsum: gx per element; out[:Creal] (+)= the column sums of gx AS STORED, in float32; out[Creal:] untouched"""

    def __init__(self, dt, kind, C, Creal, acc, npix, data):
        self.dt, self.kind, self.C, self.Creal, self.acc, self.npix, self.data = dt, kind, C, Creal, acc, npix, data
        seed = 7300 + 13 * C + npix % 1000 + 3 * kind + acc
        if data == "grid":
            self.x, self.g = grid((npix, C), seed, 0.125, -2.0, 2.0), grid((npix, C), seed + 1, 0.125, -2.0, 2.0)
        else:
            self.x, self.g = rnd(normal((npix, C), seed, std=1.5), dt), rnd(normal((npix, C), seed + 1), dt)
        sp = np.array([0.0, 20.0, -20.0])
        m = min(npix, 3)
        self.x[:m, 0] = sp[:m]
        self.out0 = np.full(C, SENTINEL)
        if acc:
            self.out0[:Creal] = grid((Creal,), seed + 2, 0.125, -2.0, 2.0)
        self.ref, self.bound = finish(*bwd_ref(kind, self.x, self.g), dt)
        self.k = ubc_roundings(npix, C, dt, acc)
        self.label = "unary_bwd_colsum %s %s C=%d Creal=%d acc=%d npix=%d %s" % (dt, KIND_NAMES[kind], C, Creal, acc, npix, data)

    def check(self, gx, out):
        gx, out = f64(gx).reshape(self.npix, self.C), f64(out)
        cr = self.Creal
        prior = self.out0[:cr] if self.acc else np.zeros(cr)
        sums, absum = gx[:, :cr].sum(0) + prior, np.abs(gx[:, :cr]).sum(0) + np.abs(prior)
        cm = [Cmp(self.label + " gx", gx, self.ref, self.bound),
              Cmp(self.label + " sums of the stored gx", out[:cr], sums, R * self.k[:cr] * absum + TINY32)]
        if cr < self.C:
            cm.append(Cmp(self.label + " out[Creal:]", out[cr:], self.out0[cr:]))
        return cm


@functools.lru_cache(maxsize=4)
def ubc_case(*key):
    return UbcCase(*key)


# ----------------------------------------------------------------------------------------------------------------- QFAttention
QF_B = 2
QF_FWD = tuple((C, ldv, hw) for C in (3, 16, 70) for ldv in (C, C + 16) for hw in (1, 5, 257))
QF_FWD_CAP = (64, 64, 8200)                               # 2 * 8200 * 64 elements: above 4096 * 256
QF_BWD = tuple((C, ldv, hw) for C in (16, 48, 64, 112) for ldv in (C, C + 16) for hw in (1, 5, 1023, 1025)) + \
    tuple((16, ldv, 64 * 1024 + 1) for ldv in (16, 32))   # above the 64-split cap


def qfatt_nsplit(hw):
    return min(max(-(-hw // 1024), 1), 64)


class QfattCase:
    """out[b,p,c] = x + gamma[b,c] * res + beta[b,c]; gres = gamma * g, ggamma[b,c] = sum_p g * res, gbeta[b,c] = sum_p g.  gamma / beta
    [B, ldv] float32 hold SENTINEL in columns [C, ldv): an index that strays there shows"""

    def __init__(self, dt, C, ldv, hw, data="grid"):
        self.dt, self.C, self.ldv, self.hw, self.data, self.B = dt, C, ldv, hw, data, QF_B
        seed = 7500 + 17 * C + ldv + hw % 1000
        shape = (QF_B, hw, C)
        if data == "pattern":
            n = QF_B * hw * C
            self.x, self.res = pattern(n).reshape(shape), pattern(n, 41).reshape(shape)
        elif data == "grid":
            self.x, self.res = grid(shape, seed, 0.125, -2.0, 2.0), grid(shape, seed + 1, 0.125, -2.0, 2.0)
        else:
            self.x, self.res = rnd(normal(shape, seed), dt), rnd(normal(shape, seed + 1), dt)
        self.g = self.x                                                       # the backward's incoming gradient
        gb = np.full((2, QF_B, ldv), SENTINEL)
        if data == "normal":
            gb[:, :, :C] = r32(normal((2, QF_B, C), seed + 2))
        else:
            gb[:, :, :C] = grid((2, QF_B, C), seed + 2, 0.25, -1.0, 1.0)
        self.gamma, self.beta = gb[0], gb[1]
        self.label = "qfatt %s C=%d ldv=%d hw=%d %s" % (dt, C, ldv, hw, data)
        ga, be = self.gamma[:, None, :C], self.beta[:, None, :C]
        # forward: the product, two sums (fused: one fewer): 3 roundings on |x| + |gamma res| + |beta|
        y = self.x + ga * self.res + be
        self.fwd_ref, self.fwd_bound = finish(y, 3 * R * (np.abs(self.x) + np.abs(ga * self.res) + np.abs(be)), dt)
        self.gres_ref, self.gres_bound = finish(r32(ga * self.g), 0.0, dt)    # one product, rounded once
        if C % 16 == 0:
            # a lane adds ceil(per / PL) values, min(PL, per) lanes are added, the ns splits are added in turn; ggamma: + the product
            ns = qfatt_nsplit(hw)
            per = -(-hw // ns)
            k = np.zeros(C)
            for c0 in range(0, C, 64):
                cw = min(64, C - c0)
                k[c0:c0 + cw] = -(-per // lanes(cw, dt)) + min(lanes(cw, dt), per) + ns
            self.gg_ref, self.gb_ref = (self.g * self.res).sum(1), self.g.sum(1)
            self.gg_bound = R * (k + 1) * np.abs(self.g * self.res).sum(1) + TINY32
            self.gb_bound = R * k * np.abs(self.g).sum(1) + TINY32

    def params(self):
        return store(self.gamma, "f32"), store(self.beta, "f32")

    def check_fwd(self, out):
        return [Cmp(self.label + " fwd", f64(out).reshape(self.x.shape), self.fwd_ref, self.fwd_bound)]

    def check_bwd(self, gres, ggamma, gbeta):
        C = self.C
        gg, gb = f64(ggamma), f64(gbeta)
        cm = [Cmp(self.label + " gres", f64(gres).reshape(self.x.shape), self.gres_ref, self.gres_bound),
              Cmp(self.label + " ggamma", gg[:, :C], self.gg_ref, self.gg_bound), Cmp(self.label + " gbeta", gb[:, :C], self.gb_ref, self.gb_bound)]
        if self.ldv > C:
            keep = np.full((QF_B, self.ldv - C), SENTINEL)
            cm += [Cmp(self.label + " ggamma[C:ldv]", gg[:, C:], keep), Cmp(self.label + " gbeta[C:ldv]", gb[:, C:], keep)]
        return cm


@functools.lru_cache(maxsize=4)
def qfatt_case(dt, C, ldv, hw, data="grid"):
    return QfattCase(dt, C, ldv, hw, data)


def qfatt_fwd_keys(dt):
    return [(dt, C, ldv, hw, "grid") for C, ldv, hw in QF_FWD] + [(dt, 70, 86, 257, "normal")]


def qfatt_bwd_keys(dt):
    return [(dt, C, ldv, hw, "grid") for C, ldv, hw in QF_BWD] + [(dt, 112, 128, 1025, "normal")]


# ----------------------------------------------------------------------------------------------------------------- global average pool
GP_B = 2
GP_KEYS = tuple((C, hw) for C in (3, 64, 70) for hw in (1, 3, 4, 5, 1001))


class GpoolCase:
    """out[b,c] = mean_p x[b,p,c]: four lanes add ceil(hw / 4) values each, (l0 + l1) + (l2 + l3), one division: ceil(hw / 4) + 3
    roundings.  gx[b,p,c] = g[b,c] * (1 / hw): the reciprocal and the product, 2 roundings -- none when hw is a power of two"""

    def __init__(self, dt, C, hw, data="grid"):
        self.dt, self.C, self.hw, self.data = dt, C, hw, data
        seed = 7700 + C + hw
        shape = (GP_B, hw, C)
        self.x = grid(shape, seed, 0.125, -2.0, 2.0) if data == "grid" else rnd(normal(shape, seed), dt)
        self.g = grid((GP_B, C), seed + 1, 0.125, -2.0, 2.0) if data == "grid" else r32(normal((GP_B, C), seed + 1))
        self.label = "gpool %s C=%d hw=%d %s" % (dt, C, hw, data)
        self.mean = self.x.sum(1) / hw
        self.mean_bound = R * (-(-hw // 4) + 3) * np.abs(self.x).sum(1) / hw + TINY32
        gx = np.broadcast_to((self.g / hw)[:, None, :], shape)
        pow2 = hw & (hw - 1) == 0
        self.gx_ref, self.gx_bound = finish(gx, 0.0 if pow2 else 2 * R * np.abs(gx), dt)

    def check_fwd(self, out):
        return [Cmp(self.label + " fwd", out, self.mean, self.mean_bound)]

    def check_bwd(self, gx):
        return [Cmp(self.label + " bwd", f64(gx).reshape(self.gx_ref.shape), self.gx_ref, self.gx_bound)]


@functools.lru_cache(maxsize=4)
def gpool_case(dt, C, hw, data="grid"):
    return GpoolCase(dt, C, hw, data)


def gpool_keys(dt):
    return [(dt, C, hw, "grid") for C, hw in GP_KEYS] + [(dt, 70, 1001, "normal")]


# ----------------------------------------------------------------------------------------------------------------- padding, unpack
PAD_SHAPES = (((1, 2, 5, 7), (2, 3, 4, 1)), ((2, 3, 32, 32), (2, 2, 2, 2)), ((1, 3, 3, 4), (5, 6, 7, 4)),     # the last wraps more than once
              ((2, 3, 4, 6), (0, 0, 0, 0)), ((1, 3, 4, 5), (3, 0, 0, 0)), ((1, 3, 4, 5), (0, 0, 0, 2)), ((1, 3, 2, 3), (0, 7, 5, 0)))
PAD_CP = (16, 32)


def pad_index(n, lo, hi, mode):
    """source index of every padded position along one axis.  mode 0, symmetric (symm_pad): the edge sample is repeated, period 2 n:
    ... 1 0 | 0 1 .. n-1 | n-1 n-2 ...; mode 1, replicate (nn.ReplicationPad2d): the edge sample, clamped"""
    t = np.arange(-lo, n + hi)
    if mode == 1:
        return np.clip(t, 0, n - 1)
    t = np.mod(t, 2 * n)
    return np.where(t < n, t, 2 * n - 1 - t)


class PadCase:
    """wm_pad_nchw_to_nhwc: out[b,py,px,c] = x[b,c,iy[py],ix[px]] stored as dt, channels >= C zero -- exact.  Backward: gx[b,c,h,w] = the
    sum of gp over the padded positions whose source is (h, w): cnt terms, cnt - 1 roundings in float32"""

    def __init__(self, dt, shape, pads, mode, CP, data="grid"):
        self.dt, self.shape, self.pads, self.mode, self.CP, self.data = dt, shape, pads, mode, CP, data
        B, C, H, W = shape
        l, r, t, b = pads
        seed = 7900 + H * W + l + 3 * t + mode
        self.x = grid(shape, seed, 0.125, 0.0, 1.0) if data == "grid" else r32(normal(shape, seed))
        self.iy, self.ix = pad_index(H, t, b, mode), pad_index(W, l, r, mode)
        self.PH, self.PW = H + t + b, W + l + r
        out = np.zeros((B, self.PH, self.PW, CP))
        out[..., :C] = self.x[:, :, self.iy][:, :, :, self.ix].transpose(0, 2, 3, 1)
        self.out = rnd(out, dt)
        pshape = (B, self.PH, self.PW, CP)
        self.gp = grid(pshape, seed + 1, 0.125, -2.0, 2.0) if data == "grid" else rnd(normal(pshape, seed + 1), dt)
        gx, ab, cnt = np.zeros(shape), np.zeros(shape), np.zeros((H, W))
        g = self.gp[..., :C].transpose(0, 3, 1, 2)
        for py in range(self.PH):
            for px in range(self.PW):
                gx[:, :, self.iy[py], self.ix[px]] += g[:, :, py, px]
                ab[:, :, self.iy[py], self.ix[px]] += np.abs(g[:, :, py, px])
                cnt[self.iy[py], self.ix[px]] += 1
        self.gx, self.cnt = gx, cnt
        self.gx_bound = R * (cnt - 1)[None, None] * ab
        self.label = "pad %s %s pads=%s mode=%d CP=%d %s" % (dt, "x".join(map(str, shape)), ",".join(map(str, pads)), mode, CP, data)

    def check_fwd(self, out):
        return [Cmp(self.label + " fwd", out, self.out)]

    def check_bwd(self, gx):
        return [Cmp(self.label + " bwd", gx, self.gx, self.gx_bound)]


@functools.lru_cache(maxsize=4)
def pad_case(dt, shape, pads, mode, CP, data="grid"):
    return PadCase(dt, shape, pads, mode, CP, data)


def pad_keys(dt):
    rows = [(dt, s, p, mode, PAD_CP[i % 2], "grid") for i, (s, p) in enumerate(PAD_SHAPES) for mode in (0, 1)]
    rows += [(dt, (1, 3, 3, 4), (5, 6, 7, 4), mode, 32, "grid") for mode in (0, 1)]       # the wrapping pads at the other CP as well
    return rows + [(dt, (1, 3, 3, 4), (5, 6, 7, 4), 0, 16, "normal")]


UNPACK_KEYS = (((2, 3, 4, 7), (6, 9, 16)), ((1, 3, 1, 1), (2, 3, 32)))       # (B, C, H, W), (PH, PW, CP): window < padded tensor, CP > C


class UnpackCase:
    """wm_gunpack_nchw: out[b,c,h,w] = x[b,h,w,c] over the top-left H x W window and the first C channels; its adjoint writes g there
    and exact zeros everywhere else (the destination starts as SENTINEL: nothing may be left unwritten)"""

    def __init__(self, dt, shape, pshape):
        self.dt, self.shape, self.pshape = dt, shape, pshape
        B, C, H, W = shape
        PH, PW, CP = pshape
        self.x = grid((B, PH, PW, CP), 8100 + PH, 0.125, -2.0, 2.0)
        self.g = grid(shape, 8101 + PH, 0.125, -2.0, 2.0)
        self.out = self.x[:, :H, :W, :C].transpose(0, 3, 1, 2)
        self.gx = np.zeros((B, PH, PW, CP))
        self.gx[:, :H, :W, :C] = self.g.transpose(0, 2, 3, 1)
        self.label = "gunpack %s %s of %s" % (dt, "x".join(map(str, shape)), "x".join(map(str, pshape)))

    def check_fwd(self, out):
        return [Cmp(self.label + " fwd", out, self.out)]

    def check_bwd(self, gx):
        return [Cmp(self.label + " bwd", gx, self.gx)]


# ----------------------------------------------------------------------------------------------------------------- spectral norm
SN_SHAPES = ((1, 1), (3, 5), (33, 257), (70, 48), (1030, 8))
SN_EPS = 1e-12
SN_ROWS = 32


class SpectralCase:
    """wm_spectral_norm_fwd on W [M, N] float32:  do_iter: v = W^T u / max(|W^T u|, eps), u = W v / max(|W v|, eps); sigma = u . (W v);
    Wsn = W / sigma.  First-order error propagation, every line the roundings of that stage (paths of the kernels' fixed orders):
      vraw_j: a product, <= 32 additions inside a row slice, RS slices                      k = 1 + min(M, 32) + RS
      |vraw|^2: a square, 6 wave levels, 2 adds over the waves, nb workgroup partials          k = 9 + nb;  sqrt: 1;  v = vraw / norm: 1
      wv_i: a product, ceil(N / 64) additions per lane, 6 wave levels                          k = 7 + ceil(N / 64)
      |wv|^2 and u . wv: a product, ceil(M / 1024) additions per thread, 10 tree levels        k = 11 + ceil(M / 1024)
      Wsn = W * (1 / sigma): the reciprocal and the product                                    k = 2
    Backward, wm_spectral_norm_bwd: gW (+)= (G - d u v^T) / sigma, d = <G, Wsn> over n = M N products: a product, ceil(n / (256 parts))
    additions per thread, 6 wave levels, 2 adds, `parts` partials; then d*u, *v, the difference, 1/sigma, the product: 5; accumulate: 1"""

    def __init__(self, M, N, zero_row=False):
        self.M, self.N, self.zero_row = M, N, zero_row
        seed = 8200 + 7 * M + N
        self.W = r32(normal((M, N), seed, std=0.5))
        u = normal((M,), seed + 1)
        v = normal((N,), seed + 2)
        self.u0, self.v0 = r32(u / np.linalg.norm(u)), r32(v / np.linalg.norm(v))
        if zero_row:
            self.W[0] = 0.0
            self.u0 = np.zeros(M)
            self.u0[0] = 1.0
        self.label = "spectral_norm M=%d N=%d%s" % (M, N, " zero row" if zero_row else "")
        self.fwd = {it: self._fwd(it) for it in (0, 1)}
        # backward operands: independent inputs of the entry
        self.G = r32(normal((M, N), seed + 3))
        self.sigma_in = 1.75
        self.Wsn_in = r32(self.W / self.sigma_in)
        self.gW0 = r32(normal((M, N), seed + 4))
        n = M * N
        parts = min(max(-(-n // 256), 1), 256)
        kd = 1 + -(-n // (256 * parts)) + 8 + parts
        d = float((self.G * self.Wsn_in).sum())
        dd = R * kd * float(np.abs(self.G * self.Wsn_in).sum())
        uv = np.outer(self.u0, self.v0)
        val = (self.G - d * uv) / self.sigma_in
        bval = dd * np.abs(uv) / self.sigma_in + 5 * R * (np.abs(self.G) + np.abs(d * uv)) / self.sigma_in
        self.bwd = {0: (val, bval + TINY32), 1: (self.gW0 + val, bval + R * (np.abs(self.gW0) + np.abs(val)) + TINY32)}

    def _fwd(self, do_iter):
        W, M, N = self.W, self.M, self.N
        aW = np.abs(W)
        if do_iter:
            RS, nb = -(-M // SN_ROWS), -(-N // 256)
            vraw = W.T @ self.u0
            dvraw = R * (1 + min(M, SN_ROWS) + RS) * (aW.T @ np.abs(self.u0))
            t = float(vraw @ vraw)
            nv = max(math.sqrt(t), SN_EPS)
            dnv = (float(2 * np.abs(vraw) @ dvraw) + R * (9 + nb) * t) / (2 * nv) + R * nv
            v = vraw / nv
            dv = dvraw / nv + np.abs(v) * dnv / nv + R * np.abs(v)
        else:
            v, dv = self.v0, np.zeros(N)
        wv = W @ v
        dwv = aW @ dv + R * (7 + -(-N // 64)) * (aW @ np.abs(v))
        ks = 11 + -(-M // 1024)
        if do_iter:
            t = float(wv @ wv)
            un = max(math.sqrt(t), SN_EPS)
            dun = (float(2 * np.abs(wv) @ dwv) + R * ks * t) / (2 * un) + R * un
            u = wv / un
            du = dwv / un + np.abs(u) * dun / un + R * np.abs(u)
        else:
            u, du = self.u0, np.zeros(M)
        sigma = float(u @ wv)
        dsigma = float(np.abs(wv) @ du + np.abs(u) @ dwv) + R * ks * float(np.abs(u * wv).sum())
        out = {"u": (u, du + (TINY32 if do_iter else 0.0)), "v": (v, dv + (TINY32 if do_iter else 0.0)), "sigma": (np.array([sigma]), np.array([dsigma + TINY32]))}
        if not self.zero_row:
            wsn = W / sigma
            out["Wsn"] = (wsn, aW * dsigma / sigma ** 2 + 2 * R * np.abs(wsn) + TINY32)
        return out

    def check_fwd(self, do_iter, u, v, sigma, Wsn):
        got = {"u": u, "v": v, "sigma": sigma, "Wsn": Wsn}
        ref = self.fwd[do_iter]
        if self.zero_row:       # v = 0 / eps, wv = 0, u = 0 / eps, sigma = 0: exact; Wsn is not finite in the reference either
            return [Cmp("%s it=%d %s" % (self.label, do_iter, k), f64(got[k]).reshape(-1), np.zeros(ref[k][0].size)) for k in ("u", "v", "sigma")]
        return [Cmp("%s it=%d %s" % (self.label, do_iter, k), f64(got[k]).reshape(ref[k][0].shape), ref[k][0], ref[k][1]) for k in ref]

    def check_bwd(self, acc, gW):
        return [Cmp("%s bwd acc=%d" % (self.label, acc), f64(gW).reshape(self.M, self.N), *self.bwd[acc])]


@functools.lru_cache(maxsize=8)
def spectral_case(M, N, zero_row=False):
    return SpectralCase(M, N, zero_row)


# ----------------------------------------------------------------------------------------------------------------- Haar
HAAR_SIGN = np.array([[[1, 1], [1, 1]], [[1, -1], [1, -1]], [[1, 1], [-1, -1]], [[1, -1], [-1, 1]]], dtype=np.float64)   # [k][dy][dx]
HAAR_C = (1, 3, 12)
HAAR_HW = ((1, 1), (3, 5))
HAAR_B = 2
HAAR_CAP = (1, 260, 256, 32, 32, 128)                     # B, H, W, C, CPin, CPout: 260*256*32 threads' worth, above 8192 * 256


def up16(c):
    return -(-c // 16) * 16


class HaarCase:
    """wm_haar.  Analysis (up bit 0 clear): in [B,2H,2W,CPin] -> out [B,H,W,CPout], wavelet k of channel c = fac * sum_(dy,dx)
    HAAR_SIGN[k,dy,dx] * in(2y+dy, 2x+dx, c) at channel 4c + k, or k C + c when bit 1 is set (order_by_wavelet); every other channel of
    out zero.  Synthesis: out(2y+dy, 2x+dx, c) = fac * sum_k HAAR_SIGN[k,dy,dx] * in(y, x, channel of (c, k)); channels >= C zero.
    Three additions and the product: 4 roundings; with fac = 0.5 on multiples of 1/8 in [-2, 2] every step is exact in every dtype."""

    def __init__(self, dt, up, C, H, W, fac, B=HAAR_B, CPin=None, CPout=None, data=None):
        self.dt, self.up, self.C, self.H, self.W, self.B = dt, up, C, H, W, B
        self.fac = float(np.float32(fac))
        synth, bywav = up & 1, (up >> 1) & 1
        self.CPin = CPin or (up16(4 * C) + 16 if synth else up16(C))
        self.CPout = CPout or (up16(C) + (16 if C > 1 else 0) if synth else up16(4 * C) + 16)      # padding groups beyond the real channels
        exact = self.fac == 0.5
        data = data or ("grid" if exact else "normal")
        seed = 8400 + 5 * C + H + W + up
        ishape = (B, H, W, self.CPin) if synth else (B, 2 * H, 2 * W, self.CPin)
        if data == "pattern":
            self.x = pattern(int(np.prod(ishape))).reshape(ishape)
        else:
            self.x = grid(ishape, seed, 0.125, -2.0, 2.0) if data == "grid" else rnd(normal(ishape, seed), dt)
        chan = (np.arange(4)[None, :] * C + np.arange(C)[:, None]) if bywav else (4 * np.arange(C)[:, None] + np.arange(4)[None, :])   # [c][k]
        self.chan = chan
        if synth:
            v = self.x[..., chan]                                             # [B,H,W,C,4]
            o = np.einsum("bhwck,kyx->bhywxc", v, HAAR_SIGN).reshape(B, 2 * H, 2 * W, C) * self.fac
            a = np.einsum("bhwck,kyx->bhywxc", np.abs(v), np.abs(HAAR_SIGN)).reshape(B, 2 * H, 2 * W, C) * self.fac
            ref, ab = np.zeros((B, 2 * H, 2 * W, self.CPout)), np.zeros((B, 2 * H, 2 * W, self.CPout))
            ref[..., :C], ab[..., :C] = o, a
        else:
            v = self.x[..., :C].reshape(B, H, 2, W, 2, C)
            o = np.einsum("bhywxc,kyx->bhwck", v, HAAR_SIGN) * self.fac       # [B,H,W,C,4]
            a = np.einsum("bhywxc,kyx->bhwck", np.abs(v), np.abs(HAAR_SIGN)) * self.fac
            ref, ab = np.zeros((B, H, W, self.CPout)), np.zeros((B, H, W, self.CPout))
            ref[..., chan], ab[..., chan] = o, a
        self.raw = ref
        self.ref, self.bound = finish(ref, 0.0 if exact and data != "normal" else np.where(ab > 0, 4 * R * ab, 0.0), dt)
        self.label = "haar %s up=%d C=%d %dx%dx%d CP %d->%d fac=%g %s" % (dt, up, C, B, H, W, self.CPin, self.CPout, fac, data)

    def check(self, out):
        return [Cmp(self.label, out, self.ref, self.bound)]


@functools.lru_cache(maxsize=4)
def haar_case(dt, up, C, H, W, fac):
    return HaarCase(dt, up, C, H, W, fac)


def haar_keys(dt):
    return [(dt, up, C, H, W, fac) for up in range(4) for C in HAAR_C for H, W in HAAR_HW for fac in (0.5, 0.35)]


# ----------------------------------------------------------------------------------------------------------------- channel copy / place
CHAN_NPIX = 37
COPY_KEYS = ((48, 0, 32, 0, 5), (48, 17, 32, 9, 11), (48, 35, 32, 19, 13), (16, 0, 16, 0, 16))   # sstride, soff, dstride, doff, n


class ChanCopyCase:
    """wm_chan_copy: dst[p][doff + c] = src[p][soff + c], c < n; every other channel of dst keeps its SENTINEL"""

    def __init__(self, dt, sstride, soff, dstride, doff, n):
        self.dt, self.key = dt, (sstride, soff, dstride, doff, n)
        self.src = grid((CHAN_NPIX, sstride), 8600 + soff, 0.125, -2.0, 2.0)
        self.ref = np.full((CHAN_NPIX, dstride), SENTINEL)
        self.ref[:, doff:doff + n] = self.src[:, soff:soff + n]
        self.label = "chan_copy %s %d[%d:+%d] -> %d[%d:]" % (dt, sstride, soff, n, dstride, doff)

    def check(self, dst):
        return [Cmp(self.label, f64(dst).reshape(self.ref.shape), self.ref)]


# astride, aoff, adst, na, bstride, boff, bdst, nb, dstride (bstride 0: no b)
PLACE_KEYS = ((32, 8, 16, 16, 0, 0, 0, 0, 48), (32, 8, 16, 8, 16, 0, 32, 16, 48), (32, 0, 24, 8, 16, 8, 0, 8, 48),      # vector form
              (32, 3, 5, 7, 0, 0, 0, 0, 32), (32, 3, 20, 7, 16, 2, 1, 9, 32), (16, 1, 0, 3, 32, 4, 3, 12, 16))          # scalar form


class ChanPlaceCase:
    """wm_chan_place: dst [npix][dstride] written whole: a's window at adst, b's at bdst, zero elsewhere (dst starts as SENTINEL)"""

    def __init__(self, dt, key):
        self.dt, self.key = dt, key
        astride, aoff, adst, na, bstride, boff, bdst, nb, dstride = key
        self.vector = all(v % VE[dt] == 0 for v in key)
        self.a = grid((CHAN_NPIX, astride), 8700 + aoff, 0.125, -2.0, 2.0)
        self.b = grid((CHAN_NPIX, bstride), 8701 + boff, 0.125, -2.0, 2.0) if bstride else None
        self.ref = np.zeros((CHAN_NPIX, dstride))
        self.ref[:, adst:adst + na] = self.a[:, aoff:aoff + na]
        if bstride:
            self.ref[:, bdst:bdst + nb] = self.b[:, boff:boff + nb]
        self.label = "chan_place %s %s %s" % (dt, "vector" if self.vector else "scalar", key)

    def check(self, dst):
        return [Cmp(self.label, f64(dst).reshape(self.ref.shape), self.ref)]


# ----------------------------------------------------------------------------------------------------------------- affine coupling
CP_EPS = 1e-4                                             # RNVPCouplingBlock.affine_eps and clamp = 1.0, as models/invertible_net.py passes them
CP_CLAMP = 1.0
CP_N = (1, 257)
CP_CAP = 8192 * 256 + 3


class CouplingCase:
    """e(s) = exp(clamp * (2 / (1 + exp(-s)) - 1)) + eps.  Error of e, stage by stage:
      q = 2 sigmoid(s): exp's U ulp through -q*q/2, the sum and the division: 2 roundings;  m = q - 1: 1 rounding on q + 1
      a = clamp * m: |clamp| dm + 1 rounding (none of it when clamp = 0: a = 0 and e = fl(1 + eps));  ex = exp(a): ex * da + U ulp
      e = ex + eps: 1 rounding
    forward  rev 0: y = e x + t: |x| de + 2 roundings on |e x| + |t|;  rev 1: y = (x - t) / e: |y| de / e + 2 roundings on (|x| + |t|) / e
    backward de/ds = ex * clamp * 2 * sg * (1 - sg): ex's error, sg's through (1 - 2 sg), 1 - sg: 1 rounding on 1 + sg (absolute near
      saturation), three products;  rev 0: gx = e g, gt = g, gs = g v de;  rev 1: ge = g / e, gx = ge, gt = -ge, gs = -ge v de (v = y)"""

    def __init__(self, dt, n, rev, clamp, data="normal"):
        self.dt, self.n, self.rev, self.data = dt, n, rev, data
        self.clamp, self.eps = float(np.float32(clamp)), float(np.float32(CP_EPS))
        seed = 8800 + n % 1000 + rev
        if data == "pattern":
            self.x, self.s, self.t, self.g = pattern(n), pattern(n, 41), pattern(n, 43), pattern(n, 47)
        else:
            self.x, self.t, self.g = (rnd(normal((n,), seed + i), dt) for i in range(3))
            self.s = grid((n,), seed + 3, 0.125, -2.0, 2.0)
            sp = np.array([0.0, 20.0, -20.0])
            m = min(n, 3)
            self.s[:m] = sp[:m]
            if n > 8:
                self.s[8::2] = rnd(normal((len(self.s[8::2]),), seed + 4, std=2.0), dt)
        s, c = self.s, self.clamp
        sg, dsg = sigmoid_ref(s)
        q, dq = 2 * sg, 2 * dsg
        mm = q - 1.0
        dm = dq + R * (q + 1.0)
        a = c * mm
        da = (abs(c) * dm + R * np.abs(a)) if c != 0 else np.zeros(n)
        ex = np.exp(a)
        dex = ex * da + U["exp"] * ulp32(ex)
        e = ex + self.eps
        de = dex + R * (ex + self.eps)
        x, t, g = self.x, self.t, self.g
        if rev:
            y = (x - t) / e
            by = np.abs(y) * de / e + 2 * R * (np.abs(x) + np.abs(t)) / e
        else:
            y = e * x + t
            by = np.abs(x) * de + 2 * R * (np.abs(e * x) + np.abs(t))
        self.y = finish(y, by, dt)
        self.v = rnd(y, dt) if rev else x                                     # the backward reads the stored output for rev 1
        v = self.v
        der = ex * c * 2 * sg * (1 - sg)
        dder = np.abs(c * 2 * sg * (1 - sg)) * dex + np.abs(ex * c * 2) * (dsg * np.abs(1 - 2 * sg) + sg * R * (1 + sg)) + 3 * R * np.abs(der)
        if rev:
            ge = g / e
            dge = np.abs(ge) * de / e + R * np.abs(ge)
            gs = -ge * v * der
            self.gx, self.gt = finish(ge, dge, dt), finish(-ge, dge, dt)
            self.gs = finish(gs, np.abs(v * der) * dge + np.abs(ge * v) * dder + 2 * R * np.abs(gs), dt)
        else:
            gs = g * v * der
            self.gx = finish(e * g, np.abs(g) * de + R * np.abs(e * g), dt)
            self.gt = finish(g, 0.0, dt)
            self.gs = finish(gs, np.abs(g * v) * dder + 2 * R * np.abs(gs), dt)
        self.label = "coupling %s n=%d rev=%d clamp=%g %s" % (dt, n, rev, clamp, data)

    def check_fwd(self, y):
        return [Cmp(self.label + " y", f64(y).reshape(-1), *self.y)]

    def check_bwd(self, gx, gs, gt):
        return [Cmp(self.label + " " + k, f64(got).reshape(-1), *ref) for k, got, ref in (("gx", gx, self.gx), ("gs", gs, self.gs), ("gt", gt, self.gt))]


@functools.lru_cache(maxsize=4)
def coupling_case(dt, n, rev, clamp, data="normal"):
    return CouplingCase(dt, n, rev, clamp, data)


def coupling_keys(dt):
    return [(dt, n, rev, clamp, "normal") for n in CP_N for rev in (0, 1) for clamp in (CP_CLAMP, 0.0)]


# ----------------------------------------------------------------------------------------------------------------- observed ulps
def observed_ulps(case, got):
    """largest error of a UnaryCase result in float32 ulps of the reference, net of the storage type's half ulp: for ELU forward (x <= 0)
    that is expm1's error, for tanh forward tanh's, for the ELU backward exp's plus the product's rounding; GELU forward: the error over
    |0.5 x| in ulps of erf(a) where |erf(a)| >= 0.5 -- erf's error plus the expression's three roundings"""
    g = f64(got)[case.off:case.off + case.n]
    err = np.maximum(np.abs(g - case.y32) - half_ulp(case.y32, case.dt), 0.0)
    inexact = case.b32 > 0
    if case.op == "fwd" and case.kind == GELU:
        a = case.x / math.sqrt(2.0)
        ok = inexact & (np.abs(erf64(a)) >= 0.5) & (np.abs(case.x) < 1e30)       # where erf's ulp is 2**-24, the size of the roundings beside it
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(ok, err / (np.abs(0.5 * case.x) * ulp32(erf64(a))), 0.0)
    else:
        r = np.where(inexact & np.isfinite(err), err / ulp32(case.y32), 0.0)
    return float(r.max()) if r.size else 0.0
