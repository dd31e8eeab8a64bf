"""Float64 restatements of the scalar-loss and step-glue kernels: csrc/losses.hip (nn.SmoothL1Loss, nn.BCELoss, nn.CrossEntropyLoss,
torch.clamp(x, 0, 1), the PSNR of postprocess()ed images), csrc/localise.hip (the tamper splice, its PSNR gate, the gated MSE,
nn.BCEWithLogitsLoss against a tensor, a += g (1 - mask), p > threshold, x *= s) and the loss half of csrc/optim.hip (nn.MSELoss forward
and backward, its fusion with the discriminator's image gradient, nn.BCEWithLogitsLoss against a constant, the decoder's message loss
with torch.round / clip, the seven logged scalars, the sum of squares, a += s b, the inf / nan flags), written from include/wm_hip.h, the
kernels' comments and the torch definitions they cite, with the case tables and the per-element comparisons built on them.  A plain helper
module (CPU only, never imports the HIP package): tests/test_cpu_steploss_exact.py runs float32 imitations -- faithful and defective --
through these comparisons, tests/test_gpu_steploss_exact.py runs the kernels through them.

Bounds follow the rule of tests/layers_exact.py and tests/gelem_exact.py: a float32 result formed with k roundings from exact inputs is
accepted within FACTOR * k * 2**-24 * (the sum of the absolute values of its terms) + TINY32; k stands next to each formula.  A sum is
charged its longest path, not its term count: path(n, nparts) = the sequential additions of one thread, ceil(n / (256 nparts)), + 6 wave
levels + 3 for the four wave totals (added in turn: 3; paired, as losses.hip does: 2 -- the larger count covers both).  The partials are
then summed in double, which is exact next to float32.  logf, log1pf and expf take gelem_exact.U ulps of their float32 result (OpenCL
full profile: log 3, log1p 2, exp 3), propagated through each expression's conditioning.  Division and sqrtf are correctly rounded: one
rounding each.  Where float32 has no value for a result -- exp(-x) beyond the largest float32 makes 1 / (1 + exp(-x)), which is below
2**-128, come out as 0 -- the smallest normal, 2**-126, is charged (sigmoid_b); a float64 result beyond the largest float32 is expected as +-inf.

Exact, with no tolerance: every copy, select and threshold (clamp01 forward and backward, mask_threshold, nonfinite, the clamp's gating),
every gradient that is a chain of single correctly rounded float32 operations which nothing can contract (float64 holds the exact sum or
product of two float32 values, so rounding it once IS the float32 result: d = fl(a - b), fl(G d), fl(g + fl(G d)), +-fl(1 / n),
fl(x f)), clamp_quant (product, rint, division), the PSNR partial sums (sums of squared integer differences, in double: their total equals the
integer numpy computes from np.float32 products, the arithmetic postprocess() itself uses), message_loss' bit error
(an integer count over n: one division), hidden_metrics' six pass-throughs, and SENTINEL in every value around a destination.
Exact comparisons take -0.0 for 0.0 and a nan for a nan, nothing else.

torch.clamp(nan, 0, 1) is nan (ATen's clamp propagates nan; its backward mask (x >= 0) & (x <= 1) is false there, so the gradient is 0):
clamp01_fwd must return nan for nan, clamp01_bwd 0.

No comparison leaves an element out: every branch a case takes is decided by an input value or by a reproducible single float32
operation on inputs (fl(a - b) against beta), never by a computed result that could legitimately differ.
"""
import functools

import numpy as np

import detgen
from gelem_exact import F32_MAX, TINY32, U, pattern, r32, sigmoid_ref, ulp32
from layers_exact import EPS32, FACTOR, SENTINEL, TORCH, Cmp, f64, grid, normal, pick, rnd, store  # noqa: F401  (re-exported to the two test files)

R = FACTOR * EPS32                                        # one counted rounding, relative
INF = float("inf")
NAN = float("nan")
MIN_NORMAL32 = 2.0 ** -126
FLAT_N = (1, 63, 64, 65, 255, 257, 4096, 4097, 2 * 4096 + 513)
FREE_NPARTS = (1, 3, 2048)                                # at n = 4097, through the C entry
MSE_LARGE = 4096 * 1024 + 4097                            # above the wrappers' 1024-partial cap
ONE_WG_N = (1, 64, 255, 256, 257, 1000)
CAP_CLAMP, CAP_ELEM, CAP_SPLICE = 8192 * 256, 2048 * 256, 1024 * 256
SMALL_N = (1, 63, 64, 65, 255, 257)


class ECmp(Cmp):
    """layers_exact.Cmp that names the first offending element, takes nan for nan and inf for inf (got == ref), and leaves nothing out"""

    def __init__(self, what, got, ref, bound=0.0):
        got, ref = f64(got), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            same = (got == ref) | (np.isnan(got) & np.isnan(ref))
            err = np.where(same, 0.0, np.abs(got - ref))
            err = np.where(np.isnan(err), INF, err)
            bad = ~(same | (err <= bound))
            ratio = np.where(err == 0, 0.0, err / bound)
        self.what, self.n, self.nbad, self.skipped = what, ref.size, int(bad.sum()), 0
        self.err = float(err.max()) if err.size else 0.0
        self.bound = float(bound.max()) if bound.size else 0.0
        self.worst = float(ratio.max()) if ratio.size else 0.0
        self.exact = not bool(bound.any())
        self.first = ""
        if self.nbad:
            i = np.unravel_index(int(np.argmax(bad)), bad.shape)
            self.first = "  first at element %s: got %r, expected %r (bound %.3e)" % (list(map(int, i)), float(got[i]), float(ref[i]), float(bound[i]))

    def line(self):
        return Cmp.line(self) + self.first


def all_ok(cmps):
    return all(c.ok for c in cmps)


def path(n, nparts, per=1):
    """roundings on the longest path of a float32 sum of n terms over nparts workgroups of 256 threads (per: terms a thread adds per trip)"""
    return -(-n // (256 * nparts)) * per + 6 + 3


def wrapper_nparts(n):
    """ops.*: one partial per 4096 elements, at most 1024"""
    return max(1, min(1024, -(-n // 4096)))


def uni(shape, seed, lo=0.0, hi=1.0):
    return detgen.uniform(shape, seed, lo, hi).double().numpy()


def data32(shape, seed, std=1.0):
    return r32(normal(shape, seed, std=std))


def nxt(v, up):
    return float(np.nextafter(np.float32(v), np.float32(INF if up else -INF)))


def around(v):
    """v as float32 and its two float32 neighbours"""
    v = float(np.float32(v))
    return [nxt(v, False), v, nxt(v, True)]


def put(a, vals, at=0):
    """hand-placed values (rounded to float32) at the start (or at `at`) of a flat array, as many as fit"""
    v = r32(np.asarray(vals, dtype=np.float64))
    m = max(0, min(a.size - at, v.size))
    a[at:at + m] = v[:m]
    return a


def fl(v):
    """a float64 scalar rounded once to float32 (to nearest even)"""
    return float(np.float32(v))


def overflow32(y):
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(y) > F32_MAX, np.sign(y) * INF, y)


def sigmoid_b(x):
    """gelem_exact.sigmoid_ref, and where exp(-x) exceeds float32 (x < -88.7) the quotient, below 2**-128, has no normal float32: it
    evaluates to 0 (1 / inf) or to any subnormal: charged 2**-126, the smallest normal"""
    s, ds = sigmoid_ref(x)
    with np.errstate(over="ignore"):
        return s, ds + np.where(np.exp(-x) > F32_MAX, MIN_NORMAL32, 0.0)


def gscale_of(gscale, gdev):
    """the scale a kernel multiplies by: float32(gscale), times the device scalar when given -- one product, rounded once"""
    g = float(np.float32(gscale))
    return g if gdev is None else fl(g * float(np.float32(gdev)))


# ----------------------------------------------------------------------------------------------------------------- SmoothL1
class SmoothL1Case:
    """nn.SmoothL1Loss(beta): l = 0.5 d^2 / beta if |d| < beta else |d| - 0.5 beta, d = a - b; mean; grad = dl/da / n.
    d = fl(a - b) is one rounding and reproducible; 0.5 d exact, (0.5 d) d, / beta: k = 2; |d| - 0.5 beta: k = 1.
    grad: d / beta, 1 / n, their product: k = 3; beyond beta +-fl(1 / n): exact.  `edge`: b = 0 and a = +-beta and its neighbours."""

    def __init__(self, n, beta=1.0, edge=False):
        self.n, self.beta = n, float(np.float32(beta))
        self.a, self.b = data32((n,), 9000 + n, 1.5), data32((n,), 9001 + n)
        if edge:
            e = around(self.beta) + [-v for v in around(self.beta)]
            self.b[:len(e)] = 0.0
            put(self.a, e)
        self.label = "smooth_l1 n=%d beta=%g%s" % (n, beta, " edge" if edge else "")
        d = r32(self.a - self.b)
        ad, be = np.abs(d), self.beta
        self.quad = quad = ad < be
        self.t = np.where(quad, 0.5 * d * d / be, ad - 0.5 * be)
        self.bt = np.where(quad, 2 * R * np.abs(self.t), R * (ad + 0.5 * be))
        self.loss = self.t.sum() / n
        inv = fl(1.0 / n)
        self.grad = np.where(quad, d / be / n, np.where(d > 0, inv, -inv))
        self.bgrad = np.where(quad, 3 * R * np.abs(self.grad) + TINY32, 0.0)

    def check(self, loss, grad, nparts=None):
        nparts = nparts or wrapper_nparts(self.n)
        bl = (self.bt.sum() + R * path(self.n, nparts) * np.abs(self.t).sum()) / self.n + R * abs(self.loss) + TINY32    # + the cast
        lab = "%s nparts=%d" % (self.label, nparts)
        return [ECmp(lab + " loss", f64(loss).reshape(1), [self.loss], [bl]), ECmp(lab + " grad", f64(grad).reshape(-1), self.grad, self.bgrad)]


@functools.lru_cache(maxsize=8)
def smooth_l1_case(n, beta=1.0, edge=False):
    return SmoothL1Case(n, beta, edge)


SMOOTH_L1_KEYS = tuple((n, 1.0, False) for n in FLAT_N) + tuple((n, beta, True) for n in (8, 257) for beta in (1.0, 0.25))


# ----------------------------------------------------------------------------------------------------------------- BCELoss on probabilities
LOG_CLAMP = -100.0
BCE_DEN = float(np.float32(1e-12))
BCE_EDGE_P = (0.0, 1.0, 1e-45, 1.0 - 2.0 ** -24)


class BceProbCase:
    """nn.BCELoss()(p, full(target)): l = -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)); grad = (p - t) / max((1 - p) p, 1e-12) / n.
    log p: U log ulps; q = fl(1 - p): 1 rounding, which log passes on as R (absolute); the two products, 1 - t and the sum: k = 4 (exact for
    t in {0, 1}).  A logarithm at or below the clamp is -100 exactly.  grad: p - t, 1 - p, their product with p, the division, 1 / n, the
    product: k = 6, all relative (products and quotients only)."""

    def __init__(self, n, target, edge=False):
        self.n, self.target = n, float(target)
        self.p = r32(uni((n,), 9100 + n, 0.01, 0.99))
        if edge:
            put(self.p, r32(np.array(BCE_EDGE_P)))
        self.label = "bce_prob n=%d target=%g%s" % (n, target, " edge" if edge else "")
        p, t = self.p, self.target
        with np.errstate(divide="ignore"):
            lp, lq = np.log(p), np.log(1.0 - p)
        cp, cq = lp <= LOG_CLAMP, lq <= LOG_CLAMP
        blp = np.where(cp, 0.0, U["log"] * ulp32(np.maximum(lp, LOG_CLAMP)))
        blq = np.where(cq, 0.0, U["log"] * ulp32(np.maximum(lq, LOG_CLAMP)) + R)
        lp, lq = np.maximum(lp, LOG_CLAMP), np.maximum(lq, LOG_CLAMP)
        self.t = -(t * lp + (1.0 - t) * lq)
        self.at = np.abs(t * lp) + np.abs((1.0 - t) * lq)
        self.bt = abs(t) * blp + abs(1.0 - t) * blq + (0.0 if t in (0.0, 1.0) else 4 * R * self.at)
        self.loss = self.t.sum() / n
        self.grad = (p - t) / np.maximum((1.0 - p) * p, BCE_DEN) / n
        self.bgrad = 6 * R * np.abs(self.grad) + TINY32

    def check(self, loss, grad, nparts=None):
        nparts = nparts or wrapper_nparts(self.n)
        bl = (self.bt.sum() + R * path(self.n, nparts) * self.at.sum()) / self.n + R * abs(self.loss) + TINY32
        lab = "%s nparts=%d" % (self.label, nparts)
        return [ECmp(lab + " loss", f64(loss).reshape(1), [self.loss], [bl]), ECmp(lab + " grad", f64(grad).reshape(-1), self.grad, self.bgrad)]


@functools.lru_cache(maxsize=8)
def bce_prob_case(n, target, edge=False):
    return BceProbCase(n, target, edge)


BCE_PROB_KEYS = tuple((n, t, False) for n in FLAT_N for t in (0.0, 1.0)) + tuple((n, t, True) for n in (4, 257) for t in (0.0, 1.0))


# ----------------------------------------------------------------------------------------------------------------- CrossEntropyLoss
CE_B, CE_K, CE_PAD = (1, 255, 257, 600), (1, 2, 6, 33), 3


class CrossEntropyCase:
    """nn.CrossEntropyLoss()(z [B, K], y): mean_r (lse_r - z[r, y_r]); grad = (softmax - onehot) / B.  Row by row, m = max z (exact):
      e_k = exp(z_k - m): the difference's rounding through exp, + U exp ulps;  se = sum e_k: K - 1 roundings
      L = log se: dse / se + U log ulps;  lse = m + L: 1;  row = lse - z_y: 1;  the mean is formed in double and cast: 1
      grad: x = z_k - lse: dlse + 1;  p = exp x: p dx + U exp ulps;  p - 1 at the label: 1 on p + 1;  1 / B and the product: 2"""

    def __init__(self, B, K, ld=None):
        self.B, self.K, self.ld = B, K, ld or K
        self.z = data32((B, K), 9200 + 7 * B + K, 3.0)
        self.y = np.minimum(np.floor(uni((B,), 9201 + B + K) * K), K - 1).astype(np.int64)
        self.label = "cross_entropy B=%d K=%d ld=%d" % (B, K, self.ld)
        z, rows = self.z, np.arange(B)
        m = z.max(1, keepdims=True)
        x = z - m
        e = np.exp(x)
        de = e * R * np.abs(x) + U["exp"] * ulp32(e)
        se = e.sum(1, keepdims=True)
        dse = de.sum(1, keepdims=True) + R * (K - 1) * se
        L = np.log(se)
        dL = dse / se + U["log"] * ulp32(L)
        lse = m + L
        dlse = dL + R * (np.abs(m) + np.abs(L))
        zy = z[rows, self.y][:, None]
        row = lse - zy
        drow = dlse + R * (np.abs(lse) + np.abs(zy))
        self.loss = float(row.mean())
        self.bloss = float(drow.mean()) + R * abs(self.loss) + TINY32
        xx = z - lse
        dx = dlse + R * (np.abs(z) + np.abs(lse))
        p = np.exp(xx)
        dp = p * dx + U["exp"] * ulp32(p)
        hot = np.zeros((B, K))
        hot[rows, self.y] = 1.0
        self.grad = (p - hot) / B
        self.bgrad = (dp + hot * R * (p + 1.0)) / B + 2 * R * np.abs(self.grad) + TINY32

    def logits(self):
        buf = np.full((self.B, self.ld), SENTINEL)
        buf[:, :self.K] = self.z
        return store(buf, "f32")

    def check(self, loss, grad):
        g = f64(grad).reshape(self.B, self.ld)
        cm = [ECmp(self.label + " loss", f64(loss).reshape(1), [self.loss], [self.bloss]), ECmp(self.label + " grad", g[:, :self.K], self.grad, self.bgrad)]
        if self.ld > self.K:
            cm.append(ECmp(self.label + " grad columns K..ld-1", g[:, self.K:], np.full((self.B, self.ld - self.K), SENTINEL)))
        return cm


@functools.lru_cache(maxsize=8)
def cross_entropy_case(B, K, ld=None):
    return CrossEntropyCase(B, K, ld)


CE_KEYS = tuple((B, K) for B in CE_B for K in CE_K)


# ----------------------------------------------------------------------------------------------------------------- clamp(x, 0, 1)
CLAMP_EDGE = (-0.0, 0.0, 1.0, 1.0 + 2.0 ** -23, -2.0 ** -149, INF, -INF, NAN)


class Clamp01Case:
    """torch.clamp(x, 0, 1) and its backward g * [0 <= x <= 1]: selections, exact; nan -> nan forward, 0 backward (module docstring)"""

    def __init__(self, n, data="normal"):
        self.n = n
        if data == "pattern":
            self.x, self.g = pattern(n), pattern(n, 41)
        else:
            self.x, self.g = data32((n,), 9300 + n), data32((n,), 9301 + n)
            put(self.x, CLAMP_EDGE)
        self.label = "clamp01 n=%d %s" % (n, data)
        x = self.x
        with np.errstate(invalid="ignore"):
            self.fwd = np.where(np.isnan(x), NAN, np.minimum(np.maximum(x, 0.0), 1.0))
            self.bwd = np.where((x >= 0.0) & (x <= 1.0), self.g, 0.0)

    def check_fwd(self, y):
        return [ECmp(self.label + " fwd", f64(y).reshape(-1), self.fwd)]

    def check_bwd(self, gx):
        return [ECmp(self.label + " bwd", f64(gx).reshape(-1), self.bwd)]


@functools.lru_cache(maxsize=4)
def clamp01_case(n, data="normal"):
    return Clamp01Case(n, data)


CLAMP_KEYS = tuple((n, "normal") for n in SMALL_N + (4097,)) + ((CAP_CLAMP + 3, "pattern"),)


# ----------------------------------------------------------------------------------------------------------------- PSNR of 8-bit images
def trunc255(x, clamp):
    """(x * 255).int() as postprocess() forms it: the float32 product, truncated; clamp: x clamped to [0, 1] first"""
    v = np.asarray(x, dtype=np.float64).astype(np.float32)
    if clamp:
        v = np.minimum(np.maximum(v, np.float32(0)), np.float32(1))
    return np.trunc(v * np.float32(255.0)).astype(np.int64)


def seam_values():
    """k / 255 as float32 and its neighbours, for k where the product with 255 lands on, above and below the integer; below 0, above 1"""
    out = []
    for k in (1, 3, 7, 13, 85, 127, 128, 200, 254, 255):
        out += around(np.float32(k) / np.float32(255))
    return np.array(out + [-0.25, -2.0 ** -149, 1.0 + 2.0 ** -23, 1.5, 0.0, 1.0])


def tie_values(count=6):
    """float32 x whose float32 product with 255 is exactly k + 0.5, k even and odd: where round half to even and half away part"""
    out = []
    for k in range(0, 255):
        x = np.float32(k + 0.5) / np.float32(255)
        if float(x * np.float32(255)) == k + 0.5:
            out.append(float(x))
    return np.array(out[:count] + out[-count:])


class Psnr255Case:
    """wm_psnr255_partials: partial sums of (int(255 a) - int(255 b))^2, a and b clamped to [0, 1]: integers in double, the total exact"""

    def __init__(self, n):
        self.n = n
        self.a, self.b = r32(uni((n,), 9400 + n, -0.1, 1.1)), r32(uni((n,), 9401 + n, -0.1, 1.1))
        sv = seam_values()
        put(self.a, sv)
        put(self.b, sv[::-1])
        put(self.a, sv, at=n - len(sv) if n > 2 * len(sv) else n)            # and in the last trip
        self.label = "psnr255 n=%d" % n
        d = trunc255(self.a, True) - trunc255(self.b, True)
        self.total = int((d * d).sum())

    def check(self, partials, nparts=None):
        pv = f64(partials).reshape(-1)
        return [ECmp("%s nparts=%d total" % (self.label, pv.size), [pv.sum()], [float(self.total)]),
                ECmp("%s nparts=%d integer partials" % (self.label, pv.size), pv, np.round(pv))]


@functools.lru_cache(maxsize=8)
def psnr255_case(n):
    return Psnr255Case(n)


LN10 = float(np.log(10.0))


def psnr_ref(total, n):
    """metrics.py:30-46, max_val 255: 20 log(255) / log(10) - 10 log(mse) / log(10); mse == 0 -> 0.  (value, bound):
    mse = fl(total / n): 1 rounding, R absolute through its logarithm; base = logf(10), logf(255), logf(mse): U log ulps each, the base's
    error relative on both quotients; 20 * and 10 *, the two divisions, the subtraction: k = 2 + 2 + 1"""
    mse = fl(total / n)
    if mse == 0.0:
        return 0.0, 0.0
    db = U["log"] * float(ulp32(LN10)) / LN10
    l255, lm = float(np.log(255.0)), float(np.log(mse))
    maxv, t = 20.0 * l255 / LN10, 10.0 * lm / LN10
    dmax = 20.0 * U["log"] * float(ulp32(l255)) / LN10 + abs(maxv) * db + 2 * R * abs(maxv)
    dt = 10.0 * (R + U["log"] * float(ulp32(lm))) / LN10 + abs(t) * db + 2 * R * abs(t)
    return maxv - t, dmax + dt + R * (abs(maxv) + abs(t)) + TINY32


GATE_NPARTS = (1, 255, 257, 2048)
GATE_W = (1.0, 0.8)


class PsnrGateCase:
    """wm_psnr_gate on a hand-made vector of double partials (integers): out[0] = the PSNR, out[1] = w_below if out[0] < threshold else
    w_above -- a condition on the RETURNED out[0], tried with the threshold at that value and at its two float32 neighbours"""

    def __init__(self, nparts, zero=False):
        self.nparts, self.zero = nparts, zero
        self.partials = np.zeros(nparts) if zero else np.floor(uni((nparts,), 9500 + nparts) * 4000.0) + 1.0
        self.n = float(nparts * 97)
        self.total = float(self.partials.sum())
        self.psnr, self.bound = psnr_ref(self.total, self.n)
        self.label = "psnr_gate nparts=%d%s" % (nparts, " zero" if zero else "")

    def check(self, out, threshold):
        o = f64(out).reshape(2)
        thr = float(np.float32(threshold))
        want = GATE_W[0] if o[0] < thr else GATE_W[1]
        return [ECmp(self.label + " psnr", o[:1], [self.psnr], [self.bound]),
                ECmp("%s weight at threshold %.9g" % (self.label, thr), o[1:], r32(np.array([want])))]


def check_psnr(label, out1, total, n):
    v, b = psnr_ref(total, n)
    return [ECmp(label + " psnr", f64(out1).reshape(1), [v], [b])]


# ----------------------------------------------------------------------------------------------------------------- tamper splice
def clamp_quant(x):
    """Quantization(clamp(x, 0, 1)) = round(255 c) / 255 on float32: the product, torch.round (half to even), the division -- three single
    float32 operations, exact"""
    c = np.minimum(np.maximum(np.asarray(x, dtype=np.float64).astype(np.float32), np.float32(0)), np.float32(1))
    return (np.rint(c * np.float32(255.0)) / np.float32(255.0)).astype(np.float64)


PLANE_KEYS = tuple((B, C, HW) for B in (1, 3) for C in (1, 3) for HW in (1, 5, 257 * 3))
SPLICE_MODES = ("fwd_q", "tampered", "real", "all")


def batch_masks(B, HW, seed):
    """[B, HW]: a different mask per batch item, values on a grid of 1/4 with whole stretches of 0 and 1"""
    return pick((B, HW), seed, (0.0, 0.0, 1.0, 1.0, 0.25, 0.75))


class SpliceCase:
    """wm_splice_fwd: q = clamp_quant(enc) (exact); tampered = q (1 - mask[b]) + prev mask[b]: 1 - m, two products, the sum: k = 4, the first
    through q; partials of (int(255 real) - int(255 q))^2 -- real is NOT clamped here (IRNcrop_model.py:660-664) -- integers, total exact"""

    def __init__(self, B, C, HW, data="normal"):
        self.B, self.C, self.HW = B, C, HW
        n = B * C * HW
        seed = 9600 + 31 * B + 7 * C + HW % 1000
        if data == "pattern":
            self.enc, self.real, self.prev = pattern(n) / 2 + 0.5, pattern(n, 41) / 2 + 0.5, pattern(n, 43)
        else:
            self.enc, self.real, self.prev = r32(uni((n,), seed, -0.2, 1.2)), r32(uni((n,), seed + 1, -0.5, 1.5)), data32((n,), seed + 2)
            sv = seam_values()
            put(self.real, sv)
            put(self.enc, np.concatenate([sv[::-1], tie_values()]))
        self.mask = batch_masks(B, HW, seed + 3)
        self.label = "splice B=%d C=%d HW=%d %s" % (B, C, HW, data)
        self.q = clamp_quant(self.enc)
        m = np.broadcast_to(self.mask[:, None, :], (B, C, HW)).reshape(-1)
        self.m_elem = m
        self.tam = self.q * (1.0 - m) + self.prev * m
        self.btam = R * (1.0 + np.abs(m)) * np.abs(self.q) + 3 * R * (np.abs(self.q * (1.0 - m)) + np.abs(self.prev * m)) + TINY32
        d = trunc255(self.real, False) - trunc255(self.q, False)
        self.total = int((d * d).sum())

    def check(self, mode, fwd_q, tampered, partials):
        cm = []
        if mode in ("fwd_q", "all"):
            cm.append(ECmp(self.label + " fwd_q", f64(fwd_q).reshape(-1), self.q))
        if mode in ("tampered", "all"):
            cm.append(ECmp(self.label + " tampered", f64(tampered).reshape(-1), self.tam, self.btam))
        if mode in ("real", "all"):
            pv = f64(partials).reshape(-1)
            cm.append(ECmp("%s psnr partials (%d) total" % (self.label, pv.size), [pv.sum()], [float(self.total)]))
        return cm


@functools.lru_cache(maxsize=4)
def splice_case(B, C, HW, data="normal"):
    return SpliceCase(B, C, HW, data)


SPLICE_CAP_KEY = (1, 1, CAP_SPLICE + 3, "pattern")


class MaskedAxpyCase:
    """a += g (1 - mask[b]): 1 - m through g, the product, the sum: k = 3"""

    def __init__(self, B, C, HW, data="normal"):
        self.B, self.C, self.HW = B, C, HW
        n = B * C * HW
        seed = 9700 + 31 * B + 7 * C + HW % 1000
        self.a, self.g = (pattern(n), pattern(n, 41)) if data == "pattern" else (data32((n,), seed), data32((n,), seed + 1))
        self.mask = batch_masks(B, HW, seed + 2)
        m = np.broadcast_to(self.mask[:, None, :], (B, C, HW)).reshape(-1)
        self.ref = self.a + self.g * (1.0 - m)
        self.bound = R * (1.0 + np.abs(m)) * np.abs(self.g) + 2 * R * (np.abs(self.a) + np.abs(self.g * (1.0 - m))) + TINY32
        self.label = "masked_axpy B=%d C=%d HW=%d %s" % (B, C, HW, data)

    def check(self, a):
        return [ECmp(self.label, f64(a).reshape(-1), self.ref, self.bound)]


# ----------------------------------------------------------------------------------------------------------------- flat elementwise glue
ELEM_KEYS = tuple((n, "normal") for n in SMALL_N) + ((CAP_ELEM + 3, "pattern"),)


class AxpyCase:
    """a += s b: the product and the sum, k = 2 (one fma: fewer)"""

    def __init__(self, n, data, s=-0.3):
        self.n, self.s = n, float(np.float32(s))
        self.a, self.b = (pattern(n), pattern(n, 41)) if data == "pattern" else (data32((n,), 9800 + n), data32((n,), 9801 + n))
        self.ref = self.a + self.s * self.b
        self.bound = 2 * R * (np.abs(self.a) + np.abs(self.s * self.b)) + TINY32
        self.label = "axpy n=%d s=%g %s" % (n, s, data)

    def check(self, a):
        return [ECmp(self.label, f64(a).reshape(-1), self.ref, self.bound)]


class ScaleDevCase:
    """x *= s[0]: one product, exact; s == 1 leaves x as it is"""

    def __init__(self, n, data, s):
        self.n, self.s = n, float(np.float32(s))
        self.x = pattern(n) if data == "pattern" else data32((n,), 9900 + n)
        self.ref = r32(self.x * self.s)
        self.label = "scale_dev n=%d s=%g %s" % (n, s, data)

    def check(self, x):
        return [ECmp(self.label, f64(x).reshape(-1), self.ref)]


class MaskThresholdCase:
    """out = p > threshold as uint8 (a nan is not above anything): exact; the threshold, its neighbours and nan come first"""

    def __init__(self, n, data, thr=0.5):
        self.n, self.thr = n, float(np.float32(thr))
        self.p = pattern(n) / 4 + 0.5 if data == "pattern" else r32(uni((n,), 9950 + n))
        put(self.p, around(self.thr) + [NAN])
        with np.errstate(invalid="ignore"):
            self.ref = (self.p > self.thr).astype(np.float64)
        self.label = "mask_threshold n=%d thr=%.9g %s" % (n, self.thr, data)

    def check(self, out):
        return [ECmp(self.label, f64(out).reshape(-1), self.ref)]


# ----------------------------------------------------------------------------------------------------------------- MSE, sum of squares
class MseCase:
    """nn.MSELoss: partials of d^2, d = fl(a - b) (reproducible), one product each: sum within R (1 + path) sum d^2;
    grad = fl(G d), G = gscale (x gate) (x gscale_dev), each product rounded once: exact"""

    def __init__(self, n, gscale=0.7, gdev=None, gate=None, data="normal"):
        self.n, self.gdev, self.gate = n, gdev, gate
        self.a, self.b = (pattern(n), pattern(n, 41)) if data == "pattern" else (data32((n,), 10000 + n), data32((n,), 10001 + n))
        self.gscale = float(np.float32(gscale))
        G = self.gscale
        if gate is not None:
            G = fl(G * float(np.float32(gate)))
        if gdev is not None:
            G = fl(G * float(np.float32(gdev)))
        self.G = G
        d = r32(self.a - self.b)
        self.ssq, self.grad = float((d * d).sum()), r32(G * d)
        self.label = "mse%s n=%d %s%s" % ("_gated" if gate is not None else "", n, data, " gscale_dev" if gdev is not None else "")

    def check(self, partials, grad, nparts=None):
        pv = f64(partials).reshape(-1)
        nparts = nparts or pv.size
        assert pv.size == nparts
        lab = "%s nparts=%d" % (self.label, nparts)
        cm = [ECmp(lab + " sum d^2", [pv.sum()], [self.ssq], [R * (1 + path(self.n, nparts)) * self.ssq + TINY32])]
        if grad is not None:
            cm.append(ECmp(lab + " grad", f64(grad).reshape(-1), self.grad))
        return cm


@functools.lru_cache(maxsize=4)
def mse_case(n, gscale=0.7, gdev=None, gate=None, data="normal"):
    return MseCase(n, gscale, gdev, gate, data)


class SumsqCase:
    def __init__(self, n):
        self.n, self.x = n, data32((n,), 10100 + n)
        self.ssq = float((self.x * self.x).sum())
        self.label = "sumsq n=%d" % n

    def check(self, partials):
        pv = f64(partials).reshape(-1)
        return [ECmp("%s nparts=%d" % (self.label, pv.size), [pv.sum()], [self.ssq], [R * (1 + path(self.n, pv.size)) * self.ssq + TINY32])]


NONFINITE_KEYS = tuple((n, at, v) for n in (4097, 2 * 4096 + 513) for at in (0, -1, 4096) for v in (INF, NAN)) + \
    ((4097, None, None), (257, 0, -INF), (1, 0, NAN), (1, None, None))


class NonfiniteCase:
    """wm_nonfinite: row k = 1 if workgroup k met an inf / nan among the elements it owns (i with (i / 256) % nparts == k), else 0: exact.
    Every case also holds a finite 3e19, whose square is beyond float32 and which must not be flagged."""

    def __init__(self, n, at, value):
        self.n = n
        self.x = data32((n,), 10200 + n)
        self.x[n // 2] = 3e19
        self.x = r32(self.x)
        if at is not None:
            self.x[at] = value
        self.label = "nonfinite n=%d %r at %r" % (n, value, at)

    def check(self, partials):
        pv = f64(partials).reshape(-1)
        owner = (np.arange(self.n) // 256) % pv.size
        ref = (np.bincount(owner, weights=(~np.isfinite(self.x)).astype(np.float64), minlength=pv.size) > 0).astype(np.float64)
        return [ECmp("%s nparts=%d" % (self.label, pv.size), pv, ref)]


IMG_LD, IMG_C0, IMG_DT = (16, 32), (0, 5), ("f32", "bf16", "f16")


class ImageGradMseCase:
    """wm_image_grad_mse: out[b, c, q] = fl(float(g[b, q, c0 + c]) + fl(G (a - b))) with d = fl(a - b): exact (the kernel keeps the product's
    own rounding); partials of d^2 as MseCase, a thread adding C terms per pixel.  g [B, HW, ld] holds SENTINEL outside [c0, c0 + C)."""

    def __init__(self, B, C, HW, dt, ld, c0, gdev=None):
        self.B, self.C, self.HW, self.dt, self.ld, self.c0, self.gdev = B, C, HW, dt, ld, c0, gdev
        seed = 10300 + 31 * B + 7 * C + HW % 1000 + ld + c0
        self.a, self.b = data32((B, C, HW), seed), data32((B, C, HW), seed + 1)
        self.gv = rnd(normal((B, HW, C), seed + 2), dt)
        self.gscale = float(np.float32(0.7))
        self.G = gscale_of(self.gscale, gdev)
        d = r32(self.a - self.b)
        self.ssq = float((d * d).sum())
        self.out = r32(self.gv.transpose(0, 2, 1) + r32(self.G * d))
        self.label = "image_grad_mse B=%d C=%d HW=%d %s ld=%d c0=%d%s" % (B, C, HW, dt, ld, c0, " gscale_dev" if gdev is not None else "")

    def g(self):
        buf = np.full((self.B, self.HW, self.ld), SENTINEL)
        buf[:, :, self.c0:self.c0 + self.C] = self.gv
        return store(buf, self.dt)

    def check(self, out, partials):
        pv = f64(partials).reshape(-1)
        k = 1 + path(self.B * self.HW, pv.size, per=self.C)
        return [ECmp(self.label + " out", f64(out).reshape(self.out.shape), self.out),
                ECmp("%s nparts=%d sum d^2" % (self.label, pv.size), [pv.sum()], [self.ssq], [R * k * self.ssq + TINY32])]


def image_grad_keys():
    rows, i = [], 0
    for B, C, HW in PLANE_KEYS:
        for dt in IMG_DT:
            rows.append((B, C, HW, dt, IMG_LD[i % 2], IMG_C0[(i // 2) % 2]))
            i += 1
    rows += [(3, 3, 771, dt, ld, c0) for dt in IMG_DT for ld in IMG_LD for c0 in IMG_C0]
    return sorted(set(rows))


# ----------------------------------------------------------------------------------------------------------------- BCEWithLogitsLoss
BCEL_EDGE = (0.0, -0.0, 20.0, -20.0, 90.0, -90.0, 1e30, -1e30)


def bcel_terms(x, t):
    """l = max(x, 0) - x t + log(1 + exp(-|x|)): x t: 1;  e = exp(-|x|): U exp ulps, which log1p passes on as de / (1 + e), + U log1p
    ulps;  the two sums: k = 2.  -> (term, bound, sum of the absolute terms)"""
    mx, xt = np.maximum(x, 0.0), x * t
    e = np.exp(-np.abs(x))
    l1p = np.log1p(e)
    ab = mx + np.abs(xt) + l1p
    return mx - xt + l1p, R * np.abs(xt) + U["exp"] * ulp32(e) / (1.0 + e) + U["log1p"] * ulp32(l1p) + 2 * R * ab, ab


def bcel_grad(x, t, G, n, kG):
    """(sigmoid(x) - t) G / n: the sigmoid's bound (sigmoid_b), s - t: 1 on s + |t|, the products with G and 1 / n (or the division
    by n): kG = 3 with 1 / n formed first, 2 with a division"""
    s, ds = sigmoid_b(x)
    g = (s - t) * G / n
    return g, (ds + R * (s + np.abs(t))) * abs(G) / n + kG * R * np.abs(g) + TINY32


class BceLogitsCase:
    """wm_bce_logits (one workgroup, constant target; mean = sum / n: one division) and wm_bce_logits_target (tensor target, nparts
    workgroups; each partial is multiplied by fl(1 / n): 2 more; chain: grad * p * (1 - p): the product, 1 - p: 1 on 1 + |p|, the product)"""

    def __init__(self, n, tensor_target, target=1.0, gdev=None, chain=False, edge=False, gscale=0.7):
        self.n, self.tensor_target, self.gdev, self.chain, self.edge = n, tensor_target, gdev, chain, edge
        seed = 10400 + n + (50 if tensor_target else 0)
        self.x = r32(uni((n,), seed, 0.0, 1.0)) if chain and not edge else data32((n,), seed, 3.0)
        if edge:
            put(self.x, BCEL_EDGE)
        self.t = pick((n,), seed + 1, (0.0, 1.0, 0.5, 0.25)) if tensor_target else np.full(n, float(target))
        if edge and tensor_target:
            put(self.t, [0.0, 1.0] * 4)
            if n >= 16:
                put(self.x, BCEL_EDGE, at=8)
                put(self.t, [1.0, 0.0] * 4, at=8)
        self.gscale = float(np.float32(gscale))
        self.G = gscale_of(gscale, gdev)
        self.label = "bce_logits%s n=%d%s%s%s%s" % ("_target" if tensor_target else " target=%g" % target, n, " edge" if edge else "",
                                                   " chain" if chain else "", " gscale_dev" if gdev is not None else "", "")
        with np.errstate(over="ignore"):
            self.term, self.bterm, self.aterm = bcel_terms(self.x, self.t)
            self.loss = float(self.term.sum() / n)
            g, bg = bcel_grad(self.x, self.t, self.G, n, (3 if tensor_target else 2) + (1 if gdev is not None else 0))
            if chain:
                v = self.x
                g2 = g * v * (1.0 - v)
                bg = bg * np.abs(v * (1.0 - v)) + np.abs(g * v) * R * (1.0 + np.abs(v)) + 2 * R * np.abs(g2) + TINY32
                g = g2
        over = np.abs(g) > F32_MAX
        self.grad, self.bgrad = overflow32(g), np.where(over, 0.0, bg)

    def check(self, loss, grad, nparts=1):
        extra = 2 if self.tensor_target else 1
        bl = (self.bterm.sum() + R * (path(self.n, nparts) + extra) * self.aterm.sum()) / self.n + (R * abs(self.loss) if self.tensor_target else 0.0) + TINY32
        lab = "%s nparts=%d" % (self.label, nparts)
        cm = [ECmp(lab + " loss", f64(loss).reshape(1), [self.loss], [bl])]
        if grad is not None:
            cm.append(ECmp(lab + " grad", f64(grad).reshape(-1), self.grad, self.bgrad))
        return cm


@functools.lru_cache(maxsize=8)
def bce_logits_case(n, tensor_target, target=1.0, gdev=None, chain=False, edge=False):
    return BceLogitsCase(n, tensor_target, target, gdev, chain, edge)


BCE_LOGITS_KEYS = tuple((n, False, t, None, False, False) for n in ONE_WG_N for t in (0.0, 1.0)) + \
    tuple((n, False, t, gd, False, True) for n in (8, 257) for t in (0.0, 1.0) for gd in (None, 1.5))
BCE_TARGET_KEYS = tuple((n, True, 1.0, None, ch, False) for n in FLAT_N for ch in (False, True)) + \
    tuple((n, True, 1.0, gd, ch, True) for n in (16, 257) for gd in (None, 1.5) for ch in (False, True))


# ----------------------------------------------------------------------------------------------------------------- message loss
MSG_EDGE = (-0.5, 0.5, 1.5, 2.5, -0.0, 0.49999997, 0.50000006)


class MessageLossCase:
    """hidden.py:96-99,109-111: out[0] = mean (d - m)^2: df = fl(d - m), its square: 1, the path, the division by n: 1;
    out[1] = sum |clip(round(d), 0, 1) - m| / n with messages in {0, 1}: an integer count below 2**24, one division: exact;
    grad = fl(fl(d - m) G): exact"""

    def __init__(self, n, gdev=None, edge=False):
        self.n, self.gdev = n, gdev
        self.m = pick((n,), 10500 + n, (0.0, 1.0))
        self.d = r32(self.m + normal((n,), 10501 + n, std=0.6))
        if edge:
            put(self.d, MSG_EDGE + MSG_EDGE)
            put(self.m, [0.0] * len(MSG_EDGE) + [1.0, 0.0, 1.0, 1.0, 1.0, 0.0, 1.0])   # both ties against a 0 bit twice: no defect cancels in the count
        self.gscale = float(np.float32(0.7))
        self.G = gscale_of(self.gscale, gdev)
        df = r32(self.d - self.m)
        self.ssq = float((df * df).sum())
        self.bits = np.abs(np.clip(np.rint(self.d), 0.0, 1.0) - self.m)
        self.out = np.array([self.ssq / n, fl(self.bits.sum() / n)])
        self.bound = np.array([R * (2 + path(n, 1)) * self.ssq / n + TINY32, 0.0])
        self.grad = r32(df * self.G)
        self.label = "message_loss n=%d%s%s" % (n, " edge" if edge else "", " gscale_dev" if gdev is not None else "")

    def check(self, out, grad):
        return [ECmp(self.label + " out", f64(out).reshape(2), self.out, self.bound), ECmp(self.label + " grad", f64(grad).reshape(-1), self.grad)]


@functools.lru_cache(maxsize=8)
def message_loss_case(n, gdev=None, edge=False):
    return MessageLossCase(n, gdev, edge)


MESSAGE_KEYS = tuple((n, None, False) for n in ONE_WG_N) + tuple((n, gd, True) for n in (14, 257) for gd in (None, 1.5))


# ----------------------------------------------------------------------------------------------------------------- the seven scalars
class HiddenMetricsCase:
    """out = [w_adv adv + w_enc enc + w_dec dec, enc, dec, bit error, adv, d_cover, d_enc], enc = fl(sum(partials) / n_img).  The partials
    are multiples of 1/8, so their double sum is exact and enc is one division in double and its cast: exact, like the other five
    pass-throughs.  The total: three products and two sums, k = 5, on the absolute terms."""

    def __init__(self, nparts):
        self.nparts = nparts
        seed = 10600 + nparts
        self.partials = grid((nparts,), seed, 0.125, 0.0, 64.0)
        self.n_img = float(nparts * 193)
        self.msg2, self.adv, self.d_cover, self.d_enc = (data32((k,), seed + 1 + i) for i, k in enumerate((2, 1, 1, 1)))
        self.w = tuple(float(np.float32(v)) for v in (1e-3, 0.7, 1.0))
        enc = fl(np.float64(self.partials.sum()) / np.float64(self.n_img))
        terms = np.array([self.w[0] * self.adv[0], self.w[1] * enc, self.w[2] * self.msg2[0]])
        self.ref = np.array([terms.sum(), enc, self.msg2[0], self.msg2[1], self.adv[0], self.d_cover[0], self.d_enc[0]])
        self.bound = np.array([5 * R * np.abs(terms).sum() + TINY32] + [0.0] * 6)
        self.label = "hidden_metrics nparts=%d" % nparts

    def check(self, out):
        return [ECmp(self.label, f64(out).reshape(7), self.ref, self.bound)]


def worst(cmps):
    """largest multiple of its bound over a list of comparisons (exact ones count 0 when they hold)"""
    return max([c.worst for c in cmps if not c.exact] + [0.0])
