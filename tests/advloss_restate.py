"""Float64 numpy restatement of what the kernels of csrc/advloss.hip compute, written from the definitions (the reference's loss.py
AdversarialLoss, models/modules/loss.py GANLoss and CWLoss, and the torch modules they are built on): every element objective with its
gradient, the masked labels, the Carlini-Wagner margin with its gradient.  It is the yardstick of the GPU tests; the CPU tests compare it
with the reference's recorded float64 results in tests/golden/advloss.npz.

    elem(objective, x, t) -> (v, dv/dx) per element;  loss = mean v, gradient = dv / n
        bce_prob    v = -(t max(log x, -100) + (1 - t) max(log(1 - x), -100)),  dv = (x - t) / max(x (1 - x), 1e-12)   nn.BCELoss and ITS backward
                    (torch holds that 1e-12 as a float32 constant: BCE_EPS)
        bce_logits  v = (1 - t) x + max(-x, 0) + log(1 + exp(-|x|)),            dv = sigmoid(x) - t
        mse         v = (x - t)^2,  dv = 2 (x - t)
        hinge_disc  v = relu(1 + s x),  dv = s [1 + s x > 0]  (0 at the kink, as nn.ReLU),  s = t = -1 (real) / +1 (fake)
        neg_mean / pos_mean   v = -+x
    masked_labels(mask, (H, W), real) = real * (1 - bilinear(mask)), align_corners = False, no antialiasing
    cw_margin(logits, target, targeted, kappa) = sum_b max(+-(other_b - real_b), kappa); gradient +-w at the target column and at the LOWEST
        column attaining `other` (none when that is the target's own -10000 slot), w = 1 / 0.5 (margin == kappa) / 0
Every input is a float32 value (labels and kappa included: 0.9 means float32(0.9), which is what a float32 tensor filled with 0.9 holds).

Also here: the fixture's case tables with their seeded inputs, and the tolerance rule.  numpy and torch (for the seeded generators) only."""
import numpy as np
import torch

SIZES = (1, 3, 255, 256, 257, 1027)
# variant -> (objective, label, input family, how the reference computes it: (class, type, (real label, fake label), call arguments))
VARIANTS = {
    "nsgan_real": ("bce_prob", 1.0, "prob", ("adv", "nsgan", (1.0, 0.0), (True, True))),
    "nsgan_fake": ("bce_prob", 0.0, "prob", ("adv", "nsgan", (1.0, 0.0), (False, True))),
    "nsgan_soft": ("bce_prob", 0.9, "prob", ("adv", "nsgan", (0.9, 0.1), (True, False))),
    "gan_real": ("bce_logits", 0.9, "logit", ("gan", "gan", (0.9, 0.1), (True,))),
    "gan_fake": ("bce_logits", 0.1, "logit", ("gan", "ragan", (0.9, 0.1), (False,))),
    "lsgan_real": ("mse", 1.0, "plain", ("adv", "lsgan", (1.0, 0.0), (True, True))),
    "lsgan_fake": ("mse", 0.0, "plain", ("adv", "lsgan", (1.0, 0.0), (False, True))),
    "lsgan_soft": ("mse", 0.9, "plain", ("gan", "lsgan", (0.9, 0.1), (True,))),
    "hinge_real": ("hinge_disc", -1.0, "hinge", ("adv", "hinge", (1.0, 0.0), (True, True))),
    "hinge_fake": ("hinge_disc", 1.0, "hinge", ("adv", "hinge", (1.0, 0.0), (False, True))),
    "hinge_gen": ("neg_mean", None, "plain", ("adv", "hinge", (1.0, 0.0), (True, False))),
    "wgan_real": ("neg_mean", None, "plain", ("gan", "wgan-gp", (1.0, 0.0), (True,))),
    "wgan_fake": ("pos_mean", None, "plain", ("gan", "wgan-gp", (1.0, 0.0), (False,))),
}
CASES = {"%s_n%d" % (v, n): (v, n) for v in VARIANTS for n in SIZES}
# masked labels: name -> (outputs shape, mask shape); every one with a {0, 1} mask ("bin") and a fractional one ("frac"), real_label 0.9,
# under nsgan (bce_prob) and lsgan (mse)
MASK_SHAPES = {
    "down": ((2, 1, 5, 7), (2, 1, 16, 16)),
    "up": ((1, 1, 8, 8), (1, 1, 3, 3)),
    "same": ((1, 1, 4, 4), (1, 1, 4, 4)),
    "chan": ((1, 2, 3, 5), (1, 2, 6, 4)),        # a mask per output channel
    "bcast": ((2, 2, 3, 5), (2, 1, 6, 4)),       # one mask channel for both
}
MASK_CASES = {"mask_%s_%s_%s" % (s, m, t): (s, m, t) for s in MASK_SHAPES for m in ("bin", "frac") for t in ("nsgan", "lsgan")}
MASK_REAL_LABEL = 0.9
CW_SHAPES = ((1, 2), (3, 6), (2, 1000), (65, 7))
CW_CASES = {"cw_%dx%d_%s_k%g" % (B, K, "t" if tg else "u", kp): (B, K, tg, kp) for B, K in CW_SHAPES for tg in (True, False) for kp in (0.0, 0.5)}


BCE_EPS = float(np.float32(1e-12))      # torch's binary_cross_entropy_backward: `constexpr float EPSILON = 1e-12`


def f32(v):
    """the float32 value nearest v, as a Python float"""
    return float(np.float32(v))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def gen_input(family, n):
    """float32 [n], with the family's branch points planted exactly at the front"""
    g = _gen(100 + 7 * n + sorted(("prob", "logit", "plain", "hinge")).index(family))
    z = torch.randn(n, generator=g)
    if family == "prob":
        x = torch.sigmoid(3.0 * z)
        x[0] = 0.0                                # the -100 clamp of log x, the 1e-12 denominator
        if n >= 3:
            x[1], x[2] = 1.0, 1e-30               # the clamp of log(1 - x); x (1 - x) far below 1e-12 with a finite log
    elif family == "logit":
        x = 3.0 * z
        x[0] = 40.0
        if n >= 3:
            x[1], x[2] = -40.0, 0.0
    elif family == "hinge":
        x = 1.5 * z
        x[0] = -1.0                               # the kink of relu(1 + x)
        if n >= 3:
            x[1], x[2] = 1.0, 0.0                 # the kink of relu(1 - x)
    else:
        x = 1.5 * z
    return x.numpy().astype(np.float32)


def gen_mask_case(name):
    """(outputs float32 probabilities, mask float32) of a MASK_CASES entry"""
    shape, kind, _ = MASK_CASES[name]
    so, sm = MASK_SHAPES[shape]
    g = _gen(300 + 11 * sorted(MASK_SHAPES).index(shape) + (kind == "frac"))
    out = torch.sigmoid(2.0 * torch.randn(so, generator=g))
    m = torch.rand(sm, generator=g)
    if kind == "bin":
        m = (m > 0.5).float()
    return out.numpy().astype(np.float32), m.numpy().astype(np.float32)


def gen_cw_case(name):
    """(logits float32 [B,K], target int64 [B]).  With B >= 3 the first rows are planted on eighths, so every difference is exact:
    row 0 the clamp at kappa wins; row 1 the margin EQUALS kappa; row 2 the two largest non-target logits are equal (and the margin wins);
    with B >= 4 row 3 holds every non-target logit below -10000, so `other` is the target's own -10000 slot"""
    B, K, targeted, kappa = CW_CASES[name]
    g = _gen(500 + 13 * CW_SHAPES.index((B, K)))
    z = (3.0 * torch.randn(B, K, generator=g)).numpy().astype(np.float32)
    t = torch.randint(0, K, (B,), generator=g).numpy().astype(np.int64)
    if B >= 3:
        sgn = 1.0 if targeted else -1.0          # margin = sgn * (other - real)
        for r in range(3):
            z[r] = -4.0 - 0.125 * np.arange(K)
        t[0], t[1], t[2] = 1, 0, K - 1
        z[0, 1], z[0, 3] = 0.0, -sgn * 2.0       # margin -2 < kappa
        z[1, 0], z[1, 2] = 1.0, 1.0 + sgn * kappa    # margin = kappa exactly
        z[2, K - 1], z[2, 1], z[2, 3] = -sgn * 3.0, 2.0, 2.0    # margin 2 + 3 > kappa, `other` attained at columns 1 and 3
    if B >= 4:
        z[3] = -20000.0 - np.arange(K)
        t[3] = 2
        z[3, 2] = 1.0
    return z, t


# ----------------------------------------------------------------------------- element objectives
def elem(objective, x, t):
    """(v, dv/dx) per element, float64; x float32 values, t a float32 value or an array of float64 labels"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if objective == "bce_prob":
            v = -(t * np.maximum(np.log(x), -100.0) + (1.0 - t) * np.maximum(np.log1p(-x), -100.0))
            dv = (x - t) / np.maximum(x * (1.0 - x), BCE_EPS)
        elif objective == "bce_logits":
            e = np.exp(-np.abs(x))
            v = (1.0 - t) * x + np.maximum(-x, 0.0) + np.log1p(e)
            dv = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)) - t
        elif objective == "mse":
            v, dv = (x - t) ** 2, 2.0 * (x - t)
        elif objective == "hinge_disc":
            z = 1.0 + t * x
            v, dv = np.maximum(z, 0.0), np.where(z > 0, t, 0.0)
        elif objective == "neg_mean":
            v, dv = -x, -np.ones_like(x)
        elif objective == "pos_mean":
            v, dv = x, np.ones_like(x)
        else:
            raise ValueError(objective)
    return v, dv


def adv_loss(objective, x, t=None):
    """(loss, gradient) of the mean over every element"""
    v, dv = elem(objective, x, 0.0 if t is None else t)
    return float(np.sum(v) / v.size), dv / v.size


def _source(n_in, n_out):
    src = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), src - i0


def bilinear(mask, size):
    """F.interpolate(mask, size, mode="bilinear", align_corners=False) of a [B,C,Hm,Wm] array, float64"""
    m = np.asarray(mask, dtype=np.float64)
    y0, y1, ly = _source(m.shape[2], size[0])
    x0, x1, lx = _source(m.shape[3], size[1])
    top = m[:, :, y0][:, :, :, x0] * (1 - lx) + m[:, :, y0][:, :, :, x1] * lx
    bot = m[:, :, y1][:, :, :, x0] * (1 - lx) + m[:, :, y1][:, :, :, x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def masked_labels(mask, out_shape, real_label):
    """loss.py:83-85: real_label * (1 - mask_down), broadcast over the outputs' channels"""
    return np.broadcast_to(f32(real_label) * (1.0 - bilinear(mask, out_shape[2:])), out_shape)


# ----------------------------------------------------------------------------- Carlini-Wagner margin
def cw_margin(logits, target, targeted, kappa):
    """(loss, gradient [B,K]), float64"""
    z = np.asarray(logits, dtype=np.float64)
    B, K = z.shape
    kappa = f32(kappa)
    onehot = np.eye(K)[target]
    real = np.sum(onehot * z, axis=1)
    masked = (1 - onehot) * z - onehot * 10000.0
    arg = np.argmax(masked, axis=1)                   # the first of equal maxima
    other = masked[np.arange(B), arg]
    d = other - real if targeted else real - other
    w = np.where(d > kappa, 1.0, np.where(d == kappa, 0.5, 0.0)) * (1.0 if targeted else -1.0)
    grad = np.zeros_like(z)
    grad[np.arange(B), target] -= w
    live = arg != target                              # the target's own slot of `masked` is the constant -10000
    grad[np.arange(B)[live], arg[live]] += w[live]
    return float(np.sum(np.maximum(d, kappa))), grad


# ----------------------------------------------------------------------------- the tolerance rule
def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def bound(dev, want, scale=1.0):
    """per element: 4 x the reference's own |float32 result - float64 restatement| on the same inputs, with a floor of 2 float32 ulp of the
    value.  scale: the upstream factor a gradient was asked with (the recorded deviation is of the unscaled gradient)"""
    return np.maximum(4.0 * abs(scale) * np.asarray(dev, dtype=np.float64), 2.0 * ulp32(want))


def check(what, got, want, dev, scale=1.0):
    """assert |got - want| <= bound elementwise; prints the worst figure first.  NaN / inf in got fail unless want holds the same"""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    b = np.broadcast_to(bound(dev, want, scale), want.shape)
    with np.errstate(invalid="ignore"):
        err = np.where(got == want, 0.0, np.abs(got - want))
    err = np.where(np.isnan(err), np.inf, err)
    i = int(np.argmax(err - b))
    print("%s: worst |got - want| %.3e at %d (bound %.3e, reference's deviation %.3e)" % (what, err.flat[i], i, b.flat[i],
                                                                                          np.max(np.asarray(dev, dtype=np.float64))))
    assert (err <= b).all(), (what, float(err.flat[i]), float(b.flat[i]))
    return float(err.flat[i]), float(b.flat[i])
