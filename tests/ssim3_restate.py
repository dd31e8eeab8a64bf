"""Float64 numpy restatement of the reference's SSIM_Loss (loss.py:9-39 = models/modules/loss.py:44-74), ExtendedL1Loss (loss.py:363-376),
NonBlurryLoss (:379-388) and GrayLoss (:403-410), their gradients, the fixture's cases, and the comparisons of tests/test_gpu_ssim3.py.

The gradient of the map is written in SCATTER form -- every output's coefficients are added onto the padded image, then the one-pixel pad is
folded back onto the pixels it mirrors -- where the kernel (csrc/ssim3.hip) gathers: the two share no index arithmetic.

Cases (tests/golden/ssim3.npz stores the inputs): x, y independent and uniform in [0, 1), float32; `low` is the low-contrast pair
y = x + 0.02 * standard normal noise; `tile` is one pixel over the kernel's 16 x 64 tile in both axes, four planes."""
import numpy as np

C1, C2 = 0.01 ** 2, 0.03 ** 2
KINK = 1e-4          # outputs whose float64 unclamped value lies this close to 0 or 1 are kept out of the gradient comparisons
KINK_SHARE = 0.01    # at most this share of a case's outputs
MARGIN = 4.0         # bound = MARGIN x the reference's own float32-vs-float64 deviation of the case
MEAN_FLOOR = 2.0 ** -22  # 2 float32 ulp, relative: the least bound of the mean (one float32 mean can meet the float64 one by luck)
RED_BOUND = 2.0 ** -23   # the three reductions: sums in double, ONE rounding to float32 (2^-24 relative), with a factor 2 to spare

CASES = {
    "s22": (1, 1, 2, 2),
    "s25": (1, 1, 2, 5),
    "s33": (2, 3, 3, 3),
    "s52": (1, 3, 5, 2),
    "s1733": (2, 3, 17, 33),
    "tile": (2, 2, 17, 65),
    "low": (1, 3, 9, 9),
}
RED_SHAPES = {"r57": (2, 3, 5, 7), "r1": (1, 1, 1, 1)}


def case_inputs(name):
    """(x, y, g) float32: the images and the seeded upstream map of the (g * map).sum() gradient"""
    shape = CASES[name]
    rs = np.random.RandomState(7000 + 100 * sorted(CASES).index(name))
    x = rs.rand(*shape).astype(np.float32)
    if name == "low":
        y = (x + np.float32(0.02) * rs.randn(*shape).astype(np.float32)).astype(np.float32)
    else:
        y = rs.rand(*shape).astype(np.float32)
    g = (rs.rand(*shape) * 2 - 1).astype(np.float32)
    return x, y, g


def red_inputs(name):
    """a, b, x float32 and the three masks of the ExtendedL1Loss cases: binary; `zeros`: a general mask, with b made EQUAL to a on a third of
    the elements so that a - b holds exact zeros (sign(0) = 0); the zero mask"""
    shape = RED_SHAPES[name]
    rs = np.random.RandomState(7900 + sorted(RED_SHAPES).index(name))
    a, b, x = (rs.rand(*shape).astype(np.float32) for _ in range(3))
    binary = (rs.rand(*shape) < 0.6).astype(np.float32)
    if binary.sum() == 0:
        binary[...] = 1
    general = (rs.rand(*shape) + 0.25).astype(np.float32)
    b_eq = b.copy()
    eq = rs.rand(*shape) < 1 / 3
    eq.reshape(-1)[0] = shape != (1, 1, 1, 1)      # (the one-element case keeps a != b: an all-zero numerator says nothing)
    b_eq[eq] = a[eq]
    return {"a": a, "b": b, "x": x, "binary": (a, b, binary), "zeros": (a, b_eq, general), "zeromask": (a, b, np.zeros(shape, np.float32))}


# ----------------------------------------------------------------------------- SSIM_Loss
def _box(p):
    """sum of the nine taps of a reflect-padded [.., H+2, W+2] array -> [.., H, W], / 9"""
    H, W = p.shape[-2] - 2, p.shape[-1] - 2
    s = np.zeros(p.shape[:-2] + (H, W))
    for i in range(3):
        for j in range(3):
            s += p[..., i:i + H, j:j + W]
    return s / 9.0


def _pad(a):
    return np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)], mode="reflect")


def _stats(x, y):
    x, y = _pad(np.asarray(x, np.float64)), _pad(np.asarray(y, np.float64))
    return _box(x), _box(y), _box(x * x), _box(y * y), _box(x * y)


def ssim3_unclamped(x, y):
    mx, my, ex2, ey2, exy = _stats(x, y)
    n = (2 * mx * my + C1) * (2 * (exy - mx * my) + C2)
    d = (mx * mx + my * my + C1) * ((ex2 - mx * mx) + (ey2 - my * my) + C2)
    return (1 - n / d) / 2


def ssim3_map(x, y):
    return np.clip(ssim3_unclamped(x, y), 0.0, 1.0)


def _scatter(c):
    """adjoint of pad + box: coefficients [.., H, W] -> gradient wrt the unpadded image"""
    H, W = c.shape[-2:]
    p = np.zeros(c.shape[:-2] + (H + 2, W + 2))
    for i in range(3):
        for j in range(3):
            p[..., i:i + H, j:j + W] += c / 9.0
    # fold the pad back: padded row 0 mirrors image row 1 (padded row 2), padded row H+1 mirrors image row H-2 (padded row H-1)
    p[..., 2, :] += p[..., 0, :]
    p[..., H - 1, :] += p[..., H + 1, :]
    p = p[..., 1:H + 1, :]
    p[..., :, 2] += p[..., :, 0]
    p[..., :, W - 1] += p[..., :, W + 1]
    return p[..., :, 1:W + 1]


def ssim3_grads(x, y, g):
    """(d/dx, d/dy) of sum(g * ssim3_map(x, y)); torch.clamp's backward: the gradient passes where 0 <= unclamped <= 1"""
    x, y, g = (np.asarray(t, np.float64) for t in (x, y, g))
    mx, my, ex2, ey2, exy = _stats(x, y)
    A1, A2 = 2 * mx * my + C1, 2 * (exy - mx * my) + C2
    B1, B2 = mx * mx + my * my + C1, (ex2 - mx * mx) + (ey2 - my * my) + C2
    S = A1 * A2 / (B1 * B2)
    v = (1 - S) / 2
    w = np.where((v >= 0) & (v <= 1), g, 0.0) * -0.5
    dS_dmx = (2 * my * A2 - 2 * my * A1) / (B1 * B2) - S * (2 * mx / B1 - 2 * mx / B2)
    dS_dmy = (2 * mx * A2 - 2 * mx * A1) / (B1 * B2) - S * (2 * my / B1 - 2 * my / B2)
    dS_dq = -S / B2
    dS_dr = 2 * A1 / (B1 * B2)
    gx = _scatter(w * dS_dmx) + 2 * x * _scatter(w * dS_dq) + y * _scatter(w * dS_dr)
    gy = _scatter(w * dS_dmy) + 2 * y * _scatter(w * dS_dq) + x * _scatter(w * dS_dr)
    return gx, gy


def ssim3_mean_grads(x, y):
    return ssim3_grads(x, y, np.full(np.shape(x), 1.0 / np.size(x)))


def kink_outputs(x, y):
    """outputs whose float64 unclamped value lies within KINK of a bound of the clamp"""
    v = ssim3_unclamped(x, y)
    return (np.abs(v) <= KINK) | (np.abs(v - 1) <= KINK)


def grad_keep(x, y):
    """the input pixels of the gradient comparisons: those with no kinked output among the (at most nine) outputs whose window reads them --
    an output's window reaches one pixel around it, and the reflection only maps the pad onto pixels within that reach"""
    k = kink_outputs(x, y)
    H, W = k.shape[-2:]
    p = np.zeros(k.shape[:-2] + (H + 2, W + 2), bool)
    for i in range(3):
        for j in range(3):
            p[..., i:i + H, j:j + W] |= k
    return ~p[..., 1:H + 1, 1:W + 1]


# ----------------------------------------------------------------------------- the three reductions
def extended_l1(a, b, m):
    a, b, m = (np.asarray(t, np.float64) for t in (a, b, m))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(m * a - m * b).mean() / np.abs(m).mean()


def extended_l1_grads(a, b, m):
    a, b, m = (np.asarray(t, np.float64) for t in (a, b, m))
    with np.errstate(invalid="ignore", divide="ignore"):
        ga = np.sign(m * a - m * b) * m / (a.size * np.abs(m).mean())
    return ga, -ga


def non_blurry(x):
    return 1 - ((np.asarray(x, np.float64) - 0.5) ** 2).mean()


def non_blurry_grad(x):
    x = np.asarray(x, np.float64)
    return -2 * (x - 0.5) / x.size


def gray_loss(x):
    return 1 / np.abs(np.asarray(x, np.float64) - 0.5).mean()


def gray_loss_grad(x):
    x = np.asarray(x, np.float64)
    return -np.sign(x - 0.5) / (x.size * np.abs(x - 0.5).mean() ** 2)


# ----------------------------------------------------------------------------- the comparisons of the GPU tests
def abs_dev(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float("inf") if not np.isfinite(got).all() else float(np.max(np.abs(got - want)))


def grad_dev(got, want, keep=None):
    """max |got - want| over the kept elements / max |want| (over all elements)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float("inf")
    m = float(np.max(np.abs(want)))
    assert m > 0
    d = np.abs(got - want)
    if keep is not None:
        assert keep.any()
        d = d[keep]
    return float(np.max(d)) / m


def check(what, dev, bound):
    print("%s: %.3e (bound %.3e)" % (what, dev, bound))
    assert dev <= bound, (what, dev, bound)
    return dev


def bounds(g, name):
    """MARGIN x the reference's own float32-vs-float64 deviation of case `name` on the inputs the tests compare (stored by the generator):
    map absolute, mean relative (at least MEAN_FLOOR), the two gradients relative to max |grad64|"""
    b = {q: MARGIN * float(g["%s_dev_%s" % (name, q)]) for q in ("map", "mean", "gmean", "gmap")}
    b["mean"] = max(b["mean"], MEAN_FLOOR)
    return b
