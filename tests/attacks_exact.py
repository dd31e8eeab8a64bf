"""Float64 restatements of the stencil / median / resample attack kernels (csrc/attacks.hip) and of the two rounding kernels
(wm_quant_fwd, wm_clamp_quant_fwd), and the comparisons built on them.  A plain helper module (no fixtures, CPU only, never imports the
HIP package): used by tests/test_cpu_attacks_exact.py with CPU imitations standing in for the kernels, and by
tests/test_gpu_attacks_exact.py with the kernels.

The interpolation is continuous in the source coordinate and the clamp mask is read from a tensor the caller passes in, so there are no
ties to account for (tests/jpeg_exact.py needs them, this does not): a dense float64 matrix per axis is the definition, and it is exact.

    resample     y = Rh @ x[rect] @ Rw.T                       axis_matrix: one row per output index, built tap by tap
    its backward gx[rect] = Rh.T @ (gy * mask) @ Rw             mask = 0 < y_clamped < 1, strictly; zero outside the rectangle
    stencil      nine shifted adds, zero padding 1             cross-correlation: tap (a, b) multiplies x[h + a - 1, w + b - 1]
    median       not recomputed: the kernel's (y, idx) are CHECKED against the definition of a median, whichever way ties were broken,
                 and the backward is the scatter of gy to the tap idx names (nothing for a tap in the padding)
    quantisers   the same IEEE operations in numpy float32: bit-exact, no tolerance

Tolerances.  Resample: per case and per quantity, FACTOR x the largest deviation of torch's float32 CPU F.interpolate (or of its
autograd, the same mask applied to gy) from the float64 restatement ON THAT CASE, measured on the CPU at test time and never on the
kernels, with a floor of 8 * 2**-24 * max|ref| where the float32 reference is exact.  FACTOR = 4 is this project's margin for "same
arithmetic, another summation order" (tests/jpeg_exact.py).  The deviation is dominated by the float32 source coordinate
(o + 0.5) * scale - 0.5, whose round-off grows with the output index: 1e-8 for one pixel, 2e-5 for 300 -> 9, which is why it is taken
per case.  Stencil and median backward: derived from the number format (16 resp. k*k ulp of the sum of absolute terms per pixel).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import detgen

BILINEAR, BICUBIC = 0, 1                  # ops.BILINEAR, ops.BICUBIC
MODE = {BILINEAR: "bilinear", BICUBIC: "bicubic"}
KINDS = (BILINEAR, BICUBIC)
EPS32 = 2.0 ** -24
FACTOR = 4.0
OUTSIDE = 1000.0                          # the value of every pixel outside the rectangle: a tap that leaves it is an error of order 1000


# ----------------------------------------------------------------------------------------------------------------- resample
def _cubic1(x, A=-0.75):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def _cubic2(x, A=-0.75):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def axis_matrix_in_image(out, n, kind, start=0, full=None, clamp_to_image=False):
    """float64 [out, full]: row o holds the weights with which output o reads the `full` pixels of an image axis whose rectangle is
    [start, start + n).  Taps are clamped to the rectangle; clamp_to_image=True is the DEFECT of clamping them to the image."""
    full = n if full is None else full
    lo, hi = (-start, full - start - 1) if clamp_to_image else (0, n - 1)
    R = np.zeros((out, full), dtype=np.float64)
    scale = n / out
    for o in range(out):
        src = (o + 0.5) * scale - 0.5
        if kind == BILINEAR:
            src = max(src, float(lo))
            i0 = min(int(math.floor(src)), hi)
            i1 = i0 + (1 if i0 < hi else 0)
            lam = src - i0
            R[o, start + i0] += 1.0 - lam
            R[o, start + i1] += lam
        else:
            fl = math.floor(src)
            t = src - fl
            for k, wt in enumerate((_cubic2(t + 1.0), _cubic1(t), _cubic1(1.0 - t), _cubic2(2.0 - t))):
                R[o, start + min(max(int(fl) - 1 + k, lo), hi)] += wt
    return torch.from_numpy(R)


@functools.lru_cache(maxsize=None)
def axis_matrix(out, n, kind):
    """float64 [out, n] from the definition (F.interpolate, align_corners=False, no antialias).  Shared: do not write to it."""
    return axis_matrix_in_image(out, n, kind)


def _rect(rect, H, W):
    return (0, H, 0, W) if rect is None else tuple(rect)


def resample_ref(x, rect, out, kind, clamp01=False):
    h0, hs, w0, ws = _rect(rect, x.shape[2], x.shape[3])
    y = axis_matrix(out[0], hs, kind) @ x[:, :, h0:h0 + hs, w0:w0 + ws].double() @ axis_matrix(out[1], ws, kind).T
    return y.clamp(0.0, 1.0) if clamp01 else y


def clamp_mask(y_clamped):
    """clamp(0, 1) passes the gradient strictly inside the interval; evaluated in the tensor's own dtype"""
    return (y_clamped > 0) & (y_clamped < 1)


def resample_bwd_ref(gy, y_clamped, in_hw, rect, out, kind):
    H, W = in_hw
    h0, hs, w0, ws = _rect(rect, H, W)
    G = gy.double()
    if y_clamped is not None:
        G = G * clamp_mask(y_clamped)
    gx = torch.zeros(gy.shape[0], gy.shape[1], H, W, dtype=torch.float64)
    gx[:, :, h0:h0 + hs, w0:w0 + ws] = axis_matrix(out[0], hs, kind).T @ G @ axis_matrix(out[1], ws, kind)
    return gx


def axis_range(i, n, out):
    """the candidate outputs [lo, hi] of input i along one axis: csrc/attacks.hip's axis_range, in float64"""
    inv = out / n
    lo = int(math.floor((i - 2.0 + 0.5) * inv - 0.5)) - 1
    hi = int(math.ceil((i + 2.0 + 0.5) * inv - 0.5)) + 1
    return max(lo, 0), min(hi, out - 1)


def sep_path(shape, rect, out):
    """what wm_resample_bwd_sep's host code selects for a case: the x kernel (LDS form or not), its MAXC, whether a thread's candidate
    columns overflow MAXC (the `wide` loop; the gather form keeps 24), whether the y pass overflows its MAXT = 12 registers, the column
    blocks, and whether a block of either pass walks more than one row or plane."""
    B, C, H, W = shape
    h0, hs, w0, ws = _rect(rect, H, W)
    OH, OW = out
    N = B * C
    span = int(4.0 * OW / ws) + 5
    maxc = 8 if span <= 8 else (12 if span <= 12 else 24)
    cols = max(b - a + 1 for a, b in (axis_range(i, ws, OW) for i in range(ws)))
    rows = max(b - a + 1 for a, b in (axis_range(i, hs, OH) for i in range(hs)))
    bx = (W + 255) // 256
    ry = min(max(1024 // (bx * N), 1), OH)
    pz = min(max(1024 // (bx * H), 1), N)
    return {"lds": OW <= 1024, "maxc": maxc, "wide": cols > maxc, "wide_gather": cols > 24, "y_overflow": rows > 12, "blocks": bx,
            "x_rows_per_block": -(-OH // ry), "y_planes_per_block": -(-N // pz)}


# case, shape, rect (None: whole), out, and the path the row is there for.  The x pass of wm_resample_bwd_sep is chosen by the host from
# span = int(4 * OW / ws) + 5 (MAXC = 8 if span <= 8, 12 if span <= 12, else 24) and OW <= 1024 (the LDS form); `wide` = a pixel has more
# candidate columns than MAXC; the y pass keeps MAXT = 12 rows.  If those thresholds move, the rows to move are the ones whose numbers
# below no longer select the path named (tests/test_cpu_attacks_exact.py asserts the `path` column against sep_path):
#   resize 0.7     span  7, OW   39 <= 1024  LDS, MAXC 8
#   resize 1.3     span 10, OW   72          LDS, MAXC 12; OH / hs = 1.3: at most 11 candidate rows, all in registers
#   crop 0.3       span 18, OW   56          LDS, MAXC 24; OH / hs = 3.33: 19 candidate rows, the overflow loop
#   very wide      span 405, OW 300          LDS, MAXC 24 + wide (all 300 columns are candidates); the gather form's wide loop; 37 rows
#   seam           span 10, OW  333          LDS, MAXC 12; W = 300: two column blocks, the rectangle's columns 30..289 cross column 256
#   long rows a    span 13, OW 1040 > 1024   global-memory form, MAXC 24
#   long rows b    span  7, OW 1040          global-memory form, MAXC 8; W = 1500: six column blocks
#   long rows c    span 46, OW 1040          global-memory form, MAXC 24 + wide
#   tall           span  7, OW  182          N = 6, W = 260: the x grid is 2 x 85 x 6, a block walks 5 rows (both LDS buffers, twice);
#                                            the y grid is 2 x 520 x 1: one block walks all 6 planes
RESAMPLE_ROWS = (
    ("resize 0.7", (2, 3, 40, 56), None, (28, 39), {"lds": True, "maxc": 8, "wide": False}),
    ("resize 1.3", (2, 3, 40, 56), None, (52, 72), {"lds": True, "maxc": 12, "wide": False, "y_overflow": False}),
    ("crop 0.3 back to full", (2, 3, 40, 56), (9, 12, 20, 17), (40, 56), {"lds": True, "maxc": 24, "wide": False, "y_overflow": True}),
    ("very wide", (1, 2, 12, 16), (3, 5, 4, 3), (37, 300), {"lds": True, "maxc": 24, "wide": True, "wide_gather": True, "y_overflow": True}),
    ("seam", (1, 2, 6, 300), (1, 4, 30, 260), (9, 333), {"lds": True, "maxc": 12, "blocks": 2}),
    ("long rows a", (1, 1, 3, 520), None, (2, 1040), {"lds": False, "maxc": 24, "wide": False}),
    ("long rows b", (1, 1, 3, 1500), None, (2, 1040), {"lds": False, "maxc": 8, "wide": False}),
    ("long rows c", (1, 1, 2, 100), None, (2, 1040), {"lds": False, "maxc": 24, "wide": True}),
    ("tall", (2, 3, 520, 260), None, (364, 182), {"lds": True, "blocks": 2, "x_rows_per_block": 5, "y_planes_per_block": 6}),
    ("strong shrink", (1, 2, 300, 20), None, (9, 33), {}),
    ("one row/col", (1, 2, 5, 7), (2, 1, 3, 1), (4, 6), {}),
    ("one output", (1, 2, 5, 7), None, (1, 1), {}),
    ("one pixel to one", (1, 1, 1, 1), None, (1, 1), {}),
    ("one pixel to 3x4", (1, 1, 1, 1), None, (3, 4), {}),
)
RESAMPLE_NAMES = tuple(r[0] for r in RESAMPLE_ROWS)
MASKS = ("none", "own forward", "synthetic")


class Report:
    def __init__(self, what, dev_kernel, tol, dev_ref32, extra=""):
        self.what, self.dev_kernel, self.tol, self.dev_ref32, self.extra = what, dev_kernel, tol, dev_ref32, extra

    def line(self):
        return "%-46s f32 reference %.3e  tolerance %.3e  under test %.3e%s" % (self.what, self.dev_ref32, self.tol, self.dev_kernel, self.extra)

    def assert_ok(self):
        assert self.dev_kernel <= self.tol, self.line()      # (a NaN deviation fails too)
        return self


def _tolerance(f32, ref):
    dev = float((f32.double() - ref).abs().max())
    return max(FACTOR * dev, 8 * EPS32 * float(ref.abs().max())), dev


def _deviation(got, ref, what):
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32, (what, tuple(got.shape), got.dtype)
    d = float((got.detach().cpu().double() - ref).abs().max())
    return d if math.isfinite(d) else float("nan")


def synthetic_mask_plane(shape):
    """a y_clamped plane cycling through the values at which the mask decides (no denormals): 0, -0 and 1 block the gradient; the
    float below 1, the smallest normal float and 0.5 pass it.  The cycle advances by one per pixel and by five per row, so every
    column and every row of any size sees all six."""
    vals = torch.tensor([0.0, -0.0, 1.0, float(np.nextafter(np.float32(1), np.float32(0))), 2.0 ** -126, 0.5], dtype=torch.float32)
    B, C, OH, OW = shape
    i = torch.arange(OW).view(1, 1, OW) + 5 * torch.arange(OH).view(1, OH, 1) + torch.arange(B * C).view(B * C, 1, 1)
    return vals[i % 6].view(B, C, OH, OW)


class ResampleCase:
    """One row of RESAMPLE_ROWS for one kind: inputs (uniform inside the rectangle, OUTSIDE around it), the float64 results and the
    tolerances measured on torch's float32 CPU interpolation.  Built once (resample_case) and shared: leave its tensors unchanged."""

    def __init__(self, name, shape, rect, out, kind, seed):
        B, C, H, W = shape
        self.name, self.shape, self.out, self.kind = name, tuple(shape), tuple(out), kind
        self.rect = _rect(rect, H, W)
        h0, hs, w0, ws = self.rect
        u = detgen.uniform((B, C, hs, ws), seed)
        self.x = torch.full(shape, OUTSIDE, dtype=torch.float32)
        self.x[:, :, h0:h0 + hs, w0:w0 + ws] = u
        self.x_sat = torch.full(shape, OUTSIDE, dtype=torch.float32)           # bicubic overshoots 0 and 1 here: the clamp acts
        self.x_sat[:, :, h0:h0 + hs, w0:w0 + ws] = (3 * u - 1).clamp(0, 1)
        self.gy = detgen.normal((B, C) + tuple(out), seed + 1)
        self.outside = torch.ones(H, W, dtype=torch.bool)
        self.outside[h0:h0 + hs, w0:w0 + ws] = False
        self.label = "%s %s" % (name, MODE[kind])
        self._fwd = {}

    def _inside(self, t):
        h0, hs, w0, ws = self.rect
        return t[:, :, h0:h0 + hs, w0:w0 + ws]

    def _interp32(self, x_inside):
        return F.interpolate(x_inside, size=self.out, mode=MODE[self.kind], align_corners=False)

    def fwd_expect(self, saturated, clamp01):
        key = (bool(saturated), bool(clamp01))
        if key not in self._fwd:
            x = self.x_sat if saturated else self.x
            ref = resample_ref(x, self.rect, self.out, self.kind, clamp01)
            y32 = self._interp32(self._inside(x))
            self._fwd[key] = (ref,) + _tolerance(y32.clamp(0, 1) if clamp01 else y32, ref)
        return self._fwd[key]

    def check_fwd(self, y, saturated, clamp01):
        ref, tol, dev32 = self.fwd_expect(saturated, clamp01)
        what = "%s fwd%s%s" % (self.label, " saturated" if saturated else "", " clamp" if clamp01 else "")
        return Report(what, _deviation(y, ref, what), tol, dev32).assert_ok()

    def mask_plane(self, which, own_forward=None):
        """the y_clamped argument of the backward: None, the clamped forward of the saturated input (the caller's: the kernel's own on
        the GPU, the float32 reference's on the CPU), or the synthetic plane"""
        assert which in MASKS
        if which == "none":
            return None
        if which == "own forward":
            return own_forward.detach().cpu()
        return synthetic_mask_plane(self.gy.shape)

    def bwd_expect(self, yc):
        H, W = self.shape[2:]
        ref = resample_bwd_ref(self.gy, yc, (H, W), self.rect, self.out, self.kind)
        g32 = self.gy if yc is None else self.gy * clamp_mask(yc)
        xr = torch.zeros_like(self._inside(self.x)).requires_grad_(True)
        (gi,) = torch.autograd.grad(self._interp32(xr), xr, g32)
        gx32 = torch.zeros(self.shape, dtype=torch.float32)
        h0, hs, w0, ws = self.rect
        gx32[:, :, h0:h0 + hs, w0:w0 + ws] = gi
        return (ref,) + _tolerance(gx32, ref)

    def check_bwd(self, gx, yc, what=""):
        ref, tol, dev32 = self.bwd_expect(yc)
        what = "%s bwd %s" % (self.label, what)
        dev = _deviation(gx, ref, what)
        stray = int((gx.detach().cpu()[:, :, self.outside] != 0).sum())
        assert stray == 0, "%s: %d pixels outside the rectangle are not exactly 0" % (what, stray)
        return Report(what, dev, tol, dev32).assert_ok()


@functools.lru_cache(maxsize=None)
def resample_case(name, kind):
    i = RESAMPLE_NAMES.index(name)
    _, shape, rect, out, _ = RESAMPLE_ROWS[i]
    return ResampleCase(name, shape, rect, out, kind, 4100 + 10 * i)


@functools.lru_cache(maxsize=None)
def crop_layer_case():
    """Crop on 32 x 32 with a 10 x 10 rectangle: 3.2x, bilinear, the y pass's overflow loop through the layer's autograd"""
    return ResampleCase("Crop layer", (2, 3, 32, 32), (11, 10, 7, 10), (32, 32), BILINEAR, 4400)


class ResizeCase:
    """Resize(ratio) on a saturated image: down (or up) to int(r H) x int(r W), back, clamp.  The mask of the backward is where the
    float64 result lies strictly inside (0, 1); `margin` is the distance of the nearest UNCLAMPED float64 output from 0 or 1, which
    must exceed the tolerance for that mask to be the only right one (a seed where it does not is replaced, not tolerated)."""

    def __init__(self, shape, ratio, seed):
        B, C, H, W = shape
        self.shape, self.ratio, self.kind = tuple(shape), ratio, BICUBIC
        self.mid = (int(ratio * H), int(ratio * W))
        self.x = (3 * detgen.uniform(shape, seed) - 1).clamp(0, 1)
        self.gy = detgen.normal(shape, seed + 1)
        nh, nw = self.mid
        A = (axis_matrix(nh, H, BICUBIC), axis_matrix(nw, W, BICUBIC), axis_matrix(H, nh, BICUBIC), axis_matrix(W, nw, BICUBIC))
        u = A[2] @ (A[0] @ self.x.double() @ A[1].T) @ A[3].T
        self.y64 = u.clamp(0.0, 1.0)
        self.margin = float(torch.minimum(u.abs(), (u - 1.0).abs()).min())
        mask = (u > 0) & (u < 1)
        self.gx64 = A[0].T @ (A[2].T @ (self.gy.double() * mask) @ A[3]) @ A[1]
        xr = self.x.clone().requires_grad_(True)
        u32 = F.interpolate(F.interpolate(xr, size=self.mid, mode="bicubic", align_corners=False), size=(H, W), mode="bicubic", align_corners=False)
        (gx32,) = torch.autograd.grad(u32, xr, self.gy * mask)
        self.tol_y, self.dev_y = _tolerance(u32.detach().clamp(0, 1), self.y64)
        self.tol_g, self.dev_g = _tolerance(gx32, self.gx64)
        self.margin_needed = max(self.tol_y, FACTOR * float((u32.detach().double() - u).abs().max()))
        self.label = "Resize layer %.1f" % ratio

    def check(self, y, gx):
        ry = Report(self.label + " y", _deviation(y, self.y64, self.label), self.tol_y, self.dev_y, "  margin %.3e" % self.margin)
        rg = Report(self.label + " gx", _deviation(gx, self.gx64, self.label), self.tol_g, self.dev_g)
        return ry.assert_ok(), rg.assert_ok()


RESIZE_SHAPE = (2, 3, 32, 40)
RESIZE_SEEDS = {0.5: 4500, 1.5: 4530}      # both pass the margin check (tests/test_cpu_attacks_exact.py asserts it); 4510 and 4520 were
                                           # replaced for ratio 1.5: an unclamped output within 8e-6 resp. 2e-5 of the clamp, tolerance 1.3e-5


@functools.lru_cache(maxsize=None)
def resize_layer_case(ratio):
    return ResizeCase(RESIZE_SHAPE, ratio, RESIZE_SEEDS[ratio])


# ----------------------------------------------------------------------------------------------------------------- stencil
STENCIL_SHAPES = ((1, 1, 1, 1), (1, 2, 1, 9), (1, 2, 7, 1), (2, 3, 5, 256), (1, 2, 3, 257), (1, 1, 4, 600))
STENCIL_BWD_SHAPE = (1, 2, 3, 257)


def _w9(w9):
    w = np.asarray([float(v) for v in w9], dtype=np.float32).astype(np.float64)     # the kernel's arguments are float32
    assert w.shape == (9,)
    return w


def asymmetric_w9(seed=4600):
    w = detgen.normal((9,), seed)
    assert len(set(w.tolist())) == 9 and not torch.equal(w.view(3, 3), w.view(3, 3).t())
    return w.tolist()


def stencil3_ref(x, w9):
    """float64 cross-correlation, zero padding 1 (F.conv2d(groups=C) with the same 3 x 3 for every channel): nine shifted adds"""
    w = _w9(w9)
    H, W = x.shape[2:]
    xp = F.pad(x.double(), (1, 1, 1, 1))
    y = torch.zeros(x.shape, dtype=torch.float64)
    for a in range(3):
        for b in range(3):
            y += w[3 * a + b] * xp[:, :, a:a + H, b:b + W]
    return y


def stencil3_bwd_ref(gy, w9):
    """the float64 transpose of stencil3_ref, in scatter form: output (h, w) hands w[a, b] gy[h, w] to input (h + a - 1, w + b - 1),
    and what lands in the padding is dropped"""
    w = _w9(w9)
    H, W = gy.shape[2:]
    gp = torch.zeros(gy.shape[0], gy.shape[1], H + 2, W + 2, dtype=torch.float64)
    for a in range(3):
        for b in range(3):
            gp[:, :, a:a + H, b:b + W] += w[3 * a + b] * gy.double()
    return gp[:, :, 1:H + 1, 1:W + 1]


def _check_per_pixel(what, got, ref, bound):
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32, (what, tuple(got.shape), got.dtype)
    err = (got.detach().cpu().double() - ref).abs()
    bad = ~(err <= bound)
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert not bool(bad.any()), "%s: %d pixels beyond the bound, worst %.3f of it (largest error %.3e)" % (what, int(bad.sum()), worst, float(err.max()))
    return "%-46s largest error %.3e = %.3f of the per-pixel bound" % (what, float(err.max()), worst)


def check_stencil(x, w9, y, what="stencil"):
    """16 * 2**-24 * (|w| * |x|) per pixel: nine products and eight adds in float32, whatever their order or contraction"""
    absw = [abs(float(v)) for v in w9]
    return _check_per_pixel(what, y, stencil3_ref(x, w9), 16 * EPS32 * stencil3_ref(x.abs(), absw))


def check_stencil_bwd(gy, w9, gx, what="stencil bwd"):
    absw = [abs(float(v)) for v in w9]
    return _check_per_pixel(what, gx, stencil3_bwd_ref(gy, w9), 16 * EPS32 * stencil3_bwd_ref(gy.abs(), absw))


# ----------------------------------------------------------------------------------------------------------------- median
MEDIAN_SHAPES = ((1, 1, 1, 1), (1, 2, 2, 4), (1, 2, 4, 3), (1, 1, 1, 12),       # H or W smaller than k
                 (1, 2, 8, 4), (3, 2, 5, 12),                                  # W % 4 == 0: the four-pixel kernels
                 (2, 3, 17, 23),                                               # the one-pixel kernels
                 (1, 2, 3, 259),                                               # ... across two column blocks
                 (1, 1, 40, 1032))                                             # aligned, and shifted by one float (the one-pixel kernels)
MEDIAN_SHIFTED = ((1, 1, 40, 1032),)
MEDIAN_DATA = ("continuous", "five levels", "two levels", "saturated", "constant")


@functools.lru_cache(maxsize=None)
def median_input(shape, data):
    u = detgen.uniform(shape, 4700 + MEDIAN_SHAPES.index(shape))
    return {"continuous": u, "five levels": torch.round(u * 4) / 4, "two levels": torch.round(u), "saturated": (u * 3 - 1).clamp(0, 1),
            "constant": torch.full(shape, 0.25)}[data]


@functools.lru_cache(maxsize=None)
def median_gy(shape):
    return detgen.normal(shape, 4750 + MEDIAN_SHAPES.index(shape))


def median_taps(x, k):
    """[B, C, k*k, H, W]: tap t of output (h, w) is x[h + t // k - k // 2, w + t % k - k // 2], 0 outside the image"""
    H, W = x.shape[2:]
    p = k // 2
    xp = F.pad(x, (p, p, p, p))
    return torch.stack([xp[:, :, t // k:t // k + H, t % k:t % k + W] for t in range(k * k)], dim=2)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def median_routing_check(x, y, idx, k):
    """(y, idx) is A median of the zero-padded k x k window and a tap that holds it, for every pixel, whichever way ties were broken"""
    x, y, idx = x.detach().cpu(), y.detach().cpu(), idx.detach().cpu().long()
    K2 = k * k
    assert tuple(y.shape) == tuple(x.shape) == tuple(idx.shape)
    assert int(idx.min()) >= 0 and int(idx.max()) < K2, "tap index outside [0, %d): min %d max %d" % (K2, int(idx.min()), int(idx.max()))
    taps = median_taps(x, k)
    named = taps.gather(2, idx.unsqueeze(2)).squeeze(2)
    wrong = int((_bits(named) != _bits(y)).sum())
    assert wrong == 0, "%d pixels whose idx names a tap that is not y bit for bit" % wrong
    below = (taps < y.unsqueeze(2)).sum(2)
    upto = (taps <= y.unsqueeze(2)).sum(2)
    notmed = int(((below > K2 // 2) | (upto <= K2 // 2)).sum())
    assert notmed == 0, "%d pixels whose y is not a median of its window" % notmed


def median_bwd_ref(gy, idx, k):
    """float64 scatter of gy to the tap idx names; a tap in the padding receives nothing"""
    gy, idx = gy.detach().cpu().double(), idx.detach().cpu()
    H, W = gy.shape[2:]
    p = k // 2
    gp = torch.zeros(gy.shape[0], gy.shape[1], H + 2 * p, W + 2 * p, dtype=torch.float64)
    for t in range(k * k):
        gp[:, :, t // k:t // k + H, t % k:t % k + W] += gy * (idx == t)
    return gp[:, :, p:p + H, p:p + W]


def check_median_bwd(gy, idx, k, gx, what="median bwd"):
    """k*k * 2**-24 * the sum of |gy| routed to the pixel: at most k*k terms, added in any order"""
    return _check_per_pixel(what, gx, median_bwd_ref(gy, idx, k), k * k * EPS32 * median_bwd_ref(gy.abs(), idx, k))


# ----------------------------------------------------------------------------------------------------------------- quantisers
def quant_inputs():
    """every level k/255 and half-way point (k + 0.5)/255 formed in float32, the float32 neighbours either side of each, +-0, values
    outside [0, 1] and just outside it"""
    k = np.arange(256, dtype=np.float32)
    pts = np.concatenate([k / np.float32(255), (k + np.float32(0.5)) / np.float32(255)]).astype(np.float32)
    one, zero = np.float32(1), np.float32(0)
    edge = np.array([0.0, -0.0, -0.2, 1.2, np.nextafter(zero, -one), -2.0 ** -126, 2.0 ** -126, -1e-6, np.nextafter(one, np.float32(2)),
                     1.0 + 1e-6, -0.5 / 255, 255.5 / 255, 256.5 / 255], dtype=np.float32)
    base = np.concatenate([pts, edge])
    return np.concatenate([base, np.nextafter(base, np.float32(-np.inf)), np.nextafter(base, np.float32(np.inf))]).astype(np.float32)


def quant_ref(x):
    x = np.asarray(x, dtype=np.float32)
    y = np.rint(x * np.float32(255)) / np.float32(255)
    assert y.dtype == np.float32
    return y


def clamp_quant_ref(x):
    """the clamp is IEEE 754-2019 maximum / minimum (-0 < +0, so -0 clamps to +0: what torch.clamp gives on the device)"""
    x = np.asarray(x, dtype=np.float32)
    c = np.where(x > 0, x, np.float32(0))
    c = np.where(c < 1, c, np.float32(1)).astype(np.float32)
    return quant_ref(c)


def assert_same_bits(got, ref, x, what):
    got = np.ascontiguousarray(got, dtype=np.float32) if not torch.is_tensor(got) else got.detach().cpu().contiguous().numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape)
    bad = np.nonzero(got.view(np.int32) != ref.view(np.int32))[0]
    assert bad.size == 0, "%s: %d of %d values differ, first x = %r (x * 255 = %r): got %r, expected %r" % (
        what, bad.size, ref.size, float(x[bad[0]]), float(x[bad[0]] * np.float32(255)), float(got[bad[0]]), float(ref[bad[0]]))
