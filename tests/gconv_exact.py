"""Float64 restatements of the general convolution family (csrc/gconv.hip: wm_gconv_fwd / _dil_fwd, wm_gconv_wgrad / _dil_wgrad,
wm_gconv_pack, wm_gcolsum, wm_gcolsum_f64), written from the three formulas at the top of that file and from include/wm_hip.h as plain
loops over the filter taps on numpy float64 arrays, with the case tables and the per-element comparisons built on them.  A plain helper
module (no fixtures, CPU only, never imports the HIP package): tests/test_cpu_gconv_exact.py runs float32 imitations -- faithful and
defective -- through these comparisons, tests/test_gpu_gconv_exact.py runs the kernels through them.

    forward : out[b,oy,ox,n] = bias[n] + sum_{ky,kx,k} in[b, oy*s - p + ky*d, ox*s - p + kx*d, k] * w[n,k,ky,kx]
    dgrad   : din[b,iy,ix,k] = sum_{ky,kx,n} dout[b, (iy + p - ky*d)/s, (ix + p - kx*d)/s, n] * w[n,k,ky,kx]   (integer, in-range sources
              only; with a bias this is ConvTranspose2d's forward)
    wgrad   : dw[n,k,ky,kx] (+)= sum_{b,oy,ox} dout[b,oy,ox,n] * in[b, oy*s - p + ky*d, ox*s - p + kx*d, k],  dbias[n] (+)= sum dout[.,n]

Every restatement returns, next to the value, the sum of the absolute values of its terms and the number of non-zero terms per output
element (from |x| and |w|).  Operands are the values as stored: rounded to the dtype with rnd() before anything is computed from them.

Data.  GRID cases draw activations, filters and gradients as multiples of 1/4 in [-1, 1] and the bias (and whatever a gradient is
accumulated onto) as multiples of 1/16 -- exact in f32, bf16 and f16.  Every product is a multiple of 1/16, so every partial sum of any
subset of the terms is a multiple of UNIT = 1/16 and, as long as sum|terms| < 2**20 UNIT (asserted per case, grid_units()), is held exactly
by a float32: any order of accumulation, any split, any adder tree gives the exact result.  (The column sums add multiples of 1/4 only and
count in that unit.)  There the bound is 0 for every float32 quantity and half_ulp(ref, dt), nothing more, for a 16-bit stored output.
GENERIC cases (one per kernel path, normal data): a result of n non-zero terms takes at most n roundings to form in ANY order -- the
products of 16-bit operands are exact in float32, a float32 product is one rounding on its own term, and n terms (bias or prior value
included) take n - 1 additions; counted as n + 1 -- so it is accepted within FACTOR * (n + 1) * EPS32 * sum|terms|, plus half_ulp for a
16-bit store.  wm_gcolsum_f64 sums in double: DBL * sum|terms| plus the one float32 rounding of the result, EPS32 * |ref|.
No bound is picked and none comes from a kernel's output; there are no masks in this family, so no comparison may skip an element.

Paths.  Every case names the kernel path it is there for, and check_path() verifies it from restatements of the host's dispatch
arithmetic (wgrad_nsplit = wm_gconv_wgrad_nsplit, wgrad16_nsplit, thin_nsplit, thin_ok, the reduce's split lanes, colsum_nsplit).
"""
import functools

import numpy as np

from layers_exact import Cmp, rnd, store, f64, grid, pick, normal, EPS32, DBL, FACTOR, HALF_ULP, half_ulp

DTYPES = ("f32", "bf16", "f16")
DT16 = ("bf16", "f16")
UNIT = 1.0 / 16
MAX_UNITS = 2.0 ** 20
MAX_BYTES = 8 << 20
ESZ = {"f32": 4, "bf16": 2, "f16": 2}
KSTEP = {"f32": 4, "bf16": 32, "f16": 32}                  # channels of one MFMA step
WG_TAPS = 8                                               # taps of one workgroup of gconv_wgrad16_kernel
THIN_MAXT = 7
# channel strides of the input tensor by dtype family (f32, 16 bit): the krem tail of a 32-channel step is 16 or 48 in 16 bit
K0, K1, K2 = (4, 16), (20, 48), (64, 64)


def kc_of(KC, dt):
    return KC if isinstance(KC, int) else KC[0 if dt == "f32" else 1]


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------------------------------------------- host arithmetic
def wgrad_nsplit(B, OH, OW, KC, NC, KH, KW):
    """wm_gconv_wgrad_nsplit: pixel splits of the f32 kernel"""
    npix = B * OH * OW
    jobs = KH * KW * (NC // 16) * cdiv(KC, 16)
    ns = cdiv(4096, jobs) if jobs > 0 else 1
    return max(1, min(ns, cdiv(npix, 256), 256))


def wgrad16_nsplit(B, OH, OW, KC, NC, KH, KW):
    chunks = cdiv(B * OH * OW, 64)
    jobs = cdiv(NC, 64) * cdiv(KC, 64) * cdiv(KH * KW, WG_TAPS)
    ns = min(cdiv(2048 if jobs < 16 else 1024, jobs), 1024, cdiv(chunks, 4))
    return max(ns, 1)


def thin_ok(KC, NC, KH, KW, stride):
    return KC == 16 and NC % 16 == 0 and KH * KW <= 4 * THIN_MAXT and stride in (1, 2)


def thin_nsplit(B, OH, OW):
    return max(1, min(cdiv(B * OH * cdiv(OW, 64), 8), 1024))


def split_lanes(nsplit):
    """SL of gconv_wreduce_kernel"""
    return 16 if nsplit >= 64 else 4 if nsplit >= 8 else 1


def colsum_nsplit(npix):
    return max(1, min(cdiv(npix, 256), 512))


def wgrad_dispatch(dt, B, OH, OW, KC, NC, KH, KW, stride, dil):
    """(kernel, nsplit, SL) as gconv_wgrad_impl chooses them"""
    if dt == "f32":
        kern, ns = "f32", wgrad_nsplit(B, OH, OW, KC, NC, KH, KW)
    elif dil == 1 and thin_ok(KC, NC, KH, KW, stride):
        kern, ns = "thin", thin_nsplit(B, OH, OW)
    else:
        kern, ns = "wgrad16", wgrad16_nsplit(B, OH, OW, KC, NC, KH, KW)
    return kern, ns, split_lanes(ns)


def fwd_dispatch(dgrad, B, IH, IW, OH, OW, NC, KH, KW, stride, pad):
    """the forward entry points' paths: "linear", or the blocks' forms with the pixel walk"""
    npix = B * OH * OW
    if KH == 1 and KW == 1 and stride == 1 and pad == 0 and npix <= 32 and IH == OH and IW == OW:
        return {"linear"}
    forms = {"narrow" if NC - n0 <= 16 else "wide" for n0 in range(0, NC, 64)}
    if dgrad and stride == 2:
        forms.add("parity" if not ((OH | OW) & 1) else "general")
    return forms


# ----------------------------------------------------------------------------------------------------------------- restatements
def _axis(n_out, n_in, stride, pad, off, dgrad):
    """along one axis: the source index of each of n_out output positions under a tap at offset `off` (= tap index * dilation), and
    whether it exists"""
    o = np.arange(n_out)
    if not dgrad:
        s = o * stride - pad + off
        ok = (s >= 0) & (s < n_in)
    else:
        t = o + pad - off
        s = t // stride
        ok = (t >= 0) & (t % stride == 0) & (s < n_in)
    return np.where(ok, s, 0), ok


def _patch(x, OH, OW, stride, pad, dil, ky, kx, dgrad):
    """x [B,IH,IW,K] -> [B,OH,OW,K]: the source pixel of every output pixel under tap (ky, kx), zero where there is none"""
    sy, vy = _axis(OH, x.shape[1], stride, pad, ky * dil, dgrad)
    sx, vx = _axis(OW, x.shape[2], stride, pad, kx * dil, dgrad)
    return x[:, sy][:, :, sx] * (vy[:, None] & vx[None, :])[None, :, :, None]


def conv64(x, w, bias, OH, OW, stride, pad, dil, dgrad):
    """x [B,IH,IW,K] float64; w the layer's weight in torch's layout: [N,K,KH,KW] forward, [K,N,KH,KW] for the input gradient /
    ConvTranspose2d (K = the channels of x either way); bias [N] or None -> value, sum|terms|, non-zero terms, each [B,OH,OW,N]"""
    KH, KW = w.shape[2:]
    N = w.shape[1] if dgrad else w.shape[0]
    out = np.zeros((x.shape[0], OH, OW, N))
    ab, cnt = np.zeros_like(out), np.zeros_like(out)
    for ky in range(KH):
        for kx in range(KW):
            p = _patch(x, OH, OW, stride, pad, dil, ky, kx, dgrad)
            m = w[:, :, ky, kx] if dgrad else w[:, :, ky, kx].T                      # [K, N]
            out += p @ m
            ab += np.abs(p) @ np.abs(m)
            cnt += (p != 0).astype(np.float64) @ (m != 0).astype(np.float64)
    if bias is not None:
        out += bias
        ab += np.abs(bias)
        cnt += (bias != 0)
    return out, ab, cnt


def wgrad64(dout, x, KH, KW, stride, pad, dil):
    """dout [B,OH,OW,N], x [B,IH,IW,K] -> dw [N,K,KH,KW], sum|terms|, non-zero terms"""
    N, K = dout.shape[3], x.shape[3]
    OH, OW = dout.shape[1:3]
    dw = np.zeros((N, K, KH, KW))
    ab, cnt = np.zeros_like(dw), np.zeros_like(dw)
    d2 = dout.reshape(-1, N)
    for ky in range(KH):
        for kx in range(KW):
            p = _patch(x, OH, OW, stride, pad, dil, ky, kx, False).reshape(-1, K)
            dw[:, :, ky, kx] = d2.T @ p
            ab[:, :, ky, kx] = np.abs(d2).T @ np.abs(p)
            cnt[:, :, ky, kx] = (d2 != 0).astype(np.float64).T @ (p != 0).astype(np.float64)
    return dw, ab, cnt


def colsum64(x):
    """x [npix, C] -> column sums, sum|terms|, non-zero terms (also the bias gradient of dout)"""
    return x.sum(0), np.abs(x).sum(0), (x != 0).sum(0).astype(np.float64)


def pack64(w, RP, CP, transpose, dt):
    """w [Cout,Cin,KH,KW] -> [KH*KW][RP][CP]: rows Cout, columns Cin (transpose: swapped), rounded to dt, zero padding"""
    Cout, Cin, KH, KW = w.shape
    m = rnd(w, dt).reshape(Cout, Cin, KH * KW).transpose(2, 0, 1)
    if transpose:
        m = m.transpose(0, 2, 1)
    out = np.zeros((KH * KW, RP, CP))
    out[:, :m.shape[1], :m.shape[2]] = m
    return out


def grid_units(absum, unit=UNIT):
    """largest sum|terms| of a GRID case in grid units: below 2**20, every partial sum is an exact float32"""
    return float(np.max(absum)) / unit if np.size(absum) else 0.0


def n_bound(n, absum):
    """any-order float32 evaluation of n non-zero terms"""
    return FACTOR * (n + 1) * EPS32 * absum


def data(shape, seed, kind, dt, step=0.25):
    return grid(shape, seed, step, -1.0, 1.0) if kind == "grid" else rnd(normal(shape, seed), dt)


# ----------------------------------------------------------------------------------------------------------------- forward / dgrad
class FwdSpec:
    """one forward (dgrad 0) or input-gradient / transposed (dgrad 1) layer.  `in` is [B,IH,IW,KC] with Kr real channels, the output
    [B,OH,OW,NC] with Nr real channels; OH, OW follow from the geometry (`extra`: the transposed grid one larger, the row the forward
    floor division dropped).  entry: "plain" (ops.gconv_fwd, dilation passed on when it is not 1) or "dil" (ops.gconv_dil_fwd)."""

    def __init__(self, path, dgrad, B, IH, IW, Kr, KC, Nr, NC, k, s, p, d=1, bias=True, extra=0, kind="grid", entry="plain", npix=None):
        self.path, self.dgrad, self.B, self.IH, self.IW, self.Kr, self.KC, self.Nr, self.NC = path, dgrad, B, IH, IW, Kr, KC, Nr, NC
        self.KH, self.KW = (k, k) if isinstance(k, int) else k
        self.s, self.p, self.d, self.bias, self.extra, self.kind, self.entry = s, p, d, bias, extra, kind, entry
        eh, ew = (self.KH - 1) * d + 1, (self.KW - 1) * d + 1
        if dgrad:
            self.OH, self.OW = (IH - 1) * s - 2 * p + eh + extra, (IW - 1) * s - 2 * p + ew + extra
        else:
            self.OH, self.OW = (IH + 2 * p - eh) // s + 1, (IW + 2 * p - ew) // s + 1
        self.npix = B * self.OH * self.OW
        assert npix is None or npix == self.npix, (path, npix, self.npix)

    def label(self, dt):
        return "%s %s %dx%dx%d %d(%d)->%d(%d) k%dx%d s%d p%d d%d%s%s -> %dx%d [%s]%s" % (
            "dgrad" if self.dgrad else "fwd", dt, self.B, self.IH, self.IW, self.Kr, kc_of(self.KC, dt), self.Nr, self.NC, self.KH, self.KW,
            self.s, self.p, self.d, " bias" if self.bias else "", " dil-entry" if self.entry == "dil" else "", self.OH, self.OW, self.path,
            "" if self.kind == "grid" else " generic")


F, G = 0, 1
FWD_SPECS = (
    # forward: every NC form, the KC tails, ragged channels, the pixel counts 5 / 16 / 63 / 65 / 3*7*5, k 1..5, stride 1 / 2, pad 0 / 1 / 2 / 4
    FwdSpec("narrow", F, 1, 1, 5, 3, K0, 3, 16, 3, 1, 1, npix=5),
    FwdSpec("wide", F, 1, 4, 4, 7, K1, 40, 48, 3, 1, 1, bias=False, npix=16),
    FwdSpec("wide", F, 1, 14, 18, 40, K2, 64, 64, 4, 2, 1, npix=63),
    FwdSpec("wide+narrow", F, 1, 5, 13, 5, K1, 70, 80, 5, 1, 2, npix=65),
    FwdSpec("wide+narrow", F, 3, 14, 10, 64, K2, 130, 144, 2, 2, 0, bias=False, npix=105),
    FwdSpec("wide", F, 2, 9, 20, 3, K0, 5, 64, 3, 1, 4),                                 # pad 4 > half-width: rows 0, 1 have no source at all
    FwdSpec("narrow", F, 2, 9, 7, 7, K1, 7, 16, 1, 2, 0),
    FwdSpec("wide", F, 1, 11, 40, 40, K2, 40, 48, 5, 2, 2),
    FwdSpec("wide+narrow", F, 1, 4, 6, 3, K0, 130, 144, 2, 1, 1),
    FwdSpec("wide+narrow", F, 1, 6, 9, 40, K2, 80, 80, 4, 1, 2, bias=False),
    FwdSpec("wide", F, 2, 9, 11, 40, K2, 64, 64, 3, 1, 2, d=2),                          # dilation through gconv_fwd(dilation=)
    FwdSpec("wide+narrow", F, 1, 8, 13, 7, K1, 70, 80, 3, 1, 3, d=3, entry="dil"),       # ... and through gconv_dil_fwd
    FwdSpec("narrow", F, 1, 20, 21, 3, K0, 3, 16, 3, 1, 4, d=8),
    FwdSpec("wide", F, 1, 4, 4, 7, K1, 40, 48, 3, 1, 1, entry="dil"),                    # dilation 1 through the dilated entry point
    # the linear path (1x1, <= 32 pixels) and the same layers one pixel count later, on the MFMA kernel
    FwdSpec("linear", F, 1, 1, 1, 10, 16, 10, 16, 1, 1, 0, npix=1),
    FwdSpec("linear", F, 2, 4, 4, 70, 80, 40, 48, 1, 1, 0, bias=False, npix=32),
    FwdSpec("linear", F, 2, 4, 4, 500, 512, 70, 80, 1, 1, 0, npix=32),
    FwdSpec("wide+narrow", F, 3, 1, 11, 500, 512, 70, 80, 1, 1, 0, npix=33),
    FwdSpec("linear", G, 1, 1, 1, 10, 16, 10, 16, 1, 1, 0, bias=False, npix=1),
    FwdSpec("linear", G, 2, 4, 4, 70, 80, 40, 48, 1, 1, 0, npix=32),
    FwdSpec("linear", G, 2, 4, 4, 500, 512, 70, 80, 1, 1, 0, bias=False, npix=32),
    FwdSpec("wide+narrow", G, 3, 1, 11, 500, 512, 70, 80, 1, 1, 0, bias=False, npix=33),
    # input gradient / ConvTranspose2d: the parity walk (class size npix / 4 no multiple of 16), the general walk, the dropped row
    FwdSpec("narrow+parity", G, 1, 3, 5, 64, K2, 3, 16, 4, 2, 1, bias=False, npix=60),   # 6x10: classes of 15, wave 0 holds two
    FwdSpec("wide+narrow+parity", G, 2, 5, 7, 7, K1, 70, 80, 4, 2, 1, npix=280),         # classes of 70
    FwdSpec("narrow+parity", G, 2, 3, 4, 40, K2, 7, 16, 3, 2, 1, bias=False, extra=1),   # 6x8 through the dropped row: classes of 24
    FwdSpec("wide+parity", G, 1, 4, 4, 40, K2, 40, 48, 2, 2, 0, npix=64),                # ConvTranspose2d(2, 2): classes of 16
    FwdSpec("wide+general", G, 1, 4, 5, 3, K0, 64, 64, 3, 2, 1, bias=False, npix=63),    # 7x9: odd
    FwdSpec("wide+general", G, 1, 3, 5, 7, K1, 40, 48, 4, 2, 1, extra=1),                # 7x11: the dropped row, odd
    FwdSpec("narrow+general", G, 2, 5, 4, 5, K1, 5, 16, 1, 2, 0, bias=False),            # 9x7
    FwdSpec("wide+narrow", G, 3, 7, 5, 40, K2, 130, 144, 3, 1, 1, bias=False, npix=105),
    FwdSpec("wide+narrow", G, 1, 5, 13, 3, K0, 70, 80, 5, 1, 2, npix=65),
    FwdSpec("wide", G, 1, 12, 14, 7, K1, 64, 64, 3, 1, 4, bias=False),                   # pad 4: 6x8
    FwdSpec("wide", G, 2, 9, 11, 40, K2, 64, 64, 3, 1, 2, d=2, bias=False),
    FwdSpec("narrow", G, 1, 8, 13, 7, K1, 5, 16, 3, 1, 3, d=3, bias=False, entry="dil"),
    FwdSpec("wide+narrow", G, 1, 20, 21, 3, K0, 70, 80, 3, 1, 4, d=8, bias=False),
    # GENERIC: one per path
    FwdSpec("wide+narrow", F, 1, 5, 13, 5, K1, 70, 80, 5, 1, 2, kind="normal"),
    FwdSpec("wide+narrow", F, 1, 8, 13, 7, K1, 70, 80, 3, 1, 3, d=3, entry="dil", kind="normal"),
    FwdSpec("linear", F, 2, 4, 4, 500, 512, 70, 80, 1, 1, 0, kind="normal"),
    FwdSpec("wide+narrow+parity", G, 2, 5, 7, 7, K1, 70, 80, 4, 2, 1, kind="normal"),
    FwdSpec("wide+general", G, 1, 3, 5, 7, K1, 40, 48, 4, 2, 1, extra=1, kind="normal"),
    FwdSpec("linear", G, 2, 4, 4, 70, 80, 40, 48, 1, 1, 0, kind="normal"),
)


class FwdCase:
    def __init__(self, i, dt):
        self.spec = sp = FWD_SPECS[i]
        self.dt, self.KC = dt, kc_of(sp.KC, dt)
        self.Kr = min(sp.Kr, self.KC)
        self.label = sp.label(dt)
        seed = 7000 + 31 * i
        # the input's padding channels hold values too: the filter's padding columns are zero, so nothing of them may arrive
        self.x = data((sp.B, sp.IH, sp.IW, self.KC), seed, sp.kind, dt)
        wshape = (self.Kr, sp.Nr, sp.KH, sp.KW) if sp.dgrad else (sp.Nr, self.Kr, sp.KH, sp.KW)
        self.w = data(wshape, seed + 1, sp.kind, dt)                       # float32 values that are exact in dt: the pack rounds nothing
        self.bias = (grid((sp.Nr,), seed + 2, UNIT, -1.0, 1.0) if sp.kind == "grid" else rnd(normal((sp.Nr,), seed + 2), "f32")) if sp.bias else None
        self.wp = pack64(self.w, sp.NC, self.KC, bool(sp.dgrad), dt)       # [taps][NC][KC]
        self.bias_p = None
        if sp.bias:
            self.bias_p = np.zeros(sp.NC)
            self.bias_p[:sp.Nr] = self.bias
        self.ref, self.absum, self.count = conv64(self.x[..., :self.Kr], self.w, self.bias, sp.OH, sp.OW, sp.s, sp.p, sp.d, bool(sp.dgrad))
        self.units = grid_units(self.absum) if sp.kind == "grid" else 0.0
        self.bound = half_ulp(self.ref, dt) + (0.0 if sp.kind == "grid" else n_bound(self.count, self.absum))
        for t in (self.x, self.ref):
            assert t.size * ESZ[dt] <= MAX_BYTES, self.label

    def paths(self):
        sp = self.spec
        return fwd_dispatch(sp.dgrad, sp.B, sp.IH, sp.IW, sp.OH, sp.OW, sp.NC, sp.KH, sp.KW, sp.s, sp.p)

    def check_path(self):
        assert self.paths() == set(self.spec.path.split("+")), (self.label, self.paths())

    def check(self, out, what=""):
        sp = self.spec
        o = f64(out).reshape(sp.B, sp.OH, sp.OW, sp.NC)
        cm = [Cmp(self.label + what, o[..., :sp.Nr], self.ref, self.bound)]
        if sp.NC > sp.Nr:
            cm.append(Cmp(self.label + what + " padding channels", o[..., sp.Nr:], np.zeros(o[..., sp.Nr:].shape)))
        return cm


@functools.lru_cache(maxsize=None)
def fwd_case(i, dt):
    return FwdCase(i, dt)


def fwd_index(path, dgrad, kind="grid", **kw):
    """the first spec of that path / direction (and further attributes)"""
    return next(i for i, s in enumerate(FWD_SPECS) if s.path == path and s.dgrad == dgrad and s.kind == kind and
                all(getattr(s, k) == v for k, v in kw.items()))


# ----------------------------------------------------------------------------------------------------------------- weight gradient
class WSpec:
    """one weight / bias gradient: x [B,IH,IW,KC] (Kr real), dout [B,OH,OW,NC] (Nr real).  dts: the dtypes it runs in; kernel, SL: the
    path it is there for"""

    def __init__(self, kernel, SL, dts, B, IH, IW, Kr, KC, Nr, NC, k, s, p, d=1, kind="grid", nsplit=None, why=""):
        self.kernel, self.SL, self.dts, self.B, self.IH, self.IW, self.Kr, self.KC, self.Nr, self.NC = kernel, SL, dts, B, IH, IW, Kr, KC, Nr, NC
        self.KH, self.KW = (k, k) if isinstance(k, int) else k
        self.s, self.p, self.d, self.kind, self.nsplit, self.why = s, p, d, kind, nsplit, why
        self.OH = (IH + 2 * p - (self.KH - 1) * d - 1) // s + 1
        self.OW = (IW + 2 * p - (self.KW - 1) * d - 1) // s + 1
        self.npix = B * self.OH * self.OW

    def dispatch(self, dt):
        return wgrad_dispatch(dt, self.B, self.OH, self.OW, self.KC, self.NC, self.KH, self.KW, self.s, self.d)

    def label(self, dt):
        return "wgrad %s %dx%dx%d->%dx%d %d(%d)->%d(%d) k%dx%d s%d p%d d%d [%s, %d splits, SL %d]%s" % (
            dt, self.B, self.IH, self.IW, self.OH, self.OW, self.Kr, self.KC, self.Nr, self.NC, self.KH, self.KW, self.s, self.p, self.d,
            self.kernel, self.dispatch(dt)[1], self.SL, "" if self.kind == "grid" else " generic")


F32, B16 = ("f32",), DT16
WGRAD_SPECS = (
    # the f32 kernel
    WSpec("f32", 1, F32, 2, 8, 8, 7, 20, 5, 16, 3, 1, 1, nsplit=1, why="one split (128 pixels); KC = 20: the kok tail"),
    WSpec("f32", 4, F32, 3, 30, 35, 3, 4, 3, 16, 3, 1, 1, nsplit=13, why="13 splits of 243 pixels: boundaries off the 16-pixel step"),
    WSpec("f32", 16, F32, 1, 128, 128, 16, 16, 16, 16, 1, 1, 0, nsplit=64, why="64 splits"),
    WSpec("f32", 1, F32, 2, 12, 10, 40, 64, 40, 48, 4, 2, 1, nsplit=1, why="stride 2, Cout < NC, Cin < KC"),
    WSpec("f32", 1, F32, 1, 20, 20, 7, 20, 70, 80, 3, 1, 2, d=2, nsplit=2, why="dilation 2, two splits of 200"),
    # gconv_wgrad16_kernel: taps 1 / 8 / 9 / 25, NC, KC in {32, 64, 80}, npix % 64 != 0, the three SL classes, dilation
    WSpec("wgrad16", 16, B16, 2, 92, 89, 20, 32, 20, 32, 1, 1, 0, nsplit=64, why="1 tap; 256 chunks (the last of 56 pixels) in 64 splits"),
    WSpec("wgrad16", 4, B16, 3, 40, 39, 64, 64, 64, 64, 3, 1, 1, nsplit=19, why="9 taps: a second group of one; 74 chunks in 19 splits"),
    WSpec("wgrad16", 1, B16, 1, 10, 13, 20, 32, 70, 80, (2, 4), 1, 1, nsplit=1, why="8 taps: one full group; 132 pixels"),
    WSpec("wgrad16", 1, B16, 1, 9, 7, 70, 80, 20, 32, 5, 1, 2, nsplit=1, why="25 taps: four groups; 63 pixels"),
    WSpec("wgrad16", 1, B16, 2, 15, 14, 40, 64, 64, 64, 3, 1, 2, d=2, nsplit=2, why="dilation 2"),
    WSpec("wgrad16", 1, B16, 1, 12, 12, 3, 16, 3, 16, 3, 1, 2, d=2, why="KC = 16 but dilated: not the thin kernel"),
    WSpec("wgrad16", 1, B16, 2, 16, 20, 40, 48, 70, 80, 4, 2, 1, nsplit=1, why="stride 2; 160 pixels"),
    # gconv_wgrad_thin_kernel (KC == 16, undilated, 16 bit)
    WSpec("thin", 1, B16, 1, 10, 10, 3, 16, 16, 16, 4, 2, 1, nsplit=1, why="k 4 s 2 p 1; OW = 5"),
    WSpec("thin", 1, B16, 1, 6, 64, 3, 16, 3, 16, 5, 1, 2, nsplit=1, why="k 5 s 1 p 2 (the Bayar layer); OW = 64"),
    WSpec("thin", 4, B16, 2, 40, 65, 16, 16, 20, 32, 3, 1, 1, nsplit=20, why="k 3; OW = 65: a chunk of one pixel; 160 chunks in 20 splits"),
    WSpec("thin", 1, B16, 1, 4, 150, 7, 16, 16, 16, 3, 1, 1, nsplit=2, why="OW = 150: chunks of 64, 64, 22"),
    WSpec("thin", 1, B16, 1, 9, 11, 3, 16, 40, 48, 4, 2, 1, nsplit=1, why="odd IW at stride 2"),
    WSpec("thin", 16, B16, 8, 128, 16, 3, 16, 16, 16, 4, 2, 1, nsplit=64, why="B 8, OH 64, OW 8: 512 chunks in 64 splits"),
    # GENERIC: one per kernel
    WSpec("f32", 4, F32, 3, 30, 35, 3, 4, 3, 16, 3, 1, 1, kind="normal"),
    WSpec("wgrad16", 4, B16, 3, 40, 39, 64, 64, 64, 64, 3, 1, 1, kind="normal"),
    WSpec("thin", 4, B16, 2, 40, 65, 16, 16, 20, 32, 3, 1, 1, kind="normal"),
)


class WgradCase:
    def __init__(self, i, dt):
        self.spec = sp = WGRAD_SPECS[i]
        assert dt in sp.dts
        self.dt, self.label = dt, sp.label(dt)
        self.kernel, self.nsplit, self.SL = sp.dispatch(dt)
        seed = 8000 + 41 * i
        self.x = data((sp.B, sp.IH, sp.IW, sp.KC), seed, sp.kind, dt)
        self.dout = data((sp.B, sp.OH, sp.OW, sp.NC), seed + 1, sp.kind, dt)
        shape = (sp.Nr, sp.Kr, sp.KH, sp.KW)
        if sp.kind == "grid":
            self.dw0, self.db0 = grid(shape, seed + 2, UNIT, -1.0, 1.0), grid((sp.Nr,), seed + 3, UNIT, -1.0, 1.0)
        else:
            self.dw0, self.db0 = rnd(normal(shape, seed + 2), "f32"), rnd(normal((sp.Nr,), seed + 3), "f32")
        self.dw, self.dw_abs, self.dw_cnt = wgrad64(self.dout[..., :sp.Nr], self.x[..., :sp.Kr], sp.KH, sp.KW, sp.s, sp.p, sp.d)
        self.db, self.db_abs, self.db_cnt = colsum64(self.dout[..., :sp.Nr].reshape(-1, sp.Nr))
        self.units = max(grid_units(self.dw_abs + np.abs(self.dw0)), grid_units(self.db_abs + np.abs(self.db0))) if sp.kind == "grid" else 0.0
        for t in (self.x, self.dout):
            assert t.size * ESZ[dt] <= MAX_BYTES, self.label

    def check_path(self):
        sp = self.spec
        assert (self.kernel, self.SL) == (sp.kernel, sp.SL), (self.label, self.kernel, self.nsplit, self.SL)
        assert sp.nsplit is None or sp.nsplit == self.nsplit, (self.label, self.nsplit)

    def check(self, dw, db, accumulate, what=""):
        """accumulate: the call added to dw0 / db0 -- one more term (and one more rounding) of every sum.  db may be None."""
        sp, a = self.spec, 1 if accumulate else 0
        zero = sp.kind == "grid"
        b_dw = 0.0 if zero else n_bound(self.dw_cnt + a, self.dw_abs + a * np.abs(self.dw0))
        cm = [Cmp("%s dw acc=%d%s" % (self.label, a, what), f64(dw).reshape(self.dw.shape), self.dw + a * self.dw0, b_dw)]
        if db is not None:
            b_db = 0.0 if zero else n_bound(self.db_cnt + a, self.db_abs + a * np.abs(self.db0))
            cm.append(Cmp("%s dbias acc=%d%s" % (self.label, a, what), db, self.db + a * self.db0, b_db))
        return cm


@functools.lru_cache(maxsize=None)
def wgrad_case(i, dt):
    return WgradCase(i, dt)


def wgrad_keys():
    return [(i, dt) for i, s in enumerate(WGRAD_SPECS) for dt in s.dts]


def wgrad_index(why, dt, kind="grid"):
    """the first spec of dtype dt whose reason starts with `why`"""
    return next(i for i, s in enumerate(WGRAD_SPECS) if s.kind == kind and dt in s.dts and s.why.startswith(why))


# ----------------------------------------------------------------------------------------------------------------- column sums
QUNIT = 0.25                                              # the column sums add multiples of 1/4 (and a prior value on the same grid)
COLSUM_NPIX = (1, 255, 257, 1025)
COLSUM_CAP = 256 * 512 + 1                                # 513 splits asked for, 512 given.  8 MB allow it 16 channels of 16 bits
# (C, npix, Creal, accumulate, kind, dtypes)
COLSUM_SPECS = tuple((C, n, C if (i + j) % 2 else C - 3, (i + j // 2) % 2, "grid", DTYPES)
                     for i, C in enumerate((16, 32, 48, 64, 80)) for j, n in enumerate(COLSUM_NPIX)) + \
    ((16, COLSUM_CAP, 13, 0, "grid", DT16), (16, COLSUM_CAP, 16, 1, "grid", DT16),
     (80, 1025, 77, 1, "normal", DTYPES), (48, 257, 48, 0, "normal", DTYPES))


class ColsumCase:
    def __init__(self, i, dt):
        self.C, self.npix, self.Creal, self.accumulate, self.kind, dts = COLSUM_SPECS[i]
        assert dt in dts
        self.dt = dt
        seed = 9000 + 17 * i
        self.x = data((self.npix, self.C), seed, self.kind, dt)            # the padding channels hold values: they must not arrive anywhere
        self.out0 = grid((self.Creal,), seed + 1, QUNIT, -1.0, 1.0) if self.kind == "grid" else rnd(normal((self.Creal,), seed + 1), "f32")
        s, ab, cnt = colsum64(self.x[:, :self.Creal])
        a = self.accumulate
        self.ref, self.absum, self.count = s + a * self.out0, ab + a * np.abs(self.out0), cnt + a
        self.units = grid_units(self.absum, QUNIT) if self.kind == "grid" else 0.0
        self.nsplit = colsum_nsplit(self.npix)
        self.label = "colsum %s C=%d(%d) npix=%d acc=%d [%d splits]%s" % (dt, self.Creal, self.C, self.npix, a, self.nsplit,
                                                                         "" if self.kind == "grid" else " generic")
        assert self.x.size * ESZ[dt] <= MAX_BYTES, self.label

    def check(self, out, in_double, what=""):
        if self.kind == "grid":
            b = 0.0
        elif in_double:
            b = DBL * self.absum + EPS32 * np.abs(self.ref)                # summed in double, then the one float32 rounding of the result
        else:
            b = n_bound(self.count, self.absum)
        return [Cmp("%s %s%s" % (self.label, "in double" if in_double else "float32", what), out, self.ref, b)]


@functools.lru_cache(maxsize=None)
def colsum_case(i, dt):
    return ColsumCase(i, dt)


def colsum_keys():
    return [(i, dt) for i, s in enumerate(COLSUM_SPECS) for dt in s[5]]


# ----------------------------------------------------------------------------------------------------------------- pack
# (Cout, Cin, KH, KW, RP, CP, transpose): ragged extents both ways; (.., 4) columns: a float32 input stride
PACK_SPECS = ((3, 5, 3, 3, 16, 16, 0), (3, 5, 3, 3, 16, 16, 1), (70, 40, 2, 4, 80, 48, 0), (70, 40, 2, 4, 48, 80, 1), (64, 64, 1, 1, 64, 64, 0),
              (64, 64, 1, 1, 64, 64, 1), (7, 130, 5, 5, 16, 144, 0), (7, 130, 5, 5, 144, 16, 1), (5, 3, 4, 4, 16, 4, 0), (3, 5, 4, 4, 16, 4, 1))


class PackCase:
    """wm_gconv_pack: the float32 weight rounded to dt (round to nearest even: rnd) at its transposed place, zeros around it"""

    def __init__(self, i, dt):
        self.Cout, self.Cin, self.KH, self.KW, self.RP, self.CP, self.transpose = PACK_SPECS[i]
        self.dt = dt
        self.w = rnd(normal((self.Cout, self.Cin, self.KH, self.KW), 9500 + i), "f32")
        self.w.reshape(-1)[:4] = (1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11)   # ties of bf16 and f16: to even
        self.ref = pack64(self.w, self.RP, self.CP, self.transpose, dt)
        self.label = "pack %s %dx%dx%dx%d -> [%d][%d][%d]%s" % (dt, self.Cout, self.Cin, self.KH, self.KW, self.KH * self.KW, self.RP, self.CP,
                                                                " transposed" if self.transpose else "")

    def check(self, wp):
        r, c = (self.Cin, self.Cout) if self.transpose else (self.Cout, self.Cin)
        o = f64(wp).reshape(self.ref.shape)
        pad = np.ones(self.ref.shape, dtype=bool)
        pad[:, :r, :c] = False
        return [Cmp(self.label, o[:, :r, :c], self.ref[:, :r, :c]), Cmp(self.label + " padding", o[pad], np.zeros(int(pad.sum())))]


@functools.lru_cache(maxsize=None)
def pack_case(i, dt):
    return PackCase(i, dt)
