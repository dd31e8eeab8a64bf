"""Float64 restatement of the FORWARD half of the 3x3 convolution hot path -- wm_pack_w3x3 / wm_pack_w3x3_batch, wm_conv3x3_fwd (the
persistent kernel csrc/conv3x3_ws.hip, the streamed-filter kernel csrc/conv3x3_stream.hip, the generic 16-bit and float32 kernel of
csrc/conv3x3.hip; forward, and input gradient through the transposed pack), wm_conv3x3_fwd_addin, wm_concat_side_fwd and
wm_concat_side_msg_wgrad -- written from the comments of include/wm_hip.h, with the restated host arithmetic (which kernel, which
form, how many statistics rows, which tiles a row of the persistent kernel covers), the case tables and the per-element comparisons
built on it.  A plain helper module (no fixtures, CPU only, never imports the HIP package): tests/test_cpu_cbr_fwd_exact.py runs float32
imitations -- faithful and defective -- through these comparisons, tests/test_gpu_cbr_fwd_exact.py runs the kernels through them.

    a  = x, or relu(in_scale*x + in_shift) ROUNDED to the activation type (float32: as computed); zero outside the image AFTER that
    y  = sum_{kh,kw,ci} a[b, h+kh-1, w+kw-1, ci] * W[co,ci,kh,kw] + bias[co] (co < nbias) (+ addend[b,h,w,co]); stored rounded
    statistics row r = (sum y | sum y*y) of the UNROUNDED y over the pixels of the image the row owns:
        persistent kernel: one row per workgroup; workgroup g of G = ws_wgs(tiles) walks run xcd_run(G, g) = tiles
                           [run*per, min(tiles, (run+1)*per)) of 16 x 16 pixels, per = ceil(tiles / 256); backwards under sweep_reverse
        streamed kernel  : 4 rows per tile (4 pixel rows each);   generic kernel: one row per tile
    P  = conv3(image) + bias + sum_{taps inside the image} sum_l W[:, c_msg+l, tap] * msg[b,l]              (wm_concat_side_fwd)
    dw[:, c_msg+l, tap] (+)= sum_b msg[b,l] * S[b,tap,:],  S = sums of dy over the pixels whose `tap` lies inside the image

Data.  GRID: x, w multiples of 1/4 in [-1, 1], bias and addend multiples of 1/16, in_scale from {1/2, 1, 2}, in_shift multiples of 1/4:
a is a multiple of 1/8 with |a| <= 3 (asserted: a == rnd(a) in bf16 and f16), every term of y a multiple of 1/32, and the reference
asserts max|a| * max_co sum|w[co]| + |bias| + |addend| < 2**24 such units: the float32 accumulator is exact in any order and MFMA
shape, and y is compared BIT FOR BIT with rnd(exact).  SPARSE: x from {-1, -1/2, 0, 1/2, 1}, in_scale from {1/2, 1}, in_shift from
{0, 1/2}, four non-zero weights from {+-1/2, +-1} per filter row at positions that differ per output channel, no bias: y is a multiple
of 1/8 with |y| <= 6 and sum y*y over any one row stays below 2**24 units of 1/64 (asserted on the reference alone) -- the statistics
rows are exact too: each restated row of the persistent kernel is compared bit for bit, for both sweep directions, and the column sums
of the other kernels' rows.  On dense GRID data a row of n pixels is held within FACTOR * (n - 1) * 2**-24 * sum|y| (sum y: its terms
are exact float32 values), and sum y*y within the same FACTOR * (n - 1) * 2**-24 * sum y*y for its additions plus 2**-24 * y*y per
term: a y of more than 12 bits has no exact float32 square, so each square rounds once (to nearest) before it is added.
GENERIC (normal data on the scales of tests/test_gpu_conv_ops.py): a float32 sum of n non-zero terms (the bias and the addend count) is
held within FACTOR * (n - 1) * 2**-24 * sum|terms| (float32 operands: the products round too, n roundings in all, which FACTOR * (n - 1)
covers from n = 2 on -- asserted); a 16-bit store adds half an ulp; a staged a whose float64 value lies within its own float32 error
(one fused multiply-add: FACTOR * 2**-24 * (|in_scale*x| + |in_shift|)) of a 16-bit rounding boundary or of the ReLU kink may round
either way: the distance between the two candidates, times |w|, is added to the bound of every output it enters.  At most 1 % of a
case's a may be ambiguous (asserted on the reference alone).  Nothing is skipped.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from layers_exact import (Cmp, rnd, store, grid, pick, normal, strided, sentinel_dest, gap_cmps, f64, half_ulp, HALF_ULP, FACTOR, EPS32, GAP, SENTINEL)

DT16 = ("bf16", "f16")
TILE = 16
MAX_WGS = 256
MAX_UNITS = 2.0 ** 24
AMBIGUOUS_CAP = 0.01
DW_START = 0.25
DROP = 1 << 20                                            # a perm entry >= CinP: "this reference channel is not in the packed operand"
assert HALF_ULP["bf16"] == 2.0 ** -8 and DW_START != SENTINEL


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------------------------------------------- host arithmetic
def ntiles(B, H, W):
    return B * cdiv(H, TILE) * cdiv(W, TILE)


def use_ws(Cin, CoutP, dt):
    """the persistent kernel (csrc/conv3x3_ws.hip): 16-bit types, 16 / 32 / 64 -> 64 or 64 -> 32, a dense output"""
    return dt in DT16 and ((Cin in (16, 32, 64) and CoutP == 64) or (Cin == 64 and CoutP == 32))


def stream_supported(Cin, CoutP):
    """wm_conv3x3_stream_supported (not part of the C ABI: the library shows it through wm_conv3x3_nparts, 4 rows per tile)"""
    return Cin % 16 == 0 and Cin >= 32 and CoutP % 64 == 0


def use_stream(Cin, CoutP, dt):
    return dt in DT16 and not use_ws(Cin, CoutP, dt) and stream_supported(Cin, CoutP)


def kernel_of(Cin, CoutP, dt):
    return "ws" if use_ws(Cin, CoutP, dt) else "stream" if use_stream(Cin, CoutP, dt) else "generic"


def ws_wgs(n):
    return cdiv(n, cdiv(n, MAX_WGS))


def nparts(B, H, W, Cin, CoutP, dt):
    """wm_conv3x3_nparts"""
    n = ntiles(B, H, W)
    return {"ws": ws_wgs(n), "stream": 4 * n, "generic": n}[kernel_of(Cin, CoutP, dt)]


def ws_form(Cin, CoutP, xform, stats, H, W):
    """the persistent forward kernel's form: WHOLE (no inside-the-image mask) needs whole tiles AND (64 -> 64 with transform and
    statistics, or 16 -> 64 with statistics and no transform); everything else takes the masked form"""
    whole = H % TILE == 0 and W % TILE == 0 and CoutP == 64 and stats and ((Cin == 64 and xform) or (Cin == 16 and not xform))
    return "WHOLE" if whole else "masked"


def fwd_elu_supported(Cin, CoutP, dt):
    """wm_conv3x3_fwd_elu_supported"""
    return dt in DT16 and CoutP == 64 and Cin in (16, 32, 64)


def dgrad_elufused_supported(CinP, dt):
    """wm_conv3x3_dgrad_elufused_supported"""
    return dt in DT16 and CinP in (16, 32, 64)


def dgrad_elufused_nparts(B, H, W):
    return ws_wgs(ntiles(B, H, W))


def xcd_run(G, g):
    """the run of the work list workgroup g of a grid of G walks: G / 8 consecutive runs per group of workgroups g % 8 == const"""
    return (g & 7) * (G >> 3) + (g >> 3) if G % 8 == 0 else g


def tile_box(t, B, H, W):
    """tile index -> (b, h0, h1, w0, w1), the part of the tile inside the image"""
    tx, ty = cdiv(W, TILE), cdiv(H, TILE)
    b, i, j = t // (tx * ty), (t // tx) % ty, t % tx
    return b, i * TILE, min(i * TILE + TILE, H), j * TILE, min(j * TILE + TILE, W)


def ws_rows(B, H, W, reverse=False):
    """the persistent kernel's statistics rows: row g -> the tiles it covers, in the order it walks them"""
    n = ntiles(B, H, W)
    per, G = cdiv(n, MAX_WGS), ws_wgs(n)
    rows = []
    for g in range(G):
        run = xcd_run(G, g)
        t = list(range(run * per, min(n, run * per + per)))
        rows.append(t[::-1] if reverse else t)
    return rows


def stat_rows(kernel, B, H, W, reverse=False):
    """row -> list of (b, h0, h1, w0, w1) pixel boxes whose y it sums; generic and streamed rows in tile order (the kernels permute
    them over the workgroups: only their column sums are compared)"""
    n = ntiles(B, H, W)
    if kernel == "ws":
        return [[tile_box(t, B, H, W) for t in run] for run in ws_rows(B, H, W, reverse)]
    if kernel == "generic":
        return [[tile_box(t, B, H, W)] for t in range(n)]
    rows = []
    for t in range(n):
        b, h0, h1, w0, w1 = tile_box(t, B, H, W)
        rows += [[(b, min(h0 + 4 * q, h1), min(h0 + 4 * q + 4, h1), w0, w1)] for q in range(4)]
    return rows


# ----------------------------------------------------------------------------------------------------------------- pack
def pack64(w, CoutP, CinP, perm, transpose, dt):
    """w [Cout,Cin,3,3] -> [9][CoutP][CinP], tap = 3*kh + kw, packed input channel perm[ci] (or ci) holds reference channel ci, an entry
    >= CinP is dropped, padding exact zeros, rounded once to dt; transpose: [9][CinP][CoutP] with the taps flipped"""
    Cout, Cin = w.shape[:2]
    out = np.zeros((9, CoutP, CinP))
    for ci in range(Cin):
        p = ci if perm is None else perm[ci]
        if p < CinP:
            out[:, :Cout, p] = w[:, ci].reshape(Cout, 9).T
    if transpose:
        out = np.ascontiguousarray(out[::-1].transpose(0, 2, 1))
    return rnd(out, dt)


def encoder_perms(L, c=64):
    """hidden_models/encoder.py: the reference concat is [message L | features c | image 3]; (c_msg, c_img, the perm of the feature
    operand, the perm of the 16-channel image operand, the perm of the packed concat tensor [features | message | image])"""
    return 0, L + c, [DROP] * L + list(range(c)) + [DROP] * 3, [DROP] * (L + c) + [0, 1, 2], [c + i for i in range(L)] + list(range(c)) + [c + L + i for i in range(3)]


# (Cout, Cin, CoutP, CinP, perm)
PACK_SHAPES = ((64, 64, 64, 64, None), (30, 64, 32, 64, None), (64, 3, 64, 16, None), (64, 97, 64, 64, "features"), (64, 97, 64, 16, "image"),
               (64, 97, 64, 112, "concat"))


def pack_perm(name):
    return None if name is None else encoder_perms(30)[2 + ("features", "image", "concat").index(name)]


@functools.lru_cache(maxsize=None)
def pack_weight(k):
    Cout, Cin = PACK_SHAPES[k][:2]
    return rnd(normal((Cout, Cin, 3, 3), 31000 + k, std=0.2), "f32")


def pack_cmps(k, transpose, dt, got, what="pack"):
    Cout, Cin, CoutP, CinP, pn = PACK_SHAPES[k]
    ref = pack64(pack_weight(k), CoutP, CinP, pack_perm(pn), transpose, dt)
    lab = "%s %s %d,%d->%d,%d %s%s" % (what, dt, Cout, Cin, CoutP, CinP, pn or "no perm", " transposed" if transpose else "")
    g = f64(got).reshape(ref.shape)
    real = pack64(np.ones((Cout, Cin, 3, 3)), CoutP, CinP, pack_perm(pn), transpose, "f32") != 0
    return [Cmp(lab + " values", g[real], ref[real]), Cmp(lab + " padding", g[~real], np.zeros(int((~real).sum())))]


# ----------------------------------------------------------------------------------------------------------------- the restatement
def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def conv64(a, w, want_count=False, want_abs=True):
    """a [B,H,W,Cin], w [Cout,Cin,3,3] -> y [B,H,W,Cout], sum|terms| (or None), non-zero terms (or None)"""
    at, wt = nchw(a), torch.from_numpy(np.ascontiguousarray(w))
    out = nhwc(F.conv2d(at, wt, padding=1))
    ab = nhwc(F.conv2d(at.abs(), wt.abs(), padding=1)) if want_abs else None
    cnt = nhwc(F.conv2d((at != 0).double(), (wt != 0).double(), padding=1)) if want_count else None
    return out, ab, cnt


def spread64(slack, w):
    return nhwc(F.conv2d(nchw(slack), torch.from_numpy(np.abs(w)), padding=1))


def sparse_weight(Cout, Cin, seed, k=4):
    """k non-zero weights from {+-1/2, +-1} per filter row, at positions that differ per output channel"""
    w = np.zeros((Cout, Cin * 9))
    vals = pick((Cout, k), seed, (-1.0, -0.5, 0.5, 1.0))
    pos = grid((Cout, k), seed + 1, 1.0, 0.0, Cin * 9 - 1.0).astype(np.int64)
    for co in range(Cout):
        for j in range(k):
            w[co, (pos[co, j] + 37 * co) % (Cin * 9)] = vals[co, j]       # (a collision only drops a weight)
    return w.reshape(Cout, Cin, 3, 3)


class Ref:
    """one forward call's operands (float64 arrays holding dtype-exact values) and its float64 result.  kind: "grid", "sparse" (exact
    for both 16-bit types and float32: dt None) or "normal" (operands rounded to dt).  transposed: the call is an input gradient -- x is
    dy, the kernel gets the transposed pack of w [Cin(=Cout of the layer), CoutP(=Cin of the layer), 3, 3] and the reference is
    conv_transpose2d."""

    def __init__(self, Cin, CoutP, B, H, W, xform, nbias, kind, dt, addin=False, transposed=False):
        self.Cin, self.CoutP, self.B, self.H, self.W, self.xform, self.nbias, self.kind, self.dt = Cin, CoutP, B, H, W, xform, nbias, kind, dt
        self.addin, self.transposed, self.exact = addin, transposed, kind != "normal"
        seed = 21000 + 131 * Cin + 7 * CoutP + 977 * B + 13 * H + W + (500 if xform else 0) + {"grid": 0, "sparse": 3000, "normal": 6000}[kind]
        shp = (B, H, W, Cin)
        self.in_scale = self.in_shift = self.addend = None
        self.bias = np.zeros(CoutP)
        if kind == "grid":
            self.x, self.w = grid(shp, seed, 0.25, -1.0, 1.0), grid((CoutP, Cin, 3, 3), seed + 1, 0.25, -1.0, 1.0)
            if nbias:
                self.bias[:nbias] = grid((nbias,), seed + 2, 1.0 / 16, -1.0, 1.0)
            if xform:
                self.in_scale, self.in_shift = pick((Cin,), seed + 3, (0.5, 1.0, 2.0)), grid((Cin,), seed + 4, 0.25, -1.0, 1.0)
            if addin:
                self.addend = grid((B, H, W, CoutP), seed + 5, 1.0 / 16, -2.0, 2.0)
            self.unit = 32.0
        elif kind == "sparse":
            assert not nbias
            self.x, self.w = pick(shp, seed, (-1.0, -0.5, 0.0, 0.5, 1.0)), sparse_weight(CoutP, Cin, seed + 1)
            if xform:
                self.in_scale, self.in_shift = pick((Cin,), seed + 3, (0.5, 1.0)), pick((Cin,), seed + 4, (0.0, 0.5))
            if addin:
                self.addend = pick((B, H, W, CoutP), seed + 5, (-1.0, -0.5, 0.0, 0.5, 1.0))
            self.unit = 8.0
        else:
            self.x = rnd(normal(shp, seed, mean=0.1), dt)
            self.w = rnd(normal((CoutP, Cin, 3, 3), seed + 1, std=(2.0 / (9 * Cin)) ** 0.5), dt)          # exact in dt: the pack rounds nothing
            if nbias:
                self.bias[:nbias] = rnd(normal((nbias,), seed + 2, std=0.1), "f32")
            if xform:
                self.in_scale, self.in_shift = rnd(normal((Cin,), seed + 3, std=0.3, mean=1.0), "f32"), rnd(normal((Cin,), seed + 4, std=0.3), "f32")
            if addin:
                self.addend = rnd(normal((B, H, W, CoutP), seed + 5), dt)
        if transposed:                                                       # w as the LAYER holds it: [Cout_layer = Cin here][Cin_layer = CoutP here]
            self.w_layer = np.ascontiguousarray(self.w.transpose(1, 0, 2, 3))
            self.w = np.ascontiguousarray(self.w_layer.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])          # conv_transpose2d as a conv2d
        self._forward()

    def _forward(self):
        dts = (DT16 + ("f32",)) if self.exact else (self.dt,)
        slack = None
        if self.xform:
            z = self.in_scale * self.x + self.in_shift
            a = np.maximum(z, 0.0)
            if self.exact:
                for dt in dts:
                    assert np.array_equal(rnd(a, dt), a), "a is not exact in %s" % dt
                assert np.array_equal(a * 8, np.round(a * 8))
                self.amb_share = 0.0
            else:
                e = FACTOR * EPS32 * (np.abs(self.in_scale * self.x) + np.abs(self.in_shift))
                if self.dt == "f32":
                    slack, amb = np.minimum(e, np.maximum(z + e, 0.0)), np.zeros(a.shape, dtype=bool)      # no 16-bit boundary to cross
                else:
                    lo, hi = rnd(np.maximum(z - e, 0.0), self.dt), rnd(np.maximum(z + e, 0.0), self.dt)
                    a = rnd(a, self.dt)
                    amb = lo != hi
                    slack = np.maximum(hi - a, a - lo)                      # relu and the rounding are monotone: covers kink and boundary
                self.amb_share = float(amb.mean())
        else:
            a, self.amb_share = self.x, 0.0
        self.a = a
        want = not self.exact
        y, ab, cnt = conv64(a, self.w, want, want)
        extra = np.abs(self.bias)
        y = y + self.bias
        if self.addin:
            y = y + self.addend
            extra = extra + np.abs(self.addend)
        self.y = y
        if self.exact:
            top = np.abs(a).max() * np.abs(self.w).sum((1, 2, 3)).max() + np.max(extra)
            assert top * self.unit < MAX_UNITS, "y: sum|terms| may reach %g units" % (top * self.unit)
            assert np.array_equal(y * self.unit, np.round(y * self.unit))
            self.y_bound = np.zeros(y.shape)
        else:
            n = cnt + (self.bias != 0) + (1 if self.addin else 0)
            assert self.dt != "f32" or n.min() >= 2
            self.y_bound = FACTOR * np.maximum(n - 1, 0) * EPS32 * (ab + extra) + (spread64(slack, self.w) if slack is not None else 0.0)

    def y_ref(self, dt):
        """(y, its bound) as stored in dt: exact kinds rnd(exact sum), bit for bit; GENERIC the float64 value, + half an ulp of the store"""
        if self.exact:
            return rnd(self.y, dt), self.y_bound
        return self.y, self.y_bound + half_ulp(np.abs(self.y) + self.y_bound, dt)

    def stats_ref(self, rows):
        """rows: stat_rows(...) -> (ref [nrows,2,CoutP], bound [nrows,2,CoutP]) of the unrounded y"""
        y, yb = self.y, self.y_bound
        ref, bound = np.zeros((len(rows), 2, self.CoutP)), np.zeros((len(rows), 2, self.CoutP))
        for r, boxes in enumerate(rows):
            v = np.concatenate([y[b, h0:h1, w0:w1].reshape(-1, self.CoutP) for b, h0, h1, w0, w1 in boxes])
            e = np.concatenate([yb[b, h0:h1, w0:w1].reshape(-1, self.CoutP) for b, h0, h1, w0, w1 in boxes])
            n = v.shape[0]
            ref[r, 0], ref[r, 1] = v.sum(0), (v * v).sum(0)
            if self.kind == "sparse":
                assert (v * v).sum(0).max(initial=0.0) * 64 < MAX_UNITS and np.abs(v).max(initial=0.0) <= 6, "a SPARSE row leaves 2**24 units"
            else:
                hi = np.abs(v) + e
                bound[r, 0] = e.sum(0) + FACTOR * max(n - 1, 0) * EPS32 * hi.sum(0)
                bound[r, 1] = (2 * np.abs(v) * e + e * e).sum(0) + (FACTOR * max(n - 1, 0) + 1) * EPS32 * (hi * hi).sum(0)     # n - 1 additions; each square rounds once: EPS32 * y*y
        return ref, bound


@functools.lru_cache(maxsize=4)
def reference(Cin, CoutP, B, H, W, xform, nbias, kind, dt, addin=False, transposed=False):
    return Ref(Cin, CoutP, B, H, W, xform, nbias, kind, dt, addin, transposed)


# ----------------------------------------------------------------------------------------------------------------- cases
class Case:
    """one call of wm_conv3x3_fwd (or _fwd_addin): family is the kernel (and form) the case is there for"""

    def __init__(self, family, Cin, CoutP, B, H, W, xform=False, stats=False, nbias=0, kind="grid", reverse=False, ldx_gap=0, ldy_gap=0,
                 dts=DT16, addin=False, transposed=False, why=""):
        self.family, self.Cin, self.CoutP, self.B, self.H, self.W, self.xform, self.stats, self.nbias, self.kind = family, Cin, CoutP, B, H, W, xform, stats, nbias, kind
        self.reverse, self.ldx_gap, self.ldy_gap, self.dts, self.addin, self.transposed, self.why = reverse, ldx_gap, ldy_gap, dts, addin, transposed, why
        self.kernel = {"ws-whole": "ws", "ws-masked": "ws", "addin": "ws"}.get(family, family)
        self.ldx, self.ldy = Cin + ldx_gap, CoutP + ldy_gap

    @property
    def id(self):
        return "%s-%dto%d-%dx%dx%d-%s%s%s%s%s%s%s%s" % (self.family, self.Cin, self.CoutP, self.B, self.H, self.W, self.kind, "-xf" if self.xform else "",
                                                      "-st" if self.stats else "", "-b%d" % self.nbias if self.nbias else "", "-rev" if self.reverse else "",
                                                      "-ldx" if self.ldx_gap else "", "-ldy" if self.ldy_gap else "", "-T" if self.transposed else "")

    def label(self, dt):
        return "%s %s" % (self.id, dt)

    def ref(self, dt):
        return reference(self.Cin, self.CoutP, self.B, self.H, self.W, self.xform, self.nbias, self.kind, None if self.kind != "normal" else dt, self.addin,
                         self.transposed)

    def expected_rows(self, dt):
        return nparts(self.B, self.H, self.W, self.Cin, self.CoutP, dt)

    def check_dispatch(self, dt, nparts_fn=None):
        """the case reaches the kernel, the form and the row count it is there for; the GPU test passes the library's functions"""
        k = kernel_of(self.Cin, self.CoutP, dt)
        assert k == self.kernel, (self.label(dt), k)
        if self.family in ("ws-whole", "ws-masked"):
            assert "ws-" + ws_form(self.Cin, self.CoutP, self.xform, self.stats, self.H, self.W).lower() == self.family, self.label(dt)
        if self.family == "addin":
            assert (self.Cin, self.CoutP, self.xform, self.stats) == (64, 64, True, True)
        assert k != "ws" or self.ldy_gap == 0
        assert dt in DT16 or (self.Cin % 4 == 0 and k == "generic")
        shape = (self.B, self.H, self.W, self.Cin, self.CoutP)
        assert nparts_fn is None or nparts_fn(*shape, dt) == self.expected_rows(dt), self.label(dt)
        return k

    def operands(self, dt):
        """the tensors of one call, on the CPU: x [npix, ldx] (SENTINEL in the stride gap), w [Cout,Cin,3,3] float32 as the pack gets it (transposed:
        the layer's weight, to be packed with transpose = 1), bias, in_scale, in_shift, addend, y0 [npix, ldy] SENTINEL-filled"""
        r = self.ref(dt)
        npix = self.B * self.H * self.W
        o = {"x": strided(r.x.reshape(npix, self.Cin), self.ldx, dt), "w": store(r.w_layer if self.transposed else r.w, "f32"),
             "bias": store(r.bias[:self.nbias], "f32") if self.nbias else None, "y0": sentinel_dest(npix, self.ldy, dt)}
        o["in_scale"], o["in_shift"] = (store(r.in_scale, "f32"), store(r.in_shift, "f32")) if self.xform else (None, None)
        o["addend"] = store(r.addend, dt) if self.addin else None
        return o

    def check(self, dt, ybuf, stat, reverse=None):
        """ybuf [npix, ldy] after the call, stat [rows,2,CoutP] or None -> comparisons"""
        r, lab = self.ref(dt), self.label(dt)
        rev = self.reverse if reverse is None else reverse
        yb = f64(ybuf).reshape(-1, self.ldy)
        ref, bound = r.y_ref(dt)
        cm = [Cmp(lab + " y", yb[:, :self.CoutP], ref.reshape(-1, self.CoutP), bound.reshape(-1, self.CoutP))] + gap_cmps(lab + " y", yb, 0, self.CoutP)
        assert (stat is not None) == self.stats, lab
        if self.stats:
            rows = stat_rows(self.kernel, self.B, self.H, self.W, rev)
            s = f64(stat)
            assert s.shape == (self.expected_rows(dt), 2, self.CoutP) and len(rows) == s.shape[0], (lab, s.shape, len(rows))
            sref, sb = r.stats_ref(rows)
            if self.kernel == "ws":                              # every restated row
                cm += [Cmp(lab + " rows sum y", s[:, 0], sref[:, 0], sb[:, 0]), Cmp(lab + " rows sum y*y", s[:, 1], sref[:, 1], sb[:, 1])]
            else:                                                # the column sums over all rows
                cm += [Cmp(lab + " column sums of sum y", s[:, 0].sum(0), sref[:, 0].sum(0), sb[:, 0].sum(0)),
                       Cmp(lab + " column sums of sum y*y", s[:, 1].sum(0), sref[:, 1].sum(0), sb[:, 1].sum(0))]
        return cm


def _cases():
    c = []
    # persistent, WHOLE
    for B, H, W in ((1, 16, 16), (2, 32, 32)):
        c.append(Case("ws-whole", 64, 64, B, H, W, xform=True, stats=True, nbias=30, kind="grid", reverse=B == 2))
        c.append(Case("ws-whole", 16, 64, B, H, W, stats=True, nbias=64, kind="grid", reverse=B == 1))
        c.append(Case("ws-whole", 64, 64, B, H, W, xform=True, stats=True, kind="sparse"))
        c.append(Case("ws-whole", 16, 64, B, H, W, stats=True, kind="sparse", reverse=True))
        c.append(Case("ws-whole", 64, 64, B, H, W, xform=True, stats=True, nbias=30, kind="normal"))
        c.append(Case("ws-whole", 16, 64, B, H, W, stats=True, nbias=64, kind="normal", reverse=True))
    c.append(Case("ws-whole", 64, 64, 1, 32, 128, xform=True, stats=True, kind="sparse", why="16 workgroups: the runs are permuted over them"))
    c.append(Case("ws-masked", 32, 64, 1, 32, 128, xform=True, stats=True, kind="sparse", reverse=True, why="16 workgroups, masked form"))
    # persistent, masked: every flag pair, bias with nbias = 30 < CoutP
    k = 0
    for Cin, CoutP in ((16, 64), (32, 64), (64, 64), (64, 32)):
        for B, H, W in ((1, 17, 33), (1, 1, 1), (1, 16, 1), (3, 15, 18)):
            for xf in (False, True):
                for st in (False, True):
                    c.append(Case("ws-masked", Cin, CoutP, B, H, W, xform=xf, stats=st, nbias=30, kind="grid", reverse=k % 2 == 1, ldx_gap=GAP if k % 3 == 0 else 0))
                    k += 1
        c.append(Case("ws-masked", Cin, CoutP, 1, 17, 33, xform=True, stats=True, kind="sparse"))
        c.append(Case("ws-masked", Cin, CoutP, 3, 15, 18, xform=False, stats=True, kind="sparse", reverse=True))
        c.append(Case("ws-masked", Cin, CoutP, 1, 17, 33, xform=True, stats=True, nbias=30, kind="normal"))
    # whole-tile shape without transform or statistics: the masked form
    c.append(Case("ws-masked", 64, 64, 1, 16, 16, kind="grid", why="whole tiles, no flags"))
    c.append(Case("ws-masked", 64, 64, 1, 16, 16, xform=True, kind="grid", why="whole tiles, no statistics"))
    c.append(Case("ws-masked", 64, 64, 1, 16, 16, stats=True, kind="grid", why="whole tiles, no transform"))
    c.append(Case("ws-masked", 16, 64, 1, 16, 16, xform=True, stats=True, kind="grid", why="whole tiles, 16 -> 64 WITH transform"))
    # two tiles per workgroup
    for rev in (False, True):
        c.append(Case("ws-whole", 64, 64, 1, 16, 16 * 257, xform=True, stats=True, kind="sparse", reverse=rev, dts=("bf16",), why="257 tiles"))
    # streamed filter: strided output into a sentinel-filled destination
    for Cin, CoutP, shapes in ((128, 128, ((1, 17, 33), (2, 16, 16))), (112, 64, ((1, 17, 33), (2, 16, 16))), (256, 64, ((1, 20, 21),))):
        for B, H, W in shapes:
            for xf in (False, True):
                c.append(Case("stream", Cin, CoutP, B, H, W, xform=xf, stats=True, nbias=30, kind="grid", ldy_gap=GAP, ldx_gap=GAP if xf else 0))
        c.append(Case("stream", Cin, CoutP, *shapes[0], xform=True, stats=True, kind="sparse", ldy_gap=GAP))
        c.append(Case("stream", Cin, CoutP, *shapes[0], xform=True, stats=True, nbias=30, kind="normal", ldy_gap=GAP))
    c.append(Case("stream", 128, 128, 1, 17, 33, kind="grid", why="no statistics, dense"))
    # generic 16-bit
    for Cin, CoutP in ((16, 32), (48, 96), (16, 128)):
        for xf in (False, True):
            c.append(Case("generic", Cin, CoutP, 1, 17, 33, xform=xf, stats=True, nbias=30, kind="grid", ldx_gap=GAP, ldy_gap=GAP))
        c.append(Case("generic", Cin, CoutP, 1, 17, 33, xform=True, stats=True, kind="sparse"))
        c.append(Case("generic", Cin, CoutP, 1, 17, 33, xform=True, stats=True, nbias=30, kind="normal", ldy_gap=GAP))
    c.append(Case("generic", 16, 32, 2, 16, 16, kind="grid", why="no statistics"))
    # generic float32
    for Cin in (4, 12, 16, 64):
        for CoutP in (32, 64):
            for j, (B, H, W) in enumerate(((1, 17, 33), (2, 16, 16))):
                c.append(Case("generic", Cin, CoutP, B, H, W, xform=j == 0, stats=True, nbias=30, kind="grid", dts=("f32",), ldy_gap=GAP * j))
            c.append(Case("generic", Cin, CoutP, 1, 17, 33, xform=True, stats=True, nbias=30, kind="normal", dts=("f32",)))
            c.append(Case("generic", Cin, CoutP, 2, 16, 16, xform=True, stats=True, kind="sparse", dts=("f32",)))
    # wm_conv3x3_fwd_addin
    for j, (B, H, W) in enumerate(((1, 16, 16), (1, 17, 33), (2, 32, 32))):
        for rev in (False, True):
            c.append(Case("addin", 64, 64, B, H, W, xform=True, stats=True, kind="grid", reverse=rev, addin=True))
        c.append(Case("addin", 64, 64, B, H, W, xform=True, stats=True, kind="sparse", reverse=j == 1, addin=True))
    c.append(Case("addin", 64, 64, 1, 17, 33, xform=True, stats=True, kind="normal", addin=True))
    # plain input gradient: the same entry point with the transposed pack, one per kernel, against conv_transpose2d
    c.append(Case("ws-masked", 64, 64, 1, 17, 33, kind="grid", transposed=True))
    c.append(Case("ws-masked", 64, 32, 1, 17, 33, kind="grid", transposed=True, reverse=True))
    c.append(Case("stream", 128, 64, 1, 17, 33, kind="grid", transposed=True))
    c.append(Case("generic", 32, 96, 1, 17, 33, kind="grid", transposed=True))
    c.append(Case("generic", 16, 32, 1, 17, 33, kind="grid", transposed=True, dts=("f32",)))
    return tuple(c)


CASES = _cases()
CASE_IDS = tuple(c.id for c in CASES)
assert len(set(CASE_IDS)) == len(CASE_IDS)


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def case_keys():
    return [(c.id, dt) for c in CASES for dt in c.dts]


# ----------------------------------------------------------------------------------------------------------------- the after-concat layer
SIDE_L = (30, 64, 1)
SIDE_SHAPES = ((1, 2, 2), (1, 17, 33), (2, 32, 32))


def taps_inside(H, W):
    """[9, H, W]: 1 where tap (kh, kw) of the pixel lies inside the image"""
    m = np.zeros((9, H, W))
    for kh in range(3):
        for kw in range(3):
            hh, ww = np.arange(H)[:, None] + kh - 1, np.arange(W)[None, :] + kw - 1
            m[3 * kh + kw] = ((hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)).astype(np.float64)
    return m


class SideRef:
    """the encoder's after-concat layer without the concat, all on GRID data (exact): img [B,3,H,W], msg [B,L], w [64][L+64+3][3][3] in
    the reference's channel order [message | features | image], bias or none; features: raw x [B,H,W,64] with in_scale / in_shift."""

    def __init__(self, L, B, H, W, with_bias):
        self.L, self.B, self.H, self.W, self.with_bias = L, B, H, W, with_bias
        self.c_msg, self.c_img, self.fperm, _, _ = encoder_perms(L)
        self.Cin = L + 64 + 3
        seed = 26000 + 101 * L + 977 * B + 13 * H + W + (7 if with_bias else 0)
        self.img = grid((B, 3, H, W), seed, 0.25, 0.0, 1.0)
        self.msg = grid((B, L), seed + 1, 0.25, -1.0, 1.0)
        self.w = grid((64, self.Cin, 3, 3), seed + 2, 0.25, -1.0, 1.0)
        self.bias = grid((64,), seed + 3, 1.0 / 16, -1.0, 1.0) if with_bias else np.zeros(64)
        self.x = grid((B, H, W, 64), seed + 4, 0.25, -1.0, 1.0)
        self.in_scale, self.in_shift = pick((64,), seed + 5, (0.5, 1.0, 2.0)), grid((64,), seed + 6, 0.25, -1.0, 1.0)
        self.dy = grid((B, H, W, 64), seed + 7, 0.125, -2.0, 2.0) if B * H * W <= 1024 else pick((B, H, W, 64), seed + 7, (-1.0, -0.5, 0.0, 0.5, 1.0))
        self.a = np.maximum(self.in_scale * self.x + self.in_shift, 0.0)
        for dt in DT16:
            assert np.array_equal(rnd(self.a, dt), self.a)
        # P from the header's formula
        wi = self.w[:, self.c_img:self.c_img + 3]
        wm = self.w[:, self.c_msg:self.c_msg + L].reshape(64, L, 9)
        img_nhwc = np.ascontiguousarray(self.img.transpose(0, 2, 3, 1))
        inside = taps_inside(H, W)
        mterm = np.einsum("olt,bl->bto", wm, self.msg)                           # [B, 9, 64]: the message's share per tap
        self.P = conv64(img_nhwc, wi, want_abs=False)[0] + self.bias + np.einsum("bto,thw->bhwo", mterm, inside)
        top = np.abs(wi).sum((1, 2, 3)).max() + 1.0 + np.abs(wm).sum((1, 2)).max() * np.abs(self.msg).max()
        assert top * 16 < MAX_UNITS
        self.conv_feat = conv64(self.a, self.w[:, L:L + 64], want_abs=False)[0]
        assert (np.abs(self.a).max() * np.abs(self.w[:, L:L + 64]).sum((1, 2, 3)).max() + np.abs(self.P).max()) * 32 < MAX_UNITS
        # the message channels' weight gradient
        S = np.einsum("bhwo,thw->bto", self.dy, inside)
        assert np.einsum("bhwo,thw->bto", np.abs(self.dy), inside).max() * 8 * 4 * B < MAX_UNITS        # msg * S in units of 1/32, summed over b
        self.S = S
        self.dwm = np.einsum("bl,bto->olt", self.msg, S).reshape(64, L, 3, 3)

    def cat_conv(self):
        """the float64 conv2d of the ACTUAL concat tensor cat([message planes, features, image]) -- what the header's identity promises"""
        B, H, W, L = self.B, self.H, self.W, self.L
        planes = np.broadcast_to(self.msg[:, None, None, :], (B, H, W, L))
        cat = np.concatenate([planes, self.a, self.img.transpose(0, 2, 3, 1)], axis=3)
        return conv64(cat, self.w, want_abs=False)[0] + self.bias

    def label(self, dt):
        return "concat_side %s L=%d %dx%dx%d%s" % (dt, self.L, self.B, self.H, self.W, " bias" if self.with_bias else "")

    def check_P(self, dt, P):
        return [Cmp(self.label(dt) + " P", f64(P).reshape(self.P.shape), rnd(self.P, dt))]

    def check_y(self, dt, y):
        """y of wm_conv3x3_fwd_addin(features, P as stored): rnd(conv64 + rnd(P)) bit for bit, and the identity: within the two roundings
        (of P, of y) of the concat's conv2d"""
        Pq = rnd(self.P, dt)
        got, cc = f64(y).reshape(self.P.shape), self.cat_conv()
        return [Cmp(self.label(dt) + " y = conv64 + P", got, rnd(self.conv_feat + Pq, dt)),
                Cmp(self.label(dt) + " y against the concat's conv2d", got, cc, half_ulp(self.P, dt) + half_ulp(np.abs(cc) + half_ulp(self.P, dt), dt))]

    def check_dw(self, dt, dw, accumulate):
        """dw [64][Cin][3][3] after the call on a tensor filled with DW_START: message channels (+)= dwm, all others untouched"""
        ref = np.full((64, self.Cin, 3, 3), DW_START)
        ref[:, self.c_msg:self.c_msg + self.L] = self.dwm + (DW_START if accumulate else 0.0)
        g = f64(dw)
        keep = np.ones(self.Cin, dtype=bool)
        keep[self.c_msg:self.c_msg + self.L] = False
        lab = "%s msg_wgrad acc=%d" % (self.label(dt), accumulate)
        return [Cmp(lab + " dw message channels", g[:, ~keep], ref[:, ~keep]), Cmp(lab + " dw other channels", g[:, keep], ref[:, keep])]


@functools.lru_cache(maxsize=4)
def side_ref(L, B, H, W, with_bias):
    return SideRef(L, B, H, W, with_bias)


SIDE_KEYS = [(L, B, H, W, bool((i + j) % 2 == 0)) for i, L in enumerate(SIDE_L) for j, (B, H, W) in enumerate(SIDE_SHAPES)] + [(30, 1, 17, 33, False), (30, 2, 32, 32, True)]


# ----------------------------------------------------------------------------------------------------------------- conv + bias + ELU
# wm_conv3x3_fwd_elu: out = rnd(elu(conv + bias)); wm_conv3x3_dgrad_elufused: gz = rnd(g * (out > 0 ? 1 : out + 1)) from the STORED out,
# dx = conv(gz, transposed pack), bias partial rows = per-workgroup column sums of the float32 product before its rounding;
# wm_conv3x3_wgrad_bias: dw (+)= sum a (x) gz, db (+)= the column sums of the partial rows.
ELU_SWITCH = 1.0 / 64                                     # |z| below it: the cubic; from it on: exp - 1
ELU_FLOOR = 2 * 2.0 ** -23                                # 2 float32 ulp of 1
ELU_SHAPES = ((1, 16, 16), (1, 17, 33), (3, 20, 20))
ELU_CIN = (16, 32, 64)
DB_START = 0.5


def elu64(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


def elu_np32(z, always_exp=False):
    """the two formulas in numpy float32: float32(exp(z)) - 1 from 1/64 on, z*(1 + z*(1/2 + z/6)) below it"""
    z = np.asarray(z, dtype=np.float32)
    one, half, sixth = np.float32(1), np.float32(0.5), np.float32(0.16666667)
    with np.errstate(over="ignore"):
        e = np.exp(np.minimum(z, np.float32(0))).astype(np.float32) - one
    p = z * (z * (z * sixth + half) + one)
    neg = e if always_exp else np.where(np.abs(z) < np.float32(ELU_SWITCH), p, e)
    return np.where(z > 0, z, neg).astype(np.float32)


def elu_allowance(z):
    """what the float32 ELU value may deviate before the store: FACTOR x the largest deviation from float64, over the case's z, of the
    same formulas in numpy float32 on the CPU; at least 2 float32 ulp of 1.  The code under test does not enter it."""
    z32 = np.asarray(z, dtype=np.float32)
    dev = np.abs(elu_np32(z32).astype(np.float64) - elu64(z32.astype(np.float64)))
    return max(FACTOR * float(dev.max(initial=0.0)), ELU_FLOOR), float(dev.max(initial=0.0))


def neighbours16(v, dt, steps=(-2, -1, 0, 1, 2)):
    """the 16-bit values `steps` places from v (a negative value: +1 is the next larger magnitude)"""
    from layers_exact import TORCH
    bits = torch.tensor([v], dtype=TORCH[dt]).view(torch.int16)
    return [float((bits + s).view(TORCH[dt]).double()[0]) for s in steps]


def planted_x(dt):
    """pre-activations to plant (z = x + bias with a one-hot filter): zeros of both signs, +-1/64 and the two 16-bit neighbours of -1/64
    on each side, -2**-14, -1, -20, -100, +3, and the x whose z = x + 1 is a rounding tie of the 16-bit type (odd channels: bias 1)"""
    tie = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}[dt]
    return [0.0, -0.0, 1.0 / 64] + neighbours16(-1.0 / 64, dt) + [-2.0 ** -14, -1.0, -20.0, -100.0, 3.0, tie]


class EluRef:
    """one conv + ELU layer: x [B,H,W,Cin] -> out [B,H,W,64], and its backward from (g, the stored out).  kind "grid" / "normal" as Ref;
    "planted": 64 -> 64 one-hot filter (centre tap, weight 1), bias 0 on even and 1 on odd channels, z = x + bias exactly."""

    def __init__(self, Cin, B, H, W, kind, dt):
        self.Cin, self.B, self.H, self.W, self.kind, self.dt = Cin, B, H, W, kind, dt
        seed = 41000 + 131 * Cin + 977 * B + 13 * H + W
        if kind == "planted":
            assert Cin == 64
            vals = np.array(planted_x(dt))
            idx = (np.arange(B * H * W)[:, None] + 5 * np.arange(64)[None, :]) % len(vals)
            x = vals[idx].reshape(B, H, W, 64)
            w = np.zeros((64, 64, 3, 3))
            w[np.arange(64), np.arange(64), 1, 1] = 1.0
            bias = (np.arange(64) % 2).astype(np.float64)
            z = x + bias
            assert np.array_equal(rnd(x, dt), x) and np.array_equal(z.astype(np.float32).astype(np.float64), z)
            self.x, self.w, self.bias, self.z, self.z_bound = x, w, bias, z, np.zeros(z.shape)
        else:
            r = Ref(Cin, 64, B, H, W, False, 64, kind, dt)
            self.x, self.w, self.bias, self.z, self.z_bound = r.x, r.w, r.bias, r.y, r.y_bound
        self.allow, self.measured = elu_allowance(self.z)
        self.out = elu64(self.z)
        # the backward's operands: the out a correct forward stores, and a 16-bit g
        dts = DT16 if dt is None else (dt,)
        self.bwd = {}
        for d in dts:
            outq = rnd(self.out, d)
            g = grid((B, H, W, 64), seed + 9, 0.125, -2.0, 2.0) if kind != "normal" else rnd(normal((B, H, W, 64), seed + 9), d)
            fac = np.where(outq > 0, 1.0, (outq.astype(np.float32) + np.float32(1)).astype(np.float64))      # float32: out + 1 may round
            p = (g.astype(np.float32) * fac.astype(np.float32)).astype(np.float64)                           # ... and so may the product
            self.bwd[d] = {"out": outq, "g": g, "p": p, "gz": rnd(p, d)}

    def out_ref(self, dt):
        """(out, bound): where z > 0 the output is z itself (the store's rounding only: exact data bit for bit); where exp underflows
        against 1 (z <= -20) exactly -1; elsewhere the accumulator's bound (elu is 1-Lipschitz), the ELU allowance and half an ulp"""
        exactz = not self.z_bound.any()
        ref = np.where(self.z <= -20, -1.0, self.out)
        b = self.z_bound + self.allow
        b = b + half_ulp(np.abs(ref) + b, dt)
        if exactz:
            sure = (self.z > 0) | (self.z <= -20) | (self.z == 0)
            ref = np.where(sure, rnd(ref, dt), ref)
            b = np.where(sure, 0.0, b)
        return ref, b

    def check_out(self, dt, out):
        ref, b = self.out_ref(dt)
        return [Cmp(self.label(dt) + " out", f64(out).reshape(ref.shape), ref, b)]

    def label(self, dt):
        return "elu %s %d->64 %dx%dx%d %s" % (dt, self.Cin, self.B, self.H, self.W, self.kind)

    # ---- backward
    def rows(self, dt):
        """the bias partial rows [ws_wgs, 64]: sums of the float32 product p over the pixels of the row's tiles, and their bound"""
        p = self.bwd[dt]["p"]
        rr = stat_rows("ws", self.B, self.H, self.W)
        ref, bound = np.zeros((len(rr), 64)), np.zeros((len(rr), 64))
        for r, boxes in enumerate(rr):
            v = np.concatenate([p[b, h0:h1, w0:w1].reshape(-1, 64) for b, h0, h1, w0, w1 in boxes])
            ref[r], bound[r] = v.sum(0), FACTOR * max(v.shape[0] - 1, 0) * EPS32 * np.abs(v).sum(0)
        return ref, bound

    def check_dgrad(self, dt, CinP, dx, gz, rows):
        """CinP 64 / 32 / 16: dx [B,H,W,CinP] = conv_transpose(gz, w[:, :CinP]) (the layer's first CinP input channels)"""
        d, lab = self.bwd[dt], "%s CinP=%d" % (self.label(dt), CinP)
        w = self.w[:, :min(CinP, self.Cin)]
        wt = np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
        s, ab, cnt = conv64(d["gz"], wt, True, True)
        bound = FACTOR * np.maximum(cnt - 1, 0) * EPS32 * ab
        bound = bound + half_ulp(np.abs(s) + bound, dt)
        got = f64(dx).reshape(self.B, self.H, self.W, CinP)
        cm = [Cmp(lab + " gz", f64(gz).reshape(d["gz"].shape), d["gz"]), Cmp(lab + " dx", got[..., :w.shape[1]], s, bound)]
        if CinP > w.shape[1]:
            cm.append(Cmp(lab + " dx padding channels", got[..., w.shape[1]:], np.zeros(got[..., w.shape[1]:].shape)))
        ref, rb = self.rows(dt)
        r = f64(rows)
        assert r.shape == ref.shape, (lab, r.shape, ref.shape)
        return cm + [Cmp(lab + " bias partial rows", r, ref, rb)]

    def wgrad_ref(self, dt, acc):
        from cbr_bwd_exact import wgrad64
        d = self.bwd[dt]
        dw, ab, cnt = wgrad64(self.x, d["gz"], True)
        ref, _ = self.rows(dt)
        rows32 = ref.astype(np.float32).astype(np.float64)                      # the rows handed to the call: float32 values
        db = rows32.sum(0)
        return (dw + acc * DW_START, FACTOR * np.maximum(cnt + acc - 1, 0) * EPS32 * (ab + acc * DW_START),
                db + acc * DB_START, FACTOR * (rows32.shape[0] + acc) * EPS32 * (np.abs(rows32).sum(0) + acc * DB_START), rows32)

    def check_wgrad(self, dt, acc, dw, db):
        rdw, bdw, rdb, bdb, _ = self.wgrad_ref(dt, acc)
        lab = "%s wgrad_bias acc=%d" % (self.label(dt), acc)
        return [Cmp(lab + " dw", f64(dw), rdw, bdw), Cmp(lab + " db", f64(db), rdb, bdb)]


@functools.lru_cache(maxsize=4)
def elu_ref(Cin, B, H, W, kind, dt):
    return EluRef(Cin, B, H, W, kind, dt)


# (Cin, B, H, W, kind): dtype-specific references ("planted", "normal") are built per dtype
ELU_KEYS = [(Cin, B, H, W, "grid") for Cin in ELU_CIN for B, H, W in ELU_SHAPES] + [(Cin, 1, 17, 33, "normal") for Cin in ELU_CIN] + [(64, 1, 16, 16, "planted")]


def elu_case(key, dt):
    Cin, B, H, W, kind = key
    return elu_ref(Cin, B, H, W, kind, None if kind == "grid" else dt)

