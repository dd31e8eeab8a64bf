"""Float64 restatement of the backward of one ConvBNRelu layer -- what wm_conv3x3_bwd_fused (csrc/bwd_ws8.hip, csrc/bwd_ws.hip),
wm_conv3x3_bwd_fused16 (csrc/bwd_ws16.hip) and the two-kernel routes of engine.select_bwd_route (wm_conv3x3_dgrad_applyfused / _bwdstats /
_gvfused, wm_conv3x3_wgrad / _bnfused / _gvfused: ROUTES) compute -- written from the comments of include/wm_hip.h and of csrc/wm_common.h, with the case
tables and the per-element comparisons built on it.  A plain helper module (no fixtures, CPU only, never imports the HIP package):
tests/test_cpu_cbr_bwd_exact.py runs float32 imitations -- faithful and defective -- through these comparisons,
tests/test_gpu_cbr_bwd_exact.py runs the kernels through them.

    dy  = ca*(g*[z > 0]) + (k3 - k2*y),  z = scale*y + shift,  k2 = ca*invstd*c2,  k3 = k2*mean - ca*c1     (stats4 = scale | shift | mean |
          invstd, coef = ca | c1 | c2 as in layers_exact.BnBwdCase; premasked: g as given; gvec: g = gvec[b, co]); ROUNDED to the 16-bit
          type: it enters both GEMMs rounded
    dx[b,h,w,ci]      = sum_{kh,kw,co} dy[b, h+1-kh, w+1-kw, co] * W[co,ci,kh,kw], zero outside the image; in the 64 -> 64 one-pass form
                        times [in_scale*xr + in_shift > 0]; rounded to 16 bits
    partials          : per channel sum gz and sum gz*xr over the pixels, gz = dx AS STORED (rounded and masked)
    dW[co,ci,kh,kw] (+)= sum_{b,h,w} a[b, h+kh-1, w+kw-1, ci] * dy[b,h,w,co],  a = relu(in_scale*xr + in_shift) rounded to 16 bits, zero
                        outside the image (the image-fed first layer: a = its 16-channel image tensor, dx has no mask, and the 13 padding
                        channels of dx are exact zeros)

Data.  GRID cases make every intermediate exact: y, g, xr multiples of 1/8 in [-2, 2]; scale, in_scale, ca, invstd from {0.5, 1, 2};
shift, in_shift, mean multiples of 1/4 in [-1, 1]; k2 a multiple of 1/2 with |k2| <= 1 (c2 = k2 / (ca*invstd)); c1 multiples of 1/8;
weights multiples of 1/4 in [-1, 1]; gvec multiples of 1/8.  z is then a multiple of 1/16 (0 or >= 1/16 away from it), dy a multiple
of 1/16 with |dy| <= 9 (8 significant bits: exact in bf16 and f16), a a multiple of 1/16 with |a| <= 5.  Nothing of this is assumed: the
reference asserts rnd(dy) == dy, rnd(a) == a, z_is_exact, and per output of dx, of the partial sums and of dW that sum|terms| stays below
2**24 grid units, so that every float32 partial sum is exact in any order, whatever the tiling.  COARSE is the same with values from
{-1, -1/2, 0, 1/2, 1} and constants from {1/2, 1}, for the cases whose dW sums over tens of thousands of pixels.  There dW, the column sums
of the partial rows and dx (the 16-bit rounding of an exact sum) are compared bit for bit.

GENERIC cases (one per kernel: normal data on the scales of tests/test_gpu_conv_ops.py) get derived bounds: a float32 sum of n non-zero
terms is allowed FACTOR * (n - 1) * 2**-24 * sum|terms| (products of 16-bit operands are exact in float32); a stored 16-bit value adds
half_ulp; a dy whose float64 value lies within its own float32 error bound (the roundings each term of the expanded sum passes in the
folded evaluation of csrc/wm_common.h, counted in dy64) of a 16-bit rounding boundary may round either way: one 16-bit ulp of it, times |w| or |a|, is added to the bound of
every dx and dW entry it enters; an element whose z is layers_exact.ambiguous contributes |ca*g| the same way.  The staged activation a is
a float32 value rounded to 16 bits too (one fused multiply-add): the same rule, its ulp times |dy|, on dW; an ambiguous feeding mask lets
that one dx element be 0 or the sum.  No element is skipped.  The partial rows are, by the header's definition, sums of the dx the same
call stored: they are compared with the float64 sums of that tensor (itself compared per element), within the float32 roundings of one
workgroup's row (terms_per_row), AND with the restated sums, where every term carries its own per-element bound (partial_cmps).
The two-kernel entry points that are not given the feeding layer leave dx unmasked; dy_out is compared bit for bit on GRID data.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import detgen
from layers_exact import (rnd, store, grid, pick, normal, f64, Cmp, FACTOR, EPS32, half_ulp, SENTINEL, ambiguous, z_is_exact)

DT16 = ("bf16", "f16")
C = 64
TILE_H, TILE_W = 8, 16
MAX_WGS = 256
GVEC_MAX_BATCH = 24                                       # wm_conv3x3_bwd_fused_gvec_max_batch(); the GPU test asserts the equality
MAX_UNITS = 2.0 ** 24
# grid units (their reciprocals) of a dx term dy*w, a partial-row term gz*xr and a dW term a*dy
UNITS = {"grid": (64.0, 512.0, 256.0), "coarse": (8.0, 16.0, 16.0)}
AMBIGUOUS_CAP = 0.01
DW_START = 0.25                                           # what an accumulating call adds onto: a grid constant (SENTINEL-free, exact)
assert DW_START != SENTINEL


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------------------------------------------- host arithmetic
def fused_kernel(H, W, premasked, has_gvec):
    """wm_conv3x3_bwd_fused_kernel: 8 = csrc/bwd_ws8.hip, 1 = csrc/bwd_ws.hip"""
    return 8 if (has_gvec or premasked) and H % TILE_H == 0 and W % TILE_W == 0 else 1


def fused_nwg(B, H, W):
    """wm_conv3x3_bwd_fused_nwg"""
    return min(B * cdiv(H, TILE_H) * cdiv(W, TILE_W), MAX_WGS)


def fused16_supported(B, H, W, dt):
    """wm_conv3x3_bwd_fused16_supported"""
    return dt in DT16 and B > 0 and H > 0 and W > 0 and H % TILE_H == 0 and W % TILE_W == 0 and B * H * W * 64 <= 2 ** 31 - 2 ** 19


def fused16_nwg(B, H, W):
    """wm_conv3x3_bwd_fused16_nwg"""
    return min(B * (H // TILE_H) * (W // TILE_W), MAX_WGS)


def ntiles16(B, H, W):
    return B * cdiv(H, 16) * cdiv(W, 16)


def nparts16(B, H, W):
    """wm_conv3x3_nparts of the 64-channel MFMA input-gradient kernels: every persistent workgroup takes ceil(tiles / 256) tiles of
    16 x 16 pixels, and there are as many workgroups (one partial row each) as that needs"""
    n = ntiles16(B, H, W)
    return cdiv(n, cdiv(n, MAX_WGS))


def nslabs16(B, H, W):
    """wm_conv3x3_wgrad_nslabs: one slab per persistent workgroup, at most 256"""
    return min(ntiles16(B, H, W), MAX_WGS)


def terms_per_row16(B, H, W):
    return cdiv(ntiles16(B, H, W), MAX_WGS) * 256


def applyfused_supported(CoutY, CinP, dt):
    """wm_conv3x3_dgrad_applyfused_supported"""
    return dt in DT16 and CoutY == 64 and CinP in (64, 32)


def bwdstats_supported(CoutY, CinP, dt):
    """wm_conv3x3_dgrad_bwdstats_supported"""
    return dt in DT16 and CoutY in (64, 32) and CinP == 64


def gvfused_supported(CinX, CoutY, dt):
    """wm_conv3x3_gvfused_supported"""
    return dt in DT16 and CinX == 64 and CoutY in (64, 32)


def wgrad_bnfused_supported(CinX, CoutY, dt):
    """wm_conv3x3_wgrad_bnfused_supported"""
    return dt in DT16 and CinX <= 16 and CoutY % 64 == 0


def ntiles(B, H, W):
    return B * cdiv(H, TILE_H) * cdiv(W, TILE_W)


def terms_per_row(B, H, W):
    """pixels behind one channel of one workgroup's partial row: its run is at most ceil(tiles / workgroups) tiles of 8 x 16 pixels"""
    return cdiv(ntiles(B, H, W), fused_nwg(B, H, W)) * TILE_H * TILE_W


# ----------------------------------------------------------------------------------------------------------------- the restatement
def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2))))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def dy64(g, y, stats4, coef, masked):
    """g, y [B,H,W,C] (g broadcastable), stats4 [4,C], coef [3,C] -> dy, z, the |terms| of the expanded sum; masked: apply [z > 0] to g"""
    sc, sh, mu, isd = stats4
    ca, c1, c2 = coef
    z = sc * y + sh
    gm = np.where(z > 0, g, 0.0) if masked else g * np.ones_like(y)
    k2 = ca * isd * c2
    k3 = k2 * mu - ca * c1
    dy = ca * gm + (k3 - k2 * y)
    # float32 roundings behind each term of the expanded sum as csrc/wm_common.h evaluates it (k2: two products; k3 = fma(k2, mean,
    # -(ca*c1)); then fma(ca, g, fma(-k2, y, k3)), or with a per-sample g fma(-k2, y, fma(ca, g, k3))): ca*g passes 2 of them at most,
    # k2*y 4 (k2, and two fused multiply-adds), k2*mean 5 (k2 and three), ca*c1 4 (its product and three)
    rounded = 2 * np.abs(ca * gm) + 4 * np.abs(k2 * y) + 5 * np.abs(k2 * mu) + 4 * np.abs(ca * c1)
    return dy, z, rounded, k2


def dgrad64(dy, w, want_count):
    """dy [B,H,W,Cout], w [Cout,Cin,3,3] -> dx [B,H,W,Cin], sum|terms|, non-zero terms (or None)"""
    d = nchw(dy)
    wt = torch.from_numpy(w)
    out = nhwc(F.conv_transpose2d(d, wt, padding=1))
    ab = nhwc(F.conv_transpose2d(d.abs(), wt.abs(), padding=1))
    cnt = nhwc(F.conv_transpose2d((d != 0).double(), (wt != 0).double(), padding=1)) if want_count else None
    return out, ab, cnt


def wgrad64(a, dy, want_count):
    """a [B,H,W,Cin], dy [B,H,W,Cout] -> dW [Cout,Cin,3,3], sum|terms|, non-zero terms (or None)"""
    at, d = nchw(a), nchw(dy)
    shape = (dy.shape[3], a.shape[3], 3, 3)
    cw = torch.nn.grad.conv2d_weight
    out = cw(at, shape, d, padding=1).numpy()
    ab = cw(at.abs(), shape, d.abs(), padding=1).numpy()
    cnt = cw((at != 0).double(), shape, (d != 0).double(), padding=1).numpy() if want_count else None
    return out, ab, cnt


def spread64(slack, w):
    """slack [B,H,W,Cout] >= 0 of dy -> what it may move every dx entry it enters by"""
    return nhwc(F.conv_transpose2d(nchw(slack), torch.from_numpy(np.abs(w)), padding=1))


# ----------------------------------------------------------------------------------------------------------------- data
def _consts(n, seed, kind):
    return pick((n,), seed, (0.5, 1.0, 2.0) if kind == "grid" else (0.5, 1.0))


def _vals(shape, seed, kind, lim=2.0):
    return grid(shape, seed, 0.125, -lim, lim) if kind == "grid" else pick(shape, seed, (-1.0, -0.5, 0.0, 0.5, 1.0))


def _shifts(n, seed, kind):
    return grid((n,), seed, 0.25, -1.0, 1.0) if kind == "grid" else pick((n,), seed, (-0.5, 0.0, 0.5))


class Ref:
    """one layer's operands (float64 arrays holding dtype-exact values) and its float64 backward.  layer: "body" (64 -> 64, fed by another
    ConvBNRelu) or "first" (image-fed, 16-channel input).  gform: "g" (unmasked tensor), "premasked" (g already times [z > 0], used as
    given) or "gvec" (one row per sample).  kind: "grid", "coarse" or "normal"; dt matters for "normal" only (the operands are rounded to
    it), the exact kinds are checked for both 16-bit types."""

    def __init__(self, layer, B, H, W, gform, kind, dt, std_g=1.0):
        self.layer, self.B, self.H, self.W, self.gform, self.kind, self.dt = layer, B, H, W, gform, kind, dt
        self.exact = kind != "normal"
        self.Cin = Cin = C if layer == "body" else 3
        self.CinP = C if layer == "body" else 16
        seed = 11000 + 97 * B + 13 * H + W + {"g": 0, "premasked": 1000, "gvec": 2000}[gform] + (5000 if layer == "first" else 0)
        shp = (B, H, W, C)
        if self.exact:
            sc, sh, mu, isd = _consts(C, seed, kind), _shifts(C, seed + 1, kind), _shifts(C, seed + 2, kind), _consts(C, seed + 3, kind)
            ca = _consts(C, seed + 4, kind)
            c1 = grid((C,), seed + 5, 0.125, -1.0, 1.0) if kind == "grid" else _shifts(C, seed + 5, kind)
            k2 = pick((C,), seed + 6, (-1.0, -0.5, 0.0, 0.5, 1.0))
            c2 = k2 / (ca * isd)                                            # a power of two times k2: exact in float32
            self.y = _vals(shp, seed + 10, kind)
            g = _vals((B, C) if gform == "gvec" else shp, seed + 11, kind)
            self.in_scale, self.in_shift = _consts(C, seed + 12, kind), _shifts(C, seed + 13, kind)
            self.w = grid((C, Cin, 3, 3), seed + 14, 0.25, -1.0, 1.0) if kind == "grid" else pick((C, Cin, 3, 3), seed + 14, (-1.0, -0.5, 0.0, 0.5, 1.0))
            xin = _vals((B, H, W, C), seed + 15, kind) if layer == "body" else grid((B, H, W, 3), seed + 15, 0.125, 0.0, 1.0)
        else:
            sc, sh = normal((C,), seed, std=0.3, mean=1.0), normal((C,), seed + 1, std=0.3)
            mu, isd = normal((C,), seed + 2, std=0.2), detgen.uniform((C,), seed + 3).double().numpy() + 0.5
            cstd = 1e-5 if gform == "gvec" else 0.01
            ca, c1, c2 = normal((C,), seed + 4, std=0.2, mean=1.0), normal((C,), seed + 5, std=cstd), normal((C,), seed + 6, std=cstd)
            sc, sh, mu, isd, ca, c1, c2 = (rnd(v, "f32") for v in (sc, sh, mu, isd, ca, c1, c2))
            self.y = rnd(normal(shp, seed + 10, mean=0.2), dt)
            g = rnd(normal((B, C), seed + 11) / (H * W), "f32") if gform == "gvec" else rnd(normal(shp, seed + 11, std=std_g), dt)
            self.in_scale, self.in_shift = rnd(normal((C,), seed + 12, std=0.3, mean=1.0), "f32"), rnd(normal((C,), seed + 13, std=0.3), "f32")
            self.w = rnd(normal((C, Cin, 3, 3), seed + 14, std=0.05 if layer == "body" else 0.2), dt)     # exact in dt: the pack rounds nothing
            xin = rnd(normal((B, H, W, C), seed + 15, mean=0.1), dt) if layer == "body" else rnd(detgen.uniform((B, H, W, 3), seed + 15).double().numpy(), dt)
        self.stats4, self.coef = np.stack([sc, sh, mu, isd]), np.stack([ca, c1, c2])
        if gform == "premasked":                                           # the contract: such a g is already multiplied by this layer's mask
            g = np.where(sc * self.y + sh > 0, g, 0.0)
        self.g = g
        if layer == "body":
            self.xr = xin
        else:
            self.x16 = np.concatenate([xin, np.zeros((B, H, W, 13))], axis=3)
        self._backward()

    # ---- the float64 backward and its bounds
    def _backward(self):
        B, H, W = self.B, self.H, self.W
        gfull = self.g[:, None, None, :] if self.gform == "gvec" else self.g
        dy, self.z, terms, _ = dy64(gfull, self.y, self.stats4, self.coef, masked=self.gform != "premasked")
        sc, sh = self.stats4[0], self.stats4[1]
        ca = self.coef[0]
        dts = DT16 if self.exact else (self.dt,)
        if self.exact:
            for dt in dts:
                assert z_is_exact(self.z, dt), "z off its grid"
                assert np.array_equal(rnd(dy, dt), dy), "dy is not exact in %s" % dt
            self.dyq, slack = dy, None
            self.dy_raw, self.dy_f32_bound = dy, np.zeros(dy.shape)
            self.amb_share = 0.0
        else:
            dt = self.dt
            e = FACTOR * EPS32 * terms                                      # dy's own float32 error bound (terms: weighted by their roundings)
            self.dyq = rnd(dy, dt)
            lo, hi = rnd(dy - e, dt), rnd(dy + e, dt)
            amb_r = lo != hi                                                # a rounding boundary within the float32 error: either way
            amb_z = ambiguous(self.z, sc, self.y, sh) if self.gform != "premasked" else np.zeros(dy.shape, dtype=bool)
            slack = np.where(amb_r, hi - lo, 0.0) + np.where(amb_z, np.abs(ca * gfull), 0.0)
            self.dy_raw, self.dy_f32_bound = dy, e + np.where(amb_z, np.abs(ca * gfull), 0.0)
            self.amb_r_share, self.amb_z_share = float(amb_r.mean()), float(amb_z.mean())
            self.amb_share = float((amb_r | amb_z).mean())
        # the staged activation of the feeding layer / the image
        if self.layer == "body":
            zin = self.in_scale * self.xr + self.in_shift
            self.zin = zin
            a = np.maximum(zin, 0.0)
            self.mask_in = zin > 0
            if self.exact:
                for dt in dts:
                    assert z_is_exact(zin, dt) and np.array_equal(rnd(a, dt), a), "a is not exact in %s" % dt
                self.a, slack_a, self.amb_in = a, None, None
            else:
                ein = FACTOR * EPS32 * (np.abs(self.in_scale * self.xr) + np.abs(self.in_shift))      # one fused multiply-add
                self.a = rnd(a, self.dt)
                alo, ahi = rnd(np.maximum(zin - ein, 0.0), self.dt), rnd(np.maximum(zin + ein, 0.0), self.dt)
                slack_a = np.maximum(ahi - self.a, self.a - alo)            # relu and the rounding are monotone: covers mask and boundary
                self.amb_in = ambiguous(zin, self.in_scale, self.xr, self.in_shift)
        else:
            self.a, slack_a, self.amb_in, self.mask_in = self.x16[..., :3], None, None, None
        # dx
        want = not self.exact
        s, ab, cnt = dgrad64(self.dyq, self.w, want)
        self.dx_absum = ab
        if self.exact:
            assert ab.max() * UNITS[self.kind][0] < MAX_UNITS, "dx: sum|terms| = %g units" % (ab.max() * UNITS[self.kind][0])
            self.dx_raw = s
            self.dx_f32_bound = np.zeros(s.shape)
        else:
            self.dx_raw = s
            self.dx_f32_bound = FACTOR * np.maximum(cnt - 1, 0) * EPS32 * ab + spread64(slack, self.w)
        # dW
        dw, wab, wcnt = wgrad64(self.a, self.dyq, want)
        self.dw, self.dw_absum = dw, wab
        if self.exact:
            assert (wab.max() + DW_START) * UNITS[self.kind][2] < MAX_UNITS, "dW: sum|terms| = %g units" % (wab.max() * UNITS[self.kind][2])
            self.dw_bound = {0: 0.0, 1: 0.0}
        else:
            amb = wgrad64(np.abs(self.a), slack, False)[0]
            if slack_a is not None:
                amb = amb + wgrad64(slack_a, np.abs(self.dyq) + slack, False)[0]
            self.dw_bound = {acc: FACTOR * np.maximum(wcnt + acc - 1, 0) * EPS32 * (wab + acc * DW_START) + amb for acc in (0, 1)}

    # ---- per stored dtype
    def dy_ref(self, dt):
        """(dy, its bound): GRID the stored value, exact; GENERIC the float64 value within its float32 bound (+ |ca*g| at an ambiguous
        mask) and the half ulp of the store"""
        if self.exact:
            return self.dyq, self.dy_f32_bound
        return self.dy_raw, self.dy_f32_bound + half_ulp(np.abs(self.dy_raw) + self.dy_f32_bound, dt)

    def dx_ref(self, dt, masked=True, CinP=None):
        """(dx, its bound) [B,H,W,CinP]: the sum (GRID: as stored, rnd(sum)) * mask; the padding channels of the first layer: exact zeros.
        masked False: the two-kernel entry points that leave the feeding layer's mask to the consumer"""
        if self.exact:
            r, b = rnd(self.dx_raw, dt), self.dx_f32_bound                   # the 16-bit rounding of an exact float32 sum: bit for bit
        else:
            r = self.dx_raw                                                 # the float64 sum itself; the store adds half an ulp
            b = self.dx_f32_bound + half_ulp(np.abs(r) + self.dx_f32_bound, dt)
        if self.layer == "body" and not masked:
            return r, b * np.ones_like(r)
        if self.layer == "body":
            sure0 = ~self.mask_in
            if self.amb_in is not None:
                b = np.where(self.amb_in, np.abs(r) + b, b)                 # an ambiguous feeding mask: 0 or the sum
                sure0 = sure0 & ~self.amb_in
            return np.where(self.mask_in, r, 0.0), np.where(sure0, 0.0, b)  # a surely masked element is an exact zero
        z13 = np.zeros(r.shape[:3] + ((CinP or self.CinP) - 3,))
        return np.concatenate([r, z13], axis=3), np.concatenate([b * np.ones_like(r), z13], axis=3)

    def sums_ref(self, dt):
        """GRID: the column sums of the partial rows (sum gz, sum gz*xr) [2,C], exact; asserts their sum|terms| in grid units"""
        gz, _ = self.dx_ref(dt)
        t2 = gz * self.xr
        u = UNITS[self.kind]
        assert np.abs(gz).sum((0, 1, 2)).max() * u[0] < MAX_UNITS and np.abs(t2).sum((0, 1, 2)).max() * u[1] < MAX_UNITS, "partial sums leave 2**24 units"
        return np.stack([gz.sum((0, 1, 2)), t2.sum((0, 1, 2))])


@functools.lru_cache(maxsize=3)
def reference(layer, B, H, W, gform, kind, dt, std_g=1.0):
    """dt: None for the exact kinds (one reference serves both 16-bit types), the storage type for "normal\""""
    return Ref(layer, B, H, W, gform, kind, dt, std_g)


# ----------------------------------------------------------------------------------------------------------------- comparisons
def dy_cmps(r, lab, dt, dy):
    ref, bound = r.dy_ref(dt)
    return [Cmp(lab + " dy_out", f64(dy).reshape(ref.shape), ref, bound)]


def dx_cmps(r, lab, dt, dx, masked, CinP):
    got = f64(dx).reshape(r.B, r.H, r.W, CinP)
    ref, bound = r.dx_ref(dt, masked, CinP)
    if r.layer == "body":
        return [Cmp(lab + " dx", got, ref, bound)]
    return [Cmp(lab + " dx", got[..., :3], ref[..., :3], bound[..., :3]), Cmp(lab + " dx padding channels", got[..., 3:], ref[..., 3:])]


def partial_cmps(r, lab, dt, dx, partials, nrows, n):
    """partials [nrows,2,64] beside the (masked) dx of the same call; n: the terms behind one channel of one row.  GRID: the column sums
    against the restated ones, exact.  GENERIC, two comparisons: (1) against the float64 sums of the dx the call stored -- the header's
    definition, gz = dx as stored -- within the row's float32 roundings: n - 1 additions (+ 1: the product gz*xr); (2) against the
    restated sums, independent of any kernel output: every term may differ from the restated one by its own per-element bound (the
    half ulp of the store and the ambiguity included), plus the same float32 roundings on |restated| + bound"""
    got, p = f64(dx).reshape(r.B, r.H, r.W, C), f64(partials)
    assert p.shape == (nrows, 2, C), p.shape
    col, ax = p.sum(0), (0, 1, 2)
    if r.exact:
        s = r.sums_ref(dt)
        return [Cmp(lab + " partials sum gz", col[0], s[0]), Cmp(lab + " partials sum gz*xr", col[1], s[1])]
    t2 = got * r.xr
    cm = [Cmp(lab + " partials sum gz", col[0], got.sum(ax), FACTOR * (n - 1) * EPS32 * np.abs(got).sum(ax)),
          Cmp(lab + " partials sum gz*xr", col[1], t2.sum(ax), FACTOR * n * EPS32 * np.abs(t2).sum(ax))]
    ref, b = r.dx_ref(dt)
    hi, xa = np.abs(ref) + b, np.abs(r.xr)
    cm += [Cmp(lab + " partials sum gz (restated)", col[0], ref.sum(ax), b.sum(ax) + FACTOR * (n - 1) * EPS32 * hi.sum(ax)),
           Cmp(lab + " partials sum gz*xr (restated)", col[1], (ref * r.xr).sum(ax), (b * xa).sum(ax) + FACTOR * n * EPS32 * (hi * xa).sum(ax))]
    return cm


def dw_cmps(r, lab, dw, accumulate):
    a = 1 if accumulate else 0
    return [Cmp(lab + " dW", f64(dw).reshape(r.dw.shape), r.dw + a * DW_START, r.dw_bound[a])]


# ----------------------------------------------------------------------------------------------------------------- cases
class Case:
    """one call of a one-pass kernel: kernel in ("ws8", "ws", "ws16") is the path the case is there for"""

    def __init__(self, kernel, B, H, W, gform, kind="grid", reverse=False, accumulate=False, why=""):
        self.kernel, self.B, self.H, self.W, self.gform, self.kind, self.reverse, self.accumulate, self.why = kernel, B, H, W, gform, kind, reverse, accumulate, why
        self.layer = "first" if kernel == "ws16" else "body"
        self.premasked = gform == "premasked"
        self.CinP, self.dx_masked = (C, True) if self.layer == "body" else (16, False)

    @property
    def id(self):
        return "%s-%dx%dx%d-%s-%s%s%s" % (self.kernel, self.B, self.H, self.W, self.gform, self.kind, "-rev" if self.reverse else "", "-acc" if self.accumulate else "")

    def label(self, dt):
        return "%s %s %dx%dx%d %s %s%s%s" % (self.kernel, dt, self.B, self.H, self.W, self.gform, self.kind, " reverse" if self.reverse else "",
                                             " accumulate" if self.accumulate else "")

    def ref(self, dt):
        exact = self.kind != "normal"
        return reference(self.layer, self.B, self.H, self.W, self.gform, self.kind, None if exact else dt, 0.1 if self.layer == "first" and not exact else 1.0)

    def expected_nwg(self):
        return fused16_nwg(self.B, self.H, self.W) if self.kernel == "ws16" else fused_nwg(self.B, self.H, self.W)

    def check_dispatch(self, dt, kernel_fn=fused_kernel, nwg_fn=None, supported16_fn=fused16_supported):
        """the case reaches the kernel it is there for; the functions default to the restated arithmetic, the GPU test passes the library's"""
        B, H, W = self.B, self.H, self.W
        if self.kernel == "ws16":
            assert supported16_fn(B, H, W, dt), self.label(dt)
            assert (nwg_fn or fused16_nwg)(B, H, W) == fused16_nwg(B, H, W), self.label(dt)
        else:
            k = kernel_fn(H, W, int(self.premasked), int(self.gform == "gvec"))
            assert k == fused_kernel(H, W, self.premasked, self.gform == "gvec") == (8 if self.kernel == "ws8" else 1), (self.label(dt), k)
            assert (nwg_fn or fused_nwg)(B, H, W) == fused_nwg(B, H, W), self.label(dt)
            assert self.gform != "gvec" or B <= GVEC_MAX_BATCH

    tile_h, tile_w = TILE_H, TILE_W

    def check(self, dt, dx, partials, dw, what=""):
        """dx [B,H,W,CinP] as stored, partials [nwg,2,64] or None (ws16), dw [64,Cin,3,3] after the call -> comparisons"""
        r, lab = self.ref(dt), self.label(dt) + what
        cm = dx_cmps(r, lab, dt, dx, True, r.CinP)
        if partials is not None:
            cm += partial_cmps(r, lab, dt, dx, partials, self.expected_nwg(), terms_per_row(r.B, r.H, r.W))
        return cm + dw_cmps(r, lab, dw, self.accumulate)

    def ambiguous_share(self, dt):
        return self.ref(dt).amb_share


G, PM, GV = "g", "premasked", "gvec"
CASES = (
    # csrc/bwd_ws8.hip: whole tiles, a premasked tensor gradient or a per-sample gradient
    Case("ws8", 1, 8, 16, PM, why="one tile, all four borders in it"),
    Case("ws8", 1, 16, 32, PM, accumulate=True, why="2 x 2 tiles, every seam"),
    Case("ws8", 2, 8, 32, PM, why="a sample seam beside a tile seam"),
    Case("ws8", 3, 80, 144, PM, kind="coarse", why="270 tiles: runs of two and of one"),
    Case("ws8", 3, 80, 144, PM, kind="coarse", reverse=True, accumulate=True, why="270 tiles, reverse"),
    Case("ws8", 2, 8, 16, GV, why="gvec"),
    Case("ws8", GVEC_MAX_BATCH, 8, 16, GV, kind="coarse", accumulate=True, why="gvec at the largest batch, one tile per sample"),
    Case("ws8", 2, 16, 32, PM, kind="normal", accumulate=True, why="GENERIC"),
    # csrc/bwd_ws.hip: an unmasked g on whole tiles (ALIGNED), ragged shapes with every g form
    Case("ws", 1, 8, 16, G, why="ALIGNED, one tile"),
    Case("ws", 1, 16, 32, G, accumulate=True, why="ALIGNED, 2 x 2 tiles"),
    Case("ws", 1, 1, 1, G, why="one pixel"),
    Case("ws", 1, 1, 1, PM, why="one pixel, premasked"),
    Case("ws", 1, 7, 15, G, why="one ragged tile"),
    Case("ws", 1, 7, 15, PM, accumulate=True, why="premasked on a ragged shape selects kernel 1"),
    Case("ws", 1, 9, 17, G, why="2 x 2 tiles, three of them slivers"),
    Case("ws", 1, 9, 17, GV, why="gvec on a ragged shape"),
    Case("ws", 2, 13, 37, G, accumulate=True, why="ragged, two samples"),
    Case("ws", 2, 13, 37, PM, why="ragged, two samples, premasked"),
    Case("ws", 2, 13, 37, GV, why="ragged, two samples, gvec"),
    Case("ws", 3, 75, 140, G, kind="coarse", why="270 ragged tiles"),
    Case("ws", 3, 75, 140, G, kind="coarse", reverse=True, accumulate=True, why="270 ragged tiles, reverse"),
    Case("ws", 5, 8, 200, G, kind="coarse", why="one tile row"),
    Case("ws", 2, 16, 16, G, why="one tile column"),
    Case("ws", 2, 13, 37, G, kind="normal", accumulate=True, why="GENERIC"),
    # csrc/bwd_ws16.hip: the image-fed first layer
    Case("ws16", 1, 8, 16, G, why="one tile"),
    Case("ws16", 1, 8, 16, PM, accumulate=True, why="one tile, premasked"),
    Case("ws16", 1, 16, 32, G, accumulate=True, why="2 x 2 tiles"),
    Case("ws16", 1, 16, 32, PM, why="2 x 2 tiles, premasked"),
    Case("ws16", 2, 8, 32, G, why="a sample seam beside a tile seam"),
    Case("ws16", 2, 8, 32, PM, accumulate=True, why="the same, premasked"),
    Case("ws16", 3, 80, 144, G, kind="coarse", accumulate=True, why="270 tiles"),
    Case("ws16", 3, 80, 144, PM, kind="coarse", reverse=True, why="270 tiles, reverse, premasked"),
    Case("ws16", 2, 16, 32, G, kind="normal", accumulate=True, why="GENERIC"),
)


# ----------------------------------------------------------------------------------------------------------------- two-kernel routes
# route of engine.select_bwd_route -> the layer it belongs to, the form of g, the entry points it runs (in this order)
ROUTES = {
    "body_two_kernels": ("body", G, ("dgrad_applyfused", "wgrad", "dgrad_bwdstats")),      # (+ wm_conv3x3_dgrad_bwdstats on the dy it wrote)
    "dx_only": ("body", G, ("dgrad_applyfused",)),                                        # want_dy = False, no feeding sums: dx unmasked
    "pooled": ("body", GV, ("wgrad_gvfused", "dgrad_gvfused")),
    "pooled_feed": ("body", GV, ("dgrad_bwdstats", "wgrad_gvfused")),
    "first_two_kernels": ("first", G, ("dgrad_applyfused", "wgrad")),                     # body_two_kernels of an image-fed layer: CinP = 32
    "first_layer_weights_only": ("first", G, ("wgrad_bnfused",)),
}


class Route:
    """one two-kernel route on one shape: 16 x 16 tiles, one partial row / slab per persistent workgroup (nparts16)"""
    tile_h = tile_w = 16
    premasked = False

    def __init__(self, route, B, H, W, kind="grid", reverse=False, accumulate=False, dts=DT16, why=""):
        self.route, self.B, self.H, self.W, self.kind, self.reverse, self.accumulate, self.dts, self.why = route, B, H, W, kind, reverse, accumulate, dts, why
        self.layer, self.gform, self.entries = ROUTES[route]
        self.kernel = route
        self.CinP = C if self.layer == "body" else 32
        self.dx_masked = route in ("body_two_kernels", "pooled_feed")                     # the entry points that were given the feeding layer
        self.outputs = {"body_two_kernels": ("dy", "dx", "partials", "dw", "dx_b", "partials_b"), "dx_only": ("dx",), "pooled": ("dx", "dw"),
                        "pooled_feed": ("dx", "partials", "dw"), "first_two_kernels": ("dy", "dx", "dw"), "first_layer_weights_only": ("dw",)}[route]

    @property
    def id(self):
        return "%s-%dx%dx%d-%s%s%s" % (self.route, self.B, self.H, self.W, self.kind, "-rev" if self.reverse else "", "-acc" if self.accumulate else "")

    def label(self, dt):
        return "%s %s %dx%dx%d %s%s%s" % (self.route, dt, self.B, self.H, self.W, self.kind, " reverse" if self.reverse else "", " accumulate" if self.accumulate else "")

    ref = Case.ref
    ambiguous_share = Case.ambiguous_share

    def expected_nwg(self):
        return nparts16(self.B, self.H, self.W)

    def check_dispatch(self, dt, supported=None, nparts_fn=None, nslabs_fn=None):
        """every entry point of the route takes this layer (supported: name -> the library's *_supported(a, b, dt), default the restated
        ones) and the row / slab count is the restated one"""
        own = {"dgrad_applyfused": applyfused_supported, "dgrad_bwdstats": bwdstats_supported, "dgrad_gvfused": gvfused_supported,
               "wgrad_gvfused": gvfused_supported, "wgrad_bnfused": wgrad_bnfused_supported}
        args = {"dgrad_applyfused": (64, self.CinP), "dgrad_bwdstats": (64, 64), "dgrad_gvfused": (64, 64), "wgrad_gvfused": (64, 64), "wgrad_bnfused": (16, 64)}
        for e in self.entries:
            if e in own:
                assert own[e](*args[e], dt) and (supported is None or supported[e](*args[e], dt)), (self.label(dt), e)
        shape = (self.B, self.H, self.W)
        assert nparts_fn is None or nparts_fn(*shape, dt) == nparts16(*shape), self.label(dt)
        assert nslabs_fn is None or nslabs_fn(*shape) == nslabs16(*shape), self.label(dt)

    def check(self, dt, out):
        """out: dict of the route's outputs (dy, dx, partials, dw; dx_b, partials_b: wm_conv3x3_dgrad_bwdstats on the dy the route wrote)"""
        assert set(out) == set(self.outputs), (sorted(out), self.outputs)
        r, lab = self.ref(dt), self.label(dt)
        n, rows = terms_per_row16(r.B, r.H, r.W), self.expected_nwg()
        cm = []
        if "dy" in out:
            cm += dy_cmps(r, lab, dt, out["dy"])
        if "dx" in out:
            cm += dx_cmps(r, lab, dt, out["dx"], self.dx_masked, self.CinP)
        if "partials" in out:
            cm += partial_cmps(r, lab, dt, out["dx"], out["partials"], rows, n)
        if "dw" in out:
            cm += dw_cmps(r, lab, out["dw"], self.accumulate)
        if "dx_b" in out:
            cm += dx_cmps(r, lab + " bwdstats(dy)", dt, out["dx_b"], True, C) + partial_cmps(r, lab + " bwdstats(dy)", dt, out["dx_b"], out["partials_b"], rows, n)
        return cm


ROUTE_SHAPES = ((1, 16, 16), (1, 17, 33), (2, 32, 32))
MANY_TILES = (1, 16, 16 * 257)                             # 257 tiles of 16 x 16: the persistent loops run two tiles somewhere; 8.4 MB a tensor


def _route_cases():
    rows = []
    for route in ROUTES:
        for k, (B, H, W) in enumerate(ROUTE_SHAPES):
            kind = "coarse" if B * H * W > 1024 else "grid"        # the partial sums of 2048 pixels leave 2**24 units of the fine grid
            rows.append(Route(route, B, H, W, kind, reverse=k == 1, accumulate=k != 1))
        rows.append(Route(route, 1, 17, 33, "normal", accumulate=True, why="GENERIC"))
    rows.append(Route("body_two_kernels", *MANY_TILES, kind="coarse", reverse=True, dts=("bf16",), why="257 tiles on 256 workgroups"))
    return tuple(rows)


ROUTE_CASES = _route_cases()
ROUTE_IDS = tuple(c.id for c in ROUTE_CASES)
assert len(set(ROUTE_IDS)) == len(ROUTE_IDS)


def route_case(cid):
    return ROUTE_CASES[ROUTE_IDS.index(cid)]


def route_keys():
    return [(c.id, dt) for c in ROUTE_CASES for dt in c.dts]


CASE_IDS = tuple(c.id for c in CASES)
assert len(set(CASE_IDS)) == len(CASE_IDS)


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def operands(c, dt):
    """the tensors of one call, on the CPU: dict of g / gvec, y, stats4, coef, w (float32, exact in dt), xr / x16, in_scale, in_shift, dw0"""
    r = c.ref(dt)
    o = {"y": store(r.y, dt), "stats4": store(r.stats4, "f32"), "coef": store(r.coef, "f32"), "w": store(r.w, "f32"),
         "dw0": torch.full(r.dw.shape, DW_START if c.accumulate else 0.0, dtype=torch.float32)}
    if c.gform == "gvec":
        o["gvec"] = store(r.g, "f32")
    else:
        o["g"] = store(r.g, dt)
    if c.layer == "body":
        o.update(xr=store(r.xr, dt), in_scale=store(r.in_scale, "f32"), in_shift=store(r.in_shift, "f32"))
    else:
        o["x16"] = store(r.x16, dt)
    return o
