"""The per-element comparisons of tests/imgloss_exact.py without a GPU.  Per kernel family one faithful imitation -- the streaming kernels'
split16 / stream16 walked trip by trip with the terms in double, GradientLoss in gather form, ExclusionLoss tile by tile in float32 with
its halo and in-tile pooling, SSIM_Loss in float32 with contraction off and the gather's multiplicities -- passes every comparison of every
case the GPU file runs, and each named defect, applied to the imitation, FAILS a comparison of a named case.  The case tables assert their
own coverage, the either-way shares stay under their cap from the float64 reference alone, and COUNT images saturate the float32
sigmoid.  So a green tests/test_gpu_imgloss_exact.py means something."""
import numpy as np
import pytest

import imgloss_exact as IX

f32, f64t = np.float32, np.float64


def must_pass(cmps):
    for c in cmps:
        c.assert_ok()
        assert c.skipped == 0
    return cmps


def must_fail(cmps, defect, named):
    bad = [c.line() for c in cmps if not c.ok]
    assert bad, "the defect `%s` passed every comparison of %s" % (defect, named)
    assert any(named in b and "first at element [" in b for b in bad), (defect, named, bad[0])
    return bad[0]


def fma32(a, b, c):
    return (np.asarray(a, dtype=f64t) * np.asarray(b, dtype=f64t) + np.asarray(c, dtype=f64t)).astype(f32)


# ----------------------------------------------------------------------------------------------------------------- stream16, trip by trip
def walk(n, offs, G, defect=None):
    """(element, workgroup) of everything G workgroups of 256 threads touch, in the order of the two loops of stream16"""
    head = min((4 - offs[0]) % 4, n)
    same = all((o - offs[0]) % 4 == 0 for o in offs)
    nv = (n - head) // 4 if same else 0
    tail0 = head + 4 * ((n - head) // 4)
    if nv == 0 and defect != "scalar fallback indexed with the vector offsets":
        head, tail0 = 0, 0
    elif nv == 0:
        pass                                              # head and tail0 of the float4 split kept while nothing is read as float4
    else:
        tail0 = head + 4 * nv
    stride = G * 256
    lane = np.arange(stride)
    el, wg = [], []
    for trip in range(-(-nv // stride) if nv else 0):
        if trip > 0 and defect == "the second trip of the stride loop skipped":
            break
        v = lane + trip * stride
        keep = v < nv
        el.append((head + 4 * v[keep])[:, None] + np.arange(4)[None, :])
        wg.append(np.repeat(lane[keep] // 256, 4).reshape(-1, 4))
    nscalar = head + (n - tail0)
    for trip in range(-(-nscalar // stride)):
        if trip > 0 and defect == "the second trip of the stride loop skipped":
            break
        i = lane + trip * stride
        keep = i < nscalar
        i, w = i[keep], lane[keep] // 256
        if defect == "tail dropped":
            i, w = i[i < head], w[i < head]
        idx = np.where(i < head, i, tail0 + (i - head))
        el.append(idx)
        wg.append(w)
        if defect == "head counted twice":
            el.append(idx[i < head])
            wg.append(w[i < head])
    if not el:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate([e.reshape(-1) for e in el]).astype(np.int64), np.concatenate([w.reshape(-1) for w in wg]).astype(np.int64)


def store_walk(dest, el, values, accumulate, defect=None):
    """the gradient store over a walk: dest[el] = v, or with accumulate fl(dest[el] + fl(v)) once per visit"""
    times = np.bincount(el, minlength=dest.size)
    v32 = values.astype(f32)
    for k in range(1, int(times.max()) + 1 if times.size else 1):
        at = times >= k
        if not accumulate:
            dest[at] = v32[at]
        elif defect == "accumulate added in double instead of float":
            dest[at] = (values[at] + dest[at].astype(f64t)).astype(f32)
        else:
            dest[at] = dest[at] + v32[at]
    return dest


class Imitation:
    """the engine tests/imgloss_exact.py's drivers call: every entry point in numpy, with one named defect or none"""

    def __init__(self, defect=None):
        self.defect, self.guards = defect, []

    # ------------------------------------------------------------------------------------------------------------- reconstruction
    def recon_fwd(self, c):
        part = np.zeros((c.B, c.P))
        for b in range(c.B):
            el, wg = walk(c.per, c.sample_offs(b, c.offs[:2]), c.P, self.defect)
            part[b] = np.bincount(wg, weights=c.terms[b][el], minlength=c.P)
        return part, np.array([part.sum() * (1.0 / c.B)]).astype(f32)

    def recon_bwd(self, c, m):
        k = IX.up_of(m) / f64t(c.B)
        acc = bool(m.get("accumulate"))
        out = (c.old if acc else np.full((c.B, c.per), IX.SENTINEL)).astype(f32)
        for b in range(c.B):
            d = c.d[b]
            v = (2.0 * d) * k if c.kind == "l2" else d / np.sqrt(d * d + c.eps) * k if c.kind == "l_char" else np.full(c.per, k)
            el, _ = walk(c.per, c.sample_offs(b, c.offs), c.G, self.defect)
            store_walk(out[b], el, v, acc, self.defect)
        return out

    # ------------------------------------------------------------------------------------------------------------- pixel losses
    def pix_fwd(self, c):
        el, wg = walk(c.n, c.sums_offs(), c.P, self.defect)
        part = np.stack([np.bincount(wg, weights=t[el], minlength=c.P) for t in (c.t0, c.t1)], 1)
        m0, m1 = part[:, 0].sum() / f64t(c.n), part[:, 1].sum() / f64t(c.n)
        with np.errstate(divide="ignore", invalid="ignore"):
            loss = m0 / m1 if c.kind == "maskl1" else 1.0 - m0 if c.kind == "nonblurry" else 1.0 / m0
        return part, np.array([m0, m1]), np.array([loss]).astype(f32)

    def pix_bwd(self, c, coef, m):
        g, n, acc = IX.up_of(m), f64t(c.n), bool(m.get("accumulate"))
        coef = IX.f64(coef)
        if c.kind == "maskl1":
            v = (g / (n * coef[1])) * (np.sign(c.dm) * c.m)
        elif c.kind == "nonblurry":
            v = ((-2.0 * g) / n) * c.dm
        else:
            v = ((-g) / ((n * coef[0]) * coef[0])) * np.sign(c.dm)
        el, _ = walk(c.n, c.bwd_offs(), c.G, self.defect)
        out = []
        for name, sign, old in (("ga", 1.0, c.old_a), ("gb", -1.0, c.old_b)):
            if c.want not in ("both", name):
                out.append(None)
                continue
            if name == "gb" and self.defect == "gb given ga's sign":
                sign = 1.0
            dest = (old if acc else np.full(c.n, IX.SENTINEL)).astype(f32)
            out.append(store_walk(dest, el, sign * v, acc, self.defect))
        return out

    # ------------------------------------------------------------------------------------------------------------- GradientLoss
    def gradl_fwd(self, c):
        N, H, W = c.a.shape
        a = c.a
        tx, ty = np.zeros(a.shape), np.zeros(a.shape)
        tx[:, :, :-1] = np.abs(a[:, :, :-1] - a[:, :, 1:])
        ty[:, :-1, :] = np.abs(a[:, :-1, :] - a[:, 1:, :])
        if self.defect == "the last row's x-differences dropped":
            tx[:, -1, :] = 0.0
        wg = (np.arange(H * W) // 256) % c.P
        part = np.stack([np.stack([np.bincount(wg, weights=t[n].reshape(-1), minlength=c.P) for t in (tx, ty)], 1) for n in range(N)])
        cx, cy = (c.cy, c.cx) if self.defect == "divisors swapped" else (c.cx, c.cy)
        return part, np.array([part[..., 0].sum() / cx + part[..., 1].sum() / cy]).astype(f32)

    def gradl_bwd(self, c, m):
        g = IX.up_of(m)
        cx, cy = (c.cy, c.cx) if self.defect == "divisors swapped" else (c.cx, c.cy)
        gx, gy = g / cx, g / cy
        a = c.a.astype(f32)

        def sgn(d):
            if self.defect == "a subnormal difference flushed":
                d = np.where(np.abs(d) < f32(2.0 ** -126), f32(0), d)
            s = np.sign(d).astype(f64t)
            return np.where(d == 0, 1.0, s) if self.defect == "sgn(0) = 1" else s
        nx, ny = np.zeros(a.shape), np.zeros(a.shape)
        nx[:, :, :-1] += sgn(a[:, :, :-1] - a[:, :, 1:])
        nx[:, :, 1:] -= sgn(a[:, :, :-1] - a[:, :, 1:])
        ny[:, :-1, :] += sgn(a[:, :-1, :] - a[:, 1:, :])
        ny[:, 1:, :] -= sgn(a[:, :-1, :] - a[:, 1:, :])
        r = (nx * gx + ny * gy).astype(f32)
        return c.old.astype(f32) + r if m.get("accumulate") else r

    # ------------------------------------------------------------------------------------------------------------- ExclusionLoss
    @staticmethod
    def _sig(d):
        with np.errstate(over="ignore"):
            return (f32(1) / (f32(1) + np.exp(-d))) * f32(2) - f32(1)

    @staticmethod
    def _pool(a):
        h, w = a.shape[-2] // 2, a.shape[-1] // 2
        return (((a[..., 0:2 * h:2, 0:2 * w:2] + a[..., 0:2 * h:2, 1:2 * w:2]) + a[..., 1:2 * h:2, 0:2 * w:2]) + a[..., 1:2 * h:2, 1:2 * w:2]) * f32(0.25)

    def excl_fwd(self, c, off):
        """tile by tile: the tile of every channel with its 4-pixel halo below and right (zero outside the image), pooled in the tile"""
        d = self.defect
        imgs = np.concatenate([c.img1, c.img2], 1).astype(f32)
        B, nch, H, W = imgs.shape
        R0, C0 = IX.ETH + 4, IX.ETW + 4
        part = np.zeros((c.nslots, c.nwg))
        up = (lambda n, l: -(-n // (1 << l))) if d == "ceil pooling" else (lambda n, l: n >> l)
        for b in range(B):
            for ty in range(c.ty):
                for tx in range(c.tx):
                    y0, x0 = ty * IX.ETH, tx * IX.ETW
                    t = np.zeros((nch, R0, C0), dtype=f32)
                    h, w = min(R0, H - y0), min(C0, W - x0)
                    if d == "halo read as zero":
                        h, w = min(h, IX.ETH), min(w, IX.ETW)
                    t[:, :h, :w] = imgs[b, :, y0:y0 + h, x0:x0 + w]
                    wg = (b * c.ty + ty) * c.tx + tx
                    for l in range(c.levels):
                        Hl, Wl, th, tw, Y0, X0 = up(H, l), up(W, l), IX.ETH >> l, IX.ETW >> l, y0 >> l, x0 >> l
                        rr, cc = np.arange(th)[:, None], np.arange(tw)[None, :]
                        inside = (Y0 + rr < Hl) & (X0 + cc < Wl)
                        for dr in range(2):
                            last = Hl + 1 if (d == "a pooled pixel of the odd last row counted" and l > 0 and dr == 0) else Hl
                            ok = inside & ((Y0 + rr + 1 < last) if dr == 0 else (X0 + cc + 1 < Wl))
                            if d == "a seam difference dropped" and dr == 0:
                                ok = ok & (rr + 1 < th)
                            second = t[:, 1:th + 1, :tw] if dr == 0 else t[:, :th, 1:tw + 1]
                            s = self._sig(second - t[:, :th, :tw])
                            sq = s * s
                            for i2 in range(c.C2):
                                for i1 in range(c.C1):
                                    k = i1 * c.C2 + i2 if d == "i1 and i2 transposed" else i2 * c.C1 + i1
                                    part[(l * 2 + dr) * c.CC + k, wg] = (sq[i1] * sq[c.C1 + i2]).astype(f64t)[ok].sum()
                        t = self._pool(t)
        means, coef, term = np.zeros(c.nslots), np.zeros(c.nslots), np.zeros(c.nslots)
        for s in range(c.nslots):
            l, dr = (s // c.CC) >> 1, (s // c.CC) & 1
            Hl, Wl = f64t(up(H, l)), f64t(up(W, l))
            cnt = f64t(B) * ((Hl - 1.0) * Wl if dr == 0 else Hl * (Wl - 1.0))
            if d == "a level-2 divisor off by one row" and l == 2 and dr == 0:
                cnt = f64t(B) * Hl * Wl
            m = part[s].sum() / cnt
            r = np.sqrt(np.sqrt(m))
            means[s], term[s] = m, r
            coef[s] = 0.25 / (r * r * r) / c.norm / cnt if m > 0 else 0.0
        return part, means, coef, np.array([term.sum() / c.norm]).astype(f32)

    def excl_bwd(self, c, coef, want, m, off):
        """gather form on whole planes: levels 2 and 1 first (times 4**-level), then level 0 adds its own and those above it"""
        cf = (IX.f64(coef) * IX.up_of(m)).astype(f32)
        lv = [np.concatenate([c.img1, c.img2], 1).astype(f32)]
        for l in range(1, c.levels):
            lv.append(self._pool(lv[-1]))
        C1, C2 = c.C1, c.C2
        ups = []
        g0 = None
        for l in range(c.levels - 1, -1, -1):
            a = lv[l]
            B, nch, hl, wl = a.shape
            g = np.zeros(a.shape, dtype=f32)
            for dr in range(2):
                base = (l * 2 + dr) * c.CC
                s = self._sig((a[:, :, 1:, :] - a[:, :, :-1, :]) if dr == 0 else (a[:, :, :, 1:] - a[:, :, :, :-1]))
                sq = s * s
                T = np.zeros(s.shape, dtype=f32)
                for i2 in range(C2):
                    for i1 in range(C1):
                        cc = cf[base + i2 * C1 + i1]
                        T[:, i1] = fma32(cc, sq[:, C1 + i2], T[:, i1])
                        T[:, C1 + i2] = fma32(cc, sq[:, i1], T[:, C1 + i2])
                A = s * (f32(1) - sq)
                # as the first pixel (sign -1) where a next one exists, then as the second (+1) where a previous one does
                Af, As, Tf, Ts = (np.zeros(a.shape, dtype=f32) for _ in range(4))
                if dr == 0:
                    Af[:, :, :-1, :], Tf[:, :, :-1, :], As[:, :, 1:, :], Ts[:, :, 1:, :] = -A, T, A, T
                else:
                    Af[:, :, :, :-1], Tf[:, :, :, :-1], As[:, :, :, 1:], Ts[:, :, :, 1:] = -A, T, A, T
                g = fma32(As, Ts, fma32(Af, Tf, g))
            if l > 0:
                scale = f32(0.5) if (l == 1 and self.defect == "the level-1 gradient scaled by 1/2") else f32(0.25 if l == 1 else 0.0625)
                u = np.zeros(lv[0].shape, dtype=f32)
                rep = np.repeat(np.repeat(g * scale, 1 << l, -2), 1 << l, -1)
                u[..., :rep.shape[-2], :rep.shape[-1]] = rep
                ups.append(u)
            else:
                g0 = g
        for u in ups[::-1]:                               # up1 first, then up2
            g0 = g0 + u
        out = []
        for k, (lo, hi, old) in enumerate(((0, C1, c.old1), (C1, C1 + C2, c.old2))):
            if not want[k]:
                out.append(None)
                continue
            v = g0[:, lo:hi]
            out.append(old.astype(f32) + v if m.get("accumulate") else v.copy())
        return out

    # ------------------------------------------------------------------------------------------------------------- SSIM_Loss
    def _ssim3_terms(self, c):
        d = self.defect
        mode = "edge" if d == "replicate padding instead of reflect padding" else "reflect"
        x, y = (np.pad(v.astype(f32), ((0, 0), (1, 1), (1, 1)), mode=mode) for v in (c.x, c.y))
        N, H, W = c.shape
        nine = f32(9)
        acc = [np.zeros(c.shape, dtype=f32) for _ in range(5)]
        for i in range(3):
            row = [np.zeros(c.shape, dtype=f32) for _ in range(5)]
            for j in range(3):
                u, v = x[:, i:i + H, j:j + W], y[:, i:i + H, j:j + W]
                for k, t in enumerate((u, v, u * u, v * v, v * v if d == "E[xy] taken with y's square" else u * v)):
                    if d == "division by 9 taken per row":
                        row[k] = row[k] + t
                    else:
                        acc[k] = acc[k] + t
            if d == "division by 9 taken per row":
                acc = [(a + r) / nine for a, r in zip(acc, row)]          # the division inside the loop over the rows
        mx, my, ex2, ey2, exy = acc if d == "division by 9 taken per row" else [a / nine for a in acc]
        C1, C2 = f32(0.01 * 0.01), f32(0.03 * 0.03)
        mxy, mxx, myy = mx * my, mx * mx, my * my
        sgx, sgy, sgxy = ex2 - mxx, ey2 - myy, exy - mxy
        return mx, my, (f32(2) * mxy + C1, f32(2) * sgxy + C2, mxx + myy + C1, sgx + sgy + C2)

    def ssim3_fwd(self, c):
        _, _, (A1, A2, B1, B2) = self._ssim3_terms(c)
        v = (f32(1) - (A1 * A2) / (B1 * B2)) / f32(2)
        out = np.minimum(np.maximum(v, f32(0)), f32(1))
        part = np.zeros((c.N, c.tiles_y, c.tiles_x))
        for ty in range(c.tiles_y):
            for tx in range(c.tiles_x):
                part[:, ty, tx] = out[:, ty * IX.STH:(ty + 1) * IX.STH, tx * IX.STW:(tx + 1) * IX.STW].astype(f64t).sum((1, 2))
        return out, part, np.array([part.sum() * (1.0 / (f64t(c.N) * c.H * c.W))]).astype(f32)

    def ssim3_bwd(self, c, g, want, m):
        d = self.defect
        N, H, W = c.shape
        mx, my, (A1, A2, B1, B2) = self._ssim3_terms(c)
        v = (f32(1) - (A1 * A2) / (B1 * B2)) / f32(2)
        passes = ((v > 0) & (v < 1)) if d == "the clamp cutting the gradient at its bounds" else ((v >= 0) & (v <= 1))
        k = f32(IX.up_of(m))
        gp = np.full(c.shape, k * (f32(1) / f32(c.count)), dtype=f32) if g is None else np.asarray(g, dtype=f64t).astype(f32) * k
        w = gp * f32(-0.5) / f32(9)
        inv, i1, i2 = f32(1) / (B1 * B2), f32(1) / B1, f32(1) / B2
        S = (A1 * A2) * inv
        da, db = f32(2) * (A2 - A1) * inv, f32(2) * S * (i1 - i2)
        cf = [w * (my * da - mx * db), w * (mx * da - my * db), w * -(S * i2), w * (f32(2) * A1 * inv)]
        cf = [np.pad(np.where(passes, t, f32(0)), ((0, 0), (1, 1), (1, 1))) for t in cf]

        def mult(n, lo_defect, hi_defect):
            i = np.arange(n)
            lo = np.where(i >= 1, np.where((i == 1) & (d != lo_defect), 2.0, 1.0), 0.0)
            hi = np.where(i + 1 < n, np.where((i == n - 2) & (d != hi_defect), 2.0, 1.0), 0.0)
            return [lo.astype(f32), np.ones(n, dtype=f32), hi.astype(f32)]
        wy, wx = mult(H, "multiplicity 1 at row 1", "multiplicity 2 missing at H - 2"), mult(W, "-", "-")
        s = [np.zeros(c.shape, dtype=f32) for _ in range(4)]
        for dy in range(3):
            for dx in range(3):
                mm = wy[dy][:, None] * wx[dx][None, :]
                for q in range(4):
                    s[q] = s[q] + mm * cf[q][:, dy:dy + H, dx:dx + W]
        x, y = c.x.astype(f32), c.y.astype(f32)
        vx = s[0] + f32(2) * x * s[2] + y * s[3]
        vy = s[1] + f32(2) * y * s[2] + x * s[3]
        old = c.old.astype(f32)
        acc = bool(m.get("accumulate"))
        return (old + vx if acc else vx) if want[0] else None, (old + vy if acc else vy) if want[1] else None


FAITHFUL = Imitation()


def report(title, worst, either=None):
    print()
    for q, (v, what, n) in sorted(worst.items()):
        print("   %-10s %-14s worst multiple of the bound %.3f over %9d elements  in %s" % (title, q, v, n, what))
        assert v <= 1.0
    if either is not None:
        print("   %-10s either-way elements: %d" % (title, either))


def run_all(keys, make, run):
    worst, either = {}, 0
    for key in keys:
        c = make(*key)
        for q, cmps in run(c, FAITHFUL).items():
            for x in must_pass(cmps):
                v, what, n = worst.get(q, (-1.0, "", 0))
                worst[q] = (max(v, x.worst), x.what if x.worst >= v else what, n + x.n)
                either += getattr(x, "either", 0)
    return worst, either


# ----------------------------------------------------------------------------------------------------------------- tables
def test_case_tables_hold_what_they_name():
    rk = IX.recon_keys()
    assert {k[1] for k in rk} == set(IX.LENGTHS) | {IX.RECON_CAP} and {k[0] for k in rk} == set(IX.RECON_KINDS) and {k[2] for k in rk} == {1, 3}
    assert {k[3] for k in rk} == set(IX.RECON_ALIGN)
    for differing in range(3):                            # exactly one pointer apart, each in turn; all equal at 0, 1 and 3
        assert any(len(set(o)) == 2 and sum(v == o[differing] for v in o) == 1 for o in IX.RECON_ALIGN)
    assert {(0, 0, 0), (1, 1, 1), (3, 3, 3)} <= set(IX.RECON_ALIGN)
    assert any(k[0] == "l1" and k[4] == "zerosum" for k in rk)
    for kind in IX.RECON_KINDS:
        cap = [k for k in rk if k[0] == kind and k[1] == IX.RECON_CAP]
        paths = set()
        for k in cap:
            for offs, G in ((k[3][:2], IX.groups(k[1], 4096, 64)), (k[3], IX.groups(k[1], 1024, 256))):
                head, nv, tail0 = IX.split16(k[1], offs)
                paths.add((len(offs), "fallback" if nv == 0 else "head+float4+tail" if head and tail0 < k[1] else "float4"))
                t4, t1 = IX.trips(k[1], offs, G)
                paths |= {(len(offs), "second float4 trip")} if t4 >= 2 else set()
                paths |= {(len(offs), "second fallback trip")} if nv == 0 and t1 >= 2 else set()
                assert G in (64, 256)
        assert {(n, w) for n in (2, 3) for w in ("head+float4+tail", "fallback", "second float4 trip", "second fallback trip")} <= paths, (kind, paths)
        assert any(k[2] == 3 and k[1] % 4 for k in rk if k[0] == kind)      # per % 4 != 0 with B = 3: every sample a head of its own
    pk = IX.pix_keys()
    assert {k[1] for k in pk} == set(IX.LENGTHS) | {IX.PIX_SUMS_CAP, IX.PIX_BWD_CAP} and {k[0] for k in pk} == set(IX.PIX_KINDS)
    assert {k[2] for k in pk if k[0] == "maskl1" and k[1] == 1027} == set(IX.PIX_ALIGN)
    assert {k[4] for k in pk if k[0] == "maskl1"} == set(IX.PIX_WANT)
    for differing in range(5):
        assert any(sum(v != o[(differing + 1) % 5] for v in o) == 1 and o[differing] != o[(differing + 1) % 5] for o in IX.PIX_ALIGN)
    for kind in IX.PIX_KINDS:
        for cap, unit, G, sel in ((IX.PIX_SUMS_CAP, 4096, 256, "sums_offs"), (IX.PIX_BWD_CAP, 1024, 2048, "bwd_offs")):
            paths = set()
            for k in pk:
                if k[0] == kind and k[1] == cap:
                    c = IX.PixCase.__new__(IX.PixCase)
                    c.kind, c.offs, c.want = k[0], k[2], k[4] if k[0] == "maskl1" else "ga"
                    offs = getattr(c, sel)()
                    head, nv, tail0 = IX.split16(cap, offs)
                    paths.add("fallback" if nv == 0 else "head+float4+tail" if head and tail0 < cap else "float4")
                    t4, t1 = IX.trips(cap, offs, G)
                    paths |= {"second float4 trip"} if t4 >= 2 else set()
                    paths |= {"second fallback trip"} if nv == 0 and t1 >= 2 else set()
                    assert IX.groups(cap, unit, G) == G
            want = {"head+float4+tail", "second float4 trip"} | ({"fallback", "second fallback trip"} if (sel == "bwd_offs" or kind == "maskl1") else set())
            assert want <= paths, (kind, cap, paths)
    gk = IX.gradl_keys()
    assert {(k[1], k[2]) for k in gk} == set(IX.GRADL_SHAPES) and {k[0] for k in gk} == {1, 6} and {k[3] for k in gk} == set(IX.GRADL_DATA)
    assert IX.groups(17 * 241, 4096, 64) == 2 and IX.groups(513 * 512, 4096, 64) == 64 and 513 * 512 > 64 * 4096
    ek = IX.excl_keys()
    assert {k[0] for k in ek} == set(IX.EXCL_H) and {k[1] for k in ek} == set(IX.EXCL_W) and {k[2] for k in ek} == {1, 2, 3}
    assert {(k[3], k[4]) for k in ek} == set(IX.EXCL_PAIRS) and {k[5] for k in ek} == {1, 2} and {k[6] for k in ek} == set(IX.EXCL_DATA)
    for k in ek:
        assert k[0] >= 2 << (k[2] - 1) and k[1] >= 2 << (k[2] - 1)
    assert set(IX.EXCL_SEAM_H) <= {k[0] for k in ek if k[2] == 3} and set(IX.EXCL_SEAM_W) <= {k[1] for k in ek if k[2] == 3}
    assert {k[1] for k in ek if k[1] % 4 == 0} == {4, 8, 32, 36, 64}                  # each of them runs on both stagings (run_excl)
    assert any(k[2] < 3 and (k[0], k[1]) != (32, 32) and k[0] > 16 for k in ek)
    sk = IX.ssim3_keys()
    assert {k[0] for k in sk} == set(IX.SSIM3_H) and {k[1] for k in sk} == set(IX.SSIM3_W) and max(k[2] for k in sk) == 3
    assert {k[3] for k in sk} == set(IX.SSIM3_KINDS) and max(k[0] * k[1] for k in sk) == 33 * 129
    for H, W, N in IX.SSIM3_FULL:
        pos = IX.marks(H, W)
        assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= set(pos)
        assert {1, H - 2} & set(range(H)) <= {r for r, _ in pos} and {1, W - 2} & set(range(W)) <= {q for _, q in pos}
        if H > 16 and W > 64:
            assert {15, 16} <= {r for r, _ in pos} and {63, 64} <= {q for _, q in pos}
        covered = set()
        for k in sk:
            if k[:3] == (H, W, N) and k[3] == "impulse":
                covered |= {pos[(k[4] + n) % len(pos)] for n in range(N)}
        assert covered == set(pos)


def test_either_way_shares_stay_under_the_cap_from_the_reference_alone():
    worst = {}
    for key in IX.recon_keys():
        if key[0] == "l_char" and key[1] >= 1023:         # (below that one element is more than the cap: counted, and 0 in every case)
            worst["l_char"] = max(worst.get("l_char", 0.0), IX.recon_case(*key).either_share())
        elif key[0] == "l_char":
            assert IX.recon_case(*key).either_share() == 0.0
    for key in IX.ssim3_keys():
        c = IX.ssim3_case(*key)
        share = c.either_share()
        worst["ssim3 " + c.kind] = max(worst.get("ssim3 " + c.kind, 0.0), share)
        assert share <= IX.EITHER_CAP, (c.label, share)
        if c.kind == "equal":
            assert c.ref()["same"].all() and (c.ref()["v"] == 0).all() and share == 0.0
    print()
    for k, v in sorted(worst.items()):
        print("   largest either-way share  %-14s %.4f" % (k, v))
        assert v <= IX.EITHER_CAP


def test_count_images_saturate_the_float32_sigmoid():
    for key in IX.excl_keys():
        if key[6] == "count":
            c = IX.excl_case(*key)
            assert set(np.unique(c.img1)) <= {0.0, 100.0} and set(np.unique(c.img2)) <= {0.0, 100.0}
            assert c.saturated(), c.label
            assert c.tile_counts().sum() > 0 or c.H * c.W <= 9, c.label
    c = IX.ExclCase(20, 37, 3, 1, 1, 1, "count")
    c.img1 = 100.0 * (IX.uni(c.img1.shape, 5) < 0.5)       # without the 4 x 4 fix-up the level-2 differences are multiples of 6.25
    assert not c.saturated()


# ----------------------------------------------------------------------------------------------------------------- faithful imitations
def test_faithful_streaming_imitation_passes_every_case():
    w, e = run_all(IX.recon_keys(), IX.recon_case, IX.run_recon)
    report("recon", w, e)
    w, e = run_all(IX.pix_keys(), IX.pix_case, IX.run_pix)
    report("pixloss", w)


def test_faithful_gradient_loss_imitation_passes_every_case():
    report("gradloss", run_all(IX.gradl_keys(), IX.gradl_case, IX.run_gradl)[0])


def test_faithful_exclusion_imitation_passes_every_case():
    report("exclusion", run_all(IX.excl_keys(), IX.excl_case, IX.run_excl)[0])


def test_faithful_ssim3_imitation_passes_every_case():
    report("ssim3", run_all(IX.ssim3_keys(), IX.ssim3_case, IX.run_ssim3)[0])


# ----------------------------------------------------------------------------------------------------------------- defects
STREAM_DEFECTS = (      # (defect, family, key)
    ("tail dropped", "recon", ("l1", 1027, 3, (1, 1, 1), "zerosum", 1e-6)),
    ("head counted twice", "recon", ("l2", IX.RECON_CAP, 1, (1, 1, 1), "grid", 1e-6)),
    ("scalar fallback indexed with the vector offsets", "recon", ("l1", IX.RECON_CAP, 1, (0, 2, 0), "grid", 1e-6)),
    ("the second trip of the stride loop skipped", "recon", ("l_char", IX.RECON_CAP, 1, (1, 1, 1), "grid", 1e-6)),
    ("accumulate added in double instead of float", "recon", ("l2", IX.RECON_CAP, 3, (3, 3, 3), "uniform", 1e-6)),
    ("tail dropped", "pix", ("maskl1", 1027, (3, 3, 3, 3, 3), "grid", "both")),
    ("head counted twice", "pix", ("gray", IX.PIX_SUMS_CAP, (1, 1, 1, 1, 1), "grid", "both")),
    ("scalar fallback indexed with the vector offsets", "pix", ("nonblurry", IX.PIX_BWD_CAP, (0, 0, 0, 1, 0), "grid", "both")),
    ("the second trip of the stride loop skipped", "pix", ("maskl1", IX.PIX_BWD_CAP, (1, 1, 1, 1, 1), "grid", "both")),
    ("gb given ga's sign", "pix", ("maskl1", 1027, (0, 0, 0, 0, 1), "grid", "gb")),
)


def test_each_streaming_defect_fails_a_named_case():
    print()
    for defect, family, key in STREAM_DEFECTS:
        assert key in (IX.recon_keys() if family == "recon" else IX.pix_keys()), key
        c = IX.recon_case(*key) if family == "recon" else IX.pix_case(*key)
        res = (IX.run_recon if family == "recon" else IX.run_pix)(c, Imitation(defect))
        print("   %-52s caught: %s" % (defect, must_fail(IX.flat(res), defect, c.label)))


GRADL_DEFECTS = (
    ("divisors swapped", (1, 3, 257, "grid")),
    ("the last row's x-differences dropped", (6, 2, 9, "checker")),
    ("sgn(0) = 1", (1, 17, 241, "quarters")),
    ("a subnormal difference flushed", (1, 9, 2, "subnormal")),
)


def test_each_gradient_loss_defect_fails_a_named_case():
    print()
    for defect, key in GRADL_DEFECTS:
        assert key in IX.gradl_keys()
        c = IX.gradl_case(*key)
        print("   %-52s caught: %s" % (defect, must_fail(IX.flat(IX.run_gradl(c, Imitation(defect))), defect, c.label)))


EXCL_DEFECTS = (
    ("a seam difference dropped", (17, 33, 3, 3, 3, 2, "count")),
    ("halo read as zero", (20, 65, 3, 4, 4, 1, "count")),
    ("ceil pooling", (17, 37, 3, 4, 1, 1, "count")),
    ("a level-2 divisor off by one row", (33, 70, 3, 3, 3, 1, "count")),
    ("i1 and i2 transposed", (16, 36, 3, 2, 4, 1, "count")),
    ("the level-1 gradient scaled by 1/2", (18, 36, 3, 1, 1, 1, "low")),
    ("a pooled pixel of the odd last row counted", (33, 65, 3, 4, 1, 1, "count")),
)


def test_each_exclusion_defect_fails_a_named_case():
    print()
    for defect, key in EXCL_DEFECTS:
        assert key in IX.excl_keys(), key
        c = IX.excl_case(*key)
        print("   %-52s caught: %s" % (defect, must_fail(IX.flat(IX.run_excl(c, Imitation(defect))), defect, c.label)))


SSIM3_DEFECTS = (
    ("replicate padding instead of reflect padding", (17, 65, 2, "indep", 0)),
    ("multiplicity 1 at row 1", (17, 65, 2, "indep", 0)),
    ("multiplicity 2 missing at H - 2", (17, 65, 2, "indep", 0)),
    ("division by 9 taken per row", (33, 129, 1, "grid", 0)),
    ("the clamp cutting the gradient at its bounds", (17, 65, 2, "equal", 0)),
    ("E[xy] taken with y's square", (2, 2, 3, "indep", 0)),
)


def test_each_ssim3_defect_fails_a_named_case():
    print()
    for defect, key in SSIM3_DEFECTS:
        assert key in IX.ssim3_keys(), key
        c = IX.ssim3_case(*key)
        print("   %-52s caught: %s" % (defect, must_fail(IX.flat(IX.run_ssim3(c, Imitation(defect))), defect, c.label)))


# ----------------------------------------------------------------------------------------------------------------- reference-side checks
def test_restatements_agree_with_the_fixture_checked_ones_at_float64():
    """the SSIM_Loss map and both gradients against tests/ssim3_restate.py (checked against the reference's fixture), the exclusion loss
    and its gradients against finite differences of this module's own forward"""
    import ssim3_restate as SR
    for key in ((17, 65, 2, "indep", 0), (2, 2, 3, "near", 0), (33, 129, 1, "indep", 0)):
        c = IX.ssim3_case(*next(k for k in IX.ssim3_keys() if k[:2] == key[:2] and k[3] == key[3]))
        assert np.abs(c.ref()["map"] - SR.ssim3_map(c.x, c.y)).max() <= 1e-13
        (gx, _), (gy, _) = c.grads(c.g, {})
        wx, wy = SR.ssim3_grads(c.x, c.y, c.g)
        scale = max(np.abs(wx).max(), np.abs(wy).max())
        assert np.abs(gx - wx).max() <= 1e-12 * scale and np.abs(gy - wy).max() <= 1e-12 * scale
    c = IX.excl_case(9, 32, 3, 3, 3, 1, "uniform")
    g1 = c.unit_grads()[0]
    for at in ((0, 0, 0, 0), (0, 2, 8, 31), (0, 1, 4, 15), (0, 1, 7, 16)):
        h = 1e-6
        vals = []
        for sgn in (1.0, -1.0):
            d = IX.ExclCase(9, 32, 3, 3, 3, 1, "uniform")
            d.img1 = c.img1.copy()
            d.img1[at] += sgn * h
            vals.append(d.fwd()["loss"])
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - g1[at]) <= 1e-6 * max(abs(g1[at]), 1e-3), (at, fd, g1[at])


@pytest.mark.parametrize("n,offs,G", ((1027, (1, 1, 1), 2), (1027, (0, 1, 0), 2), (3, (1, 1), 1), (8193, (3, 3), 3), (5, (2, 2), 1)))
def test_the_closed_form_of_owners_is_the_trip_by_trip_walk(n, offs, G):
    el, wg = walk(n, offs, G)
    assert sorted(el) == list(range(n))
    assert np.array_equal(IX.owners(n, offs, G)[el], wg)
