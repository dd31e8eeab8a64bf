"""The per-element comparisons of tests/ssim_exact.py without a GPU: a float32 imitation of every kernel of csrc/ssim.hip (numpy: each fma
a float64 product and sum rounded once to float32, the separable order, tiles of 64 x 16 with their staged halo, S summed in double)
passes every case of every table the GPU tests run, and the worst multiple of its bound is printed per quantity; each named defect,
applied to the imitation, FAILS a named case at a named element; and the float64 restatement agrees with tests/metrics_restate.py (the
fixture-checked restatement and torch autograd) and with finite differences of S.  So a green tests/test_gpu_ssim_exact.py means something."""
import numpy as np
import torch

import metrics_restate as MR
import ssim_exact as SX

f32 = np.float32
W32 = SX.WIN.astype(f32)
SH, SW = SX.TH + 2 * SX.RAD, SX.TW + 16


def fma(w, a, acc):
    return (np.float64(w) * a.astype(np.float64) + acc.astype(np.float64)).astype(f32)


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


# ----------------------------------------------------------------------------------------------------------------- the SSIM imitation
def stage(planes, tx0, ty0, defect=None):
    """rows ty0-5 .. ty0+20, columns tx0-8 .. tx0+71 of every plane [N, H, W] -> [N, 26, 80] float32, zero outside the image"""
    N, H, W = planes.shape
    gy, gx = ty0 - SX.RAD + np.arange(SH), tx0 - 8 + np.arange(SW)
    if defect == "halo read one column left":
        gx = gx - 1
    if defect == "halo read one column right":
        gx = gx + 1
    if defect == "halo one row up":
        gy = gy - 1
    if defect == "edge-clamped instead of zero padding":
        return planes[:, np.clip(gy, 0, H - 1)[:, None], np.clip(gx, 0, W - 1)[None, :]]
    vy, vx = (gy >= 0) & (gy < H), (gx >= 0) & (gx < W)
    if defect == "halo zeroed at a seam between tile columns":
        vx &= (gx >= tx0) & (gx < tx0 + SX.TW)
    if defect == "halo zeroed at a seam between tile rows":
        vy &= (gy >= ty0) & (gy < ty0 + SX.TH)
    if defect == "float4 path taken at W % 4 != 0":          # a vector whose first column is inside is read whole: it runs into the next row
        g0 = gx - np.arange(SW) % 4
        vx = (g0 >= 0) & (g0 < W)
        flat = np.concatenate([planes.reshape(-1), np.zeros(4, dtype=f32)])
        idx = np.arange(N)[:, None, None] * (H * W) + np.where(vy, gy, 0)[None, :, None] * W + np.where(vx, gx, 0)[None, None, :]
        return np.where((vy[:, None] & vx[None, :])[None], flat[idx], f32(0))
    s = planes[:, np.clip(gy, 0, H - 1)[:, None], np.clip(gx, 0, W - 1)[None, :]]
    return np.where((vy[:, None] & vx[None, :])[None], s, f32(0))


def window(t):
    """[N, 26, 80] staged values -> [N, 16, 64]: 11 fmas along the row, then 11 down the column, taps ascending, from 0"""
    h = np.zeros(t.shape[:2] + (SX.TW,), dtype=f32)
    for k in range(SX.NT):
        h = fma(W32[k], t[:, :, 3 + k:3 + k + SX.TW], h)
    acc = np.zeros((t.shape[0], SX.TH, SX.TW), dtype=f32)
    for k in range(SX.NT):
        acc = fma(W32[k], h[:, k:k + SX.TH, :], acc)
    return acc


def tiles(H, W):
    return [(tx0, ty0) for ty0 in range(0, H, SX.TH) for tx0 in range(0, W, SX.TW)]


def imit_fwd(c, side=0, defect=None):
    """-> (out [1 + B] float32, dplanes [3, B, C, H, W] float32, SENTINEL where nothing was written)"""
    B, C, H, W = c.shape
    a, b = (v.astype(f32).reshape(B * C, H, W) for v in c.xy(side))
    c1, c2 = f32(0.01 * 0.01), f32(0.03 * 0.03)
    if defect == "C1 and C2 unsquared":
        c1, c2 = f32(0.01), f32(0.03)
    if defect == "C1 and C2 swapped":
        c1, c2 = c2, c1
    dpl = np.full((3, B * C, H, W), SX.SENTINEL, dtype=f32)
    total = np.zeros(B * C)
    two = f32(2)
    for tx0, ty0 in tiles(H, W):
        sx, sy = stage(a, tx0, ty0, defect), stage(b, tx0, ty0, defect)
        p, m, q, q2 = window(sx), window(sy), window(sx * sx), window(sy * sy)
        r = window(sx * sx if defect == "x.y plane fed x.x" else sx * sy)
        pm, pp, mm = p * m, p * p, m * m
        s1, s2, s12 = q - pp, q2 - mm, r - pm
        A1, A2, B1, B2 = two * pm + c1, two * s12 + c2, pp + mm + c1, s1 + s2 + c2
        S = (A1 * A2) / (B1 * B2)
        inv, i1, i2 = f32(1) / (B1 * B2), f32(1) / B1, f32(1) / B2
        Dp = two * m * (A2 - A1) * inv - two * p * S * (i1 - i2)
        Dq = S * i2 if defect == "Dq with the wrong sign" else -S * i2
        Dr = two * A1 * inv
        h, w = min(SX.TH, H - ty0), min(SX.TW, W - tx0)
        total += S[:, :h, :w].astype(np.float64).sum((1, 2))
        for i, D in enumerate((Dp, Dq, Dr)):
            dpl[i, :, ty0:ty0 + h, tx0:tx0 + w] = D[:, :h, :w]
    per = total.reshape(B, C).sum(1)
    n = float(C * H * W)
    out = np.empty(1 + B, dtype=f32)
    out[0] = f32(per.sum() / (n * B))
    out[1:] = (per / (n * B if defect == "per-image mean divided by B C H W" else n)).astype(f32)
    return out, dpl.reshape((3,) + c.shape)


def imit_bwd_sums(c, planes32, defect=None):
    """the three window sums of the planes the backward is fed [3, B, C, H, W] -> [3, N, H, W] float32"""
    B, C, H, W = c.shape
    d = planes32.astype(f32).reshape(3, B * C, H, W)
    a = np.zeros((3, B * C, H, W), dtype=f32)
    for tx0, ty0 in tiles(H, W):
        h, w = min(SX.TH, H - ty0), min(SX.TW, W - tx0)
        for i in range(3):
            a[i, :, ty0:ty0 + h, tx0:tx0 + w] = window(stage(d[i], tx0, ty0, defect))[:, :h, :w]
    return a


def imit_bwd(c, a, side, m, defect=None, up=None):
    """the gradient from the window sums `a` of imit_bwd_sums; the destination holds c.old (accumulate) or SENTINEL before the launch"""
    B, C, H, W = c.shape
    x, y = (v.astype(f32).reshape(B * C, H, W) for v in c.xy(side))
    if up is None:
        up, acc = c.mode(m)
    else:
        acc = bool(m.get("accumulate"))
    per = bool(up.get("per_image"))
    g = f32(np.float64(f32(up.get("gscale", 1.0))) / (float(C) * H * W * (float(B) if not per or defect == "per-image weight missing the factor B" else 1.0)))
    g = np.full(B * C, g, dtype=f32)
    if up.get("gdev") is not None and defect != "gscale_dev ignored":
        g = g * f32(up["gdev"])
    if up.get("gout") is not None:
        go = np.asarray(up["gout"], dtype=np.float64).astype(f32)
        n = np.arange(B * C)
        g = g * (go[np.minimum(n, B - 1) if defect == "per-image weight indexed by n" else n // C] if per else go[0])
    t1 = (x if defect == "the factor 2 of 2x missing" else f32(2) * x) * a[1]
    t2 = (x if defect == "y replaced by x in the last term" else y) * a[2]
    v = g[:, None, None] * (a[0] + t1 + t2)
    dest = c.old.astype(f32).reshape(v.shape) if acc else np.full(v.shape, SX.SENTINEL, dtype=f32)
    adds = (acc and defect != "accumulate overwriting") or (not acc and defect == "accumulate adding when off")
    return (dest + v if adds else v).reshape(c.shape)


def ssim_run(c, defect=None, sides=(0, 1), modes=SX.GRAD_MODES):
    """every comparison the GPU file makes of one case, on the imitation: {quantity: [comparisons]}"""
    res = {"planes": [], "mean": [], "per-image means": [], "gradient": [], "gradient chained": [], "exact": []}
    for side in sides:
        out, dpl = imit_fwd(c, side, defect)
        res["planes"] += c.check_planes(dpl, side)
        vals = c.check_values(out, side)
        res["mean"] += vals[:1]
        res["per-image means"] += vals[1:]
        own = imit_bwd_sums(c, c.fwd(side)["planes32"], defect)
        chained = imit_bwd_sums(c, dpl, defect)
        for i, m in enumerate(modes if side == 0 else modes[1:3]):
            res["gradient"] += c.check_grad(imit_bwd(c, own, side, m, defect), m, side)
            if i < 2:
                res["gradient chained"] += c.check_grad(imit_bwd(c, chained, side, m, defect), m, side, chain=True)
        if side == 0:                                        # accumulate with power-of-two scales: fl(old + plain), to the bit
            up = c.pow2_scales()
            plain = imit_bwd(c, own, 0, {}, defect, up=up)
            acc = imit_bwd(c, own, 0, {"accumulate": True}, defect, up=up)
            want = (c.old + plain.astype(np.float64)).astype(f32)
            res["exact"] += [SX.ECmp(c.label + " accumulate, power-of-two scales", acc, want)]
    return res


def flat(res):
    return [x for v in res.values() for x in v]


def test_taps_are_the_window_of_the_fixture_checked_restatement():
    assert np.array_equal(SX.WIN, MR.window11(torch.float64).numpy())
    assert np.array_equal(SX.WIN2, MR.window2d(1, torch.float64).numpy()[0, 0])
    assert abs(SX.WIN.sum() - 1.0) < 4 * SX.EPS32 and (SX.WIN > 0).all()


def test_case_tables_hold_what_they_name():
    keys = SX.ssim_keys()
    shapes = {(k[0], k[1]) for k in keys}
    for hw in ((1, 1), (3, 5), (17, 65), (17, 68), (33, 70), (16, 132), (33, 132)):
        assert hw in shapes
    assert {k[0] for k in keys} == set(SX.HEIGHTS) and {k[1] for k in keys} == set(SX.WIDTHS)
    for H in SX.HEIGHTS:
        ws = [w for h, w in shapes if h == H]
        assert min(ws) <= 11 and max(ws) >= 43, H
    for W in SX.WIDTHS:
        hs = [h for h, w in shapes if w == W]
        assert min(hs) <= 11 and max(hs) >= 16, W
    assert {(k[2], k[3]) for k in keys} == set(SX.BCS) and {k[4] for k in keys} == set(SX.KINDS)
    assert max(k[0] * k[1] for k in keys) == 33 * 132 and max(k[2] for k in keys) <= 3 and max(k[3] for k in keys) <= 4
    assert sorted(k for g in SX.SSIM_GROUPS for k in SX.ssim_group_keys(g)) == sorted(keys)
    pos = SX.impulse_positions(33, 132)
    for want in ((0, 0), (0, 131), (32, 0), (32, 131), (15, 63), (16, 64), (15, 64), (16, 63)):
        assert want in pos
    assert {5, 6, 10, 11, 21, 22} <= {r for r, _ in pos} and {5, 6, 58, 59, 69, 70, 126, 125} <= {c for _, c in pos}
    covered = set()
    for k in keys:
        if k[4] == "impulse" and (k[0], k[1]) == (33, 132):
            covered |= {pos[(k[5] + n) % len(pos)] for n in range(12)}
    assert covered == set(pos)
    ck = SX.conf_keys()
    assert {(k[2], k[3]) for k in ck} == set(SX.CONF_DT) and {k[0] for k in ck} == set(SX.CONF_PER) and {k[1] for k in ck} == set(SX.CONF_B)
    assert {k[4] for k in ck if k[2] == "u8"} == {127.0, 127.5, -0.5}
    assert {k[0] for k in SX.PSNR_KEYS} == set(SX.PSNR_N) and SX.PSNR_N[-1] > 4096 * SX.PSNR_CAP


def test_faithful_ssim_imitation_passes_every_case():
    worst, count = {}, {}
    for key in SX.ssim_keys():
        c = SX.ssim_case(*key)
        for q, cmps in ssim_run(c).items():
            for x in must_pass(cmps):
                count[q] = count.get(q, 0) + x.n
                if x.worst >= worst.get(q, (-1.0, ""))[0]:
                    worst[q] = (x.worst, x.what)
    print()
    for q, (v, what) in worst.items():
        print("   worst multiple of the bound  %-18s %.3f over %8d elements  in %s" % (q, v, count[q], what))
        assert v <= 1.0


def _key(H, W, kind, BC=None):
    return next(k for k in SX.ssim_keys() if (k[0], k[1], k[4]) == (H, W, kind) and (BC is None or (k[2], k[3]) == BC))


SSIM_DEFECTS = (      # (defect, the case that must catch it, the quantity it shows in)
    ("halo read one column left", (33, 132, "impulse", (3, 4)), "planes"),
    ("halo read one column right", (33, 132, "impulse", (3, 4)), "planes"),
    ("halo one row up", (33, 132, "impulse", (3, 4)), "planes"),
    ("edge-clamped instead of zero padding", (33, 132, "impulse", (3, 4)), "planes"),
    ("halo zeroed at a seam between tile columns", (17, 65, "impulse", (3, 4)), "planes"),
    ("halo zeroed at a seam between tile rows", (17, 65, "impulse", (3, 4)), "planes"),
    ("float4 path taken at W % 4 != 0", (33, 70, "indep", (1, 3)), "planes"),
    ("C1 and C2 unsquared", (17, 68, "indep", (2, 3)), "planes"),
    ("C1 and C2 swapped", (17, 68, "indep", (2, 3)), "planes"),
    ("x.y plane fed x.x", (17, 68, "indep", (2, 3)), "planes"),
    ("Dq with the wrong sign", (17, 68, "indep", (2, 3)), "planes"),
    ("the factor 2 of 2x missing", (17, 68, "indep", (2, 3)), "gradient"),
    ("y replaced by x in the last term", (17, 68, "indep", (2, 3)), "gradient"),
    ("per-image weight indexed by n", (17, 68, "indep", (2, 3)), "gradient"),
    ("per-image weight missing the factor B", (17, 68, "indep", (2, 3)), "gradient"),
    ("gscale_dev ignored", (17, 68, "indep", (2, 3)), "gradient"),
    ("accumulate overwriting", (17, 68, "indep", (2, 3)), "gradient"),
    ("accumulate adding when off", (17, 68, "indep", (2, 3)), "gradient"),
    ("per-image mean divided by B C H W", (17, 68, "indep", (2, 3)), "per-image means"),
)


def test_each_ssim_defect_fails_a_named_case():
    print()
    for defect, (H, W, kind, BC), quantity in SSIM_DEFECTS:
        c = SX.ssim_case(*_key(H, W, kind, BC))
        res = ssim_run(c, defect, sides=(0,))
        print("   %-44s caught: %s" % (defect, must_fail(res[quantity], defect, c.label)))
    # the seam defects also show in the backward alone, fed exact planes, at a dense two-tile case
    c = SX.ssim_case(*_key(33, 70, "indep"))
    for defect in ("halo zeroed at a seam between tile columns", "halo zeroed at a seam between tile rows", "halo read one column left"):
        own = imit_bwd_sums(c, c.fwd(0)["planes32"], defect)
        must_fail(c.check_grad(imit_bwd(c, own, 0, {}), {}, 0), defect, c.label)


def test_an_impulse_names_the_tap_pair_of_every_pixel_it_reaches():
    """x = y = one 1 at (r, c): p = m = q = q2 = r = W2[5 + r - i, 5 + c - j] at pixel (i, j) and 0 out of reach"""
    c = SX.ssim_case(33, 132, 3, 4, "impulse", 0)
    p = c.fwd(0)["sums"][0]
    for n in range(0, 12, 2):
        (r0,), (c0,) = (v for v in np.nonzero(c.x[n // 4, n % 4]))
        for i in range(max(0, r0 - 6), min(33, r0 + 7)):
            for j in range(max(0, c0 - 6), min(132, c0 + 7)):
                want = SX.WIN2[5 + r0 - i, 5 + c0 - j] if abs(r0 - i) <= 5 and abs(c0 - j) <= 5 else 0.0
                assert p[n // 4, n % 4, i, j] == want, (n, i, j)


# ----------------------------------------------------------------------------------------------------------------- reference-side checks
def rel(a, b, scale=None):
    """largest difference relative to the largest reference value -- or, for a gradient (which vanishes where the images are equal), to the
    largest sum of the absolute values of its three terms"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() if scale is None else scale))


def test_restatement_agrees_with_metrics_restate_at_float64():
    """ssim, ssim_autograd and ssim_backward_formula on the four old shapes (the first image of the 16 x 3 x 256 x 256 one: every
    per-image quantity is that image's alone), to 1e-12 relative"""
    print()
    for si in range(4):
        for kind in MR.KINDS if si < 3 else ("near",):
            x, y = (t.double()[:2 if si < 3 else 1] for t in MR.case_inputs(si, kind))
            B, C, H, W = x.shape
            gout = MR.case_gout(si).double()[:B]
            xn, yn = x.numpy(), y.numpy()
            f = SX.forward_ref(xn, yn)
            mean, _, img, _ = SX.means_ref(f["S"], f["bS"])
            d = [rel(f["S"], MR.ssim_map(x, y).numpy()), rel(mean, float(MR.ssim(x, y, True))), rel(img, MR.ssim(x, y, False).numpy())]
            for side, (a, b) in enumerate(((x, y), (y, x))):
                fs = f if side == 0 else SX.forward_ref(yn, xn)
                an, bn = a.numpy(), b.numpy()
                g_mean, _ = SX.grad_ref(fs["planes"], an, bn)
                g_img, _ = SX.grad_ref(fs["planes"], an, bn, per_image=True, gout=gout.numpy())
                w = [SX.wsum(np.abs(fs["planes"][i])) for i in range(3)]
                terms = float((w[0] + 2 * np.abs(an) * w[1] + np.abs(bn) * w[2]).max()) / x.numel()
                d += [rel(g_mean, MR.ssim_autograd(x, y, True, wrt=side).numpy(), terms), rel(g_img, MR.ssim_autograd(x, y, False, gout=gout, wrt=side).numpy(), terms),
                      rel(g_mean, MR.ssim_backward_formula(a, b, torch.full((B, 1, 1, 1), 1.0 / x.numel(), dtype=torch.float64)).numpy(), terms)]
            print("   %-18s %-6s largest relative difference %.2e" % (MR.SHAPES[si], kind, max(d)))
            assert max(d) <= 1e-12, (si, kind, d)


def s_of(v):
    p, m, q, q2, r = v
    return (2 * p * m + SX.C1) * (2 * (r - p * m) + SX.C2) / ((p * p + m * m + SX.C1) * ((q - p * p) + (q2 - m * m) + SX.C2))


def test_planes_agree_with_finite_differences_of_s():
    for key in ((17, 68, 2, 3, "indep", 0), (33, 70, 1, 3, "near", 0), (16, 132, 3, 4, "const", 0), (33, 132, 3, 4, "impulse", 0)):
        c = SX.ssim_case(*next(k for k in SX.ssim_keys() if k[:2] == key[:2] and k[4] == key[4]))
        f = c.fwd(0)
        H, W = c.H, c.W
        for at in ((0, 0, 0, 0), (c.B - 1, c.C - 1, H - 1, W - 1), (0, 0, H // 2, W // 2), (0, c.C - 1, min(15, H - 1), min(63, W - 1)), (c.B - 1, 0, min(16, H - 1), min(64, W - 1))):
            v = np.array([s[at] for s in f["sums"]])
            assert abs(s_of(v) - f["S"][at]) <= 1e-13 * abs(f["S"][at])
            for plane, i in ((0, 0), (1, 2), (2, 4)):
                h = 1e-6 * max(abs(v[i]), 1e-3)
                e = np.zeros(5)
                e[i] = h
                fd = (s_of(v + e) - s_of(v - e)) / (2 * h)
                got = f["planes"][plane][at]
                assert abs(fd - got) <= 1e-5 * max(abs(got), 1.0), (c.label, at, plane, fd, got)


# ----------------------------------------------------------------------------------------------------------------- PSNR
def imit_psnr(c, defect=None):
    d = (c.a.astype(f32) - c.b.astype(f32)).astype(np.float64)
    mse = f32((d * d).sum() / float(c.n))
    base = np.log(f32(10.0))
    mv = f32(c.max_val)
    if mse == 0:
        return np.array([np.inf if defect == "gate returning inf for equal inputs" else 0.0], dtype=f32)
    first = np.log(mv * mv) / base if defect == "log of max_val squared once instead of 20 log" else f32(20) * np.log(mv) / base
    return np.array([first - f32(10) * np.log(mse) / base], dtype=f32)


def test_faithful_psnr_imitation_and_its_defects():
    w = 0.0
    for key in SX.PSNR_KEYS:
        c = SX.psnr_case(*key)
        cm = must_pass(c.check(imit_psnr(c)))
        w = max(w, SX.worst(cm))
        if c.kind == "equal":
            assert float(imit_psnr(c)[0]) == 0.0 and c.bound == 0.0
    print("\n   worst multiple of the bound  psnr %.3f over %d cases" % (w, len(SX.PSNR_KEYS)))
    c = SX.psnr_case(257, 255.0, "equal")
    print("   caught:", must_fail(c.check(imit_psnr(c, "gate returning inf for equal inputs")), "gate returning inf", c.label))
    c = SX.psnr_case(257, 255.0, "noisy")
    print("   caught:", must_fail(c.check(imit_psnr(c, "log of max_val squared once instead of 20 log")), "log of max_val squared", c.label))


def test_derived_psnr_bound_against_the_literals_of_test_gpu_metrics():
    """tests/test_gpu_metrics.py::test_psnr_against_restatement bounds its cases by 2e-5 (max_val 1) and 4e-5 dB (255); the derived bound is
    larger than the literal in every case at max_val 255 (20 log10(255) = 48 dB alone carries 2 R 48 = 2.3e-5 for its product and
    quotient) and in some at max_val 1, so that test keeps its literals"""
    for si in range(3):
        for kind in ("indep", "near", "smooth"):
            x, y = MR.case_inputs(si, kind)
            _, b = SX.psnr_of((255.0 * x).double().numpy(), (255.0 * y).double().numpy(), 255.0)
            assert b > 4e-5, (si, kind, b)


# ----------------------------------------------------------------------------------------------------------------- confusion counts
def imit_confusion(c, defect=None):
    B, per = c.B, c.per
    P = SX.conf_nparts(per)
    out = np.zeros((1 + B, 4), dtype=np.int64)
    pf, gf = c.pred.reshape(-1), c.gt.reshape(-1)
    stride = per - 1 if defect == "image base from the wrong per_image" else per
    for b in range(B):
        lo = b * stride
        parts = np.zeros((P, 4), dtype=np.int64)
        for j in range(P):                                   # workgroup j: elements j*256 + t + k*P*256
            i = np.arange(per)
            mine = (i // 256) % P == j
            pv, gv = pf[lo:lo + per][mine], gf[lo:lo + per][mine]
            with np.errstate(invalid="ignore"):
                tp, tg = f32(c.thr_pred), f32(c.thr_gt)
                if defect == "uint8 threshold truncated to an integer":
                    tp, tg = (f32(int(tp)) if c.pdt == "u8" else tp), (f32(int(tg)) if c.gdt == "u8" else tg)
                p = pv.astype(f32) >= tp if defect == ">= for >" else pv.astype(f32) > tp
                g = gv.astype(f32) >= tg if defect == ">= for >" else gv.astype(f32) > tg
            parts[j] = [(~p & ~g).sum(), (p & g).sum(), (~p & g).sum(), (p & ~g).sum()]
        out[1 + b] = parts.sum(0)
    if defect == "FN and FP swapped":
        out[:, [2, 3]] = out[:, [3, 2]]
    out[0] = out[1:B if defect == "totals row omitting the last image" else 1 + B].sum(0)
    return out


CONF_DEFECTS = (
    (">= for >", lambda k: k[2] == "f32" and k[0] == 65),
    ("uint8 threshold truncated to an integer", lambda k: k[2] == "u8" and k[4] == -0.5 and k[0] == 65),
    ("image base from the wrong per_image", lambda k: k[1] == 3 and k[6] == "blocks" and k[0] == 4097),
    ("FN and FP swapped", lambda k: k[0] == 4097 and k[6] == "mixed"),
    ("totals row omitting the last image", lambda k: k[1] == 3 and k[0] == 257),
)


def test_faithful_confusion_imitation_and_its_defects():
    n = 0
    for key in SX.conf_keys():
        c = SX.conf_case(*key)
        must_pass(c.check(imit_confusion(c)))
        n += c.ref.size
        assert int(c.ref[0].sum()) == c.B * c.per
    print("\n   confusion: %d cases, %d counts, all exact" % (len(SX.conf_keys()), n))
    c = SX.conf_case(65, 3, "f32", "u8", 0.5, 127.0, "mixed")
    with np.errstate(invalid="ignore"):
        assert np.isnan(c.pred).any() and (c.pred == f32(0.5)).any() and (c.gt == 127).any() and (c.gt == 128).any()
    for defect, want in CONF_DEFECTS:
        c = SX.conf_case(*next(k for k in SX.conf_keys() if want(k)))
        print("   %-44s caught: %s" % (defect, must_fail(c.check(imit_confusion(c, defect)), defect, c.label)))
