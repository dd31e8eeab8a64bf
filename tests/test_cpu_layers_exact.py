"""The per-element comparisons of tests/layers_exact.py without a GPU: a float32 imitation of every operation (numpy, its own summation
order) passes the checks the GPU tests call, each planted defect of the kinds these kernels can have FAILS them, and the input conditions
hold: grid data makes z = scale*y + shift exact in every dtype and 0 or a grid step from 0, the generic cases hold at most 0.1 % ambiguous
elements, the max-pool cases hold at least 5 % windows with a tie between non-zero maxima.  So a green tests/test_gpu_layers_exact.py
means something."""
import numpy as np
import pytest

import layers_exact as LX

f32 = np.float32


def a32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def must_fail(cmps, what):
    assert not LX.all_ok(cmps), "the defect `%s` passed every comparison" % what


def must_pass(cmps):
    for c in cmps:
        c.assert_ok()


# ----------------------------------------------------------------------------------------------------------------- partial rows
def fold32(rows, defect=None):
    """rows [n, ...] float32 -> at most 64 rows, in float32, above 256 rows (defects: at 256 already; the last partial group dropped)"""
    n = rows.shape[0]
    if n <= (255 if defect == "fold at 256" else 256):
        return rows
    last = (n // 64) * 64 if defect == "drop the partial group" else n
    out = np.zeros((64,) + rows.shape[1:], dtype=np.float32)
    for r in range(last):
        out[r % 64] += rows[r]
    return out


def imit_bn_finalize(c, defect=None):
    rows = fold32(a32(c.rows), defect).astype(np.float64)
    C, CP, n = c.C, c.CP, c.count
    s1, s2 = rows[:, 0].sum(0), rows[:, 1].sum(0)
    m = s1 / n
    var = s2 / n - m * m
    if defect != "no var guard":
        var = np.maximum(var, 0.0)
    unb = var * n / (n - 1.0) if n > 1 else var
    if defect == "unbiased batch variance":
        var, unb = unb, unb
    if defect == "biased running variance":
        unb = var
    with np.errstate(invalid="ignore"):
        invstd = (1.0 / np.sqrt(var + LX.BN_EPS)).astype(f32)
    out = {k: np.zeros(CP, dtype=f32) for k in ("scale", "shift", "mean", "invstd")}
    if defect == "padding not zeroed":
        for k in out:
            out[k][:] = f32(0.5)
    sc = a32(c.gamma) * invstd[:C]
    out["scale"][:C], out["invstd"][:C], out["mean"][:C] = sc, invstd[:C], m[:C].astype(f32)
    out["shift"][:C] = a32(c.beta) - m[:C].astype(f32) * sc
    mom = f32(LX.MOMENTUM)
    out["running_mean"] = (f32(1) - mom) * a32(c.rmean) + mom * m[:C].astype(f32)
    out["running_var"] = (f32(1) - mom) * a32(c.rvar) + mom * unb[:C].astype(f32)
    return out


@pytest.mark.parametrize("nparts,C,CP,one", LX.BN_FINALIZE_CASES)
def test_bn_finalize_imitation_passes(nparts, C, CP, one):
    c = LX.bn_finalize_case(nparts, C, CP, one)
    must_pass(c.check(imit_bn_finalize(c)))


def test_bn_finalize_cases_hold_what_they_are_there_for():
    neg = [c for c in (LX.bn_finalize_case(*k) for k in LX.BN_FINALIZE_CASES) if any(c.raw_var[j] < 0 for j in c.const)]
    assert {(c.C, c.CP) for c in neg} >= {(64, 64), (30, 32)}, "no constant channel whose sumsq/count - m*m rounds below 0"
    assert any(c.count == 1 for c in (LX.bn_finalize_case(*k) for k in LX.BN_FINALIZE_CASES))
    assert LX.fold_adds(256) == 0 and LX.fold_adds(257) == 4 and LX.fold_adds(1000) == 15


@pytest.mark.parametrize("defect,key", [("drop the partial group", (257, 64, 64, False)), ("drop the partial group", (1000, 30, 32, False)),
                                        ("fold at 256", (256, 64, 64, False)), ("fold at 256", (256, 3, 16, False)),
                                        ("unbiased batch variance", (33, 30, 32, False)), ("biased running variance", (33, 64, 64, False)),
                                        ("no var guard", None), ("padding not zeroed", (33, 3, 16, False))])
def test_bn_finalize_defects_fail(defect, key):
    if key is None:     # the case whose constant channel has a negative raw variance
        key = next(k for k in LX.BN_FINALIZE_CASES if any(LX.bn_finalize_case(*k).raw_var[j] < 0 for j in LX.bn_finalize_case(*k).const))
    c = LX.bn_finalize_case(*key)
    must_fail(c.check(imit_bn_finalize(c, defect)), defect)


def imit_bn_bwd_finalize(c, defect=None):
    C, CP = c.C, c.CP
    if c.kind == "pooled":
        rows = np.stack([a32(c.gvec) * a32(c.npos), a32(c.gvec) * a32(c.ysum)], axis=1).astype(np.float64)
    else:
        rows = fold32(a32(c.rows), defect).astype(np.float64)
    a1, a2 = rows[:, 0, :C].sum(0), rows[:, 1, :C].sum(0)
    if c.kind != "xhat" and defect != "mean not applied":
        a2 = (a2 - c.mean * a1) * c.invstd
    acc = c.accumulate and defect != "accumulate ignored"
    coef = np.full((3, CP), 0.25 if defect == "padding not zeroed" else 0.0, dtype=f32)
    coef[0, :C], coef[1, :C], coef[2, :C] = a32(c.gamma) * a32(c.invstd), (a1 / c.count).astype(f32), (a2 / c.count).astype(f32)
    return {"dbeta": (a32(c.dbeta0) if acc else f32(0)) + a1.astype(f32), "dgamma": (a32(c.dgamma0) if acc else f32(0)) + a2.astype(f32),
            "coef": coef, "rows": rows.astype(f32)}


@pytest.mark.parametrize("kind,n,C,CP,acc", LX.BN_BWD_FINALIZE_CASES)
def test_bn_bwd_finalize_imitation_passes(kind, n, C, CP, acc):
    c = LX.bn_bwd_finalize_case(kind, n, C, CP, acc)
    out = imit_bn_bwd_finalize(c)
    must_pass(c.check(out))
    if kind == "pooled":
        must_pass(c.check_rows(out["rows"]))


@pytest.mark.parametrize("defect,key", [("drop the partial group", ("xhat", 1000, 64, 64, 0)), ("drop the partial group", ("raw", 257, 30, 32, 1)),
                                        ("mean not applied", ("raw", 33, 64, 64, 0)), ("mean not applied", ("pooled", 17, 30, 32, 0)),
                                        ("accumulate ignored", ("xhat", 33, 3, 16, 1)), ("accumulate ignored", ("pooled", 1, 64, 64, 1)),
                                        ("padding not zeroed", ("raw", 1, 30, 32, 0)), ("padding not zeroed", ("pooled", 17, 3, 16, 1))])
def test_bn_bwd_finalize_defects_fail(defect, key):
    c = LX.bn_bwd_finalize_case(*key)
    must_fail(c.check(imit_bn_bwd_finalize(c, defect)), defect)


def test_pooled_rows_defect_fails():
    c = LX.bn_bwd_finalize_case("pooled", 17, 30, 32, 0)
    rows = imit_bn_bwd_finalize(c)["rows"]
    must_fail(c.check_rows(rows[:, ::-1]), "N+ and S+ swapped")


def imit_colsum(c, defect=None):
    rows = fold32(a32(c.rows), defect).astype(np.float64)
    s = rows[:, :c.C].sum(0).astype(f32)
    return (a32(c.out0) if c.accumulate and defect != "accumulate ignored" else f32(0)) + s


@pytest.mark.parametrize("n,C,ldp,acc", LX.COLSUM_CASES)
def test_colsum_imitation_passes_and_defects_fail(n, C, ldp, acc):
    c = LX.colsum_case(n, C, ldp, acc)
    must_pass(c.check(imit_colsum(c)))
    if n > 256:
        must_fail(c.check(imit_colsum(c, "drop the partial group")), "drop the partial group")
    if acc:
        must_fail(c.check(imit_colsum(c, "accumulate ignored")), "accumulate ignored")


# ----------------------------------------------------------------------------------------------------------------- input conditions
def test_grid_data_makes_z_exact_in_every_dtype():
    for dt in LX.DTYPES:
        for CP, B, hw, gf, gap, data in LX.bn_bwd_cases(dt):
            if data == "grid":
                c = LX.bn_bwd_case(dt, CP, B, hw, gf, gap, data)
                assert LX.z_is_exact(c.z, dt), c.label
                assert np.array_equal(LX.rnd(c.y, dt), c.y) and np.array_equal(LX.rnd(c.g, dt), c.g), c.label
        for CP, hw, gap, data in LX.avgpool_cases(dt):
            if data == "grid":
                assert LX.z_is_exact(LX.avgpool_case(dt, CP, hw, gap, data).z, dt)
        for C, c0, s in LX.copy_cases(dt):
            assert LX.z_is_exact(LX.CopyCase(dt, C, c0, s).z, dt)
        for B, H, W in LX.POOL2_SHAPES:
            for C in LX.POOL2_C[dt]:
                assert LX.z_is_exact(LX.maxpool_case(dt, B, H, W, C).z, dt)
        for row in LX.upconv_cases() + LX.upconv_cases(mfma=True):
            c = LX.upconv_case(dt, *row)
            assert LX.z_is_exact(c.z, dt), c.label
        for B, H, W in LX.LAYOUT_SHAPES:
            assert LX.z_is_exact(LX.layout_case(dt, B, H, W).z, dt)
        for row in LX.head_fwd_cases(dt) + LX.head_bwd_cases(dt):
            c = LX.HeadCase(dt, *row)
            assert LX.z_is_exact(c.z, dt) and np.array_equal(LX.rnd(c.y, dt), c.y), c.label
    dt, CP, B, hw = LX.BWD_LARGE
    for gf in ("g", "gvec"):
        c = LX.BnBwdCase(dt, CP, B, hw, gf, 0)
        assert LX.z_is_exact(c.z, dt) and np.array_equal(LX.rnd(c.y, dt), c.y) and np.array_equal(LX.rnd(c.g, dt), c.g), c.label


def test_generic_cases_hold_at_most_one_per_mille_ambiguous_elements():
    for dt in LX.DTYPES:
        for CP, B, hw, gf, gap, data in LX.bn_bwd_cases(dt):
            if data != "grid":
                c = LX.bn_bwd_case(dt, CP, B, hw, gf, gap, data)
                assert float(c.amb.mean()) <= 1e-3, (c.label, float(c.amb.mean()))
        for CP, hw, gap, data in LX.avgpool_cases(dt):
            if data != "grid":
                c = LX.avgpool_case(dt, CP, hw, gap, data)
                assert float(c.amb.mean()) <= 1e-3, (c.label, float(c.amb.mean()))


def test_maxpool_cases_hold_ties_between_non_zero_maxima():
    for dt in LX.DTYPES:
        for B, H, W in LX.POOL2_SHAPES:
            for C in LX.POOL2_C[dt]:
                c = LX.maxpool_case(dt, B, H, W, C)
                if c.pooled.size >= 64:          # (a 2 x 2 image with 4 channels is 4 windows)
                    assert c.tie_share >= 0.05, (c.label, c.tie_share)


# ----------------------------------------------------------------------------------------------------------------- BN backward passes
def imit_bn_bwd(c, defect=None):
    """float32, numpy's pairwise sums; -> (rows [1, 2, CP], dy buffer [npix, ld], bias rows [1, CP])"""
    y, sc, sh, mu, isd = a32(c.y), a32(c.sc), a32(c.sh), a32(c.mu), a32(c.isd)
    ca, c1, c2 = a32(c.coef)
    npix = c.npix
    if c.gform == "gvec":
        hw = c.hw + 1 if defect == "gvec of sample p / (hw + 1)" else c.hw
        g = a32(c.gvec)[np.minimum(np.arange(npix) // hw, c.B - 1)]
    else:
        g = a32(c.g)
    z = sc * y + sh
    gz = np.where(z > 0, g, f32(0))
    xh = (y - mu) * isd
    dy = LX.rnd(ca * (gz - c1 - xh * c2), c.dt)
    ppb = LX.BWD_BT // (c.CP // LX.VE[c.dt])
    done = (npix // ppb) * ppb if defect == "pixel tail skipped" else npix
    rows = np.stack([gz[:done].sum(0, dtype=f32), (gz * xh)[:done].sum(0, dtype=f32)])[None]
    buf = LX.sentinel_dest(npix, c.ld, c.dt).double().numpy()
    if defect == "ld ignored":
        flat = buf.reshape(-1)
        flat[:npix * c.CP] = dy.reshape(-1)
    else:
        buf[:done, :c.CP] = dy[:done]
    bias = (ca * (gz - c1 - xh * c2))[:done].sum(0, dtype=f32)[None]
    return rows, buf, bias


@pytest.mark.parametrize("dt", LX.DTYPES)
def test_bn_bwd_imitation_passes(dt):
    for row in LX.bn_bwd_cases(dt):
        c = LX.bn_bwd_case(dt, *row)
        rows, buf, bias = imit_bn_bwd(c)
        must_pass(c.check_reduce(rows) + c.check_apply(buf, bias, "imitation"))


@pytest.mark.parametrize("dt", LX.DTYPES)
def test_bn_bwd_defects_fail(dt):
    CP = LX.CPS[dt][1]
    c = LX.bn_bwd_case(dt, CP, 5, 480, "g", 0)
    assert c.npix % (LX.BWD_BT // (CP // LX.VE[dt])) != 0
    rows, buf, bias = imit_bn_bwd(c, "pixel tail skipped")
    must_fail(c.check_reduce(rows), "pixel tail skipped (reduce)")
    must_fail(c.check_apply(buf, None, "defect"), "pixel tail skipped (dy)")
    must_fail(c.check_apply(imit_bn_bwd(c)[1], bias, "defect"), "pixel tail skipped (dbias)")
    c = LX.bn_bwd_case(dt, CP, 3, 43, "gvec", 0)
    rows, buf, bias = imit_bn_bwd(c, "gvec of sample p / (hw + 1)")
    must_fail(c.check_reduce(rows), "gvec of sample p / (hw + 1) (reduce)")
    must_fail(c.check_apply(buf, None, "defect"), "gvec of sample p / (hw + 1) (dy)")
    c = LX.bn_bwd_case(dt, CP, 3, 43, "g", LX.GAP)
    must_fail(c.check_apply(imit_bn_bwd(c, "ld ignored")[1], None, "defect"), "ld ignored")


# ----------------------------------------------------------------------------------------------------------------- average pool
def imit_avgpool(c, defect=None):
    y = a32(c.y).reshape(c.B, c.hw, c.CP)
    z = a32(c.sc) * y + a32(c.sh)
    ppb = 256 // (c.CP // LX.VE[c.dt])
    done = (c.hw // ppb) * ppb if defect == "pixel tail skipped" else c.hw
    pos = (z >= 0) if defect == "N+ counts z >= 0" else (z > 0)
    mean = (np.maximum(z, f32(0))[:, :done].sum(1, dtype=f32).astype(np.float64) * float(f32(1.0 / c.hw))).astype(f32)
    return mean, pos[:, :done].sum(1).astype(f32), np.where(pos, y, f32(0))[:, :done].sum(1, dtype=f32)


@pytest.mark.parametrize("dt", LX.DTYPES)
def test_avgpool_imitation_passes_and_defects_fail(dt):
    for row in LX.avgpool_cases(dt):
        c = LX.avgpool_case(dt, *row)
        if c.hw > 5000 and c.CP != LX.CPS[dt][0]:
            continue                              # (the 70000-pixel case once per dtype is enough here)
        must_pass(c.check(*imit_avgpool(c), form="imitation"))
    c = LX.avgpool_case(dt, LX.CPS[dt][1], 1025, 0)
    assert bool((c.z == 0).any())
    must_fail(c.check(*imit_avgpool(c, "N+ counts z >= 0")), "N+ counts z >= 0")
    must_fail(c.check(*imit_avgpool(c, "pixel tail skipped")), "pixel tail skipped")
    must_fail(c.check(imit_avgpool(c, "pixel tail skipped")[0]), "pixel tail skipped (plain form)")


# ----------------------------------------------------------------------------------------------------------------- copy, max pool
def imit_copy(c, defect=None):
    buf = c.dest().double().numpy()
    v = np.maximum(a32(c.sc) * a32(c.x) + a32(c.sh), f32(0)) if c.with_scale and defect != "scale ignored" else a32(c.x)
    c0 = 0 if defect == "c0 ignored" else c.c0
    buf[:, c0:c0 + c.C] = LX.rnd(v, c.dt)
    return buf


@pytest.mark.parametrize("dt", LX.DTYPES)
def test_copy_imitation_passes_and_defects_fail(dt):
    for C, c0, s in LX.copy_cases(dt):
        c = LX.CopyCase(dt, C, c0, s)
        must_pass(c.check(imit_copy(c)))
        if c0:
            must_fail(c.check(imit_copy(c, "c0 ignored")), "c0 ignored")
        if s:
            must_fail(c.check(imit_copy(c, "scale ignored")), "scale ignored")


def imit_maxpool(c, c0a, with_skip, defect=None):
    B, H, W, C = c.B, c.H, c.W, c.C
    a = LX.rnd(np.maximum(a32(c.sc) * a32(c.y) + a32(c.sh), f32(0)), c.dt)
    win = a.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4, C)
    pooled = win.max(3)
    sel = 3 - win[:, :, :, ::-1].argmax(3) if defect == "last maximum" else win.argmax(3)
    route = np.zeros_like(win)
    np.put_along_axis(route, sel[:, :, :, None, :], c.gp[:, :, :, None, :], axis=3)
    g = route.reshape(B, H // 2, W // 2, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    if with_skip:
        g = LX.rnd(g + c.gs, c.dt)
    act = LX.sentinel_dest(B * H * W, c0a + C + LX.GAP, c.dt).double().numpy()
    at = 0 if defect == "c0 ignored" else c0a
    act[:, at:at + C] = a.reshape(-1, C)
    return pooled, act, g


@pytest.mark.parametrize("dt", LX.DTYPES)
def test_maxpool_imitation_passes_and_defects_fail(dt):
    for B, H, W in LX.POOL2_SHAPES:
        for C in LX.POOL2_C[dt]:
            c = LX.maxpool_case(dt, B, H, W, C)
            for c0a in (0, C):
                for skip in (False, True):
                    pooled, act, g = imit_maxpool(c, c0a, skip)
                    must_pass(c.check_fwd(pooled, act, c0a) + c.check_bwd(g, skip))
            if c.pooled.size >= 64:
                must_fail(c.check_bwd(imit_maxpool(c, 0, True, "last maximum")[2], True), "last maximum")
            must_fail(c.check_fwd(*imit_maxpool(c, C, False, "c0 ignored")[:2], C), "c0 ignored")


# ----------------------------------------------------------------------------------------------------------------- up-convolution
def imit_upconv(c, accumulate, defect=None):
    B, H, W, Cin, Cout = c.B, c.H, c.W, c.Cin, c.Cout
    a = a32(c.a).reshape(B, H, W, Cin)
    w = a32(c.w_used)
    if defect == "weight read as [Cout][Cin]":
        w = np.ascontiguousarray(w.reshape(-1).reshape(Cout, Cin, 2, 2).transpose(1, 0, 2, 3))
    if defect == "taps transposed":
        w = np.ascontiguousarray(w.transpose(0, 1, 3, 2))
    times = -(-Cin // 16) + 1 if defect == "bias per partial sum" else 1
    y = np.einsum("bhwc,coij->bhiwjo", a, w).astype(f32).reshape(B, 2 * H, 2 * W, Cout) + f32(times) * a32(c.bias)
    buf = c.dest().double().numpy()
    c0 = 0 if defect == "c0 ignored" else c.c0
    buf[:, c0:c0 + Cout] = LX.rnd(y, c.dt).reshape(-1, Cout)
    g6 = a32(c.gy).reshape(B, H, 2, W, 2, Cout)
    gx = LX.rnd(np.einsum("bhiwjo,coij->bhwc", g6, w).astype(f32), c.dt)
    dw = np.einsum("bhwc,bhiwjo->coij", a, g6).astype(f32)
    db = g6.sum((0, 1, 2, 3, 4), dtype=f32)
    if accumulate:
        dw, db = dw + a32(c.dw0), db + a32(c.db0)
    return buf, gx, dw, db


@pytest.mark.parametrize("dt", LX.DTYPES)
@pytest.mark.parametrize("mfma", [False, True], ids=["scalar", "mfma"])
def test_upconv_imitation_passes_and_defects_fail(dt, mfma):
    if mfma and dt == "f32":
        return                                    # the MFMA form is 16-bit only
    for i, row in enumerate(LX.upconv_cases(mfma)):
        c = LX.upconv_case(dt, *row, w16=mfma)
        acc = bool(i % 2)
        buf, gx, dw, db = imit_upconv(c, acc)
        must_pass(c.check_fwd(buf) + c.check_bwd(gx, dw, db, acc))
        if c.H > 1 and not (mfma and i % 3):
            for defect in ("taps transposed", "weight read as [Cout][Cin]", "bias per partial sum"):
                buf, gx, dw, db = imit_upconv(c, acc, defect)
                must_fail(c.check_fwd(buf), defect)
                if defect != "bias per partial sum":
                    must_fail(c.check_bwd(gx, dw, db, acc)[:1], defect + " (gx)")
            if c.c0:
                must_fail(c.check_fwd(imit_upconv(c, acc, "c0 ignored")[0]), "c0 ignored")
            must_fail(c.check_bwd(gx, dw.transpose(0, 1, 3, 2), db, acc)[1:2], "dw taps transposed")
            must_fail(c.check_bwd(gx, dw, db, not acc)[1:], "accumulate ignored")
        if mfma:
            w16 = LX.rnd(c.w, dt)
            wf = w16.transpose(2, 3, 1, 0).reshape(4 * c.Cout, c.Cin)
            must_pass(c.check_pack(wf, wf.T))
            must_fail(c.check_pack(c.w.transpose(2, 3, 1, 0).reshape(4 * c.Cout, c.Cin), wf.T), "pack not rounded")
            must_fail(c.check_pack(w16.transpose(3, 2, 1, 0).reshape(4 * c.Cout, c.Cin), wf.T), "pack taps transposed")


# ----------------------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("dt", LX.DTYPES)
def test_layout_imitation_passes_and_defects_fail(dt):
    ve = LX.VE[dt]
    for B, H, W in LX.LAYOUT_SHAPES:
        c = LX.layout_case(dt, B, H, W)
        npix = B * H * W
        # nchw -> nhwc: the 3 -> 16 image path and the general one (5 planes at c0 = 8, 3 zero channels)
        for planes, c0, tail, ld, what in ((c.img, 0, 13, 16, "image"), (c.planes, 8, 3, 8 + 5 + 3 + 16, "general")):
            buf = LX.sentinel_dest(npix, ld, dt).double().numpy()
            buf[:, c0:c0 + planes.shape[1]] = c.to_nhwc(planes)
            must_fail(c.check_nchw_to_nhwc(buf, planes, c0, tail, what), "padding not zeroed")
            buf[:, c0 + planes.shape[1]:c0 + planes.shape[1] + tail] = 0
            must_pass(c.check_nchw_to_nhwc(buf, planes, c0, tail, what))
            bad = LX.sentinel_dest(npix, ld, dt).double().numpy()
            bad[:, :planes.shape[1] + tail] = buf[:, c0:c0 + planes.shape[1] + tail]
            if c0:
                must_fail(c.check_nchw_to_nhwc(bad, planes, c0, tail, what), "c0 ignored")
        vals = c.to_nhwc(c.planes)
        back = vals.reshape(B, H * W, 5).transpose(0, 2, 1).reshape(B, 5, H, W)
        must_pass(c.check_nhwc_to_nchw(back, vals, "imitation"))
        must_fail(c.check_nhwc_to_nchw(back, vals[:, ::-1], "defect"), "channels reversed")
        c0, tail, ld = 2 * ve, 40, 2 * ve + 40 + 16
        buf = LX.sentinel_dest(npix, ld, dt).double().numpy()
        buf[:, c0:c0 + tail] = c.tail_ref(tail)
        must_pass(c.check_concat_tail(buf, c0, tail))
        bc = LX.sentinel_dest(npix, c0 + 30 + 1, dt).double().numpy()
        bc[:, c0:c0 + 30] = np.repeat(c.msg, H * W, axis=0)
        must_pass(c.check_broadcast(bc, c0))
        if B > 1:
            bc[:, c0:c0 + 30] = np.repeat(c.msg[::-1], H * W, axis=0)
            must_fail(c.check_broadcast(bc, c0), "message of another sample")
        if H > 1:
            swapped = buf.copy()
            swapped[:, c0 + 30:c0 + 33] = swapped[:, c0 + 30:c0 + 33][::-1]
            must_fail(c.check_concat_tail(swapped, c0, tail), "image pixels of another position")
            first = buf.copy()
            first[:, c0:c0 + 30] = c.msg[0]
            must_fail(c.check_concat_tail(first, c0, tail), "message of sample 0 everywhere")
        full = np.concatenate([np.maximum(c.z, 0.0), c.tail_ref(40)], axis=1)
        must_pass(c.check_concat_full(full))
        must_fail(c.check_concat_full(np.concatenate([c.x, c.tail_ref(40)], axis=1)), "BN + ReLU not applied")


# ----------------------------------------------------------------------------------------------------------------- 1x1 heads
def imit_head_fwd(c, act, defect=None):
    a, w = a32(c.a), a32(c.w)
    pre = (a @ w.T + a32(c.bias)).astype(f32)
    if defect == "pixel tail skipped":
        p = LX.head_ppb(c.Cin, c.dt)
        pre[(c.npix // (4 * p)) * 4 * p:] = 0
    out = (f32(1) / (f32(1) + np.exp(-pre))).astype(f32) if act else pre
    a16 = np.zeros((c.npix, 16))
    if defect == "act16 tail not zero":
        a16[:, LX.VE[c.dt]:] = 0.5                      # only the first 16-byte piece written
    a16[:, :c.Cout] = LX.rnd(out, c.dt)
    if defect == "act16 not the rounding of out":
        a16[:, :c.Cout] = LX.rnd(out.astype(np.float64) * (1 + 2.0 ** -7), c.dt)
    return out.reshape(c.B, c.hw, c.Cout).transpose(0, 2, 1), a16


@pytest.mark.parametrize("dt", LX.DTYPES)
def test_head_fwd_imitation_passes_and_defects_fail(dt):
    for i, row in enumerate(LX.head_fwd_cases(dt)):
        c = LX.HeadCase(dt, *row)
        for act in (0, 1):
            out, a16 = imit_head_fwd(c, act)
            must_pass(c.check_fwd(out, act, a16 if act == 0 else None))
        if c.npix % (4 * LX.head_ppb(c.Cin, dt)) == 1 or c.npix == 231:
            must_fail(c.check_fwd(imit_head_fwd(c, 0, "pixel tail skipped")[0], 0), "pixel tail skipped")
            must_fail(c.check_fwd(imit_head_fwd(c, 1, "pixel tail skipped")[0], 1), "pixel tail skipped (sigmoid)")
        out, a16 = imit_head_fwd(c, 0, "act16 tail not zero")
        must_fail(c.check_fwd(out, 0, a16), "act16 tail not zero")
        if dt != "f32":
            out, a16 = imit_head_fwd(c, 0, "act16 not the rounding of out")
            must_fail(c.check_fwd(out, 0, a16), "act16 not the rounding of out")


def imit_head_bwd(c, accumulate, defect=None):
    a, w, go = a32(c.a), a32(c.w), a32(c.go)
    g32 = (go @ w).astype(f32)
    gst = LX.rnd(g32, c.dt)
    buf = LX.sentinel_dest(c.npix, c.ld, c.dt).double().numpy()
    if defect == "ld ignored":
        buf.reshape(-1)[:c.npix * c.Cin] = gst.reshape(-1)
    else:
        buf[:, :c.Cin] = gst
    done = (c.npix // LX.head_ppb(c.Cin, c.dt)) * LX.head_ppb(c.Cin, c.dt) if defect == "pixel tail skipped" else c.npix
    dw = (go[:done].T @ a[:done]).astype(f32) + (a32(c.dw0) if accumulate else f32(0))
    db = go[:done].sum(0, dtype=f32) + (a32(c.db0) if accumulate else f32(0))
    gm = g32.astype(np.float64) if defect == "bn rows from the unrounded g" else gst
    gz = np.where(a32(c.z) > 0, gm, 0.0).astype(f32)
    rows = np.stack([gz.sum(0, dtype=f32), (gz * a32(c.y)).sum(0, dtype=f32)])[None]
    return buf, dw, db, rows


@pytest.mark.parametrize("dt", LX.DTYPES)
def test_head_bwd_imitation_passes_and_defects_fail(dt):
    for i, row in enumerate(LX.head_bwd_cases(dt)):
        c = LX.HeadCase(dt, *row)
        acc = bool(i % 2)
        buf, dw, db, rows = imit_head_bwd(c, acc)
        must_pass(c.check_bwd(buf, dw, db, acc, rows if c.with_scale else None))
        must_fail(c.check_bwd(buf, dw, db, not acc)[-2:], "accumulate ignored")
        if c.npix == 513:
            b2, dw2, db2, r2 = imit_head_bwd(c, acc, "pixel tail skipped")
            must_fail(c.check_bwd(buf, dw2, db2, acc)[-2:], "pixel tail skipped")
        if c.gap:
            must_fail(c.check_bwd(imit_head_bwd(c, acc, "ld ignored")[0], dw, db, acc), "ld ignored")
        if c.with_scale and dt != "f32" and c.npix == 1:
            r2 = imit_head_bwd(c, acc, "bn rows from the unrounded g")[3]
            must_fail(c.check_bwd(buf, dw, db, acc, r2)[-2:], "bn rows from the unrounded g")


# ----------------------------------------------------------------------------------------------------------------- linear / pooled heads
def imit_linear(c, g, defect=None):
    """float32: -> (out, dw, db, gvec) for the gradient g [B, O]"""
    p, w = a32(c.pooled[:, :c.I]), a32(c.w)
    if defect == "ldp ignored":
        p = a32(c.pooled).reshape(-1)[:c.B * c.I].reshape(c.B, c.I)
    out = (p @ w.T + a32(c.bias)).astype(f32)
    acc = c.accumulate and defect != "accumulate ignored"
    dw = (a32(g).T @ p).astype(f32) + (a32(c.dw0) if acc else f32(0))
    db = a32(g).sum(0, dtype=f32) + (a32(c.db0) if acc else f32(0))
    gvec = np.full((c.B, c.CP), 0.25 if defect == "gvec tail not zero" else 0.0, dtype=f32)
    gvec[:, :c.I] = (a32(g) @ w).astype(f32) * f32(LX.INV_HW)
    return out, dw, db, gvec


def imit_pooled_head(c, kind, defect=None):
    logits = imit_linear(c, c.gout)[0]
    v = logits.astype(np.float64)
    n = v.size
    if kind == 0:
        loss = np.array([(np.maximum(v, 0) - v * c.target + np.log1p(np.exp(-np.abs(v)))).sum() / n], dtype=f32)
        g = ((1 / (1 + np.exp(-v)) - c.target) * c.gscale / n).astype(f32)
    else:
        d = v - c.msg
        loss = np.array([(d * d).sum() / n, np.abs(np.clip(np.rint(v), 0, 1) - c.msg).sum() / n], dtype=f32)
        g = (d * c.gscale).astype(f32)
    if defect == "gradient not divided by n":
        g = g * f32(n)
    _, dw, db, gvec = imit_linear(c, g)
    gv = gvec.astype(np.float64)
    C = c.C
    r1, r2 = (a32(gv) * a32(c.out3[1])).astype(np.float64), (a32(gv) * a32(c.out3[2])).astype(np.float64)
    s1, s2 = r1[:, :C].sum(0), r2[:, :C].sum(0)
    if defect != "mean not applied":
        s2 = (s2 - c.mean * s1) * c.invstd
    acc = 1 if c.accumulate else 0
    coef = np.zeros((3, c.CP), dtype=f32)
    coef[0, :C], coef[1, :C], coef[2, :C] = a32(c.gamma) * a32(c.invstd), (s1 / c.count).astype(f32), (s2 / c.count).astype(f32)
    return logits, loss, dw, db, gvec, (acc * a32(c.dgamma0) + s2.astype(f32)), (acc * a32(c.dbeta0) + s1.astype(f32)), coef


@pytest.mark.parametrize("B,I,O,acc", LX.LINEAR_CASES)
def test_linear_and_pooled_head_imitations_pass_and_defects_fail(B, I, O, acc):
    c = LX.linear_case(B, I, O, acc)
    assert c.ldp > I and c.CP > I
    out, dw, db, gvec = imit_linear(c, c.gout)
    must_pass(c.check_fwd(out) + c.check_bwd(dw, db, gvec))
    if B > 1 or I > 1:
        must_fail(c.check_fwd(imit_linear(c, c.gout, "ldp ignored")[0]), "ldp ignored")
    must_fail(c.check_bwd(*imit_linear(c, c.gout, "gvec tail not zero")[1:]), "gvec tail not zero")
    if acc:
        must_fail(c.check_bwd(*imit_linear(c, c.gout, "accumulate ignored")[1:]), "accumulate ignored")
    for kind in (0, 1):
        must_pass(c.check_pooled_head(kind, *imit_pooled_head(c, kind)))
        must_fail(c.check_pooled_head(kind, *imit_pooled_head(c, kind, "mean not applied")), "mean not applied")
        if kind == 0 and B * O > 1:
            must_fail(c.check_pooled_head(kind, *imit_pooled_head(c, kind, "gradient not divided by n")), "gradient not divided by n")
