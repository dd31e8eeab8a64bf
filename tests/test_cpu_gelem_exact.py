"""The per-element comparisons of tests/gelem_exact.py without a GPU: a float32 imitation of every kernel of csrc/gelem.hip and csrc/inn.hip
(numpy, its own summation order) passes every case the GPU tests run, each planted defect of the kinds these kernels can have FAILS the
case named for it, and the input conditions hold: grid data is exactly representable in every dtype, no comparison leaves an element out,
the hand-placed activation inputs are where the tables say.  So a green tests/test_gpu_gelem_exact.py means something."""
import math

import numpy as np
import pytest
import torch

import gelem_exact as GX

f32 = np.float32
f64 = np.float64


def a32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def stored(a, dt):
    """float32 values -> what a kernel's store leaves, as float64"""
    return GX.rnd(np.asarray(a, dtype=np.float64), dt)


def must_pass(cmps):
    for c in cmps:
        c.assert_ok()
        assert c.skipped == 0, "%s leaves %d elements out" % (c.what, c.skipped)


def must_fail(cmps, what):
    assert not GX.all_ok(cmps), "the defect `%s` passed every comparison" % what


def erf32(x):
    return torch.erf(torch.from_numpy(a32(x))).numpy()


# ----------------------------------------------------------------------------------------------------------------- activations
def act_f32(kind, x, defect=None):
    with np.errstate(all="ignore"):
        if kind == GX.RELU:
            return np.maximum(x, f32(0))
        if kind == GX.LRELU:
            return np.where(x > 0, x, f32(0.01 if defect == "lrelu slope 0.01" else 0.2) * x)
        if kind == GX.GELU:
            if defect == "gelu by tanh":
                return f32(0.5) * x * (f32(1) + np.tanh(f32(math.sqrt(2 / math.pi)) * (x + f32(0.044715) * x * x * x)))
            return f32(0.5) * x * (f32(1) + erf32(x * f32(GX.INV_SQRT2)))
        if kind == GX.ELU:
            return np.where(x > 0, x, np.expm1(np.minimum(x, f32(0))))
        if kind == GX.SIGMOID:
            return f32(1) / (f32(1) + np.exp(-x))
        return np.tanh(x)


def act_d32(kind, x, defect=None):
    pos = (x >= 0) if defect == "x >= 0" else (x > 0)
    with np.errstate(all="ignore"):
        if kind == GX.RELU:
            return np.where(pos, f32(1), f32(0))
        if kind == GX.LRELU:
            return np.where(pos, f32(1), f32(0.01 if defect == "lrelu slope 0.01" else 0.2))
        if kind == GX.GELU:
            return f32(0.5) * (f32(1) + erf32(x * f32(GX.INV_SQRT2))) + x * f32(GX.INV_SQRT2PI) * np.exp(f32(-0.5) * x * x)
        if kind == GX.ELU:
            return np.where(pos, f32(1), np.exp(np.minimum(x, f32(0))))
        if kind == GX.ELU_OUT:
            if defect == "elu_out as the pre-activation":
                return np.where(pos, f32(1), np.exp(np.minimum(x, f32(0))))
            return np.where(pos, f32(1), x + f32(1))
        if kind == GX.SIGMOID:
            s = f32(1) / (f32(1) + np.exp(-x))
            return s * (f32(1) - s)
        t = np.tanh(x)
        return f32(1) - t * t


def imit_unary(c, defect=None):
    n, ve = c.n, GX.VE[c.dt]
    x = a32(c.x)
    with np.errstate(all="ignore"):
        if c.op == "add":
            y = x + f32(c.alpha) * a32(c.g)
        elif c.op == "fwd":
            y = act_f32(c.kind, x, defect)
        else:
            y = a32(c.g) * act_d32(c.kind, x, defect)
    vec = (n % ve == 0 and c.off == 0) or defect == "tail not written"
    count = (n // ve) * ve if vec else n
    if defect == "one pass":
        count = min(count, GX.UNARY_CAP * (ve if vec else 1))
    buf = np.full(c.off + n + c.pad, GX.SENTINEL)
    buf[c.off:c.off + count] = stored(y[:count], c.dt)
    return buf


@pytest.mark.parametrize("dt", GX.DTYPES)
@pytest.mark.parametrize("op", GX.UNARY_OPS)
def test_unary_imitation_passes(dt, op):
    for key in GX.unary_keys(dt, op):
        c = GX.unary_case(*key)
        must_pass(c.check(imit_unary(c)))


@pytest.mark.parametrize("op", GX.UNARY_OPS)
def test_unary_imitation_passes_above_the_grid_cap(op):
    for key in GX.unary_cap_keys(op):
        c = GX.unary_case(*key)
        must_pass(c.check(imit_unary(c)))
        if op == "fwd":
            must_fail(c.check(imit_unary(c, "one pass")), "one pass")


def _ukey(dt, op, kind, which):
    n, off, data = GX.unary_shapes(dt)[which]
    return (dt, op, kind, n, off, data)


@pytest.mark.parametrize("defect,key", [("tail not written", _ukey("f32", "fwd", GX.RELU, 2)), ("tail not written", _ukey("bf16", "bwd", GX.TANH, 2)),
                                        ("tail not written", _ukey("f16", "add", 1, 2)),
                                        ("x >= 0", _ukey("f32", "bwd", GX.RELU, 2)), ("x >= 0", _ukey("bf16", "bwd", GX.LRELU, 1)),
                                        ("x >= 0", _ukey("f16", "bwd", GX.RELU, 3)),
                                        ("lrelu slope 0.01", _ukey("f32", "fwd", GX.LRELU, 0)), ("lrelu slope 0.01", _ukey("bf16", "bwd", GX.LRELU, 1)),
                                        ("gelu by tanh", _ukey("f32", "fwd", GX.GELU, 2)),
                                        ("elu_out as the pre-activation", _ukey("f32", "bwd", GX.ELU_OUT, 1)),
                                        ("elu_out as the pre-activation", _ukey("bf16", "bwd", GX.ELU_OUT, 2))])
def test_unary_defects_fail(defect, key):
    c = GX.unary_case(*key)
    must_fail(c.check(imit_unary(c, defect)), defect)


def test_unary_inputs_hold_what_they_are_there_for():
    for dt in GX.DTYPES:
        sp = GX.specials(dt)
        assert np.array_equal(GX.rnd(sp, dt), sp) and np.all(np.isfinite(sp))
        assert GX.rnd(np.array([GX.MIN_NORMAL[dt] / 2]), dt)[0] in (0.0, GX.MIN_NORMAL[dt] / 2)     # below it: subnormal
        ve = GX.VE[dt]
        shapes = GX.unary_shapes(dt)
        assert shapes[0][0] == ve and shapes[2][0] % ve == 1 and shapes[3][:2] == (4 * ve, 1)
        for op in GX.UNARY_OPS:
            for key in GX.unary_keys(dt, op):
                c = GX.unary_case(*key)
                assert np.array_equal(GX.rnd(c.x, dt), c.x), c.label
                assert np.all(np.isfinite(c.ref)) and np.all(np.isfinite(c.bound)), c.label
                if c.data == "normal" and op != "add" and c.n >= 7:
                    assert set(sp if c.kind != GX.ELU_OUT else sp[sp >= 0]) <= set(c.x), c.label     # an ELU's output is never below -1
        caps = GX.unary_caps(dt)
        assert caps[0][0] % ve == 0 and caps[0][0] // ve > GX.UNARY_CAP and caps[1][0] % ve != 0 and caps[1][0] > GX.UNARY_CAP
    # the derivative at 0, as the kernels' `x > 0` defines it
    z = np.zeros(1)
    assert [float(GX.act_dref(k, z)[0][0]) for k in (GX.RELU, GX.LRELU, GX.ELU, GX.ELU_OUT)] == [0.0, GX.SLOPE, 1.0, 1.0]
    assert all(float(GX.act_dref(k, z)[1][0]) == 0 for k in (GX.RELU, GX.LRELU, GX.ELU_OUT))


# ----------------------------------------------------------------------------------------------------------------- backward + column sums
def imit_ubc(c, defect=None):
    with np.errstate(all="ignore"):
        gx32 = a32(c.g) * act_d32(c.kind, a32(c.x))
    gx = stored(gx32, c.dt)
    src = gx32.copy() if defect == "sums of the unrounded products" else a32(gx)
    ns = GX.ubc_nsplit(c.npix)
    per = -(-c.npix // ns)
    parts = np.zeros((ns, c.C), dtype=f32)
    for s in range(ns):
        rows = src[s * per:min((s + 1) * per, c.npix)].copy()
        if defect == "lane dropped in the 48-channel block":
            for c0 in range(0, c.C, 64):
                if min(64, c.C - c0) == 48:
                    PL = GX.lanes(48, c.dt)
                    rows[PL - 1::PL, c0:c0 + 48] = 0
        parts[s] = rows.sum(0, dtype=f32)
    tot = parts.sum(0, dtype=f32)
    out = a32(c.out0).copy()
    cr = c.C if defect == "Creal ignored" else c.Creal
    prior = out[:cr] if (c.acc and defect != "accumulate ignored") else f32(0)
    out[:cr] = prior + tot[:cr]
    return gx, out


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_ubc_imitation_passes(dt):
    for key in GX.ubc_keys(dt):
        c = GX.ubc_case(*key)
        must_pass(c.check(*imit_ubc(c)))


def _ubc(dt, **want):
    names = ("dt", "kind", "C", "Creal", "acc", "npix", "data")
    return next(k for k in GX.ubc_keys(dt) if all(k[names.index(n)] == v for n, v in want.items()))


@pytest.mark.parametrize("defect,key", [("sums of the unrounded products", _ubc("bf16", kind=GX.GELU, data="normal")),
                                        ("sums of the unrounded products", _ubc("f16", kind=GX.TANH, data="normal")),
                                        ("lane dropped in the 48-channel block", _ubc("f32", C=48, Creal=48, acc=0, npix=127)),
                                        ("lane dropped in the 48-channel block", _ubc("bf16", C=112, Creal=112, acc=1, npix=1025)),
                                        ("accumulate ignored", _ubc("f32", C=16, Creal=16, acc=1, npix=1)),
                                        ("accumulate ignored", _ubc("bf16", C=64, Creal=61, acc=1, npix=129)),
                                        ("Creal ignored", _ubc("f32", C=48, Creal=45, acc=0, npix=1)),
                                        ("Creal ignored", _ubc("f16", C=112, Creal=109, acc=1, npix=1025, data="grid"))])
def test_ubc_defects_fail(defect, key):
    c = GX.ubc_case(*key)
    must_fail(c.check(*imit_ubc(c, defect)), defect)


def test_ubc_restatement_of_the_launch():
    assert [GX.ubc_nsplit(n) for n in (1, 128, 129, 128 * 512, 128 * 512 + 1)] == [1, 1, 2, 512, 512]
    assert GX.lanes(48, "f32") == 21 and 21 * 12 == 252 and GX.lanes(48, "bf16") == 42 and GX.lanes(64, "f32") == 16 and GX.lanes(16, "bf16") == 128
    assert [GX.qfatt_nsplit(n) for n in (1, 1024, 1025, 64 * 1024 + 1)] == [1, 1, 2, 64]
    for dt in GX.DTYPES:
        for key in GX.ubc_keys(dt):
            c = GX.ubc_case(*key)
            assert np.array_equal(GX.rnd(c.x, dt), c.x) and np.array_equal(GX.rnd(c.g, dt), c.g), c.label


# ----------------------------------------------------------------------------------------------------------------- QFAttention
def imit_qfatt_fwd(c, defect=None):
    B, C = c.B, c.C
    ga, be = a32(c.gamma), a32(c.beta)
    if defect == "gamma by b*C":
        gam = ga.reshape(-1)[np.arange(B)[:, None] * C + np.arange(C)[None, :]]
    else:
        gam = ga[:, :C]
    bet = np.broadcast_to(be[:1, :C], (B, C)) if defect == "beta of sample 0" else be[:, :C]
    return stored(a32(c.x) + gam[:, None, :] * a32(c.res) + bet[:, None, :], c.dt)


def imit_qfatt_bwd(c, defect=None):
    g, res, ga = a32(c.g), a32(c.res), a32(c.gamma)[:, None, :c.C]
    gg, gb = np.full((c.B, c.ldv), GX.SENTINEL), np.full((c.B, c.ldv), GX.SENTINEL)
    gg[:, :c.C], gb[:, :c.C] = (g * res).sum(1, dtype=f32), g.sum(1, dtype=f32)
    return stored(ga * g, c.dt), gg, gb


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_qfatt_imitation_passes(dt):
    for key in GX.qfatt_fwd_keys(dt):
        c = GX.qfatt_case(*key)
        must_pass(c.check_fwd(imit_qfatt_fwd(c)))
    for key in GX.qfatt_bwd_keys(dt):
        c = GX.qfatt_case(*key)
        must_pass(c.check_bwd(*imit_qfatt_bwd(c)))
    if dt == "bf16":
        c = GX.QfattCase("bf16", *GX.QF_FWD_CAP, data="pattern")
        assert c.x.size > GX.UNARY_CAP
        must_pass(c.check_fwd(imit_qfatt_fwd(c)))


@pytest.mark.parametrize("defect,key", [("gamma by b*C", ("f32", 3, 19, 5, "grid")), ("gamma by b*C", ("bf16", 70, 86, 257, "grid")),
                                        ("beta of sample 0", ("f32", 16, 16, 1, "grid")), ("beta of sample 0", ("f16", 70, 86, 257, "normal"))])
def test_qfatt_defects_fail(defect, key):
    assert key in GX.qfatt_fwd_keys(key[0])
    c = GX.qfatt_case(*key)
    must_fail(c.check_fwd(imit_qfatt_fwd(c, defect)), defect)


# ----------------------------------------------------------------------------------------------------------------- global average pool
def imit_gpool(c, defect=None):
    x = a32(c.x)
    lanes = [x[:, l::4].sum(1, dtype=f32) if l < c.hw else np.zeros((x.shape[0], c.C), dtype=f32) for l in range(4)]
    div = f32(-(-c.hw // 4)) if defect == "divided by a lane's share" else f32(c.hw)
    mean = ((lanes[0] + lanes[1]) + (lanes[2] + lanes[3])) / div
    gx = a32(c.g) * (f32(1) / f32(c.hw))
    return mean, stored(np.broadcast_to(gx[:, None, :], c.x.shape), c.dt)


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_gpool_imitation_passes(dt):
    for key in GX.gpool_keys(dt):
        c = GX.gpool_case(*key)
        mean, gx = imit_gpool(c)
        must_pass(c.check_fwd(mean) + c.check_bwd(gx))
        if c.hw & (c.hw - 1) == 0:
            assert not c.gx_bound.any(), c.label


@pytest.mark.parametrize("key", [("f32", 3, 5, "grid"), ("bf16", 64, 1001, "grid")])
def test_gpool_defect_fails(key):
    c = GX.gpool_case(*key)
    must_fail(c.check_fwd(imit_gpool(c, "divided by a lane's share")[0]), "divided by a lane's share")


# ----------------------------------------------------------------------------------------------------------------- padding, unpack
def src_index(j, lo, n, mode, defect=None):
    """the kernels' own form of the source index, one position at a time"""
    t = j - lo
    if mode == 1:
        return min(max(t, 0), n - 1)
    if defect == "reflect":                                # nn.ReflectionPad2d: the edge sample is not repeated
        if n == 1:
            return 0
        t %= 2 * n - 2
        return t if t < n else 2 * n - 2 - t
    t %= 2 * n
    return t if t < n else 2 * n - 1 - t


def imit_pad(c, defect=None):
    B, C, H, W = c.shape
    l, r, t, b = c.pads
    iy = [src_index(j, t, H, c.mode, defect) for j in range(c.PH)]
    ix = [src_index(j, l, W, c.mode, defect) for j in range(c.PW)]
    x, gp = a32(c.x), a32(c.gp)
    out = np.zeros((B, c.PH, c.PW, c.CP), dtype=f32)
    gx = np.zeros(c.shape, dtype=f32)
    for py in range(c.PH):
        for px in range(c.PW):
            out[:, py, px, :C] = x[:, :, iy[py], ix[px]]
            if defect == "second wrap missing" and not (-H <= py - t < 2 * H and -W <= px - l < 2 * W):
                continue
            gx[:, :, iy[py], ix[px]] += gp[:, py, px, :C]
    return stored(out, c.dt), gx


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_pad_imitation_passes(dt):
    for key in GX.pad_keys(dt):
        c = GX.pad_case(*key)
        out, gx = imit_pad(c)
        must_pass(c.check_fwd(out) + c.check_bwd(gx))
        assert np.array_equal(GX.rnd(c.gp, dt), c.gp)
    wraps = GX.pad_case(dt, (1, 3, 3, 4), (5, 6, 7, 4), 0, 32, "grid")
    assert wraps.cnt.max() >= 9 and wraps.pads[2] > 2 * wraps.shape[2]          # more than one wrap: (2 + 1)**2 terms somewhere


@pytest.mark.parametrize("defect,key", [("reflect", ("f32", (1, 2, 5, 7), (2, 3, 4, 1), 0, 16, "grid")),
                                        ("reflect", ("bf16", (1, 3, 4, 5), (3, 0, 0, 0), 0, 16, "grid")),
                                        ("second wrap missing", ("f32", (1, 3, 3, 4), (5, 6, 7, 4), 0, 16, "grid")),
                                        ("second wrap missing", ("f16", (1, 3, 3, 4), (5, 6, 7, 4), 1, 32, "grid"))])
def test_pad_defects_fail(defect, key):
    assert key in GX.pad_keys(key[0])
    c = GX.pad_case(*key)
    out, gx = imit_pad(c, defect)
    must_fail(c.check_fwd(out) if defect == "reflect" else c.check_bwd(gx), defect)


def imit_unpack(c, defect=None):
    B, C, H, W = c.shape
    gx = np.full(c.x.shape, GX.SENTINEL if defect == "outside not written" else 0.0)
    gx[:, :H, :W, :C] = c.g.transpose(0, 2, 3, 1)
    return a32(c.x)[:, :H, :W, :C].transpose(0, 3, 1, 2), stored(gx, c.dt)


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_unpack_imitation_and_its_defect(dt):
    for shape, pshape in GX.UNPACK_KEYS:
        c = GX.UnpackCase(dt, shape, pshape)
        assert pshape[0] > shape[2] and pshape[1] > shape[3] and pshape[2] > shape[1]
        out, gx = imit_unpack(c)
        must_pass(c.check_fwd(out) + c.check_bwd(gx))
        must_fail(c.check_bwd(imit_unpack(c, "outside not written")[1]), "outside not written")


# ----------------------------------------------------------------------------------------------------------------- spectral norm
def imit_sn_fwd(c, do_iter, defect=None):
    W, u, v = a32(c.W), a32(c.u0).copy(), a32(c.v0).copy()
    eps = f32(GX.SN_EPS)
    with np.errstate(all="ignore"):
        if do_iter:
            vraw = W.T @ u
            t = (vraw * vraw).sum(dtype=f32)
            v = vraw / max(t if defect == "normalised by the squared norm" else np.sqrt(t), eps)
        wv = W @ v
        if do_iter or defect == "u updated without an iteration":
            u = wv / max(np.sqrt((wv * wv).sum(dtype=f32)), eps)
        sigma = (u * wv).sum(dtype=f32)
        return u, v, np.array([sigma]), W * (f32(1) / sigma)


def imit_sn_bwd(c, acc, defect=None):
    G, u, v = a32(c.G), a32(c.u0), a32(c.v0)
    d = (G * a32(c.Wsn_in)).sum(dtype=f32)
    inv = f32(1) / f32(c.sigma_in)
    rank1 = d * u[:, None] * v[None, :]
    if defect == "rank-one term divided twice":
        rank1 = rank1 * inv
    val = (G - rank1) * inv
    return (a32(c.gW0) if acc and defect != "accumulate ignored" else f32(0)) + val


@pytest.mark.parametrize("M,N", GX.SN_SHAPES)
def test_spectral_imitation_passes(M, N):
    c = GX.spectral_case(M, N)
    for it in (0, 1):
        must_pass(c.check_fwd(it, *imit_sn_fwd(c, it)))
    for acc in (0, 1):
        must_pass(c.check_bwd(acc, imit_sn_bwd(c, acc)))
    z = GX.spectral_case(3, 5, True)
    cm = z.check_fwd(1, *imit_sn_fwd(z, 1))
    must_pass(cm)
    assert [x.what.split()[-1] for x in cm] == ["u", "v", "sigma"] and all(x.exact for x in cm)


@pytest.mark.parametrize("defect,shape,it", [("normalised by the squared norm", (3, 5), 1), ("normalised by the squared norm", (1030, 8), 1),
                                             ("u updated without an iteration", (33, 257), 0), ("u updated without an iteration", (1, 1), 0)])
def test_spectral_fwd_defects_fail(defect, shape, it):
    c = GX.spectral_case(*shape)
    if shape == (1, 1):
        c = GX.spectral_case(70, 48)
    must_fail(c.check_fwd(it, *imit_sn_fwd(c, it, defect)), defect)


@pytest.mark.parametrize("defect,shape,acc", [("rank-one term divided twice", (3, 5), 0), ("rank-one term divided twice", (70, 48), 1),
                                              ("accumulate ignored", (33, 257), 1)])
def test_spectral_bwd_defects_fail(defect, shape, acc):
    c = GX.spectral_case(*shape)
    must_fail(c.check_bwd(acc, imit_sn_bwd(c, acc, defect)), defect)


# ----------------------------------------------------------------------------------------------------------------- Haar
def haar_neg(k, dy, dx, defect=None):
    if defect == "wavelets 1 and 2 swapped" and k in (1, 2):
        k = 3 - k
    return (0, dx, dy, dy ^ dx)[k]


def imit_haar(c, defect=None):
    B, H, W, C = c.B, c.H, c.W, c.C
    x, fac = a32(c.x), f32(c.fac)
    synth, bywav = c.up & 1, (c.up >> 1) & 1

    def ch(cc, k, real=True):
        return k * C + cc if (bywav and real) else 4 * cc + k
    sg = lambda k, dy, dx: f32(-1.0 if haar_neg(k, dy, dx, defect) else 1.0)
    if synth:
        out = np.zeros((B, 2 * H, 2 * W, c.CPout), dtype=f32)
        for cc in range(C):
            v = [x[..., ch(cc, k)] for k in range(4)]
            for dy in range(2):
                for dx in range(2):
                    out[:, dy::2, dx::2, cc] = fac * ((sg(0, dy, dx) * v[0] + sg(1, dy, dx) * v[1]) + (sg(2, dy, dx) * v[2] + sg(3, dy, dx) * v[3]))
    else:
        out = np.zeros((B, H, W, c.CPout), dtype=f32)
        for cc in range(C):
            v = [[x[:, dy::2, dx::2, cc] for dx in range(2)] for dy in range(2)]
            for k in range(4):
                out[..., ch(cc, k)] = fac * ((sg(k, 0, 0) * v[0][0] + sg(k, 0, 1) * v[0][1]) + (sg(k, 1, 0) * v[1][0] + sg(k, 1, 1) * v[1][1]))
        if defect == "wavelet-major order on padding groups":
            for cc in range(C, c.CPout // 4):
                for k in range(4):
                    if ch(cc, k) < c.CPout:
                        out[..., ch(cc, k)] = 0
    return stored(out, c.dt)


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_haar_imitation_passes(dt):
    for key in GX.haar_keys(dt):
        c = GX.haar_case(*key)
        must_pass(c.check(imit_haar(c)))
        assert c.CPout > (c.C if c.up & 1 else 4 * c.C) or c.C == 1
        if c.fac == 0.5:
            assert not c.bound.any() and np.array_equal(GX.rnd(c.x, dt), c.x) and np.array_equal(GX.rnd(c.raw, dt), c.raw), c.label
    # analysis then synthesis with fac = 0.5 returns the grid input bit for bit
    for up in (0, 2):
        a = GX.haar_case(dt, up, 3, 3, 5, 0.5)
        s = GX.HaarCase(dt, up | 1, 3, 3, 5, 0.5, CPin=a.CPout, CPout=a.CPin)
        s.x = a.ref
        back = imit_haar(s)
        assert np.array_equal(back[..., :3], a.x[..., :3]) and not back[..., 3:].any()


def test_haar_cap_imitation_passes():
    B, H, W, C, CPin, CPout = GX.HAAR_CAP
    assert B * H * W * (CPout // 4) > 8192 * 256
    c = GX.HaarCase("bf16", 0, C, H, W, 0.5, B=B, CPin=CPin, CPout=CPout, data="pattern")
    out = np.zeros(c.ref.shape)
    x = c.x.reshape(B, H, 2, W, 2, CPin)
    for k in range(4):
        out[..., k:4 * C:4] = 0.5 * sum(GX.HAAR_SIGN[k, dy, dx] * x[:, :, dy, :, dx, :C] for dy in range(2) for dx in range(2))
    must_pass(c.check(out))


@pytest.mark.parametrize("defect,key", [("wavelets 1 and 2 swapped", ("f32", 0, 1, 1, 1, 0.5)), ("wavelets 1 and 2 swapped", ("bf16", 3, 12, 3, 5, 0.35)),
                                        ("wavelet-major order on padding groups", ("f32", 2, 3, 3, 5, 0.5)),
                                        ("wavelet-major order on padding groups", ("f16", 2, 12, 1, 1, 0.35))])
def test_haar_defects_fail(defect, key):
    assert key in GX.haar_keys(key[0])
    c = GX.haar_case(*key)
    must_fail(c.check(imit_haar(c, defect)), defect)


# ----------------------------------------------------------------------------------------------------------------- channel copy / place
@pytest.mark.parametrize("dt", GX.DTYPES)
def test_chan_copy_and_place(dt):
    offs = set()
    for key in GX.COPY_KEYS:
        c = GX.ChanCopyCase(dt, *key)
        sstride, soff, dstride, doff, n = key
        dst = np.full((GX.CHAN_NPIX, dstride), GX.SENTINEL)
        dst[:, doff:doff + n] = c.src[:, soff:soff + n]
        must_pass(c.check(dst))
        dst[:, (doff + n) % dstride] = 0.0 if doff + n < dstride else dst[:, 0]
        if doff + n < dstride:
            must_fail(c.check(dst), "one channel too many")
        offs.add("start" if doff == 0 else ("end" if doff + n == dstride else "middle"))
    assert offs == {"start", "middle", "end"}
    forms = set()
    for key in GX.PLACE_KEYS:
        c = GX.ChanPlaceCase(dt, key)
        forms.add((c.vector, c.b is not None, c.b is not None and key[6] < key[2]))
        must_pass(c.check(c.ref.copy()))
        astride, aoff, adst, na = key[:4]
        skipped = np.full(c.ref.shape, GX.SENTINEL)
        skipped[:, adst:adst + na] = c.a[:, aoff:aoff + na]
        if c.b is not None:
            skipped[:, key[6]:key[6] + key[7]] = c.b[:, key[5]:key[5] + key[7]]
        must_fail(c.check(skipped), "zero fill skipped")
    if dt == "f32":
        assert {(True, False, False), (True, True, False), (True, True, True), (False, False, False), (False, True, True)} <= forms


# ----------------------------------------------------------------------------------------------------------------- affine coupling
def imit_coupling(c, defect=None):
    x, s, t, g, v = a32(c.x), a32(c.s), a32(c.t), a32(c.g), a32(c.v)
    clamp, eps = f32(c.clamp), f32(c.eps)
    with np.errstate(all="ignore"):
        sg = f32(1) / (f32(1) + np.exp(-s))
        arg = clamp * (f32(2) * sg - f32(1))
        if defect == "eps inside the exponential":
            ex = np.exp(arg + eps)
            e = ex
        else:
            ex = np.exp(arg)
            e = ex + eps
        de = ex * clamp * f32(2) * sg * (f32(1) - sg)
        if c.rev:
            y, ge = (x - t) / e, g / e
            gx, gt, gs = ge, -ge, -ge * v * de
            if defect == "gs sign for rev":
                gs = -gs
        else:
            y, gx, gt, gs = e * x + t, e * g, g, g * v * de
    return tuple(stored(a, c.dt) for a in (y, gx, gs, gt))


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_coupling_imitation_passes(dt):
    for key in GX.coupling_keys(dt):
        c = GX.coupling_case(*key)
        y, gx, gs, gt = imit_coupling(c)
        must_pass(c.check_fwd(y) + c.check_bwd(gx, gs, gt))
        if c.n >= 3:
            assert list(c.s[:3]) == [0.0, 20.0, -20.0]
    if dt == "bf16":
        c = GX.CouplingCase("bf16", GX.CP_CAP, 0, GX.CP_CLAMP, "pattern")
        y, gx, gs, gt = imit_coupling(c)
        must_pass(c.check_fwd(y) + c.check_bwd(gx, gs, gt))


@pytest.mark.parametrize("defect,key", [("gs sign for rev", ("f32", 257, 1, 1.0, "normal")), ("gs sign for rev", ("bf16", 257, 1, 1.0, "normal")),
                                        ("eps inside the exponential", ("f32", 257, 0, 1.0, "normal")),
                                        ("eps inside the exponential", ("f32", 257, 1, 1.0, "normal"))])
def test_coupling_defects_fail(defect, key):
    assert key in GX.coupling_keys(key[0])
    c = GX.coupling_case(*key)
    y, gx, gs, gt = imit_coupling(c, defect)
    must_fail(c.check_fwd(y) + c.check_bwd(gx, gs, gt), defect)
