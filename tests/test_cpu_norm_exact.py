"""The per-element comparisons of tests/norm_exact.py without a GPU: a float32 imitation of every entry point of csrc/instnorm.hip,
csrc/dice.hip and csrc/mask_head.hip (numpy float32 operations, double sums, its own layout arithmetic and summation order) passes every
case key the GPU tests run; each planted defect FAILS a named comparison; the helper's zero-ambiguous-elements assertion holds on every
case; and the restatements agree with torch's float64 nn.InstanceNorm2d (+ ReLU), conv2d(cat(a, b)) (+ sigmoid) and tests/dice_restate.py.
So a green tests/test_gpu_norm_exact.py means something."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import dice_restate
import norm_exact as NX

f32 = np.float32


def a32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def r32_(a):
    """float64 -> the nearest float32, kept as float64"""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def must_pass(cmps):
    for c in cmps:
        c.assert_ok()
        assert c.skipped == 0


def must_fail(cmps, defect, named):
    bad = [c.line() for c in cmps if not c.ok]
    assert bad, "the defect `%s` passed every comparison" % defect
    assert any(named in b and "first at element [" in b for b in bad), (defect, named, bad[0])


# ----------------------------------------------------------------------------------------------------------------- instance normalisation
def in_geometry(c):
    ve = NX.VE[c.dt]
    nv = c.CP // ve
    slots = 256 // nv
    chunk = max(256, (c.hw + 63) // 64)
    return ve, nv, slots, chunk, (c.hw + chunk - 1) // chunk


def in_owned(c, defect):
    """the pixels a launch visits: all of them, unless a defect loses some"""
    ve, nv, slots, chunk, S = in_geometry(c)
    p = np.arange(c.hw)
    keep = np.ones(c.hw, dtype=bool)
    if defect == "last slot dropped" and 256 % nv:
        keep &= ((p % chunk) % slots) != slots - 1
    if defect == "tail of the last split dropped":
        p0 = (S - 1) * chunk
        keep &= p < p0 + ((c.hw - p0) // slots) * slots
    return keep


def in_rows(v, c):
    out = np.zeros((c.B, c.CP), dtype=np.float32)
    out[:, :c.C] = v
    return torch.from_numpy(out)


def imit_in_stats(c, defect=None):
    x = c.x[:, :, in_owned(c, defect)]
    n = c.hw
    m = x.sum(2) / n
    var = (x * x).sum(2) / n - m * m
    if defect == "unbiased variance" and n > 1:
        var = var * n / (n - 1)
    var = np.maximum(var, 0.0)
    rstd = 1.0 / (np.sqrt(var) + c.eps) if defect == "eps after the square root" else 1.0 / np.sqrt(var + c.eps)
    return in_rows(m, c), in_rows(rstd, c)


def in_xhat_z(c, mean, rstd, defect=None):
    """float32 xhat (one rounding of the double product) and z (one fma) of every element"""
    xh = r32_((c.x - mean[:, :, None]) * rstd[:, :, None])
    if c.gamma is None:
        return xh, xh
    gamma = c.gamma
    if defect == "gamma by the lane":
        gamma = c.gamma[np.arange(c.C) % NX.VE[c.dt]]
    return xh, r32_(xh * gamma[None, :, None] + c.beta[None, :, None])


def in_stored(c, v, defect=None):
    """[B, C, hw] -> the NHWC tensor a launch leaves: zeros in the padding channels, SENTINEL where a defect never wrote"""
    t = NX.nhwc(v, c.CP, c.dt, fill=0.0)
    t[:, ~torch.from_numpy(in_owned(c, defect))] = NX.SENTINEL
    return t


def imit_in_apply(c, mean, rstd, defect=None):
    _, z = in_xhat_z(c, mean, rstd, defect)
    z = NX.rnd(z, c.dt)
    return in_stored(c, np.where(z > 0, z, 0.0) if c.act else z, defect)


def in_g(c, z, defect=None):
    if not c.act:
        return c.dy
    return np.where((z if defect == "mask on the unrounded z" else NX.rnd(z, c.dt)) > 0, c.dy, 0.0)


def imit_in_sums(c, mean, rstd, params, defect=None):
    keep = in_owned(c, defect)
    xh, z = in_xhat_z(c, mean, rstd, defect)
    g = in_g(c, z, defect)
    s1, s2 = g[:, :, keep].sum(2), (g * xh)[:, :, keep].sum(2)
    n = in_geometry(c)[3] if defect == "mg divided by the chunk" else c.hw
    out = [in_rows(s1 / n, c), in_rows(s2 / n, c)]
    if params:
        t1, t2 = (s1[0], s2[0]) if defect == "dgamma from sample 0" else (s1.sum(0), s2.sum(0))
        dgamma, dbeta = (t1, t2) if defect == "dgamma and dbeta swapped" else (t2, t1)
        out += [torch.from_numpy(a32(dgamma)), torch.from_numpy(a32(dbeta))]
    return out


def imit_in_bwd_apply(c, mean, rstd, mg, mgx, defect=None):
    xh, z = in_xhat_z(c, mean, rstd, defect)
    g = in_g(c, z, defect)
    e = lambda v: v[:, :, None]
    a = e(rstd) if c.gamma is None else r32_(c.gamma[None, :, None] * e(rstd))
    inner = r32_(-xh * e(mgx) + r32_(g - e(mg)))
    return in_stored(c, r32_(a * inner), defect)


def in_synthetic(c, defect=None, params=None):
    params = c.affine if params is None else params
    return (c.check_apply(imit_in_apply(c, c.smean, c.srstd, defect)) + c.check_sums(*imit_in_sums(c, c.smean, c.srstd, params, defect))
            + c.check_bwd_apply(imit_in_bwd_apply(c, c.smean, c.srstd, c.smg, c.smgx, defect)))


def in_chain(c, defect=None):
    C = c.C
    mean, rstd = (NX.f64(t)[:, :C] for t in imit_in_stats(c, defect))
    y = imit_in_apply(c, mean, rstd, defect)
    out = imit_in_sums(c, mean, rstd, bool(c.affine), defect)
    dx = imit_in_bwd_apply(c, mean, rstd, NX.f64(out[0])[:, :C], NX.f64(out[1])[:, :C], defect)
    return c.check_chain(y, dx, *out[2:])


@pytest.mark.parametrize("dt", NX.DTYPES)
def test_instnorm_faithful_imitation_passes_every_case(dt):
    for key in NX.in_keys(dt):
        c = NX.in_case(*key)
        assert c.ambiguous == 0
        must_pass(c.check_stats(*imit_in_stats(c)) + in_synthetic(c) + in_chain(c))
        if c.affine:
            must_pass(c.check_sums(*imit_in_sums(c, c.smean, c.srstd, False)))


def test_instnorm_the_planted_elements_split_the_storage_types():
    """z = 2**-30 at the planted elements: float16 stores 0 (no gradient), bfloat16 and float32 keep it (gradient)"""
    for dt, on in (("f32", True), ("bf16", True), ("f16", False)):
        c = NX.in_case(dt, 16, 13, 257, 3, 1, 1, NX.IN_EPS[1], "normal")
        assert c.planted.any() and bool(c.smask[c.planted].all()) == on and bool(c.smask[c.planted].any()) == on, dt


def test_instnorm_constant_planes_are_exact():
    for dt in NX.DTYPES:
        c = NX.in_case(dt, 16, 13, 257, 3, 1, 1, NX.IN_EPS[0], "const")
        for b, ch in ((0, 1), (2, 2)):
            assert c.isconst[b, ch] and c.bmean[b, ch] == 0 and not c.bcy[b, ch].any() and not c.bcdx[b, ch].any()
            assert (c.cy[b, ch] == 0).all() and (c.cdx[b, ch] == 0).all()


def in_find(dt, **want):
    """the first key of in_keys(dt) whose case has the wanted attributes"""
    names = ("dt", "CP", "C", "hw", "B", "affine", "act", "eps", "kind")
    for key in NX.in_keys(dt):
        k = dict(zip(names, key))
        if all(k[n] == v for n, v in want.items()):
            return key
    raise AssertionError((dt, want))


IN_DEFECTS = (     # (defect, dtype and attributes of a case that shows it, which check, the comparison it must fail)
    ("unbiased variance", "bf16", dict(kind="cancel", CP=16), "stats", "stats rstd"),
    ("unbiased variance", "f32", dict(hw=513, CP=48, kind="normal"), "stats", "stats rstd"),
    ("eps after the square root", "f32", dict(eps=1e-3, hw=257), "stats", "stats rstd"),
    ("last slot dropped", "f32", dict(CP=48, hw=255), "stats", "stats mean"),
    ("last slot dropped", "f16", dict(CP=48, hw=257, B=3), "synthetic", "apply y"),
    ("tail of the last split dropped", "f32", dict(CP=16, hw=257, B=3), "synthetic", "bwd_apply dx"),
    ("tail of the last split dropped", "bf16", dict(CP=16, hw=257), "stats", "stats mean"),
    ("mg divided by the chunk", "f32", dict(CP=48, hw=255), "synthetic", "bwd_sums mg"),
    ("dgamma and dbeta swapped", "f32", dict(CP=16, hw=257, B=3, affine=1), "synthetic", "bwd_sums dgamma"),
    ("dgamma from sample 0", "bf16", dict(CP=48, hw=257, B=3, affine=1), "synthetic", "bwd_sums dbeta"),
    ("mask on the unrounded z", "f16", dict(CP=16, hw=257, B=3, affine=1, act=1), "synthetic", "bwd_apply dx"),
    ("mask on the unrounded z", "f16", dict(CP=16, hw=257, B=3, affine=0, act=1), "synthetic", "bwd_sums mg"),
    ("gamma by the lane", "f32", dict(CP=16, hw=257, B=3, affine=1, act=0), "synthetic", "apply y"),
    ("gamma by the lane", "f16", dict(CP=48, hw=257, B=3, affine=1, act=1), "chain", "chain y"),
)


@pytest.mark.parametrize("defect,dt,want,which,named", IN_DEFECTS)
def test_instnorm_defects_fail(defect, dt, want, which, named):
    c = NX.in_case(*in_find(dt, **want))
    cmps = {"stats": lambda: c.check_stats(*imit_in_stats(c, defect)), "synthetic": lambda: in_synthetic(c, defect), "chain": lambda: in_chain(c, defect)}[which]()
    must_fail(cmps, defect, named)


def test_instnorm_split_rule():
    want = {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 513: 3, 16384: 64, 16385: 64, 16448: 64, 16449: 64}
    assert {hw: NX.in_splits(hw) for hw in NX.IN_SPLIT_SIZES} == want
    assert NX.in_chunk(16384) == 256 and NX.in_chunk(16385) == 257 and NX.in_chunk(16448) == 257 and NX.in_chunk(16449) == 258
    assert NX.in_scratch_doubles(3, 513, 48) == 3 * 3 * 2 * 48


def t64(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).requires_grad_(grad)


def close(got, ref, tol=1e-9, floor=1e-300):
    """two float64 evaluations of one formula: within tol of the largest |value| (of `floor` where everything cancels to nothing)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.all(np.abs(got - ref) <= tol * max(np.abs(ref).max(), floor)), float(np.abs(got - ref).max())


@pytest.mark.parametrize("dt", NX.DTYPES)
def test_instnorm_restatement_is_torchs(dt):
    """the chained reference against nn.InstanceNorm2d (+ nn.ReLU) in float64, on every case with more than one pixel per plane (torch
    refuses one); the cancellation plane's variance costs torch the digits it costs any one-pass formula, hence the looser figure there"""
    for key in NX.in_keys(dt):
        c = NX.in_case(*key)
        if c.hw == 1:
            continue
        m = nn.InstanceNorm2d(c.C, eps=c.eps, affine=bool(c.affine)).double()
        if c.affine:
            with torch.no_grad():
                m.weight.copy_(t64(c.gamma)), m.bias.copy_(t64(c.beta))
        x = t64(c.x.reshape(c.B, c.C, c.hw, 1), True)
        y = m(x)
        y = torch.relu(y) if c.act else y
        y.backward(t64(c.dy.reshape(y.shape)))
        tol = 1e-6 if c.kind != "normal" else 1e-9
        close(c.cy, y.detach().numpy()[..., 0], tol, 1.0), close(c.cdx, x.grad.numpy()[..., 0], tol, 1.0)
        if c.affine:
            close(c.cdgamma, m.weight.grad.numpy(), tol, 1.0), close(c.cdbeta, m.bias.grad.numpy(), tol, 1.0)


# ----------------------------------------------------------------------------------------------------------------- Dice
def dice_partials(terms, P):
    """[..., n, 3] float32 terms -> [..., P, 3] doubles: element i goes to partial (i / 256) % P"""
    n = terms.shape[-2]
    own = (np.arange(n) // 256) % P
    out = np.zeros(terms.shape[:-2] + (P, 3))
    for j in range(P):
        out[..., j, :] = terms[..., own == j, :].astype(np.float64).sum(-2)
    return out


def pow32(v, pw):
    v = a32(v)
    return v if pw == 1.0 else (v * v if pw == 2.0 else np.power(v, f32(pw)))


def powm1_32(v, pw):
    v = a32(v)
    return np.ones_like(v) if pw == 1.0 else (v if pw == 2.0 else np.power(v, f32(pw - 1.0)))


def imit_dice_sums(c, off=(0, 0), defect=None):
    p, t = a32(c.p), a32(c.t)
    terms = np.stack([p * t, pow32(p, c.pw), pow32(t, c.pw)], -1)
    if defect == "sums swapped":
        terms = terms[..., [0, 2, 1]]
    if defect == "scalar head skipped" and off[0] == off[1] and off[0] % 4:
        terms[0, :min(c.per, 4 - off[0] % 4)] = 0        # (sample 0: the later samples start wherever per puts them)
    return dice_partials(terms, NX.dice_nparts(c.per))


def imit_dice_finalize(partials, B, C, smooth, reduction, ignore_index=-1, weight=None, defect=None):
    q = np.asarray(partials, dtype=np.float64).reshape(B * C, -1, 3)
    num = q[:, :, 0].sum(1) + smooth
    den = (q[:, :, 1].sum(1) + q[:, :, 2].sum(1)) + smooth * (2 if defect == "smooth twice" else 1)
    div = C - 1 if defect == "ignored class divides by C - 1" and 0 <= ignore_index < C else C
    w = np.array([0.0 if c == ignore_index else (1.0 if weight is None else float(weight[c])) for c in range(C)]) / div
    l = (np.tile(w, B) * (1.0 - num / den)).reshape(B, C).sum(1)
    if reduction != "none":
        l = np.array([l.sum() / (B if reduction == "mean" and defect != "mean without 1/B" else 1)])
    return np.stack([num, den], 1), a32(l)


def up32(B, reduction, gscale=1.0, gdev=None, gout=None):
    return NX.upstream(B, reduction, gscale, gdev, gout)


def imit_dice_bwd(c, reduction="mean", gscale=1.0, gdev=None, gout=None, chain=False, accumulate=False, defect=None):
    g = up32(c.B, reduction, gscale, gdev, gout)[:, None]
    num, den = c.coef[:, :1], c.coef[:, 1:]
    kt, kp = a32(g / den), a32(g * num * c.pw / (den * den))
    x, y = a32(c.p), a32(c.t)
    v = kp * powm1_32(x, c.pw) - kt * y
    if chain and defect != "chain omitted":
        v = v * (x * (f32(1) - x))
    return a32(c.old) + v if accumulate and defect != "accumulate overwrites" else v


def softmax32(z):
    z = a32(z)
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    d = np.zeros_like(m)
    for k in range(z.shape[1]):
        d = d + e[:, k:k + 1]
    return e * (f32(1) / d)


def strided_index(HW, defect):
    """the pixels the strided path touches, thread by thread: pix0 + 256 k, k < 4 (the defect: pix0 + k)"""
    tiles = (HW + 1023) // 1024
    t, k, tile = np.meshgrid(np.arange(256), np.arange(4), np.arange(tiles), indexing="ij")
    idx = tile * 1024 + t + (k if defect == "strided by k" else 256 * k)
    return idx[idx < HW].reshape(-1)


def imit_soft_sums(c, defect=None):
    s, t = softmax32(c.z), a32(c.t)
    terms = np.stack([s * t, pow32(s, c.pw), pow32(t, c.pw)], -1)
    if c.HW % 4 and defect == "strided by k":
        terms = terms[:, :, strided_index(c.HW, defect)]
        return terms.astype(np.float64).sum(2)[:, :, None, :] * np.eye(1, NX.dice_nparts(c.HW))[0][None, None, :, None]
    return dice_partials(terms, NX.dice_nparts(c.HW))


def imit_soft_bwd(c, reduction="mean", ignore_index=-1, weighted=False, gscale=1.0, gdev=None, gout=None, accumulate=False, defect=None):
    B, C = c.B, c.C
    w = np.array([0.0 if k == ignore_index else (float(c.weight[k]) if weighted else 1.0) for k in range(C)]) / C
    g = up32(B, reduction, gscale, gdev, gout)[:, None] * w[None, :]
    num, den = c.coef[:, 0].reshape(B, C), c.coef[:, 1].reshape(B, C)
    kt, kp = a32(g / den)[..., None], a32(g * num * c.pw / (den * den))[..., None]
    s, y = softmax32(c.z), a32(c.t)
    gc = kp * powm1_32(s, c.pw) - kt * y
    dot = np.zeros((B, 1, c.HW), dtype=np.float32)
    for k in range(C):
        dot = dot + gc[:, k:k + 1] * s[:, k:k + 1]
    dz = s * (gc - dot)
    out = a32(c.old) + dz if accumulate and defect != "accumulate overwrites" else dz
    if c.HW % 4 and defect == "strided by k":
        keep = np.zeros(c.HW, dtype=bool)
        keep[strided_index(c.HW, defect)] = True
        out = np.where(keep, out, f32(NX.SENTINEL))
    return out


def test_dice_binary_faithful_imitation_passes_every_case():
    for key in NX.DICE_BIN_KEYS:
        c = NX.dice_bin_case(*key)
        part = imit_dice_sums(c)
        cm = c.check_sums(part)
        for red in NX.REDUCTIONS:
            cm += NX.check_finalize(c.label, *imit_dice_finalize(part, c.B, 1, NX.SMOOTH, red), part, c.B, 1, NX.SMOOTH, red)
        for mode in NX.BIN_GRAD_MODES:
            m = NX.resolve_mode(mode, c.B)
            cm += c.check_grad(imit_dice_bwd(c, **m), **m)
        must_pass(cm)


def test_dice_softmax_faithful_imitation_passes_every_case():
    for key in NX.dice_soft_keys():
        c = NX.dice_soft_case(*key)
        part = imit_soft_sums(c)
        cm = c.check_sums(part)
        for red, ig, wt in (("mean", -1, None), ("sum", 0, c.weight), ("none", c.C - 1, None)):
            cm += NX.check_finalize(c.label, *imit_dice_finalize(part, c.B, c.C, NX.SMOOTH, red, ig, wt), part, c.B, c.C, NX.SMOOTH, red, ig, wt)
        for mode in NX.SOFT_GRAD_MODES:
            m = NX.resolve_mode(mode, c.B, c.C)
            cm += c.check_grad(imit_soft_bwd(c, **m), **m)
        must_pass(cm)


def test_dice_dominated_logits():
    """a margin of 80 leaves the other classes a tiny NORMAL float32 probability; 120 leaves exactly 0 in float32"""
    c = NX.dice_soft_case(2, 5, 1029, 2.0, True, False)
    s = softmax32(c.z)
    assert (s[:, 1:, 0::3] > 0).all() and (s[:, 1:, 0::3] < 1e-30).all() and (s[:, 1:, 1::3] == 0).all() and (c.s[:, 1:, 1::3] > 0).all()


def test_dice_defects_fail():
    c = NX.dice_bin_case(1027, 5, 3.0)
    part = imit_dice_sums(c)
    must_fail(c.check_sums(imit_dice_sums(c, defect="sums swapped")), "sums swapped", "sums per unit")
    must_fail(c.check_sums(imit_dice_sums(c, (1, 1), "scalar head skipped")), "scalar head skipped", "sums per unit")
    for defect, red in (("smooth twice", "sum"), ("mean without 1/B", "mean")):
        must_fail(NX.check_finalize(c.label, *imit_dice_finalize(part, c.B, 1, NX.SMOOTH, red, defect=defect), part, c.B, 1, NX.SMOOTH, red), defect,
                  "finalize %s %s" % (red, "coef" if defect == "smooth twice" else "loss"))
    m = NX.resolve_mode(NX.BIN_GRAD_MODES[5], c.B)
    must_fail(c.check_grad(imit_dice_bwd(c, defect="accumulate overwrites", **m), **m), "accumulate overwrites", "bwd")
    must_fail(c.check_grad(imit_dice_bwd(c, defect="chain omitted", **m), **m), "chain omitted", "bwd")
    s = NX.dice_soft_case(2, 5, 1029, 2.0, True, False)
    part = imit_soft_sums(s)
    ig = s.C - 1
    must_fail(NX.check_finalize(s.label, *imit_dice_finalize(part, s.B, s.C, NX.SMOOTH, "mean", ig, defect="ignored class divides by C - 1"), part, s.B, s.C,
                                NX.SMOOTH, "mean", ig), "ignored class divides by C - 1", "finalize mean loss")
    must_fail(s.check_sums(imit_soft_sums(s, "strided by k")), "strided by k", "sums per unit")
    must_fail(s.check_grad(imit_soft_bwd(s, defect="strided by k")), "strided by k", "bwd")
    m = NX.resolve_mode(NX.SOFT_GRAD_MODES[5], s.B, s.C)
    must_fail(s.check_grad(imit_soft_bwd(s, defect="accumulate overwrites", **m), **m), "accumulate overwrites", "bwd")


def test_dice_restatement_is_dice_restate():
    for key in NX.DICE_BIN_KEYS:
        c = NX.dice_bin_case(*key)
        p, t = t64(c.p), t64(c.t)
        for red in NX.REDUCTIONS:
            want = dice_restate.binary_dice(p, t, NX.SMOOTH, c.pw, red)
            _, _, loss, _ = NX.finalize_ref(np.stack([c.S], 1), c.B, 1, NX.SMOOTH, red)
            close(loss, want.numpy().reshape(-1))
            gr = dice_restate.grad_of(lambda v: dice_restate.binary_dice(v, t, NX.SMOOTH, c.pw, red), p)
            close(c.grad_ref(reduction=red)[0], gr.numpy())
            close(c.grad_ref(reduction=red, chain=True)[0], dice_restate.chain_sigmoid(gr, p).numpy())
    for key in NX.dice_soft_keys():
        c = NX.dice_soft_case(*key)
        z, t = t64(c.z), t64(c.t)
        for red, ig, wt in (("mean", None, None), ("sum", 0, c.weight), ("none", c.C - 1, c.weight)):
            fn = lambda v: dice_restate.dice(v, t, None if wt is None else t64(wt), ig, NX.SMOOTH, c.pw, red)
            want = fn(z)
            if not torch.is_tensor(want):                  # (every class ignored: C = 1 with ignore_index 0 -- the loop adds nothing)
                continue
            _, _, loss, _ = NX.finalize_ref(c.S.reshape(c.B * c.C, 1, 3), c.B, c.C, NX.SMOOTH, red, -1 if ig is None else ig, wt)
            close(loss, want.numpy().reshape(-1))
            close(c.grad_ref(reduction=red, ignore_index=-1 if ig is None else ig, weighted=wt is not None)[0], dice_restate.grad_of(fn, z).numpy(), 1e-8)


def test_dice_nparts_rule():
    assert [NX.dice_nparts(n) for n in (1, 4096, 4097, 64 * 4096, 64 * 4096 + 5)] == [1, 1, 2, 64, 64]
    assert NX.SOFT_HW[-1] == 2055 and NX.dice_nparts(2055) == 1


# ----------------------------------------------------------------------------------------------------------------- two-source mask head
def imit_head_fwd(c, defect=None):
    a, b, w = a32(c.a), a32(c.b), a32(c.w)
    wa, wb = w[:, :c.na], (w[:, :c.nb] if defect == "b's columns from 0" else w[:, c.na:])
    with np.errstate(all="ignore"):
        v = a @ wa.T + b @ wb.T
        if defect == "padding channel enters" and c.lda > c.na:
            v = v + f32(NX.PAD_FILL[c.dt]) * w[:, :1].T
        if c.bias is not None:
            v = v + a32(c.bias)
        if c.act:
            v = f32(1) / (f32(1) + np.exp(-v))
    out = v.reshape(c.B, c.hw, c.Cout).transpose(0, 2, 1).copy()
    if defect == "last partial group dropped":
        full = (c.npix // (4 * c.PPB)) * 4 * c.PPB
        flat = out.transpose(0, 2, 1).reshape(c.npix, c.Cout)
        flat[full:] = NX.SENTINEL
        out = flat.reshape(c.B, c.hw, c.Cout).transpose(0, 2, 1)
    return out


def imit_head_bwd(c, defect=None):
    """-> (ga, gb as the NHWC tensors, partials [nparts, Cout (nab + 1)] doubles): a lane adds its pixels in float32, the rest in double"""
    gz = a32(c.gout).transpose(0, 2, 1).reshape(c.npix, c.Cout)
    gz_db = gz
    if c.chain:
        s = a32(c.saved).transpose(0, 2, 1).reshape(c.npix, c.Cout)
        gz = gz * (s * (f32(1) - s))
        gz_db = gz_db if defect == "db without the sigmoid derivative" else gz
    w = a32(c.w)
    ga = NX.nhwc((gz @ w[:, :c.na]).astype(np.float64).T[None], c.lda, c.dt, fill=0.0)[0]
    gb = NX.nhwc((gz @ w[:, c.na:]).astype(np.float64).T[None], c.ldb, c.dt, fill=0.0)[0]
    x = np.concatenate([a32(c.a), a32(c.b)], 1)
    lanes = c.nparts * c.PPB
    T = -(-c.npix // lanes)
    pad = T * lanes - c.npix
    prod = np.concatenate([gz[:, :, None] * x[:, None, :], gz_db[:, :, None]], 2)                  # [npix, Cout, nab + 1]
    prod = np.concatenate([prod, np.zeros((pad,) + prod.shape[1:], dtype=np.float32)]).reshape(T, lanes, c.Cout, -1)
    acc = np.zeros(prod.shape[1:], dtype=np.float32)
    for k in range(T):
        acc = acc + prod[k]
    tot = acc.astype(np.float64).reshape(c.nparts, c.PPB, c.Cout, -1).sum(1)                        # [nparts, Cout, nab + 1]
    part = np.concatenate([tot[:, :, :-1].reshape(c.nparts, -1), tot[:, :, -1]], 1)
    return ga, gb, part


def head_all(c, defect=None):
    ga, gb, part = imit_head_bwd(c, defect)
    tot = part.sum(0)
    n = c.Cout * (c.na + c.nb)
    dw, db = tot[:n].reshape(c.Cout, -1), tot[n:]
    return (c.check_fwd(imit_head_fwd(c, defect)) + c.check_bwd(ga, gb) + c.check_partials(part) + c.check_params(a32(dw), a32(db))
            + c.check_params(a32(dw + c.old_w), a32(db + c.old_b), accumulate=True))


@pytest.mark.parametrize("dt", NX.DTYPES)
def test_head_faithful_imitation_passes_every_case(dt):
    for key in NX.head_keys(dt):
        must_pass(head_all(NX.head_case(*key)))
    if dt == "f32":
        c = NX.head_case(*NX.head_big_key())
        assert c.npix > NX.head_fwd_grid(c.npix, c.G) * c.PPB * NX.HEAD_FWD_UNROLL and c.G == 16
        must_pass(c.check_fwd(imit_head_fwd(c)))


def test_head_covers_what_the_issue_lists():
    for dt in NX.DTYPES:
        keys = NX.head_keys(dt)
        assert {k[5] for k in keys} == {1, 2, 3, 4} and {NX.head_G(k[1], k[3], dt) for k in keys} >= {16, 16 // (NX.VE[dt] // 4) // 4}
        assert {k[8] for k in keys} == {0, 1} and {k[9] for k in keys} == {0, 1} and {NX.head_case(*k).chain for k in keys} == {False, True}
    assert NX.head_G(64, 16, "f32") == 16 and NX.head_G(128, 16, "bf16") == 16 and NX.head_G(272, 16, "bf16") == 0 and NX.head_G(16, 16, "f16") == 2
    assert [NX.head_nparts(n) for n in (1, 128, 129, 1024 * 128 + 1)] == [1, 1, 2, 1024]


def test_head_defects_fail():
    dt = "f32"
    keys = NX.head_keys(dt)
    c = NX.head_case(*next(k for k in keys if k[1] > k[2] and (k[6] * k[7]) % (4 * 256 // NX.head_G(k[1], k[3], dt))))
    must_fail(head_all(c, "padding channel enters"), "padding channel enters", " out")
    must_fail(head_all(c, "b's columns from 0"), "b's columns from 0", " out")
    must_fail(head_all(c, "last partial group dropped"), "last partial group dropped", " out")
    c = NX.head_case(*next(k for k in keys if NX.head_case(*k).chain and k[6] * k[7] > 1))
    must_fail(head_all(c, "db without the sigmoid derivative"), "db without the sigmoid derivative", "partials db")


def test_head_restatement_is_torchs():
    for dt in NX.DTYPES:
        for key in NX.head_keys(dt):
            c = NX.head_case(*key)
            a = t64(c.a.reshape(c.B, c.hw, 1, c.na).transpose(0, 3, 1, 2), True)
            b = t64(c.b.reshape(c.B, c.hw, 1, c.nb).transpose(0, 3, 1, 2), True)
            w = t64(c.w.reshape(c.Cout, c.na + c.nb, 1, 1), True)
            bias = t64(c.bias, True) if c.has_bias else None
            v = F.conv2d(torch.cat((a, b), 1), w, bias)
            out = torch.sigmoid(v) if c.act else v
            close(c.out, out.detach().numpy()[..., 0])
            if c.chain and not np.array_equal(c.saved, c.out):
                continue                                   # (the saved output is an input of its own: float32 of out, not out)
            (out if c.chain else v).backward(t64(c.gout.reshape(out.shape)))
            close(c.ga, a.grad.numpy()[..., 0].transpose(0, 2, 1).reshape(c.npix, c.na)), close(c.gb, b.grad.numpy()[..., 0].transpose(0, 2, 1).reshape(c.npix, c.nb))
            close(c.dw, w.grad.numpy().reshape(c.dw.shape))
            if bias is not None:
                close(c.db, bias.grad.numpy())
