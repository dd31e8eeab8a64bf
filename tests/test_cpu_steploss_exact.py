"""The per-element comparisons of tests/steploss_exact.py without a GPU: a float32 imitation of every kernel of csrc/losses.hip,
csrc/localise.hip and the loss half of csrc/optim.hip (numpy float32 operations, its own summation order) passes every case key the GPU
tests run; each planted defect FAILS, and the failure names the kernel, the case key and the element; and every reference agrees with the
torch module it restates, evaluated in float64.  So a green tests/test_gpu_steploss_exact.py means something."""
import numpy as np
import pytest
import torch
from torch import nn

import steploss_exact as SX

f32 = np.float32


def a32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def must_pass(cmps):
    for c in cmps:
        c.assert_ok()
        assert c.skipped == 0


def must_fail(cmps, defect, kernel):
    bad = [c for c in cmps if not c.ok]
    assert bad, "the defect `%s` passed every comparison of %s" % (defect, kernel)
    line = bad[0].line()
    assert kernel in line and "first at element [" in line, line
    return line


def sum32(terms, nparts, defect=None):
    """float32 partials [nparts] as a grid of nparts workgroups of 256 threads forms them: a thread adds its elements in turn, a wave folds
    in six halvings, the four wave totals are added in turn"""
    t = a32(terms).reshape(-1)
    stride = nparts * 256
    trips = -(-t.size // stride)
    if defect == "tail dropped" and trips > 1:
        trips -= 1
    buf = np.zeros(max(trips, 1) * stride, dtype=f32)
    m = min(t.size, buf.size)
    buf[:m] = t[:m]
    acc = np.zeros(stride, dtype=f32)
    with np.errstate(all="ignore"):
        for r in range(trips):
            acc = acc + buf[r * stride:(r + 1) * stride]
        acc = acc.reshape(nparts, 4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc[..., :o] + acc[..., o:2 * o]
        acc = acc[..., 0]
        return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]


def fin64(partials, defect=None):
    p = np.asarray(partials, dtype=np.float64)
    return p[:-1].sum() if defect == "last partial dropped" and p.size > 1 else p.sum()


def written(vals, n, nparts, defect):
    """an elementwise output: with `tail dropped` only the first trip of the grid is written, the rest keeps SENTINEL"""
    out = a32(vals).copy()
    if defect == "tail dropped" and n > nparts * 256:
        out[nparts * 256:] = SX.SENTINEL
    return out


# ----------------------------------------------------------------------------------------------------------------- imitations
def imit_smooth_l1(c, nparts, defect=None):
    a, b, beta, n = a32(c.a), a32(c.b), f32(c.beta), c.n
    d = a - b
    ad = np.abs(d)
    lim = np.nextafter(beta, f32(np.inf)) if defect == "seam one step late" else beta
    quad = (ad <= lim) if defect in ("<= at beta", "seam one step late") else (ad < lim)
    t = np.where(quad, f32(0.5) * d * d / beta, ad - f32(0.5) * beta)
    inv = f32(1) / f32(n)
    g = np.where(quad, d / beta, np.where(d > 0, f32(1), f32(-1))) * (f32(1) if defect == "grad without 1/n" else inv)
    loss = f32(fin64(sum32(t, nparts, defect), defect) * (1.0 / n))
    return loss, written(g, n, nparts, defect)


def imit_bce_prob(c, nparts, defect=None):
    p, t, n = a32(c.p), f32(c.target), c.n
    lo = f32(-np.inf) if defect == "no -100 clamp" else f32(-100)
    with np.errstate(all="ignore"):
        term = -(t * np.maximum(np.log(p), lo) + (f32(1) - t) * np.maximum(np.log(f32(1) - p), lo))
        g = (p - t) / np.maximum((f32(1) - p) * p, f32(0) if defect == "no 1e-12 clamp" else f32(1e-12)) * (f32(1) / f32(n))
        loss = f32(fin64(sum32(term, nparts, defect), defect) * (1.0 / n))
    return loss, written(g, n, nparts, defect)


def imit_cross_entropy(c, defect=None):
    B, K, ld = c.B, c.K, c.ld
    z = a32(c.z)
    m = z.max(1, keepdims=True)
    se = np.zeros((B, 1), dtype=f32)
    for k in range(K):
        se = se + np.exp(z[:, k:k + 1] - m)
    lse = m + np.log(se)
    rows = np.arange(B)
    loss = f32((lse[:, 0] - z[rows, c.y]).astype(np.float64).sum() / (B * K if defect == "mean over B*K" else B))
    hot = np.zeros((B, K), dtype=f32)
    hot[rows, c.y] = 1
    grad = np.full((B, ld), SX.SENTINEL, dtype=f32)
    grad[:, :K] = (np.exp(z - lse) - hot) * (f32(1) / f32(B))
    if defect == "writes column K" and ld > K:
        grad[:, K] = 0
    return loss, grad


def imit_clamp01(c, defect=None):
    x, g = a32(c.x), a32(c.g)
    with np.errstate(invalid="ignore"):
        y = np.fmin(np.fmax(x, f32(0)), f32(1)) if defect == "nan clamped to 0" else np.where(np.isnan(x), x, np.minimum(np.maximum(x, f32(0)), f32(1)))
        gate = (x > 0) & (x <= 1) if defect == "x > 0" else (x >= 0) & (x <= 1)
    return y, np.where(gate, g, f32(0))


def trunc(v, defect):
    return np.rint(v) if defect == "rounding for truncation" else np.trunc(v)


def imit_psnr255(c, nparts, defect=None):
    a, b = a32(c.a), a32(c.b)
    ia = trunc(np.minimum(np.maximum(a * f32(255), f32(0)), f32(255)), defect)
    ib = trunc(np.minimum(np.maximum(b * f32(255), f32(0)), f32(255)), defect)
    d2 = (ia - ib).astype(np.float64) ** 2
    owner = (np.arange(c.n) // 256) % nparts
    if defect == "tail dropped":
        d2 = np.where(np.arange(c.n) < nparts * 256, d2, 0.0)
    return np.bincount(owner, weights=d2, minlength=nparts)


def imit_psnr_gate(partials, n, thr, defect=None):
    mse = f32(fin64(partials, defect) / n)
    if mse == 0:
        psnr = f32(0)
    else:
        base = np.log(f32(10))
        psnr = f32(20) * np.log(f32(255)) / base - f32(10) * np.log(mse) / base
    below = psnr <= f32(thr) if defect == "<= at the gate" else psnr < f32(thr)
    return np.array([psnr, f32(SX.GATE_W[0]) if below else f32(SX.GATE_W[1])], dtype=f32)


def plane_mask(c, defect):
    B, C, HW = c.B, c.C, c.HW
    plane = np.arange(B * C)
    idx = plane % B if defect == "mask indexed by plane" else plane // C
    return a32(c.mask)[idx].reshape(-1)


def imit_splice(c, defect=None):
    enc, real, prev = a32(c.enc), a32(c.real), a32(c.prev)
    cl = np.minimum(np.maximum(enc, f32(0)), f32(1))
    r = np.floor(cl * f32(255) + f32(0.5)) if defect == "round half away" else np.rint(cl * f32(255))
    q = r / f32(255)
    m = plane_mask(c, defect)
    tam = q * (f32(1) - m) + prev * m
    d = trunc(real * f32(255), defect) - trunc(q * f32(255), defect)
    nparts = min(max(-(-enc.size // 256), 1), 1024)
    part = np.bincount((np.arange(enc.size) // 256) % nparts, weights=(d * d).astype(np.float64), minlength=nparts)
    return q, tam, part


def imit_masked_axpy(c, defect=None):
    return a32(c.a) + a32(c.g) * (f32(1) - plane_mask(c, defect))


def imit_mse(c, nparts, defect=None):
    d = a32(c.a) - a32(c.b)
    G = f32(c.gscale)
    if c.gate is not None:
        G = G * f32(c.gate)
    if c.gdev is not None and defect != "gscale_dev ignored":
        G = G * f32(c.gdev)
    return sum32(d * d, nparts, defect), written(G * d, c.n, nparts, defect)


def imit_image_grad(c, nparts, defect=None):
    d = a32(c.a) - a32(c.b)
    G = f32(c.gscale) * f32(c.gdev) if c.gdev is not None else f32(c.gscale)
    g = c.g().float().numpy()
    c0 = 0 if defect == "c0 ignored" else c.c0
    out = g[:, :, c0:c0 + c.C].transpose(0, 2, 1) + G * d
    return out, sum32((d * d).transpose(0, 2, 1), nparts)


def imit_bce_logits(c, nparts, defect=None):
    x, t, n = a32(c.x), a32(c.t), c.n
    G = f32(c.gscale) * f32(c.gdev) if c.gdev is not None else f32(c.gscale)
    with np.errstate(all="ignore"):
        term = np.maximum(x, f32(0)) - x * t + np.log1p(np.exp(-np.abs(x)))
        s = f32(1) / (f32(1) + np.exp(-x))
        if defect == "target ignored in grad":
            t = np.zeros_like(t)
        if c.tensor_target:
            inv = f32(1) / f32(n)
            loss = f32(fin64(sum32(term, nparts, defect) * inv, defect))
            if defect == "1/n twice":
                loss = loss * inv
            g = (s - t) * G * inv
            if c.chain and defect != "chain factor omitted":
                g = g * x * (f32(1) - x)
        else:
            loss = sum32(term, 1, defect)[0] / f32(n)
            g = (s - t) * G / f32(n)
    return loss, written(g, n, nparts, defect)


def imit_message_loss(c, defect=None):
    d, m, n = a32(c.d), a32(c.m), c.n
    G = f32(c.gscale) * f32(c.gdev) if c.gdev is not None else f32(c.gscale)
    df = d - m
    r = np.where(d >= 0, np.floor(d + f32(0.5)), np.ceil(d - f32(0.5))) if defect == "round half away" else np.rint(d)
    bits = np.abs(np.minimum(np.maximum(r, f32(0)), f32(1)) - m)
    out = np.array([sum32(df * df, 1)[0] / f32(n), sum32(bits, 1)[0] / f32(n)], dtype=f32)
    return out, df * (f32(1) if defect == "gscale ignored" else G)


def imit_hidden_metrics(c, defect=None):
    enc = f32(fin64(c.partials, defect) / c.n_img)
    w = [f32(v) for v in c.w]
    msg2, adv = a32(c.msg2), a32(c.adv)
    total = w[0] * adv[0] + w[1] * enc + w[2] * msg2[0]
    return np.array([total, enc, msg2[0], msg2[0] if defect == "bit error slot" else msg2[1], adv[0], a32(c.d_cover)[0], a32(c.d_enc)[0]], dtype=f32)


def imit_nonfinite(c, nparts, defect=None):
    x = a32(c.x)
    owner = (np.arange(c.n) // 256) % nparts
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(x * x) if defect == "from the sum of squares" else ~np.isfinite(x)
    return (np.bincount(owner, weights=bad.astype(np.float64), minlength=nparts) > 0).astype(f32)


# ----------------------------------------------------------------------------------------------------------------- faithful imitations pass
def nparts_of(n):
    return [SX.wrapper_nparts(n)] + (list(SX.FREE_NPARTS) if n == 4097 else [])


def test_smooth_l1_imitation_passes():
    for key in SX.SMOOTH_L1_KEYS:
        c = SX.smooth_l1_case(*key)
        for npt in nparts_of(c.n):
            must_pass(c.check(*imit_smooth_l1(c, npt), nparts=npt))


def test_bce_prob_imitation_passes():
    for key in SX.BCE_PROB_KEYS:
        c = SX.bce_prob_case(*key)
        for npt in nparts_of(c.n):
            must_pass(c.check(*imit_bce_prob(c, npt), nparts=npt))


def test_cross_entropy_imitation_passes():
    for B, K in SX.CE_KEYS:
        for ld in (K, K + SX.CE_PAD):
            c = SX.cross_entropy_case(B, K, ld)
            must_pass(c.check(*imit_cross_entropy(c)))


def test_clamp01_imitation_passes():
    for key in SX.CLAMP_KEYS:
        c = SX.clamp01_case(*key)
        y, gx = imit_clamp01(c)
        must_pass(c.check_fwd(y) + c.check_bwd(gx))


def test_psnr255_and_gate_imitation_passes():
    for n in SX.FLAT_N:
        c = SX.psnr255_case(n)
        for npt in nparts_of(n):
            part = imit_psnr255(c, npt)
            must_pass(c.check(part))
            must_pass(SX.check_psnr(c.label, imit_psnr_gate(part, n, 33.0)[:1], c.total, n))
    for npt in SX.GATE_NPARTS:
        for zero in (False, True):
            c = SX.PsnrGateCase(npt, zero)
            o = imit_psnr_gate(c.partials, c.n, 33.0)
            must_pass(c.check(o, 33.0))
            for thr in SX.around(o[0]):
                must_pass(c.check(imit_psnr_gate(c.partials, c.n, thr), thr))


def test_plane_kernels_imitation_passes():
    for key in SX.PLANE_KEYS + (SX.SPLICE_CAP_KEY,):
        c = SX.splice_case(*key)
        must_pass(c.check("all", *imit_splice(c)))
    for key in SX.PLANE_KEYS + ((1, 1, SX.CAP_ELEM + 3, "pattern"),):
        c = SX.MaskedAxpyCase(*key)
        must_pass(c.check(imit_masked_axpy(c)))
    for key in SX.image_grad_keys():
        c = SX.ImageGradMseCase(*key)
        must_pass(c.check(*imit_image_grad(c, SX.wrapper_nparts(c.a.size))))
    c = SX.ImageGradMseCase(3, 3, 771, "bf16", 32, 5, gdev=1.5)
    for npt in (SX.wrapper_nparts(c.a.size),) + SX.FREE_NPARTS:
        must_pass(c.check(*imit_image_grad(c, npt)))


def test_flat_glue_imitation_passes():
    for n, data in SX.ELEM_KEYS:
        c = SX.AxpyCase(n, data)
        must_pass(c.check(a32(c.a) + f32(c.s) * a32(c.b)))
        for s in (1.0, 0.3):
            c = SX.ScaleDevCase(n, data, s)
            must_pass(c.check(a32(c.x) * f32(c.s)))
        for thr in (0.5, 0.3):
            c = SX.MaskThresholdCase(n, data, thr)
            with np.errstate(invalid="ignore"):
                must_pass(c.check((a32(c.p) > f32(c.thr)).astype(np.uint8)))


def test_mse_sumsq_nonfinite_imitation_passes():
    for n in SX.FLAT_N:
        for gate, gdev in ((None, None), (None, 1.5), (0.8, None), (0.8, 1.5)):
            c = SX.mse_case(n, 0.7, gdev, gate)
            for npt in nparts_of(n):
                must_pass(c.check(*imit_mse(c, npt), nparts=npt))
        c = SX.SumsqCase(n)
        for npt in nparts_of(n):
            must_pass(c.check(sum32(a32(c.x) * a32(c.x), npt)))
    c = SX.mse_case(SX.MSE_LARGE, 0.7, None, None, "pattern")
    must_pass(c.check(*imit_mse(c, 1024), nparts=1024))
    for key in SX.NONFINITE_KEYS:
        c = SX.NonfiniteCase(*key)
        for npt in nparts_of(c.n):
            must_pass(c.check(imit_nonfinite(c, npt)))


def test_bce_logits_imitation_passes():
    for key in SX.BCE_LOGITS_KEYS:
        c = SX.bce_logits_case(*key)
        must_pass(c.check(*imit_bce_logits(c, 1), nparts=1))
    for key in SX.BCE_TARGET_KEYS:
        c = SX.bce_logits_case(*key)
        for npt in nparts_of(c.n):
            must_pass(c.check(*imit_bce_logits(c, npt), nparts=npt))


def test_message_loss_and_hidden_metrics_imitation_passes():
    for key in SX.MESSAGE_KEYS:
        c = SX.message_loss_case(*key)
        must_pass(c.check(*imit_message_loss(c)))
    for npt in SX.GATE_NPARTS:
        c = SX.HiddenMetricsCase(npt)
        must_pass(c.check(imit_hidden_metrics(c)))


# ----------------------------------------------------------------------------------------------------------------- planted defects fail
def test_smooth_l1_defects_fail():
    for beta in (1.0, 0.25):
        c = SX.smooth_l1_case(8, beta, True)
        # at |d| == beta the two branches agree in value AND gradient (0.5 beta; +-1/n): `<=` for `<` there changes no number, so the
        # comparison cannot and need not fail; one float32 step later it does: the linear branch's gradient is exact
        must_pass(c.check(*imit_smooth_l1(c, 1, "<= at beta"), nparts=1))
        line = must_fail(c.check(*imit_smooth_l1(c, 1, "seam one step late"), nparts=1), "seam one step late", "smooth_l1 n=8 beta=%g edge" % beta)
        assert "first at element [2]" in line, line          # beta's upper neighbour
    c = SX.smooth_l1_case(4097)
    must_fail(c.check(*imit_smooth_l1(c, 2, "tail dropped"), nparts=2), "tail dropped", "smooth_l1 n=4097")
    must_fail(c.check(*imit_smooth_l1(c, 2, "last partial dropped"), nparts=2), "last partial dropped", "smooth_l1 n=4097")
    must_fail(c.check(*imit_smooth_l1(c, 2, "grad without 1/n"), nparts=2), "grad without 1/n", "smooth_l1 n=4097")


def test_bce_prob_defects_fail():
    for t in (0.0, 1.0):
        c = SX.bce_prob_case(4, t, True)
        must_fail(c.check(*imit_bce_prob(c, 1, "no -100 clamp"), nparts=1), "no -100 clamp", "bce_prob n=4 target=%g edge" % t)
        must_fail(c.check(*imit_bce_prob(c, 1, "no 1e-12 clamp"), nparts=1), "no 1e-12 clamp", "bce_prob n=4")
    c = SX.bce_prob_case(4097, 1.0)
    must_fail(c.check(*imit_bce_prob(c, 2, "tail dropped"), nparts=2), "tail dropped", "bce_prob n=4097")


def test_cross_entropy_defects_fail():
    c = SX.cross_entropy_case(257, 6, 9)
    line = must_fail(c.check(*imit_cross_entropy(c, "writes column K")), "writes column K", "cross_entropy B=257 K=6 ld=9 grad columns K..ld-1")
    assert "first at element [0, 0]" in line, line
    must_fail(c.check(*imit_cross_entropy(c, "mean over B*K")), "mean over B*K", "cross_entropy B=257 K=6 ld=9 loss")


def test_clamp01_defects_fail():
    c = SX.clamp01_case(63)
    y, gx = imit_clamp01(c, "nan clamped to 0")
    line = must_fail(c.check_fwd(y), "nan clamped to 0", "clamp01 n=63 normal fwd")
    assert "first at element [7]" in line, line
    y, gx = imit_clamp01(c, "x > 0")
    must_fail(c.check_bwd(gx), "x > 0", "clamp01 n=63 normal bwd")


def test_psnr_defects_fail():
    c = SX.psnr255_case(4097)
    must_fail(c.check(imit_psnr255(c, 2, "rounding for truncation")), "rounding for truncation", "psnr255 n=4097")
    must_fail(c.check(imit_psnr255(c, 2, "tail dropped")), "tail dropped", "psnr255 n=4097")
    for npt in (257, 2048):
        c = SX.PsnrGateCase(npt)
        must_fail(c.check(imit_psnr_gate(c.partials, c.n, 33.0, "last partial dropped"), 33.0), "last partial dropped", "psnr_gate nparts=%d psnr" % npt)
        thr = float(imit_psnr_gate(c.partials, c.n, 33.0)[0])
        must_fail(c.check(imit_psnr_gate(c.partials, c.n, thr, "<= at the gate"), thr), "<= at the gate", "psnr_gate nparts=%d weight" % npt)


def test_plane_kernel_defects_fail():
    c = SX.splice_case(3, 3, 771)
    must_fail(c.check("all", *imit_splice(c, "mask indexed by plane")), "mask indexed by plane", "splice B=3 C=3 HW=771 normal tampered")
    must_fail(c.check("all", *imit_splice(c, "rounding for truncation")), "rounding for truncation", "splice B=3 C=3 HW=771 normal psnr partials")
    must_fail(c.check("all", *imit_splice(c, "round half away")), "round half away", "splice B=3 C=3 HW=771 normal fwd_q")
    c = SX.MaskedAxpyCase(3, 3, 5)
    must_fail(c.check(imit_masked_axpy(c, "mask indexed by plane")), "mask indexed by plane", "masked_axpy B=3 C=3 HW=5")
    c = SX.ImageGradMseCase(3, 3, 5, "f16", 16, 5)
    must_fail(c.check(*imit_image_grad(c, 1, "c0 ignored")), "c0 ignored", "image_grad_mse B=3 C=3 HW=5 f16 ld=16 c0=5 out")


def test_flat_glue_defects_fail():
    c = SX.AxpyCase(65, "normal")
    must_fail(c.check(a32(c.a) + a32(c.b)), "s ignored", "axpy n=65")
    c = SX.ScaleDevCase(65, "normal", 0.3)
    must_fail(c.check(a32(c.x) * f32(c.s) * f32(c.s)), "scaled twice", "scale_dev n=65")
    c = SX.MaskThresholdCase(65, "normal", 0.5)
    with np.errstate(invalid="ignore"):
        line = must_fail(c.check((a32(c.p) >= f32(c.thr)).astype(np.uint8)), ">= for >", "mask_threshold n=65")
    assert "first at element [1]" in line, line
    c = SX.mse_case(4097, 0.7, 1.5, None)
    must_fail(c.check(*imit_mse(c, 2, "tail dropped"), nparts=2), "tail dropped", "mse n=4097")
    must_fail(c.check(*imit_mse(c, 2, "gscale_dev ignored"), nparts=2), "gscale_dev ignored", "mse n=4097")
    c = SX.SumsqCase(4097)
    must_fail(c.check(sum32(a32(c.x) * a32(c.x), 2, "tail dropped")), "tail dropped", "sumsq n=4097")
    c = SX.NonfiniteCase(4097, None, None)
    must_fail(c.check(imit_nonfinite(c, 2, "from the sum of squares")), "from the sum of squares", "nonfinite n=4097")


def test_bce_logits_defects_fail():
    c = SX.bce_logits_case(257, True, 1.0, None, True, False)
    must_fail(c.check(*imit_bce_logits(c, 1, "chain factor omitted"), nparts=1), "chain factor omitted", "bce_logits_target n=257 chain")
    must_fail(c.check(*imit_bce_logits(c, 1, "1/n twice"), nparts=1), "1/n twice", "bce_logits_target n=257 chain")
    c = SX.bce_logits_case(4097, True, 1.0, None, False, False)
    must_fail(c.check(*imit_bce_logits(c, 2, "tail dropped"), nparts=2), "tail dropped", "bce_logits_target n=4097")
    c = SX.bce_logits_case(257, False, 1.0, None, False, False)
    must_fail(c.check(*imit_bce_logits(c, 1, "target ignored in grad"), nparts=1), "target ignored in grad", "bce_logits target=1 n=257")


def test_message_loss_and_hidden_metrics_defects_fail():
    c = SX.message_loss_case(14, None, True)
    line = must_fail(c.check(*imit_message_loss(c, "round half away")), "round half away", "message_loss n=14 edge out")
    assert "first at element [1]" in line, line
    must_fail(c.check(*imit_message_loss(c, "gscale ignored")), "gscale ignored", "message_loss n=14 edge grad")
    for npt in (257, 2048):
        c = SX.HiddenMetricsCase(npt)
        must_fail(c.check(imit_hidden_metrics(c, "last partial dropped")), "last partial dropped", "hidden_metrics nparts=%d" % npt)
    line = must_fail(c.check(imit_hidden_metrics(c, "bit error slot")), "bit error slot", "hidden_metrics nparts=2048")
    assert "first at element [3]" in line, line


# ----------------------------------------------------------------------------------------------------------------- the references are torch's
def t64(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).requires_grad_(grad)


def close(got, ref, tol=1e-6):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.all(np.abs(got - ref) <= tol * np.maximum(np.abs(ref), 1e-30) + 1e-30), float(np.abs(got - ref).max())


def test_references_agree_with_torch_in_float64():
    c = SX.smooth_l1_case(4097)
    a = t64(c.a, True)
    loss = nn.SmoothL1Loss(beta=c.beta)(a, t64(c.b))
    loss.backward()
    close(c.loss, loss.item()), close(c.grad, a.grad.numpy())

    for t in (0.0, 1.0):
        c = SX.bce_prob_case(257, t)
        p = t64(c.p, True)
        loss = nn.BCELoss()(p, torch.full_like(p, t))
        loss.backward()
        close(c.loss, loss.item()), close(c.grad, p.grad.numpy())
    c = SX.bce_prob_case(4, 1.0, True)                       # the -100 clamp is torch's
    close(c.loss, nn.BCELoss()(t64(c.p), torch.ones(4, dtype=torch.float64)).item())

    c = SX.cross_entropy_case(257, 6)
    z = t64(c.z, True)
    loss = nn.CrossEntropyLoss()(z, torch.from_numpy(c.y))
    loss.backward()
    close(c.loss, loss.item()), close(c.grad, z.grad.numpy(), 1e-9)

    c = SX.clamp01_case(63)
    x = t64(c.x, True)
    y = torch.clamp(x, 0, 1)
    (y * t64(c.g)).sum().backward()
    assert np.array_equal(y.detach().numpy(), c.fwd, equal_nan=True) and np.array_equal(x.grad.numpy(), c.bwd)

    for chain in (False, True):
        c = SX.bce_logits_case(257, True, 1.0, None, chain, False)
        if chain:                                             # p = sigmoid(z), the gradient wrt z
            zz = t64(np.log(c.x / (1.0 - c.x)), True)
            x = torch.sigmoid(zz)
        else:
            x = zz = t64(c.x, True)
        loss = nn.BCEWithLogitsLoss()(x, t64(c.t))
        (loss * c.G).backward()
        close(c.loss, loss.item()), close(c.grad, zz.grad.numpy(), 1e-6)
    c = SX.bce_logits_case(257, False, 1.0, None, False, False)
    x = t64(c.x, True)
    loss = nn.BCEWithLogitsLoss()(x, t64(c.t))
    (loss * c.G).backward()
    close(c.loss, loss.item()), close(c.grad, x.grad.numpy())

    c = SX.message_loss_case(14, None, True)
    d, m = t64(c.d), t64(c.m)
    close(c.out[0], nn.MSELoss()(d, m).item())
    close(c.out[1], (torch.abs(torch.clip(torch.round(d), 0, 1) - m).sum() / c.n).item())

    c = SX.mse_case(257, 0.7, None, None)
    a, b = t64(c.a, True), t64(c.b)
    (nn.MSELoss(reduction="sum")(a, b) * 0.5 * c.G).backward()
    close(c.ssq, ((a - b) ** 2).sum().item()), close(c.grad, a.grad.numpy())

    c = SX.splice_case(3, 3, 5)
    x32 = torch.from_numpy(a32(c.enc))
    assert np.array_equal((torch.round(torch.clamp(x32, 0, 1) * 255.0) / 255.0).double().numpy(), c.q)
    r32_ = torch.from_numpy(a32(c.real))
    assert np.array_equal((r32_ * 255.0).int().numpy(), SX.trunc255(c.real, False))


def test_edge_inputs_are_where_the_tables_say():
    c = SX.smooth_l1_case(8, 0.25, True)
    assert list(c.a[:3]) == SX.around(0.25) and list(c.quad[:6]) == [True, False, False, True, False, False]
    c = SX.clamp01_case(63)
    assert np.isnan(c.x[7]) and np.isnan(c.fwd[7]) and c.bwd[7] == 0 and c.fwd[3] == 1.0 and c.bwd[3] == 0 and c.bwd[4] == 0
    c = SX.message_loss_case(14, None, True)
    assert list(c.bits[:7]) == [0, 0, 1, 1, 0, 0, 1] and list(c.bits[7:14]) == [1, 0, 0, 0, 1, 0, 0]
    c = SX.NonfiniteCase(4097, None, None)
    assert np.isfinite(c.x).all() and not np.isfinite(np.float32(c.x[4097 // 2] ** 2))
    sv = SX.seam_values()
    t = (a32(sv) * f32(255))
    assert (t == np.rint(t)).sum() >= 10 and (np.trunc(t) != np.rint(t)).sum() >= 5
