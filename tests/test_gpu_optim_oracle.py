"""GPU: the three Adam kernels of csrc/optim.hip, the GradScaler's inf check and the clip coefficient against float64 references.

  * adam_step (eager), adam_step_dev (a replayed step: every number from a device block written by adam_hyper) and adam_step_amp (under the
    device GradScaler) against torch.optim.Adam / AdamW's single-tensor formulas in float64, one step at a time from the kernel's own
    state, comparing p, m and v after every step -- at sizes below, at and past a block, and past grid_for's 2048-block cap (the grid-stride
    loop wraps), for t = 1, 2, 3 and a resumed t = 10^4;
  * adam_step_dev gives the same bytes as adam_step for every case (include/wm_hip.h promises it);
  * edge inputs: all-zero gradients, gradients near 1e-30 (eps dominates) and 1e15 (large squares), parameters of exact zeros;
  * AMP: weight decay under the scaler against torch.amp.GradScaler + Adam / AdamW; a skipped step leaves p, m and v bit-unchanged; the
    found-inf decision against torch's per-element check, including a finite gradient whose square overflows f32;
  * wm_clip_coef against nn.utils.clip_grad_norm_ in float64: norm below / above max_norm, inf, nan.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of f32
TINY = 2.0 ** -126      # smallest normal f32: a result that underflows in f32 (a square near 1e-60) may differ from float64 by this much
f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))   # noqa: E731 -- the f32 value a float launch argument becomes


def _ref_step(p0, g, m0, v0, lr, b1, b2, eps, wd, decoupled, t, gs, device_bias=False):
    """one torch.optim.Adam / AdamW step (single-tensor, non-amsgrad) in float64 from the kernel's state, with the f32-rounded
    hyperparameters the kernel receives, and an error budget per element for each result.

    The budget is what f32 arithmetic of ONE step may add, bounded to first order from the operations' magnitudes (u = 2^-24 per rounding):
      m = b1*m + (1-b1)*g'     g' = g*gs (+ wd*p): a handful of roundings of the terms       -> 6u * (|b1*m| + |1-b1|*|g'|)
      v = b2*v + (1-b2)*g'^2   g'^2 doubles g's relative error                              -> 12u * (|b2*v| + |1-b2|*|g'|^2)
      p = p' - s * m / (sqrt(v)/bc2 + eps): the update bounded over m +- em, v +- ev, plus 4u of it for s, the division and the product,
      3u of |p| for the decay p' and the subtraction.
    device_bias: the AMP kernel computes 1 - b^t in f32 on the device (powf; the others take them from the host in float64, rounded
    once): an error of a few ulp of b^t, relative to 1 - b^t -- 4u * b^t / (1 - b^t) for each correction, counted on the update.
    A mutation of one formula (a wrong coefficient, eps under the root, a dropped gradient scale, a missing bias correction) moves the
    results by orders of magnitude more; TINY covers f32 underflow."""
    gg = g * gs
    gabs = gg.abs()
    pd = p0
    if wd != 0.0:
        if decoupled:
            pd = p0 * (1.0 - lr * wd)
        else:
            gg = gg + wd * p0
            gabs = gabs + abs(wd) * p0.abs()
    m1 = b1 * m0 + (1.0 - b1) * gg
    v1 = b2 * v0 + (1.0 - b2) * gg * gg
    em = 6 * U * (abs(b1) * m0.abs() + abs(1.0 - b1) * gabs) + TINY
    ev = 12 * U * (abs(b2) * v0.abs() + abs(1.0 - b2) * gabs * gabs) + TINY
    s = lr / (1.0 - b1 ** t)
    bc2 = math.sqrt(1.0 - b2 ** t)
    denom = v1.sqrt() / bc2 + eps
    denom_lo = (v1 - ev).clamp_min(0).sqrt() / bc2 + eps - 4 * U * denom
    upd = s * m1 / denom
    upd_hi = s * (m1.abs() + em) / denom_lo
    p1 = pd - upd
    rel = 4 * U
    if device_bias:
        rel += 4 * U * (b1 ** t / (1.0 - b1 ** t) + 0.5 * b2 ** t / (1.0 - b2 ** t)) + 2 * U
    ep = (upd_hi - upd.abs()) + rel * upd_hi + 3 * U * (p0.abs() + p1.abs()) + TINY
    return (p1, m1, v1), (ep, em, ev)


def _check(name, got, ref, err, ctx):
    d = (got.double() - ref).abs()
    bad = ~(d <= err)
    if bad.any():
        i = int(bad.nonzero()[0, 0])
        raise AssertionError(f"{name} {ctx}: {int(bad.sum())} of {d.numel()} elements out of bound; first at {i}: "
                             f"got {float(got[i])!r} ref {float(ref[i])!r} bound {float(err[i])!r}")


SIZES = [1, 255, 257, 2 * 524288 + 37]      # the last is past grid_for's cap of 2048 blocks x 256 threads: the grid-stride loop wraps
BETAS = [(0.9, 0.999), (0.5, 0.9), (0.0, 0.999)]
STEPS = [1, 2, 3, 10000]                   # 10^4: a resumed run (the bias corrections are ~1)
LR, EPS = 1e-2, 1e-8


def _inputs(n, seed, kind="normal", dev="cuda"):
    gen = torch.Generator(device=dev).manual_seed(seed)
    p = torch.randn(n, device=dev, generator=gen)
    mag = 10.0 ** (torch.rand(n, device=dev, generator=gen) * 4 - 3)     # per-element magnitudes 1e-3 .. 1e1
    gs = [torch.randn(n, device=dev, generator=gen) * mag for _ in STEPS]
    if kind == "zero_grad":
        gs = [torch.zeros(n, device=dev) for _ in STEPS]
    elif kind == "tiny_grad":
        gs = [g.sign() * 1e-30 * (1 + g.abs()) for g in gs]
    elif kind == "huge_grad":
        gs = [g.sign() * 1e15 * (1 + g.abs() / 10) for g in gs]
    elif kind == "zero_p":
        p = torch.zeros(n, device=dev)
    return p, gs


class _Runner:
    """one of the three kernels over one flat buffer; `step(g, t)` runs step t on gradient g (the AMP runner stores it multiplied by its
    loss scale, as a scaled backward leaves it) and returns (the gradient buffer the kernel read, the factor it multiplied it by)"""

    def __init__(self, kernel, p, lr, betas, eps, wd, decoupled, gscale):
        from video_watermarking_forgery_detection_amd import ops
        self.ops, self.kernel = ops, kernel
        self.p, self.m, self.v = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
        self.hp = (lr, betas[0], betas[1], eps, wd)
        self.decoupled, self.gscale = decoupled, gscale
        if kernel == "dev":       # the eager twin whose bytes the replayed kernel must reproduce
            self.twin = (p.clone(), torch.zeros_like(p), torch.zeros_like(p))
        if kernel == "amp":
            self.amp = ops.AmpState(p.device, init_scale=1024.0)
            self.k = self.amp.slot()

    def step(self, g, t):
        ops = self.ops
        lr, b1, b2, eps, wd = self.hp
        if self.kernel == "eager":
            ops.adam_step(self.p, g, self.m, self.v, lr, b1, b2, eps, wd, t, decoupled=self.decoupled, grad_scale=self.gscale)
            return g, f32(self.gscale)
        if self.kernel == "dev":
            hyper = torch.tensor(ops.adam_hyper(lr, b1, b2, t, eps, wd), dtype=torch.float32, device=self.p.device)
            ops.adam_step_dev(self.p, g, self.m, self.v, hyper, decoupled=self.decoupled, grad_scale=self.gscale)
            tp, tm, tv = self.twin
            ops.adam_step(tp, g, tm, tv, lr, b1, b2, eps, wd, t, decoupled=self.decoupled, grad_scale=self.gscale)
            for a, b, nm in ((self.p, tp, "p"), (self.m, tm, "m"), (self.v, tv, "v")):
                assert torch.equal(a, b), f"adam_step_dev differs from adam_step in {nm} at t={t}"
            return g, f32(self.gscale)
        amp = self.amp
        amp.set_step_count(self.k, t - 1)          # the device step count the kernel takes t from
        gbuf = g * 1024.0                          # exact (a power of two, no overflow at these magnitudes)
        amp.found_inf(self.k, [gbuf])
        ops.adam_step_amp(self.p, gbuf, self.m, self.v, lr, b1, b2, eps, wd, amp, self.k, decoupled=self.decoupled, grad_scale=self.gscale)
        amp.update()
        assert amp.get_scale() == 1024.0 and amp.step_count(self.k) == t
        return gbuf, f32(self.gscale) / 1024.0     # the kernel multiplies the scaled gradient by grad_scale / scale (both f32: exact here)


def _run(kernel, n, betas, wd, decoupled, gscale, kind="normal", seed=0):
    p, grads = _inputs(n, 1000 + seed + n % 97, kind)
    r = _Runner(kernel, p, LR, betas, EPS, wd, decoupled, gscale)
    lr, b1, b2, eps, wdf = (f32(x) for x in (LR, betas[0], betas[1], EPS, wd))
    for t, g in zip(STEPS, grads):
        p0, m0, v0 = r.p.double(), r.m.double(), r.v.double()
        if t == STEPS[-1] and kind == "normal":      # resumed: warm moments from an earlier run
            m0 = (g.double() * 0.3).float().double(); v0 = (g.double() ** 2 * 0.7 + 1e-6).float().double()
            r.m.copy_(m0); r.v.copy_(v0)
            if kernel == "dev":
                r.twin[1].copy_(m0); r.twin[2].copy_(v0)
        gbuf, gs = r.step(g, t)
        (pr, mr, vr), (ep, em, ev) = _ref_step(p0, gbuf.double(), m0, v0, lr, b1, b2, eps, wdf, decoupled, t, gs, device_bias=kernel == "amp")
        ctx = f"[{kernel} n={n} betas={betas} wd={wd} decoupled={decoupled} gs={gscale} {kind} t={t}]"
        _check("m", r.m, mr, em, ctx)
        _check("v", r.v, vr, ev, ctx)
        _check("p", r.p, pr, ep, ctx)
    return r, p


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("betas", BETAS, ids=["b0.9-0.999", "b0.5-0.9", "b0-0.999"])
@pytest.mark.parametrize("gscale", [1.0, 0.25])
@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
@pytest.mark.parametrize("kernel", ["eager", "dev", "amp"])
def test_adam_kernels_match_float64(kernel, decoupled, wd, gscale, betas, n):
    _run(kernel, n, betas, wd, decoupled, gscale)   # (adam_step_dev: also the bytes of adam_step, every step)


@pytest.mark.parametrize("kind", ["zero_grad", "tiny_grad", "huge_grad", "zero_p"])
@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
@pytest.mark.parametrize("kernel", ["eager", "dev", "amp"])
def test_adam_kernels_edge_inputs(kernel, decoupled, kind):
    n = 257     # (1e15 gradients: 1e18 in the AMP runner's scaled buffer, squares near 1e36 -- finite in f32)
    r, p = _run(kernel, n, (0.9, 0.999), 0.05, decoupled, 1.0, kind=kind, seed=77)
    if kind == "zero_grad" and decoupled:
        # zero gradients, decoupled decay: the moments stay exactly zero and p changes by the decay alone, (1 - lr*wd) per step
        assert torch.count_nonzero(r.m) == 0 and torch.count_nonzero(r.v) == 0
        want = p.double() * (1.0 - f32(LR) * f32(0.05)) ** len(STEPS)
        _check("p", r.p, want, 4 * len(STEPS) * U * want.abs() + TINY, f"[{kernel} decay only]")
    if kind == "zero_p" and decoupled:
        assert torch.isfinite(r.p).all()


def test_scaler_skipped_step_leaves_p_m_v_bit_unchanged():
    """a step whose gradients hold an inf or nan is skipped entirely: parameters and both moments keep their bytes, the step count stays"""
    from video_watermarking_forgery_detection_amd import ops
    n = 2 * 524288 + 37
    p, grads = _inputs(n, 5)
    amp = ops.AmpState(p.device, init_scale=1024.0)
    k = amp.slot()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for decoupled in (False, True):
        for i, bad in enumerate((float("inf"), float("nan"), float("-inf"))):
            g = grads[i] * 1024.0
            amp.found_inf(k, [g])
            ops.adam_step_amp(p, g, m, v, 1e-2, 0.9, 0.999, 1e-8, 0.05, amp, k, decoupled=decoupled)   # a clean step: warm moments
            amp.update()
            before = (p.clone(), m.clone(), v.clone(), amp.step_count(k))
            g = grads[i + 1] * 1024.0
            g[n - 1 - 1000 * i] = bad                 # in the last block of the wrapped grid
            amp.found_inf(k, [g])
            ops.adam_step_amp(p, g, m, v, 1e-2, 0.9, 0.999, 1e-8, 0.05, amp, k, decoupled=decoupled)
            assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2]), (decoupled, bad)
            amp.update()
            assert amp.step_count(k) == before[3]


@pytest.mark.parametrize("decoupled", [False, True], ids=["Adam", "AdamW"])
def test_scaler_with_weight_decay_matches_torch_amp(decoupled):
    """test_gpu_fp16.py's scaler comparison with weight decay, coupled (Adam) and decoupled (AdamW): torch.amp.GradScaler + torch.optim on
    the CPU against the device scaler, step for step through skipped steps, back-off and growth; p, m and v compared"""
    from video_watermarking_forgery_detection_amd import ops
    n, steps, bad, wd = 4096, 12, (2, 5, 6), 0.05
    torch.manual_seed(4)
    p0 = torch.randn(n)
    cs = [torch.randn(n) * 10 ** float(torch.randint(-4, 1, (1,))) for _ in range(steps)]
    pr = torch.nn.Parameter(p0.clone())
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([pr], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    sc = torch.amp.GradScaler("cpu", init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    ref = []
    for t in range(steps):
        opt.zero_grad()
        c = cs[t].clone()
        if t in bad:
            c[7] = float("inf")
        sc.scale((pr * c).sum()).backward()
        sc.step(opt)
        sc.update()
        st = opt.state[pr]
        ref.append((sc.get_scale(), pr.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    dev = torch.device("cuda", 0)
    amp = ops.AmpState(dev, init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    k = amp.slot()
    p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    for t in range(steps):
        c = cs[t].clone()
        if t in bad:
            c[7] = float("inf")
        g = c.to(dev) * amp.scale
        prev = (p.clone(), m.clone(), v.clone())
        amp.found_inf(k, [g])
        ops.adam_step_amp(p, g, m, v, 1e-2, 0.9, 0.999, 1e-8, wd, amp, k, decoupled=decoupled)
        amp.update()
        assert amp.get_scale() == ref[t][0], (t, amp.get_scale(), ref[t][0])
        if t in bad:
            assert torch.equal(p, prev[0]) and torch.equal(m, prev[1]) and torch.equal(v, prev[2]), t
        torch.testing.assert_close(p.cpu(), ref[t][1], rtol=2e-6, atol=2e-7)
        # (torch's m = lerp(m, g, 1 - beta1) rounds in another order than b1*m + (1-b1)*g: where m cancels to near zero the two differ by
        # a rounding of the terms, so the absolute part is taken at the tensor's scale)
        torch.testing.assert_close(m.cpu(), ref[t][2], rtol=2e-6, atol=2e-6 * float(ref[t][2].abs().max()))
        # torch's CPU step takes 1 - beta2 in double and rounds it once (f32(0.001) for beta2 = 0.999); the kernel receives f32(0.999) and
        # subtracts: 1 - f32(0.999) is 1.29e-5 smaller, relatively -- a difference of representation, which the float64 comparison above
        # (fed the f32 hyperparameters) does not have
        torch.testing.assert_close(v.cpu(), ref[t][3], rtol=2e-5, atol=1e-14)
    assert amp.step_count(k) == steps - len(bad)


@pytest.mark.parametrize("value", [1.0, 2.0e19, 3.0e38, float("inf"), float("-inf"), float("nan")],
                         ids=["finite", "square-overflows", "near-max", "inf", "-inf", "nan"])
def test_scaler_found_inf_matches_torch_per_element_check(value):
    """GradScaler.unscale_ decides per element (torch._amp_foreach_non_finite_check_and_unscale_): a finite gradient whose square overflows
    f32 (|g * scale| > 1.9e19) is stepped, not skipped.  Two buffers, the odd value in the second one's wrapped grid."""
    from video_watermarking_forgery_detection_amd import ops
    dev = torch.device("cuda", 0)
    amp = ops.AmpState(dev, init_scale=1.0)
    k = amp.slot()
    a = torch.randn(1000, device=dev)
    b = torch.randn(2 * 524288 + 37, device=dev)
    b[-5] = value
    found = torch.zeros(1)
    torch._amp_foreach_non_finite_check_and_unscale_([a.cpu(), b.cpu()], found, torch.ones(1))
    amp.found_inf(k, [a, b])
    assert float(amp.state[8 + k]) == float(found), (value, float(amp.state[8 + k]), float(found))
    # and the step follows the decision: taken for a finite value (p moves), skipped otherwise
    p, m, v = torch.zeros(b.numel(), device=dev), torch.zeros(b.numel(), device=dev), torch.zeros(b.numel(), device=dev)
    ops.adam_step_amp(p, b, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, amp, k)
    assert bool(torch.count_nonzero(p)) == (float(found) == 0.0)
    amp.update()


@pytest.mark.parametrize("case", ["below", "above", "inf", "nan"])
def test_clip_coefficient_matches_clip_grad_norm(case):
    """ops.clip_grad_norm_ (wm_sumsq + wm_clip_coef + wm_scale_dev) over two flat buffers clipped together against
    nn.utils.clip_grad_norm_ in float64: coefficient, total norm and the clipped gradients"""
    from video_watermarking_forgery_detection_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(11)
    flats = [torch.randn(3001, device=dev, generator=gen) * 0.01, torch.randn(2 * 524288 + 37, device=dev, generator=gen) * 0.01]
    norm = math.sqrt(sum(float((f.double() ** 2).sum()) for f in flats))
    max_norm = {"below": 2.0 * norm, "above": 0.25 * norm, "inf": 1.0, "nan": 1.0}[case]
    if case == "inf":
        flats[1][-3] = float("inf")
    if case == "nan":
        flats[0][17] = float("nan")
    params = [torch.nn.Parameter(torch.zeros(f.numel(), dtype=torch.float64)) for f in flats]
    for q, f in zip(params, flats):
        q.grad = f.double().cpu()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
    coef_ref = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    out = ops.clip_grad_norm_(flats, max_norm).cpu()
    assert torch.allclose(out[1].double(), total, rtol=1e-5, atol=0, equal_nan=True), (case, float(out[1]), float(total))
    assert torch.allclose(out[0].double(), coef_ref, rtol=1e-5, atol=0, equal_nan=True), (case, float(out[0]), float(coef_ref))
    if case == "below":
        assert float(out[0]) == 1.0
    for q, f in zip(params, flats):
        torch.testing.assert_close(f.cpu().double(), q.grad, rtol=1e-5, atol=1e-12, equal_nan=True)
