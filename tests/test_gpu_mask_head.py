"""The two-source mask head (csrc/mask_head.hip: wm_head2_fwd / wm_head2_bwd / wm_head2_finalize through ops.head2_fwd / head2_bwd) against a
float64 numpy restatement written as a loop over channels on NCHW arrays -- it shares no index arithmetic with the kernel, which walks 16-byte
vectors of two NHWC tensors with lanes grouped per pixel.

Cases (the smallest at which the kernel can still go wrong):
  a  na = nb = 16 in strides of 16, B = 2, 5 x 7 pixels, Cout = 1, sigmoid: 70 pixels, a wave tail
  b  na = 12 in a stride of 16, nb = 20 in a stride of 24, B = 1, 3 x 4, Cout = 3, no activation: padding channels (filled with 3e4 on the way
     in: the head must ignore them), unequal sources, lane groups with idle lanes
  c  na = nb = 32, B = 2, 9 x 15, Cout = 1, sigmoid: 270 pixels = more than one workgroup of partial sums in every dtype
each in float32, bfloat16 and float16; for the 16-bit runs the inputs are rounded to the dtype first, so the reference sees the same numbers.

Bounds (the rule of tests/unetd_restate.py, MARGIN = 4): 4 x torch-CPU's OWN float32-vs-float64 deviation of conv2d(cat(a, b), w, bias)
(+ sigmoid) and of its autograd gradients on the same inputs, computed here and never calibrated on the kernel; never less than 2 float32 ulp
of the tensor's largest magnitude; for ga / gb in a 16-bit dtype plus half an ulp of that dtype at the value's magnitude (the store rounds).
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import unetd_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = {   # name: (B, H, W, na, lda, nb, ldb, Cout, act)
    "a": (2, 5, 7, 16, 16, 16, 16, 1, 1),
    "b": (1, 3, 4, 12, 16, 20, 24, 3, 0),
    "c": (2, 9, 15, 32, 32, 32, 32, 1, 1),
}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
PAD_FILL = 3.0e4     # what the sources' padding channels hold on the way in (finite in float16)


def _ops():
    from video_watermarking_forgery_detection_amd import ops
    return ops


def inputs(name, tag):
    """a [B,na,H,W], b [B,nb,H,W] (rounded to the dtype), w [Cout,na+nb], bias [Cout], g [B,Cout,H,W]: float32 numpy"""
    B, H, W, na, lda, nb, ldb, Cout, act = CASES[name]
    rs = np.random.RandomState(8700 + 10 * sorted(CASES).index(name))
    a, b = rs.randn(B, na, H, W).astype(np.float32), rs.randn(B, nb, H, W).astype(np.float32)
    w = (rs.randn(Cout, na + nb) * np.sqrt(2.0 / (na + nb))).astype(np.float32)
    bias = (0.1 * rs.randn(Cout)).astype(np.float32)
    g = rs.randn(B, Cout, H, W).astype(np.float32)
    rnd = lambda x: torch.from_numpy(x).to(DTYPES[tag]).float().numpy()
    return rnd(a), rnd(b), w, bias, g


def restate(a, b, w, bias, g, act, chain=True):
    """float64, a loop over channels: out, ga, gb, dw, db.  chain False: g is the gradient wrt the logits"""
    a, b, w, bias, g = (np.asarray(t, np.float64) for t in (a, b, w, bias, g))
    B, na, H, W = a.shape
    nb, Cout = b.shape[1], w.shape[0]
    z = np.zeros((B, Cout, H, W))
    for co in range(Cout):
        z[:, co] = bias[co]
        for c in range(na):
            z[:, co] += w[co, c] * a[:, c]
        for c in range(nb):
            z[:, co] += w[co, na + c] * b[:, c]
    out = 1.0 / (1.0 + np.exp(-z)) if act else z
    gz = g * out * (1.0 - out) if (act and chain) else g
    ga, gb, dw = np.zeros_like(a), np.zeros_like(b), np.zeros_like(w)
    for co in range(Cout):
        for c in range(na):
            ga[:, c] += gz[:, co] * w[co, c]
            dw[co, c] = (gz[:, co] * a[:, c]).sum()
        for c in range(nb):
            gb[:, c] += gz[:, co] * w[co, na + c]
            dw[co, na + c] = (gz[:, co] * b[:, c]).sum()
    return {"out": out, "ga": ga, "gb": gb, "dw": dw, "db": gz.sum(axis=(0, 2, 3))}


def torch_cpu(a, b, w, bias, g, act, dtype):
    """conv2d(cat(a, b), w, bias) (+ sigmoid) and its autograd gradients for the upstream gradient g, on the CPU in `dtype`"""
    a, b, w, bias = (torch.from_numpy(t).to(dtype).requires_grad_(True) for t in (a, b, w, bias))
    out = torch.nn.functional.conv2d(torch.cat((a, b), 1), w[:, :, None, None], bias)
    if act:
        out = torch.sigmoid(out)
    out.backward(torch.from_numpy(g).to(dtype))
    return {k: v.detach().double().numpy() for k, v in (("out", out), ("ga", a.grad), ("gb", b.grad), ("dw", w.grad), ("db", bias.grad))}


_REF = {}


def reference(name, tag):
    """(inputs, float64 restatement, {quantity: bound}) of a case, computed once"""
    if (name, tag) not in _REF:
        act = CASES[name][8]
        x = inputs(name, tag)
        want = restate(*x, act)
        t64, t32 = torch_cpu(*x, act, torch.float64), torch_cpu(*x, act, torch.float32)
        for k in want:     # the restatement is torch's float64 result up to float64 rounding
            assert R.maxdiff(want[k], t64[k]) <= 1e-12 * max(1.0, np.abs(t64[k]).max()), k
        bound = {k: R.bound_of(np.abs(t32[k] - t64[k]).max(), np.abs(t64[k]).max()) for k in want}
        _REF[(name, tag)] = (x, want, bound)
    return _REF[(name, tag)]


def half_ulp(v, tag):
    """half an ulp of the 16-bit dtype at |v| (0 for float32), elementwise"""
    if tag == "f32":
        return np.zeros_like(v)
    e = np.floor(np.log2(np.maximum(np.abs(v), 1e-300)))
    return 0.5 * 2.0 ** ((e - 7) if tag == "bf16" else (np.maximum(e, -14) - 10))


def nhwc(x, ld, dtype):
    """[B,C,H,W] numpy -> NHWC device tensor of channel stride ld, the padding channels filled with PAD_FILL"""
    B, C, H, W = x.shape
    out = torch.full((B, H, W, ld), PAD_FILL, dtype=dtype, device=DEV)
    out[..., :C] = torch.from_numpy(x).to(DEV).permute(0, 2, 3, 1).to(dtype)
    return out.contiguous()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(name, tag, act=None, bias=True, chain=True, g_override=None):
    """the kernel's results as float64 numpy, NCHW; also the raw ga / gb device tensors"""
    ops = _ops()
    B, H, W, na, lda, nb, ldb, Cout, act0 = CASES[name]
    act = act0 if act is None else act
    (a, b, w, bs, g), _, _ = reference(name, tag)
    ad, bd, wd = nhwc(a, lda, DTYPES[tag]), nhwc(b, ldb, DTYPES[tag]), dev(w)
    bd_ = dev(bs) if bias else torch.zeros(Cout, device=DEV)
    gd = dev(g) if g_override is None else g_override
    out = ops.head2_fwd(ad, na, bd, nb, wd, bd_, act)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, Cout, H, W)
    ga, gb, dw, db = ops.head2_bwd(ad, na, bd, nb, wd, gd, out if (act and chain) else None)
    assert ga.dtype == gb.dtype == DTYPES[tag] and ga.shape == ad.shape and gb.shape == bd.shape
    assert dw.dtype == db.dtype == torch.float32 and tuple(dw.shape) == (Cout, na + nb) and tuple(db.shape) == (Cout,)
    q = {"out": out, "ga": ga[..., :na].permute(0, 3, 1, 2), "gb": gb[..., :nb].permute(0, 3, 1, 2), "dw": dw, "db": db}
    return {k: v.double().cpu().numpy() for k, v in q.items()}, (out, ga, gb, dw, db)


def compare(label, got, want, bound, tag):
    failed = []
    for k in sorted(want):
        assert got[k].shape == want[k].shape and np.isfinite(got[k]).all(), k
        err = np.abs(got[k] - want[k])
        lim = bound[k] + (half_ulp(want[k], tag) if k in ("ga", "gb") else 0.0)
        worst = float((err / lim).max())
        print("%-34s %-3s largest error %.3e, largest share of its bound %.3f (bound %.3e)" % (label, k, float(err.max()), worst, bound[k]))
        if worst > 1.0:
            failed.append((label, k, float(err.max()), bound[k]))
    assert not failed, failed


@pytest.mark.parametrize("tag", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_against_float64(name, tag):
    B, H, W, na, lda, nb, ldb, Cout, act = CASES[name]
    _, want, bound = reference(name, tag)
    got, (out, ga, gb, dw, db) = run(name, tag)
    compare(f"case {name} {tag}", got, want, bound, tag)
    # padding channels of the gradients: exactly zero
    assert lda == na or float(ga[..., na:].float().abs().max()) == 0.0
    assert ldb == nb or float(gb[..., nb:].float().abs().max()) == 0.0
    # two runs: the same bits
    _, again = run(name, tag)
    for x, y in zip((out, ga, gb, dw, db), again):
        assert torch.equal(x, y)


@pytest.mark.parametrize("tag", sorted(DTYPES))
@pytest.mark.parametrize("name", ["a", "c"])
def test_sigmoid_chain_is_the_logit_backward(name, tag):
    """gout wrt the sigmoid output, chained in the kernel == gout * out * (1 - out) fed as the gradient wrt the logits"""
    (a, b, w, bs, g), want, bound = reference(name, tag)
    _, (out, *_rest) = run(name, tag)
    gz = dev(g) * out * (1.0 - out)
    got, _ = run(name, tag, chain=False, g_override=gz.contiguous())
    compare(f"case {name} {tag} logit form", got, want, bound, tag)


@pytest.mark.parametrize("tag", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_adjoint_identity(name, tag):
    """<out, g> with act = 0 and zero bias == <a, ga> + <b, gb>.  Each side is a sum of products of one exact factor and one that carries at
    most its bound of error, so the two sides differ by at most sum over the terms of |exact factor| x bound: the same bounds, scaled by
    the number of terms (and the factors' magnitudes)"""
    (a, b, w, bs, g), _, _ = reference(name, tag)
    x = (a, b, w, np.zeros_like(bs), g)
    t64, t32 = torch_cpu(*x, 0, torch.float64), torch_cpu(*x, 0, torch.float32)
    bound = {k: R.bound_of(np.abs(t32[k] - t64[k]).max(), np.abs(t64[k]).max()) for k in ("out", "ga", "gb")}
    got, _ = run(name, tag, act=0, bias=False, chain=False)
    lhs = float((got["out"] * g).sum())
    rhs = float((got["ga"] * a).sum() + (got["gb"] * b).sum())
    tol = (np.abs(g).sum() * bound["out"] + (np.abs(a) * (bound["ga"] + half_ulp(t64["ga"], tag))).sum()
           + (np.abs(b) * (bound["gb"] + half_ulp(t64["gb"], tag))).sum())
    print("adjoint %s %s: <out,g> %.9e, <a,ga>+<b,gb> %.9e, difference %.3e (bound %.3e over %d + %d + %d terms)"
          % (name, tag, lhs, rhs, abs(lhs - rhs), tol, g.size, a.size, b.size))
    assert abs(lhs - rhs) <= tol


def test_parameter_gradients_accumulate():
    """dw_acc / db_acc (a flat optimiser buffer's slices): the old values join the double sum"""
    ops = _ops()
    name, tag = "c", "f32"
    B, H, W, na, lda, nb, ldb, Cout, act = CASES[name]
    (a, b, w, bs, g), want, bound = reference(name, tag)
    ad, bd, wd = nhwc(a, lda, torch.float32), nhwc(b, ldb, torch.float32), dev(w)
    out = ops.head2_fwd(ad, na, bd, nb, wd, dev(bs), act)
    base_w, base_b = torch.full((Cout, na + nb), 0.5, device=DEV), torch.full((Cout,), -0.25, device=DEV)
    _, _, dw, db = ops.head2_bwd(ad, na, bd, nb, wd, dev(g), out, dw_acc=base_w, db_acc=base_b)
    assert dw.data_ptr() == base_w.data_ptr() and db.data_ptr() == base_b.data_ptr()
    R.check("accumulated dw", R.maxdiff(dw.double().cpu().numpy(), want["dw"] + 0.5), max(bound["dw"], 2 * R.ulp32(np.abs(want["dw"] + 0.5).max())))
    R.check("accumulated db", R.maxdiff(db.double().cpu().numpy(), want["db"] - 0.25), max(bound["db"], 2 * R.ulp32(np.abs(want["db"] - 0.25).max())))


def test_refusals():
    ops = _ops()
    a = torch.zeros(1, 4, 4, 16, device=DEV)
    w, bias = torch.zeros(5, 32, device=DEV), torch.zeros(5, device=DEV)
    with pytest.raises(ValueError):
        ops.head2_fwd(a, 16, a, 16, w, bias)                       # Cout <= 4
    with pytest.raises(ValueError):
        ops.head2_fwd(a, 17, a, 16, w[:1], bias[:1])               # na <= lda
    with pytest.raises(RuntimeError):                              # a stride of more than 16 vectors: the C ABI refuses (WM_E_SHAPE)
        big = torch.zeros(1, 2, 2, 272, device=DEV, dtype=torch.bfloat16)
        ops.head2_fwd(big, 272, big, 272, torch.zeros(1, 544, device=DEV), bias[:1])
