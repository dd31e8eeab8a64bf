"""The InvBlockExp kernels (csrc/invblock.hip) per element against the float64 bound model of tests/invarch_restate.py, the fused block
against the composed one, and the whole generator against the fixture made from the reference's modules (tests/golden/invarch.npz)."""
import os

import numpy as np
import pytest
import torch

import detgen
import instnorm_restate as NR
import invarch_restate as IR

GX = IR.GX
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "invarch.npz")
WM_E_BADARG = -1


def _mods():
    from video_watermarking_forgery_detection_amd import _lib, ops
    return _lib, ops, _lib.lib(), torch.cuda.current_stream().cuda_stream


def dev(a, dt, misalign=False):
    """float64 array -> device tensor of dtype dt; misalign: one element past a 16-byte boundary (the kernels' element-wise path)"""
    if a is None:
        return None
    t = GX.store(a, dt)
    if not misalign:
        return t.cuda()
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def filled(shape, dt, misalign=False):
    return dev(np.full(shape, GX.SENTINEL), dt, misalign)


def p(t):
    return None if t is None else t.data_ptr()


def report(cmps):
    for c in cmps:
        print("  ", c.line())
    for c in cmps:
        c.assert_ok()


def _worst(worst, cmps):
    for m in cmps:
        k = m.what.split()[-1]
        worst[k] = max(worst.get(k, 0.0), m.worst)


def _fractions(what, worst):
    print("worst fractions %s: %s" % (what, ", ".join("%s %.3f" % kv for kv in worst.items())))


def _run_affine(c, misalign=False, want_jac=True):
    _lib, ops, L, stream = _mods()
    dtid = ops.dt_id(GX.TORCH[c.dt])
    x, h, g, other, gout, v = (dev(a, c.dt, misalign) for a in (c.x, c.h, c.g, c.other, c.gout, c.v))
    out = filled((c.npix, c.ostride), c.dt, misalign)
    jac = torch.full((c.B,), GX.SENTINEL, device="cuda") if want_jac else None
    scratch = torch.empty(max(int(L.wm_invblock_scratch_doubles(c.B, c.hw, c.n1, c.n2)), 1), dtype=torch.float64, device="cuda") if want_jac else None
    _lib.check(L.wm_invblock_affine(p(x), c.cp, p(h), p(g), p(other), p(out), p(jac), p(scratch), c.B, c.hw, c.n1, c.n2, c.clamp, c.rev, dtid, stream), c.label)
    gx, gh, gg = filled((c.npix, c.cp), c.dt, misalign), filled((c.npix, c.cp2), c.dt, misalign), filled((c.npix, c.cp2), c.dt, misalign)
    gother = filled((c.npix, c.cp1), c.dt, misalign) if c.whole else None
    _lib.check(L.wm_invblock_affine_bwd(p(gout), int(c.whole), p(v), v.shape[1], c.voff, p(h), p(gx), c.cp, p(gh), p(gg), p(gother), c.npix,
                                        c.n1, c.n2, c.clamp, c.rev, dtid, stream), c.label)
    return (out, jac), (gx, gh, gg, gother)


def _run_shift(c, misalign=False):
    _lib, ops, L, stream = _mods()
    dtid = ops.dt_id(GX.TORCH[c.dt])
    x, f, other, g = (dev(a, c.dt, misalign) for a in (c.x, c.f, c.other, c.g))
    out = filled((c.npix, c.ostride), c.dt, misalign)
    _lib.check(L.wm_invblock_shift(p(x), c.cp, p(f), p(other), p(out), c.npix, c.n1, c.n2, c.sign, dtid, stream), c.label)
    gx, gf = filled((c.npix, c.cp), c.dt, misalign), filled((c.npix, c.cp1), c.dt, misalign)
    gother = filled((c.npix, c.cp2), c.dt, misalign) if c.whole else None
    _lib.check(L.wm_invblock_shift_bwd(p(g), int(c.whole), p(gx), c.cp, p(gf), p(gother), c.npix, c.n1, c.n2, c.sign, dtid, stream), c.label)
    return out, (gx, gf, gother)


def _same_bits(a, b):
    return all((s is None and t is None) or torch.equal(s.contiguous().view(torch.uint8), t.contiguous().view(torch.uint8)) for s, t in zip(a, b))


@pytest.mark.parametrize("dt", IR.KERNEL_DTYPES)
def test_affine_kernels_per_element(dt):
    """forward (with jac) and backward over invarch_restate.PIXELS (70 and 257 pixels; 5 and 16 samples: jac rows b >= 4) x SPLITS (3/9 and
    3/45; n1 = 4, 8, 16: the vector load at c0 + shift; 19/13: n1 > 16), rev 0 / 1, both `other` forms, clamp 1 and 0, h with 0 and +-20;
    SENTINEL in every input's padding, every destination pre-filled with SENTINEL and compared whole (padding: exact zeros); a second run
    gives the same bits.  The worst error-to-bound fraction of each quantity is printed at the end"""
    worst = {}
    for key in IR.affine_keys(dt):
        c = IR.AffineCase(*key)
        fwd, bwd = _run_affine(c)
        cmps = c.check_fwd(*fwd) + c.check_bwd(*bwd)
        report(cmps)
        _worst(worst, cmps)
        fwd2, bwd2 = _run_affine(c)
        assert _same_bits(fwd + bwd, fwd2 + bwd2), c.label + ": two runs differ"
    _fractions("invblock_affine " + dt, worst)


@pytest.mark.parametrize("dt", IR.KERNEL_DTYPES)
def test_jac_with_64_partials(dt):
    """one sample of 5462 pixels, split 3/45: hw * 48 > 64 * 4096, so the forward writes 64 partials (the cap) and the finalise's wave sums a
    full row of lanes"""
    c = IR.AffineCase(dt, *IR.P64_KEY, 0, True, 1.0)
    fwd, bwd = _run_affine(c)
    report(c.check_fwd(*fwd) + c.check_bwd(*bwd))
    fwd2, bwd2 = _run_affine(c)
    assert _same_bits(fwd + bwd, fwd2 + bwd2), c.label + ": two runs differ"


def test_second_grid_stride_trip_on_the_element_wise_path():
    """43 700 pixels, split 3/45, f32, base pointers one element past a 16-byte boundary: 43 700 * 48 elements > 8192 * 256 threads, so the
    grid-stride loops of shift_fwd / shift_bwd / affine_bwd take a second trip, and the no-jac forward's grid is at its cap of 2048; every
    output whole against the model"""
    c = IR.AffineCase("f32", *IR.BIG_KEY, 0, True, 1.0)
    fwd, bwd = _run_affine(c, misalign=True)
    report(c.check_fwd(*fwd) + c.check_bwd(*bwd))
    (out_nojac, _), _ = _run_affine(c, misalign=True, want_jac=False)
    report(c.check_fwd(out_nojac))
    c = IR.ShiftCase("f32", IR.BIG_KEY[0] * IR.BIG_KEY[1], 3, 45, -1.0, True)
    out, bwd = _run_shift(c, misalign=True)
    report(c.check_fwd(out) + c.check_bwd(*bwd))


@pytest.mark.parametrize("dt", IR.KERNEL_DTYPES)
def test_shift_kernels_per_element(dt):
    worst = {}
    for key in IR.shift_keys(dt):
        c = IR.ShiftCase(*key)
        out, bwd = _run_shift(c)
        cmps = c.check_fwd(out) + c.check_bwd(*bwd)
        report(cmps)
        _worst(worst, cmps)
        out2, bwd2 = _run_shift(c)
        assert _same_bits((out,) + bwd, (out2,) + bwd2), c.label + ": two runs differ"
    _fractions("invblock_shift " + dt, worst)


@pytest.mark.parametrize("dt", IR.KERNEL_DTYPES)
def test_element_wise_path_gives_the_vector_path_s_bits(dt):
    """base pointers one element past a 16-byte boundary take the kernels' element-wise path: within the same bounds, and bit-equal to the
    vector path; without jac the forward writes the same output"""
    for whole in (True, False):
        for rev in (0, 1):
            c = IR.AffineCase(dt, 2, 35, 3, 45, rev, whole, 1.0)
            fwd, bwd = _run_affine(c)
            fwd_m, bwd_m = _run_affine(c, misalign=True)
            report(c.check_fwd(*fwd_m) + c.check_bwd(*bwd_m))
            assert _same_bits(fwd + bwd, tuple(None if t is None else t.contiguous() for t in fwd_m + bwd_m)), c.label
            (out_nojac, none), _ = _run_affine(c, want_jac=False)
            assert none is None and _same_bits((out_nojac,), (fwd[0],)), c.label + ": jac changes the output"
        c = IR.ShiftCase(dt, 70, 3, 45, -1.0, whole)
        out, bwd = _run_shift(c)
        out_m, bwd_m = _run_shift(c, misalign=True)
        report(c.check_fwd(out_m) + c.check_bwd(*bwd_m))
        assert _same_bits((out,) + bwd, tuple(None if t is None else t.contiguous() for t in (out_m,) + bwd_m)), c.label


def test_a_window_outside_its_stride_is_refused():
    """n1 + n2 channels do not fit x's stride / v's window does not fit its stride: WM_E_BADARG, nothing launched (destinations keep SENTINEL)"""
    _lib, ops, L, stream = _mods()
    c = IR.AffineCase("f32", 2, 35, 3, 45, 0, True, 1.0)
    x, h, g, other, gout = (dev(a, "f32") for a in (c.x, c.h, c.g, c.other, c.gout))
    out = filled((c.npix, c.cp), "f32")
    outs = [filled((c.npix, s), "f32") for s in (c.cp, c.cp2, c.cp2, c.cp1)]
    assert L.wm_invblock_affine(p(x), 32, p(h), p(g), p(other), p(out), None, None, c.B, c.hw, 3, 45, 1.0, 0, 0, stream) == WM_E_BADARG
    assert b"stride" in L.wm_last_error_string()
    assert L.wm_invblock_affine(p(x), 40, p(h), p(g), p(other), p(out), None, None, c.B, c.hw, 3, 30, 1.0, 0, 0, stream) == WM_E_BADARG
    assert L.wm_invblock_shift(p(x), 32, p(other), None, p(out), c.npix, 3, 45, 1.0, 0, stream) == WM_E_BADARG
    assert L.wm_invblock_shift(p(x), c.cp, p(other), None, p(out), c.npix, 3, 45, 0.5, 0, stream) == WM_E_BADARG
    assert L.wm_invblock_shift_bwd(p(gout), 1, p(outs[0]), 32, p(outs[3]), p(outs[1]), c.npix, 3, 45, 1.0, 0, stream) == WM_E_BADARG
    assert L.wm_invblock_affine_bwd(p(gout), 1, p(x), c.cp, 4, p(h), p(outs[0]), c.cp, p(outs[1]), p(outs[2]), p(outs[3]), c.npix, 3, 45, 1.0, 0,
                                    0, stream) == WM_E_BADARG
    assert L.wm_invblock_affine_bwd(p(gout), 1, p(x), c.cp, 3, p(h), p(outs[0]), 32, p(outs[1]), p(outs[2]), p(outs[3]), c.npix, 3, 45, 1.0, 0,
                                    0, stream) == WM_E_BADARG
    assert L.wm_invblock_affine(p(x), c.cp, p(h), p(g), p(other), p(out), None, None, c.B, c.hw, 3, 45, 1.0, 0, 7, stream) == WM_E_BADARG
    torch.cuda.synchronize()
    for t in [out] + outs:
        assert bool((t == GX.SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------- the modules
class AsNCHW:
    """a HIP module that takes NHWC activations behind the NCHW interface run_cases drives (DenseBlock, InvBlockExp)"""

    def __init__(self, m, cout, dtype=torch.float32):
        self.m, self.cout, self.dtype = m, cout, dtype
        self.named_parameters, self.zero_grad = m.named_parameters, m.zero_grad

    def __call__(self, x, *a, **kw):
        from video_watermarking_forgery_detection_amd import glayers as G
        return G.to_nchw(self.m(G.to_nhwc(x, self.dtype), *a, **kw), self.cout)


def _hip_middle(net, x):
    from video_watermarking_forgery_detection_amd import glayers as G
    out = G.to_nhwc(x, net.dtype)
    for op in net.operations:
        out = op(out, False)
    return G.to_nchw(out, 3 * 4 ** IR.NET_DOWN)


def _hip_build(dtype):
    from video_watermarking_forgery_detection_amd.models.modules import Inv_arch as A
    from video_watermarking_forgery_detection_amd.models.modules import Subnet_constructor as S
    db = detgen.fill_f2(S.DenseBlock(IR.DB_CIN, IR.DB_COUT)).cuda()
    net = detgen.fill_f2(A.InvRescaleNet(3, 3, S.DenseBlock, IR.NET_BLOCKS, IR.NET_DOWN, dtype=dtype)).cuda()
    return AsNCHW(db, IR.DB_COUT, dtype), net


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_whole_net_and_dense_block_against_the_fixture(golden, tag):
    """every stored quantity -- net(x), net(y, rev=True), the round trip, (out, jac), the tensor between the two halves, gx and two
    parameter gradients each way, and the DenseBlock case -- within instnorm_restate.bound_of(the reference's own deviation in this dtype
    from float64, the quantity's largest value); each error is printed as a fraction of its bound"""
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16}[tag]
    db, net = _hip_build(dtype)
    q = IR.run_cases(db, net, IR.case_inputs(), lambda t: t.cuda().clone(), _hip_middle)
    dev_key = "dev32/" if tag == "f32" else "devbf16/"
    worst = []
    for k in sorted(q):
        bound = NR.bound_of(float(golden[dev_key + k]), float(golden["amax/" + k]))
        err = NR.maxdiff(q[k], golden[k])
        print("%-58s %.3e (bound %.3e, %.2f of it)" % (tag + " " + k, err, bound, err / bound))
        if not err <= bound:
            worst.append((k, err, bound))
    assert not worst, worst
    # the round trip returns the input, and cal_jacobian changes nothing but the return value
    x = IR.case_inputs()["net/x"].double().numpy()
    NR.check(tag + " round trip vs x", NR.maxdiff(q["net/rt"], x), NR.bound_of(float(golden[dev_key + "net/rt"]) + NR.maxdiff(golden["net/rt"], x), float(golden["amax/net/rt"])))
    assert np.array_equal(q["net/fwd_with_jac"], q["net/fwd"])


def _restate_block(n, n1, dtype):
    return detgen.fill_f2(IR.InvBlockExp(IR.DenseBlock, n, n1)).to(dtype)


@pytest.mark.parametrize("n,n1,hw", [(12, 3, (5, 7)), (48, 3, (3, 5))])
def test_fused_block_equals_the_composed_one(n, n1, hw):
    """InvBlockExp(fused=True) and (fused=False) with the same weights, forward, reverse and gradients (input, one weight of every
    subnet), each against the float64 restatement of the block: bound = instnorm_restate.bound_of(the restatement's own float32 CPU
    deviation from float64, the quantity's largest value).  The two need not be bit-equal (FMA contraction may differ)"""
    from video_watermarking_forgery_detection_amd.models.modules import Inv_arch as A
    from video_watermarking_forgery_detection_amd.models.modules import Subnet_constructor as S
    names = ("F.conv1.weight", "G.conv5.weight", "H.conv5.bias")
    x = detgen.normal((2, n) + hw, 9500 + n, std=0.5)
    gy = detgen.normal((2, n) + hw, 9501 + n)

    def run(blk, cast, rev):
        xi = cast(x).requires_grad_(True)
        out = blk(xi, rev)
        blk.zero_grad()
        (out * cast(gy)).sum().backward()
        pr = dict(blk.named_parameters())
        r = {"out": out, "gx": xi.grad}
        r.update({"g/" + k: pr[k].grad for k in names})
        return {k: v.detach().double().cpu().numpy() for k, v in r.items()}

    for rev in (False, True):
        want = run(_restate_block(n, n1, torch.float64), lambda t: t.double().clone(), rev)
        low = run(_restate_block(n, n1, torch.float32), lambda t: t.clone(), rev)
        for fused in (True, False):
            blk = detgen.fill_f2(A.InvBlockExp(S.DenseBlock, n, n1, fused=fused)).cuda()
            got = run(AsNCHW(blk, n), lambda t: t.cuda().clone(), rev)
            for k in want:
                bound = NR.bound_of(NR.maxdiff(low[k], want[k]), float(np.max(np.abs(want[k]))))
                NR.check("InvBlockExp %d/%d rev=%d fused=%d %s" % (n1, n - n1, rev, fused, k), NR.maxdiff(got[k], want[k]), bound)


def test_block_jacobian_is_the_sum_of_s():
    """jacobian() = +-sum(s) / B from the kernel's jac, against the float64 restatement's; detached; refused without the flag"""
    from video_watermarking_forgery_detection_amd import glayers as G
    from video_watermarking_forgery_detection_amd.models.modules import Inv_arch as A
    from video_watermarking_forgery_detection_amd.models.modules import Subnet_constructor as S
    x = detgen.normal((2, 12, 5, 7), 9510, std=0.5)
    blk = detgen.fill_f2(A.InvBlockExp(S.DenseBlock, 12, 3)).cuda()
    for rev in (False, True):
        want, low = (_restate_block(12, 3, dt) for dt in (torch.float64, torch.float32))
        want(x.double(), rev), low(x, rev)
        jw, jl = float(want.jacobian(x, rev).detach()), float(low.jacobian(x, rev).detach())
        xh = G.to_nhwc(x.cuda(), torch.float32)
        blk(xh, rev, cal_jacobian=True)
        j = blk.jacobian(xh, rev)
        assert j.is_cuda and j.dim() == 0 and not j.requires_grad
        NR.check("InvBlockExp jacobian rev=%d" % rev, abs(float(j) - jw), NR.bound_of(abs(jl - jw), abs(jw)))
        blk(xh, rev)
        with pytest.raises(RuntimeError, match="cal_jacobian"):
            blk.jacobian(xh, rev)


def test_reference_format_state_dict_round_trips():
    from video_watermarking_forgery_detection_amd.models.modules import Inv_arch as A
    from video_watermarking_forgery_detection_amd.models.modules import Subnet_constructor as S
    _, ref = IR.build(torch.float32)
    sd = ref.state_dict()
    net = A.InvRescaleNet(3, 3, S.DenseBlock, IR.NET_BLOCKS, IR.NET_DOWN).cuda()
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = net.state_dict()
    assert list(back) == list(sd)
    for k in sd:
        assert torch.equal(back[k].cpu(), sd[k]), k
    x = IR.case_inputs()["net/x"].cuda()
    want = ref.double()(x.double().cpu()).detach().numpy()
    with np.load(GOLDEN) as z:
        NR.check("loaded net(x) vs the restatement", NR.maxdiff(net(x).detach().cpu().numpy(), want), NR.bound_of(float(z["dev32/net/fwd"]), float(z["amax/net/fwd"])))
