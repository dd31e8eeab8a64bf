"""GPU: the general elementwise kernels (csrc/gelem.hip) and the invertible embedder's pieces (csrc/inn.hip) per element against float64
(tests/gelem_exact.py), at the smallest shapes that take each path: the vector kernels' scalar form by length and by alignment, the second
grid-stride pass above the 4096- and 8192-workgroup caps, the 512- and 64-split caps, the 48-channel tail block, ldv > C, the ELU
derivative from the output, accumulate = 1, hand-placed zeros, smallest normals and saturating arguments, and the f16 twin of everything.

Every bound follows from the number formats, the operation counts and the published accuracy of the device math functions (derived in
tests/gelem_exact.py); copies, gathers, zero fills, one-operation branches and the values around every destination are exact.  Every test
prints one line per comparison (run with -s), the activation tests the largest observed error in float32 ulps per math function, and every
test its wall time.  tests/test_cpu_gelem_exact.py shows that these comparisons fail on the defects they are there to catch.  Where ops.*
hides an argument a case needs (an offset pointer, ldv, accumulate, a stride) the call goes to _lib.lib() directly."""
import time

import numpy as np
import pytest
import torch

import gelem_exact as GX

pytestmark = pytest.mark.gpu


def dev(a, dt="f32"):
    return None if a is None else (a if torch.is_tensor(a) else GX.store(a, dt)).cuda()


def filled(shape, dt):
    return torch.full(shape, GX.SENTINEL, dtype=GX.TORCH[dt], device="cuda")


def report(cmps):
    for c in cmps:
        print("  ", c.line())
    for c in cmps:
        c.assert_ok()


class Clock:
    def __enter__(self):
        print()
        torch.cuda.synchronize()
        self.t = time.perf_counter()

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        print("   wall time %.2f s" % (time.perf_counter() - self.t))


def _mods():
    from video_watermarking_forgery_detection_amd import _lib, ops
    return _lib, ops, _lib.lib(), torch.cuda.current_stream().cuda_stream


def p(t):
    return t.data_ptr()


# ----------------------------------------------------------------------------------------------------------------- activations, add_scaled
ULP_OF = {("fwd", GX.ELU): "expm1 (ELU forward)", ("fwd", GX.TANH): "tanh (Tanh forward)", ("bwd", GX.ELU): "exp (ELU backward, with the product's rounding)",
          ("fwd", GX.GELU): "erf (GELU forward over |0.5 x|, with its three roundings)"}


def _run_unary(c, ulps=None):
    _lib, ops, L, stream = _mods()
    dtid = ops.dt_id(GX.TORCH[c.dt])
    esz = 4 if c.dt == "f32" else 2
    x, g, out = c.buffer(c.x).cuda(), (c.buffer(c.g).cuda() if c.g is not None else None), c.buffer(None).cuda()
    at = lambda t: p(t) + c.off * esz
    assert p(x) % 16 == 0 and p(out) % 16 == 0
    if c.op == "fwd":
        rc = L.wm_unary_fwd(at(x), at(out), c.n, c.kind, dtid, stream)
    elif c.op == "bwd":
        rc = L.wm_unary_bwd(at(x), at(g), at(out), c.n, c.kind, dtid, stream)
    else:
        rc = L.wm_add_scaled(at(x), at(g), at(out), c.n, c.alpha, dtid, stream)
    _lib.check(rc, c.label)
    if ulps is not None and (c.op, c.kind) in ULP_OF:
        k = (ULP_OF[(c.op, c.kind)], c.dt)
        ulps[k] = max(ulps.get(k, 0.0), GX.observed_ulps(c, out))
    return c.check(out)


@pytest.mark.parametrize("dt", GX.DTYPES)
@pytest.mark.parametrize("op", GX.UNARY_OPS)
def test_unary_and_add_scaled(dt, op):
    with Clock():
        ulps = {}
        for key in GX.unary_keys(dt, op):
            report(_run_unary(GX.unary_case(*key), ulps))
        for (fn, d), v in sorted(ulps.items()):
            allowed = GX.U[fn.split()[0]]
            print("   observed ulps %-6s %-62s %.2f (allowance %g; 16-bit: net of the storage half ulp)" % (d, fn, v, allowed))


@pytest.mark.parametrize("op", GX.UNARY_OPS)
def test_unary_above_the_grid_cap(op):
    """4096 * 256 vectors + 5 and 4096 * 256 + 3 scalars, bf16: every thread of the capped grid takes a second trip, a few a third"""
    with Clock():
        for key in GX.unary_cap_keys(op):
            report(_run_unary(GX.unary_case(*key)))


# ----------------------------------------------------------------------------------------------------------------- backward + column sums
@pytest.mark.parametrize("dt", GX.DTYPES)
def test_unary_bwd_colsum(dt):
    _lib, ops, L, stream = _mods()
    dtid = ops.dt_id(GX.TORCH[dt])
    with Clock():
        for key in GX.ubc_keys(dt):
            c = GX.ubc_case(*key)
            x, g, gx, out = dev(c.x, dt), dev(c.g, dt), filled((c.npix, c.C), dt), dev(c.out0)
            nfl = L.wm_unary_bwd_colsum_scratch_floats(c.npix, c.C)
            assert nfl == GX.ubc_nsplit(c.npix) * c.C
            part = torch.full((nfl,), GX.SENTINEL, device="cuda", dtype=torch.float32)
            rc = L.wm_unary_bwd_colsum(p(x), p(g), p(gx), c.npix, c.C, c.kind, p(part), p(out), c.Creal, c.acc, dtid, stream)
            _lib.check(rc, c.label)
            report(c.check(gx, out))


# ----------------------------------------------------------------------------------------------------------------- QFAttention
def _run_qfatt_fwd(c):
    _lib, ops, L, stream = _mods()
    gamma, beta = (t.cuda() for t in c.params())
    x, res, out = dev(c.x, c.dt), dev(c.res, c.dt), filled(c.x.shape, c.dt)
    rc = L.wm_qfatt_fwd(p(x), p(res), p(gamma), p(beta), p(out), c.B, c.hw, c.C, c.ldv, ops.dt_id(GX.TORCH[c.dt]), stream)
    _lib.check(rc, c.label)
    return c.check_fwd(out)


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_qfatt_fwd(dt):
    with Clock():
        for key in GX.qfatt_fwd_keys(dt):
            report(_run_qfatt_fwd(GX.qfatt_case(*key)))
        if dt == "bf16":        # 2 * 8200 * 64 elements: the second trip of the 4096-workgroup grid
            report(_run_qfatt_fwd(GX.QfattCase("bf16", *GX.QF_FWD_CAP, data="pattern")))


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_qfatt_bwd(dt):
    _lib, ops, L, stream = _mods()
    dtid = ops.dt_id(GX.TORCH[dt])
    with Clock():
        for key in GX.qfatt_bwd_keys(dt):
            c = GX.qfatt_case(*key)
            gamma, _ = (t.cuda() for t in c.params())
            g, res, gres = dev(c.g, dt), dev(c.res, dt), filled(c.x.shape, dt)
            gg, gb = filled((c.B, c.ldv), "f32"), filled((c.B, c.ldv), "f32")
            nfl = L.wm_qfatt_bwd_scratch_floats(c.B, c.hw, c.ldv)
            assert nfl == GX.qfatt_nsplit(c.hw) * c.B * 2 * c.ldv
            scratch = torch.full((nfl,), GX.SENTINEL, device="cuda", dtype=torch.float32)
            rc = L.wm_qfatt_bwd(p(g), p(res), p(gamma), p(gres), p(gg), p(gb), p(scratch), c.B, c.hw, c.C, c.ldv, dtid, stream)
            _lib.check(rc, c.label)
            report(c.check_bwd(gres, gg, gb))


@pytest.mark.parametrize("C", [8, 24, 70])
def test_qfatt_bwd_refuses_a_channel_count_its_kernel_cannot_take(C):
    """C % 16 != 0: a last block of fewer than VE channels divides by zero, one of fewer than 16 overruns the LDS rows -- WM_E_BADARG, and
    nothing is launched: every destination keeps its SENTINEL"""
    _lib, ops, L, stream = _mods()
    B, hw, ldv = 2, 5, 80
    for dt in GX.DTYPES:
        g, res, gres = filled((B, hw, ldv), dt), filled((B, hw, ldv), dt), filled((B, hw, ldv), dt)
        gamma, gg, gb = filled((B, ldv), "f32"), filled((B, ldv), "f32"), filled((B, ldv), "f32")
        scratch = filled((L.wm_qfatt_bwd_scratch_floats(B, hw, ldv),), "f32")
        rc = L.wm_qfatt_bwd(p(g), p(res), p(gamma), p(gres), p(gg), p(gb), p(scratch), B, hw, C, ldv, ops.dt_id(GX.TORCH[dt]), stream)
        assert rc == -1, (C, dt, rc)                        # WM_E_BADARG
        torch.cuda.synchronize()
        for t in (gres, gg, gb, scratch):
            assert bool((t == GX.SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------- global average pool
@pytest.mark.parametrize("dt", GX.DTYPES)
def test_gpool(dt):
    _lib, ops, L, stream = _mods()
    dtid = ops.dt_id(GX.TORCH[dt])
    with Clock():
        for key in GX.gpool_keys(dt):
            c = GX.gpool_case(*key)
            x, out = dev(c.x, dt), filled((GX.GP_B, c.C), "f32")
            _lib.check(L.wm_gpool_fwd(p(x), p(out), GX.GP_B, c.hw, c.C, dtid, stream), c.label)
            g, gx = dev(c.g), filled(c.x.shape, dt)
            _lib.check(L.wm_gpool_bwd(p(g), p(gx), GX.GP_B, c.hw, c.C, dtid, stream), c.label)
            report(c.check_fwd(out) + c.check_bwd(gx))


# ----------------------------------------------------------------------------------------------------------------- padding, unpack
@pytest.mark.parametrize("dt", GX.DTYPES)
def test_pad_and_unpack(dt):
    _lib, ops, L, stream = _mods()
    dtid = ops.dt_id(GX.TORCH[dt])
    with Clock():
        for key in GX.pad_keys(dt):
            c = GX.pad_case(*key)
            B, C, H, W = c.shape
            l, r, t, b = c.pads
            x, out = dev(c.x), filled((B, c.PH, c.PW, c.CP), dt)
            _lib.check(L.wm_pad_nchw_to_nhwc(p(x), p(out), B, C, H, W, l, r, t, b, c.mode, c.CP, dtid, stream), c.label)
            gp, gx = dev(c.gp, dt), filled(c.shape, "f32")
            _lib.check(L.wm_pad_nchw_to_nhwc_bwd(p(gp), p(gx), B, C, H, W, l, r, t, b, c.mode, c.CP, dtid, stream), c.label)
            report(c.check_fwd(out) + c.check_bwd(gx))
        for shape, pshape in GX.UNPACK_KEYS:
            c = GX.UnpackCase(dt, shape, pshape)
            B, C, H, W = shape
            PH, PW, CP = pshape
            x, out = dev(c.x, dt), filled(shape, "f32")
            _lib.check(L.wm_gunpack_nchw(p(x), p(out), B, C, H, W, PH, PW, CP, dtid, stream), c.label)
            g, gx = dev(c.g), filled((B, PH, PW, CP), dt)
            _lib.check(L.wm_gunpack_nchw_bwd(p(g), p(gx), B, C, H, W, PH, PW, CP, dtid, stream), c.label)
            report(c.check_fwd(out) + c.check_bwd(gx))


# ----------------------------------------------------------------------------------------------------------------- spectral norm
def _sn_fwd(c, do_iter):
    _lib, ops, L, stream = _mods()
    W, u, v = dev(c.W), dev(c.u0), dev(c.v0)
    sigma, wsn = filled((1,), "f32"), filled((c.M, c.N), "f32")
    scratch = filled((L.wm_spectral_norm_scratch_floats(c.M, c.N),), "f32")
    _lib.check(L.wm_spectral_norm_fwd(p(W), p(u), p(v), p(sigma), p(wsn), p(scratch), c.M, c.N, do_iter, stream), c.label)
    return c.check_fwd(do_iter, u, v, sigma, wsn)


def test_spectral_norm():
    _lib, ops, L, stream = _mods()
    with Clock():
        for M, N in GX.SN_SHAPES:
            c = GX.spectral_case(M, N)
            for it in (0, 1):
                report(_sn_fwd(c, it))
            for acc in (0, 1):
                G, wsn, u, v, sigma = dev(c.G), dev(c.Wsn_in), dev(c.u0), dev(c.v0), dev(np.array([c.sigma_in]))
                gW, partial = dev(c.gW0) if acc else filled((M, N), "f32"), filled((256,), "f32")
                _lib.check(L.wm_spectral_norm_bwd(p(G), p(wsn), p(u), p(v), p(sigma), p(partial), p(gW), M, N, acc, stream), c.label)
                report(c.check_bwd(acc, gW))
        report(_sn_fwd(GX.spectral_case(3, 5, True), 1))


# ----------------------------------------------------------------------------------------------------------------- Haar, channels
def _run_haar(c, x=None):
    _lib, ops, L, stream = _mods()
    x = dev(c.x, c.dt) if x is None else x
    out = filled(c.ref.shape, c.dt)
    _lib.check(L.wm_haar(p(x), p(out), c.B, c.H, c.W, c.C, c.CPin, c.CPout, c.fac, c.up, ops.dt_id(GX.TORCH[c.dt]), stream), c.label)
    return out


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_haar(dt):
    with Clock():
        for key in GX.haar_keys(dt):
            c = GX.haar_case(*key)
            report(c.check(_run_haar(c)))
        for up in (0, 2):       # analysis then synthesis, fac = 0.5 both: the grid input comes back bit for bit, padding channels zero
            a = GX.haar_case(dt, up, 3, 3, 5, 0.5)
            s = GX.HaarCase(dt, up | 1, 3, 3, 5, 0.5, CPin=a.CPout, CPout=a.CPin)
            back = _run_haar(s, _run_haar(a))
            want = np.zeros(a.x.shape)
            want[..., :3] = a.x[..., :3]
            report([GX.Cmp("haar %s round trip up=%d" % (dt, up), back, want)])


def test_haar_above_the_grid_cap():
    B, H, W, C, CPin, CPout = GX.HAAR_CAP
    with Clock():
        c = GX.HaarCase("bf16", 0, C, H, W, 0.5, B=B, CPin=CPin, CPout=CPout, data="pattern")
        report(c.check(_run_haar(c)))


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_chan_copy_and_place(dt):
    _lib, ops, L, stream = _mods()
    dtid = ops.dt_id(GX.TORCH[dt])
    with Clock():
        for key in GX.COPY_KEYS:
            c = GX.ChanCopyCase(dt, *key)
            sstride, soff, dstride, doff, n = key
            src, dst = dev(c.src, dt), filled((GX.CHAN_NPIX, dstride), dt)
            _lib.check(L.wm_chan_copy(p(src), p(dst), GX.CHAN_NPIX, sstride, soff, dstride, doff, n, dtid, stream), c.label)
            report(c.check(dst))
        for key in GX.PLACE_KEYS:
            c = GX.ChanPlaceCase(dt, key)
            astride, aoff, adst, na, bstride, boff, bdst, nb, dstride = key
            a, b, dst = dev(c.a, dt), dev(c.b, dt), filled((GX.CHAN_NPIX, dstride), dt)
            rc = L.wm_chan_place(p(a), astride, aoff, adst, na, None if b is None else p(b), bstride, boff, bdst, nb, p(dst), dstride, GX.CHAN_NPIX, dtid, stream)
            _lib.check(rc, c.label)
            report(c.check(dst))


# ----------------------------------------------------------------------------------------------------------------- affine coupling
def _run_coupling(c):
    _lib, ops, L, stream = _mods()
    dtid = ops.dt_id(GX.TORCH[c.dt])
    x, s, t, g, v = (dev(a, c.dt) for a in (c.x, c.s, c.t, c.g, c.v))
    y, gx, gs, gt = (filled((c.n,), c.dt) for _ in range(4))
    _lib.check(L.wm_coupling_fwd(p(x), p(s), p(t), p(y), c.n, c.clamp, c.eps, c.rev, dtid, stream), c.label)
    _lib.check(L.wm_coupling_bwd(p(g), p(v), p(s), p(gx), p(gs), p(gt), c.n, c.clamp, c.eps, c.rev, dtid, stream), c.label)
    return c.check_fwd(y) + c.check_bwd(gx, gs, gt)


@pytest.mark.parametrize("dt", GX.DTYPES)
def test_coupling(dt):
    with Clock():
        for key in GX.coupling_keys(dt):
            report(_run_coupling(GX.coupling_case(*key)))


def test_coupling_above_the_grid_cap():
    with Clock():
        report(_run_coupling(GX.CouplingCase("bf16", GX.CP_CAP, 0, GX.CP_CLAMP, "pattern")))
