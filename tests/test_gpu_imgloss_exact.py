"""GPU: the image-loss kernels of csrc/imgloss.hip (wm_recon_*, wm_gradloss_*, wm_excl_*) and csrc/ssim3.hip (wm_ssim3_*, wm_pixloss_*) per
element against float64 (tests/imgloss_exact.py).  Every entry point is called through the checked C ABI handle, so that the per-workgroup
partials, coef and means are seen as the kernels wrote them, with SENTINEL guard elements before and after every destination and every
tensor placed at its own element offset past a 16-byte boundary.

Bit for bit: the guards; on GRID data each workgroup's partial (predicted from the model of split16 / stream16 / wm_groups), coef and the
loss of the streaming kernels; the l2 / l1 and pixel-loss gradients and every accumulate; all of GradientLoss; ExclusionLoss on COUNT
images (each tile's partial = the count of differences whose first pixel it holds, the means); the float4 against the element-by-element
staging of ExclusionLoss; the SSIM_Loss map of equal images; the mean's backward against the map's with the mean's weight.  Bounded, with
bounds counted from the headers' arithmetic: l_char (either of two neighbours next to a rounding boundary), generic data of the streaming
kernels, the ExclusionLoss means, coef, loss and both gradients per pixel, the SSIM_Loss map, partials, mean and both gradients per pixel
(an output at the clamp's bounds counted either way).

Every test prints one line per case -- the worst multiple of a bound and the number of either-way elements -- and a summary per quantity
before it asserts (run with -s).  tests/test_cpu_imgloss_exact.py shows that these comparisons fail on the defects they are there to
catch."""
import time

import numpy as np
import pytest
import torch

import imgloss_exact as IX

pytestmark = pytest.mark.gpu
PAD = 8                                                    # guard elements on either side of a destination


def p(t):
    return None if t is None else t.data_ptr()


def placed(a, off, dtype=torch.float32):
    """a device copy of `a` whose first element lies `off` elements past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype)
    buf = torch.empty(t.numel() + off + 4, dtype=dtype, device="cuda")
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (off * buf.element_size()) % 16
    return view


class Engine:
    """the engine of tests/imgloss_exact.py's drivers: the kernels, each destination inside SENTINEL guards"""

    def __init__(self):
        from video_watermarking_forgery_detection_amd import _lib
        self.L, self.stream = _lib.checked(), torch.cuda.current_stream().cuda_stream
        self.guards, self.case, self.inputs = [], None, {}

    def dev(self, c, name, off=0):
        """the case's float32 input `name` on the device, `off` elements past a 16-byte boundary (kept while the case is the same)"""
        if self.case is not c:
            self.case, self.inputs = c, {}
        if (name, off) not in self.inputs:
            self.inputs[(name, off)] = placed(getattr(c, name), off)
        return self.inputs[(name, off)]

    def dest(self, what, shape, off=0, init=None, dtype=torch.float32):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD + off,), IX.SENTINEL, dtype=dtype, device="cuda")
        view = buf[PAD + off:PAD + off + n].view(shape)
        if init is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float64)).to(dtype))
        if dtype == torch.float32:
            assert view.data_ptr() % 16 == (4 * off) % 16
        self.pending = getattr(self, "pending", []) + [(what, buf, PAD + off, n)]
        return view

    def settle(self):
        """after the launches: the guards of every destination handed out since the last call"""
        for what, buf, lo, n in getattr(self, "pending", []):
            b = IX.f64(buf)
            rest = np.concatenate([b[:lo], b[lo + n:]])
            self.guards.append(IX.ECmp(what + " guards", rest, np.full(rest.shape, IX.SENTINEL)))
        self.pending = []

    def scales(self, m):
        one = lambda v: None if v is None else torch.full((1,), float(v), dtype=torch.float32, device="cuda")  # noqa: E731
        return one(m.get("gout")), float(m.get("gscale", 1.0)), one(m.get("gdev")), int(bool(m.get("accumulate")))

    # ------------------------------------------------------------------------------------------------------------- reconstruction
    def recon_fwd(self, c):
        L = self.L
        assert L.wm_recon_nparts(c.per) == c.P
        x, t = self.dev(c, "x", c.offs[0]), self.dev(c, "t", c.offs[1])
        part = self.dest(c.label + " partials", (c.B * c.P,), dtype=torch.float64)
        loss = self.dest(c.label + " loss", (1,))
        L.wm_recon_sums(p(x), p(t), c.B, c.per, IX.RECON_KINDS[c.kind], c.eps, p(part), self.stream)
        L.wm_recon_finalize(p(part), c.B, c.per, p(loss), self.stream)
        self.settle()
        return part, loss

    def recon_bwd(self, c, m):
        x, t = self.dev(c, "x", c.offs[0]), self.dev(c, "t", c.offs[1])
        gout, gscale, gdev, acc = self.scales(m)
        grad = self.dest("%s grad [%s]" % (c.label, IX.mode_name(m)), (c.B, c.per), c.offs[2], c.old if acc else None)
        self.L.wm_recon_bwd(p(x), p(t), p(grad), c.B, c.per, IX.RECON_KINDS[c.kind], c.eps, p(gout), gscale, p(gdev), acc, self.stream)
        self.settle()
        return grad

    # ------------------------------------------------------------------------------------------------------------- pixel losses
    def pix_in(self, c):
        a = self.dev(c, "a", c.offs[0])
        if c.kind != "maskl1":
            return a, None, None
        return a, self.dev(c, "b", c.offs[1]), self.dev(c, "m", c.offs[2])

    def pix_fwd(self, c):
        L, kind = self.L, IX.PIX_KINDS[c.kind]
        assert L.wm_pixloss_nparts(c.n) == c.P
        a, b, mk = self.pix_in(c)
        part = self.dest(c.label + " partials", (c.P * 2,), dtype=torch.float64)
        coef = self.dest(c.label + " coef", (2,), dtype=torch.float64)
        loss = self.dest(c.label + " loss", (1,))
        L.wm_pixloss_sums(kind, p(a), p(b), p(mk), c.n, p(part), self.stream)
        L.wm_pixloss_finalize(kind, p(part), c.n, p(coef), p(loss), self.stream)
        self.settle()
        return part, coef, loss

    def pix_bwd(self, c, coef, m):
        a, b, mk = self.pix_in(c)
        gout, gscale, gdev, acc = self.scales(m)
        what = "%s %%s [%s]" % (c.label, IX.mode_name(m))
        ga = self.dest(what % "ga", (c.n,), c.offs[3], c.old_a if acc else None) if c.want in ("both", "ga") else None
        gb = self.dest(what % "gb", (c.n,), c.offs[4], c.old_b if acc else None) if c.want in ("both", "gb") else None
        self.L.wm_pixloss_bwd(IX.PIX_KINDS[c.kind], p(a), p(b), p(mk), p(coef), p(ga), p(gb), c.n, p(gout), gscale, p(gdev), acc, self.stream)
        self.settle()
        return ga, gb

    # ------------------------------------------------------------------------------------------------------------- GradientLoss
    def gradl_fwd(self, c):
        L = self.L
        assert L.wm_gradloss_nparts(c.H, c.W) == c.P
        a = self.dev(c, "a")
        part = self.dest(c.label + " partials", (c.N * c.P * 2,), dtype=torch.float64)
        loss = self.dest(c.label + " loss", (1,))
        L.wm_gradloss_sums(p(a), c.N, c.H, c.W, p(part), self.stream)
        L.wm_gradloss_finalize(p(part), c.N, c.H, c.W, p(loss), self.stream)
        self.settle()
        return part, loss

    def gradl_bwd(self, c, m):
        gout, gscale, gdev, acc = self.scales(m)
        grad = self.dest("%s grad [%s]" % (c.label, IX.mode_name(m)), c.a.shape, 0, c.old if acc else None)
        self.L.wm_gradloss_bwd(p(self.dev(c, "a")), p(grad), c.N, c.H, c.W, p(gout), gscale, p(gdev), acc, self.stream)
        self.settle()
        return grad

    # ------------------------------------------------------------------------------------------------------------- ExclusionLoss
    def excl_fwd(self, c, off):
        L = self.L
        assert L.wm_excl_nparts(c.B, c.H, c.W) == c.nwg
        i1, i2 = self.dev(c, "img1", off), self.dev(c, "img2", off)
        tag = "%s off %d" % (c.label, off)
        part = self.dest(tag + " partials", (c.nslots * c.nwg,), dtype=torch.float64)
        means = self.dest(tag + " means", (c.nslots,), dtype=torch.float64)
        coef = self.dest(tag + " coef", (c.nslots,), dtype=torch.float64)
        loss = self.dest(tag + " loss", (1,))
        L.wm_excl_fwd(p(i1), p(i2), c.B, c.C1, c.C2, c.H, c.W, c.levels, p(part), self.stream)
        L.wm_excl_finalize(p(part), c.B, c.C1, c.C2, c.H, c.W, c.levels, p(means), p(coef), p(loss), self.stream)
        self.settle()
        return part, means, coef, loss

    def excl_bwd(self, c, coef, want, m, off):
        i1, i2 = self.dev(c, "img1", off), self.dev(c, "img2", off)
        gout, gscale, gdev, acc = self.scales(m)
        what = "%s off %d %%s [%s]" % (c.label, off, IX.mode_name(m))
        g1 = self.dest(what % "grad1", c.img1.shape, off, c.old1 if acc else None) if want[0] else None
        g2 = self.dest(what % "grad2", c.img2.shape, off, c.old2 if acc else None) if want[1] else None
        self.L.wm_excl_bwd(p(i1), p(i2), p(coef), p(g1), p(g2), c.B, c.C1, c.C2, c.H, c.W, c.levels, p(gout), gscale, p(gdev), acc, self.stream)
        self.settle()
        return g1, g2

    # ------------------------------------------------------------------------------------------------------------- SSIM_Loss
    def ssim3_fwd(self, c):
        L = self.L
        assert L.wm_ssim3_nparts(c.N, c.H, c.W) == c.nparts
        x, y = self.dev(c, "x"), self.dev(c, "y")
        out = self.dest(c.label + " map", c.shape)
        part = self.dest(c.label + " partials", (c.nparts,), dtype=torch.float64)
        mean = self.dest(c.label + " mean", (1,))
        L.wm_ssim3_fwd(p(x), p(y), p(out), p(part), c.N, c.H, c.W, self.stream)       # the map and the partials from one call
        L.wm_ssim3_finalize(p(part), c.N, c.H, c.W, p(mean), self.stream)
        self.settle()
        return out, part, mean

    def ssim3_bwd(self, c, g, want, m):
        x, y = self.dev(c, "x"), self.dev(c, "y")
        gd = None if g is None else placed(g, 0)
        gout, gscale, gdev, acc = self.scales(m)
        what = "%s %s %%s [%s]" % (c.label, "mean's backward" if g is None else "map's backward", IX.mode_name(m))
        gx = self.dest(what % "gx", c.shape, 0, c.old if acc else None) if want[0] else None
        gy = self.dest(what % "gy", c.shape, 0, c.old if acc else None) if want[1] else None
        self.L.wm_ssim3_bwd(p(x), p(y), p(gd), p(gx), p(gy), c.N, c.H, c.W, p(gout), gscale, p(gdev), acc, self.stream)
        self.settle()
        return gx, gy


def run_cases(keys, make, run):
    """one line per case (the worst multiple of a bound, the either-way elements), a summary per quantity, then every assertion"""
    eng = Engine()
    torch.cuda.synchronize()
    t0, worst, cmps = time.perf_counter(), {}, []
    print()
    for key in keys:
        c = make(*key)
        res = run(c, eng)
        mine = IX.flat(res)
        print("   %-78s worst multiple of a bound %.3f, %d either-way elements, %d of %d comparisons fail" % (
            c.label, IX.worst(mine), sum(getattr(x, "either", 0) for x in mine), sum(not x.ok for x in mine), len(mine)))
        for q, cs in res.items():
            for x in cs:
                v, what, nb, ne = worst.get(q, (-1.0, "-", 0, 0))
                worst[q] = (max(v, x.worst), x.what if x.worst >= v else what, nb + (0 if x.exact else x.n), ne + (x.n if x.exact else 0))
        cmps += mine
    torch.cuda.synchronize()
    print("   wall time %.2f s" % (time.perf_counter() - t0))
    for q, (v, what, nb, ne) in sorted(worst.items()):
        print("   %-14s worst multiple of the bound %.3f  over %9d bounded, %9d exact elements  in %s" % (q, max(v, 0.0), nb, ne, what))
    for x in cmps:
        if not x.ok:
            print("   FAILS:", x.line())
    for x in cmps:
        x.assert_ok()
        assert x.skipped == 0


@pytest.mark.parametrize("kind", tuple(IX.RECON_KINDS))
def test_reconstruction_loss_per_element(kind):
    run_cases([k for k in IX.recon_keys() if k[0] == kind], IX.recon_case, IX.run_recon)


@pytest.mark.parametrize("kind", tuple(IX.PIX_KINDS))
def test_pixel_losses_per_element(kind):
    run_cases([k for k in IX.pix_keys() if k[0] == kind], IX.pix_case, IX.run_pix)


@pytest.mark.parametrize("data", IX.GRADL_DATA)
def test_gradient_loss_bit_for_bit(data):
    run_cases([k for k in IX.gradl_keys() if k[3] == data], IX.gradl_case, IX.run_gradl)


@pytest.mark.parametrize("data", IX.EXCL_DATA)
def test_exclusion_loss_per_tile_and_per_pixel(data):
    run_cases([k for k in IX.excl_keys() if k[6] == data], IX.excl_case, IX.run_excl)


@pytest.mark.parametrize("kind", IX.SSIM3_KINDS)
def test_ssim3_loss_per_pixel(kind):
    run_cases([k for k in IX.ssim3_keys() if k[3] == kind], IX.ssim3_case, IX.run_ssim3)
