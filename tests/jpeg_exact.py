"""Float64 restatement of the block-JPEG attacks (Jpeg / JpegSS / JpegMask) and of DiffJPEG that knows where their discontinuities are,
and the block-by-block comparison built on it.  A plain helper module (no fixtures): used by tests/test_cpu_jpeg_exact.py with the
float32 oracle standing in for the kernels, and by tests/test_gpu_jpeg_exact.py with the kernels.

The restatement is composed from the pieces of oracle/jpeg_ref.py and oracle/diffjpeg_ref.py, applied to one block at a time: every
8x8 block (every 16x16 MCU for DiffJPEG) of the zero-padded image is an image of its own, [N,3,bs,bs].  That is exact, not an
approximation: the colour transforms act per pixel, 4:2:0 replication / averaging stays inside a block, and the DCT is per block.  The
three colour planes of a block belong together because the inverse colour transform mixes them.

    q   = quantise(x_block)                 the DCT coefficients over their table entries (JpegMask: the coefficients themselves)
    r   = rnd(q)                            round | round_ss = round_only_at_0 | diff_round | mask
    rgb = synth(r)                          de-quantise, IDCT, inverse colour transform: the 0..255 scale
    y   = post(rgb)                         / 255 (block JPEG), clamp to [0,255] then / 255 (DiffJPEG)

rnd is discontinuous: in value at q = n + 0.5 (round, diff_round) and at |q| = 0.5 (round_ss: 0.125 -> 0.5), in derivative at |q| = 0.5
(round_ss: 0.75 -> 1).  DiffJPEG's backward also masks the gradient where rgb leaves [0, 255].  A float32 evaluation whose coefficient is
within its round-off of such a point may land on either side, and a whole block follows it.  So a case is compared like this:

  * near items of a block: coefficients with |F - F_jump| <= delta_F (F = q t, the un-divided coefficient, so one delta_F serves every
    table) and, for DiffJPEG's backward, pixels with rgb within delta_F of 0 or 255;
  * strict block (no near item): every pixel within eps of the float64 result.  No exceptions, no shares;
  * near block with k <= 4 items: the whole block (all planes, all pixels, one alternate) within eps of ONE of the 2^k float64
    alternates, each near item taken on either side of its jump;
  * near block with k > 4: skipped and counted.

Conditions that keep the comparison from hiding a failure (Report.conditions_ok): a case of 200 blocks or more has at most 0.5 %
skipped and at least 70 % strict blocks; a smaller case has no skipped block and at least one strict block.  An input that misses them
with the reference alone is drawn again from another seed (build_cases); the conditions are never changed.

delta_F, eps and eps_g are measured on the reference, never on the code under test (measure): the oracle runs in float32 and float64 on
the test's own inputs, delta_F = 4 max |F32 - F64|, eps = 4 max |y32 - y64| over strict blocks, eps_g = 4 max |gx32 - gx64| / max |gx64|
over strict blocks.  The maxima are taken over all inputs of one configuration (mode, Q, subsample): the per-block arithmetic is the same
at every shape, and the maximum over the three pixels of a 1x1 image says little about the round-off of an 8-point DCT.  Factor 4 is
this project's convention (tests/test_gpu_metrics.py): another summation order, FMA contraction, f32 colour constants.
"""
import torch
import torch.nn.functional as F

import detgen
from oracle import diffjpeg_ref, jpeg_ref

KMAX = 4          # a block with more near items is skipped (and counted)
FACTOR = 4.0      # bound = FACTOR x the reference's own float32-vs-float64 deviation
SMALL = 200       # cases with fewer blocks: no skipped block, at least one strict block


# ----------------------------------------------------------------------------------------------------------------- block layout
def to_blocks(img, bs):
    """[B,C,H,W] -> zero-padded to multiples of bs -> [B*nh*nw, C, bs, bs] (block n = (b * nh + block row) * nw + block column)"""
    B, C, H, W = img.shape
    img = F.pad(img, (0, (-W) % bs, 0, (-H) % bs))
    nh, nw = img.shape[2] // bs, img.shape[3] // bs
    return img.reshape(B, C, nh, bs, nw, bs).permute(0, 2, 4, 1, 3, 5).reshape(B * nh * nw, C, bs, bs)


def from_blocks(blk, shape, bs):
    B, C, H, W = shape
    nh, nw = -(-H // bs), -(-W // bs)
    img = blk.reshape(B, nh, nw, C, bs, bs).permute(0, 3, 1, 4, 2, 5).reshape(B, C, nh * bs, nw * bs)
    return img[:, :, :H, :W]


# ----------------------------------------------------------------------------------------------------------------- rounding functions
def _other_integer(q):
    lo = torch.floor(q)
    return 2 * lo + 1 - torch.round(q)      # of floor(q), floor(q) + 1 the one torch.round did not take


def rnd(kind, q, flip, mask=None):
    """value and derivative of the rounding function at q; where `flip` is set, taken on the other side of the nearest jump"""
    if kind == "mask":
        return q * mask, mask.expand_as(q)
    if kind == "round":
        return torch.where(flip, _other_integer(q), torch.round(q)), torch.zeros_like(q)
    if kind == "diff_round":
        r = torch.where(flip, _other_integer(q), torch.round(q))
        return r + (q - r) ** 3, 3 * (q - r) ** 2
    assert kind == "ss"
    inside = (q.abs() < 0.5) ^ flip
    return torch.where(inside, q ** 3, q), torch.where(inside, 3 * q * q, torch.ones_like(q))


def jump_distance(kind, q):
    """distance (in q) to the nearest point where rnd or its derivative jumps"""
    if kind == "mask":
        return torch.full_like(q, float("inf"))
    if kind == "ss":
        return (q.abs() - 0.5).abs()
    return (q - torch.floor(q) - 0.5).abs()


# ----------------------------------------------------------------------------------------------------------------- the two families
class BlockJpeg:
    """noise_layers Jpeg / JpegSS / JpegMask: mode 'round' | 'ss' | 'mask'.  `tables` ([3,8,8], or [N,3,8,8] for one table per block)
    replaces the standard tables of Q: the CPU test plants a wrong table entry with it."""
    bs = 8
    MODE_ID = {"round": 0, "ss": 1, "mask": 2}

    def __init__(self, mode, Q, subsample=0, tables=None):
        self.mode, self.Q, self.subsample = mode, Q, subsample
        self.kind = mode
        self.zero_grad = mode == "round"
        self.clamped = False
        lum, chroma = jpeg_ref.quant_tables(jpeg_ref.scale_factor(Q))
        self.host_tables = lum.flatten().tolist() + chroma.flatten().tolist()      # what ops.jpeg_fwd takes
        self.t = torch.stack([lum, chroma, chroma]) if tables is None else tables
        if mode == "mask":
            self.t = torch.ones(3, 8, 8)
        self.label = "%s Q%d sub%d" % ({"round": "Jpeg", "ss": "JpegSS", "mask": "JpegMask"}[mode], Q, subsample)

    def table(self, dt):
        return self.t.to(dt)

    def quantise(self, xb):
        c = jpeg_ref.dct_matrix().to(xb.dtype)
        yuv = jpeg_ref.subsampling(jpeg_ref.rgb2yuv(xb * 255), self.subsample)
        return torch.matmul(torch.matmul(c, yuv), c.t()) / self.table(xb.dtype)

    def rnd(self, q, flip):
        return rnd(self.kind, q, flip, jpeg_ref.mask_tables().to(q.dtype))

    def synth(self, r):
        c = jpeg_ref.dct_matrix().to(r.dtype)
        return jpeg_ref.yuv2rgb(torch.matmul(torch.matmul(c.t(), r * self.table(r.dtype)), c))

    def oracle(self, x):
        return jpeg_ref.jpeg_layer(x, self.Q, self.mode, self.subsample)


class DiffJpeg:
    """utils.JPEG.DiffJPEG: rounding 0 torch.round | 1 round_only_at_0 | 2 diff_round (the ids of ops.diffjpeg_fwd)"""
    bs = 16
    KINDS = {0: "round", 1: "ss", 2: "diff_round"}
    ORACLE_RND = {0: torch.round, 1: diffjpeg_ref.round_only_at_0, 2: diffjpeg_ref.diff_round}

    def __init__(self, rounding, quality):
        self.rounding, self.quality = rounding, quality
        self.kind = self.KINDS[rounding]
        self.zero_grad = rounding == 0
        self.clamped = True
        self.factor = diffjpeg_ref.quality_to_factor(quality)
        self.t = torch.stack([diffjpeg_ref.Y_TABLE] * 4 + [diffjpeg_ref.C_TABLE] * 2) * self.factor      # [6,8,8]: 4 Y blocks, Cb, Cr
        self.label = "DiffJPEG q%d %s" % (quality, ("round", "round_only_at_0", "diff_round")[rounding])

    def table(self, dt):
        return self.t.to(dt)

    def quantise(self, xb):
        y, cb, cr = diffjpeg_ref.compress(xb, self.factor, lambda d: d)
        return torch.cat([y, cb, cr], 1)

    def rnd(self, q, flip):
        return rnd(self.kind, q, flip)

    def synth(self, r):
        return diffjpeg_ref.decompress_rgb(r[:, :4], r[:, 4:5], r[:, 5:6], 16, 16, self.factor)

    def oracle(self, x):
        return diffjpeg_ref.diffjpeg(x, self.quality, self.ORACLE_RND[self.rounding])


def evaluate(fam, xb, gyb=None, flip=None, pflip=None):
    """one pass over blocks xb [n,3,bs,bs] in xb's dtype -> (y, gx or None, q, rgb).  flip [n,C,8,8] / pflip [n,3,bs,bs] (bool) put
    coefficients / clamp decisions on the other side of their jump.  The derivative of rnd and of the clamp is imposed through a
    first-order surrogate, so autograd returns exactly  analysis^T diag(rnd') synth^T diag(clamp') gy  for the chosen sides."""
    xb = xb.detach().clone().requires_grad_(gyb is not None)
    q = fam.quantise(xb)
    qd = q.detach()
    if flip is None:
        flip = torch.zeros_like(qd, dtype=torch.bool)
    r, dr = fam.rnd(qd, flip)
    rgb = fam.synth(r + dr * (q - qd))
    rd = rgb.detach()
    if fam.clamped:
        inside = (rd >= 0) & (rd <= 255)
        if pflip is not None:
            inside = inside ^ pflip
        y, dy = rd.clamp(0, 255) / 255, inside.to(rd.dtype) / 255
    else:
        y, dy = rd / 255, torch.full_like(rd, 1 / 255)
    if gyb is None:
        return y, None, qd, rd
    if fam.zero_grad:
        return y, torch.zeros_like(y), qd, rd
    (gx,) = torch.autograd.grad(y + dy * (rgb - rd), xb, gyb)
    return y, gx, qd, rd


# ----------------------------------------------------------------------------------------------------------------- one case
class Case:
    """one configuration (BlockJpeg | DiffJpeg) on one input x and upstream gradient gy: everything in float64"""

    def __init__(self, fam, x, gy, name=""):
        self.fam, self.x, self.gy, self.bs = fam, x, gy, fam.bs
        self.shape = tuple(x.shape)
        B, _, H, W = x.shape
        self.nh, self.nw = -(-H // self.bs), -(-W // self.bs)
        self.N = B * self.nh * self.nw
        self.name = name or "%s %dx3x%dx%d" % (fam.label, B, H, W)
        self.xb = to_blocks(x.double(), self.bs)
        self.gyb = to_blocks(gy.double(), self.bs)
        self.valid = to_blocks(torch.ones(B, 1, H, W, dtype=torch.float64), self.bs) > 0
        self.yb, self.gxb, self.q, self.rgb = evaluate(fam, self.xb, self.gyb)
        self.y64 = from_blocks(self.yb, self.shape, self.bs)
        self.gx64 = from_blocks(self.gxb, self.shape, self.bs)
        self.gmax = max(float(self.gx64.abs().max()), 1e-300)
        # the reference's own float32 deviations
        _, _, q32, rgb32 = evaluate(fam, to_blocks(x.float(), self.bs))
        t = fam.table(torch.float64)
        self.coef_dev = float(((q32.double() - self.q).abs() * t).max())
        self._o32 = None
        self.delta = None

    # ---- classification
    def classify(self, delta):
        """near items per block for the forward (coefficients) and the backward (coefficients + clamp pixels)"""
        self.delta = delta
        t = self.fam.table(torch.float64)
        near_c = (jump_distance(self.fam.kind, self.q) * t <= delta).reshape(self.N, -1)
        self.nc = near_c.shape[1]
        if self.fam.clamped and not self.fam.zero_grad:
            near_p = ((torch.minimum(self.rgb.abs(), (self.rgb - 255).abs()) <= delta) & self.valid).reshape(self.N, -1)
        else:
            near_p = torch.zeros(self.N, 3 * self.bs * self.bs, dtype=torch.bool)
        self.near = {"y": torch.cat([near_c, torch.zeros_like(near_p)], 1), "gx": torch.cat([near_c, near_p], 1)}
        if self.fam.zero_grad:      # the gradient is exactly zero on either side of every jump
            self.near["gx"] = torch.zeros_like(self.near["gx"])
        self.k = {w: n.sum(1) for w, n in self.near.items()}
        return self

    def strict(self, which):
        return self.k[which] == 0

    def shares(self, which):
        k = self.k[which]
        return {"blocks": self.N, "strict": int((k == 0).sum()), "near": int(((k > 0) & (k <= KMAX)).sum()), "skipped": int((k > KMAX).sum())}

    def conditions_ok(self):
        for which in ("y", "gx"):
            s = self.shares(which)
            if self.N >= SMALL:
                if s["skipped"] > 0.005 * self.N or s["strict"] < 0.70 * self.N:
                    return False
            elif s["skipped"] or s["strict"] < 1:
                return False
        return True

    # ---- the float32 oracle on the whole image (the reference deviation; the CPU test's stand-in for the kernels)
    def oracle32(self):
        if self._o32 is None:
            x = self.x.float().clone().requires_grad_(True)
            y = self.fam.oracle(x)
            if self.fam.zero_grad:
                gx = torch.zeros_like(y)
            else:
                (gx,) = torch.autograd.grad(y, x, self.gy.float())
            self._o32 = (y.detach(), gx)
        return self._o32

    def block_err(self, img, refb):
        """[N] largest |img - ref| of each block over the pixels inside the image (NaN -> inf)"""
        d = ((to_blocks(img.double(), self.bs) - refb).abs() * self.valid).reshape(self.N, -1)
        return torch.nan_to_num(d, nan=float("inf")).amax(1)

    def ref_dev(self):
        """(max |y32 - y64|, max |gx32 - gx64| / max |gx64|) over the strict blocks"""
        y32, gx32 = self.oracle32()
        ey, eg = self.block_err(y32, self.yb), self.block_err(gx32, self.gxb)
        sy, sg = self.strict("y"), self.strict("gx")
        return (float(ey[sy].max()) if sy.any() else 0.0, float(eg[sg].max()) / self.gmax if sg.any() else 0.0)

    # ---- alternates
    def alternates(self, which, blocks):
        """for blocks (indices, each with 1 <= k <= KMAX near items) yields (c, sel, yb, gxb): alternate number c (bit s set = the
        block's s-th near item on the other side of its jump) of the blocks blocks[sel] -- those with c < 2^k"""
        near = self.near[which][blocks]
        k = near.sum(1)
        assert int(k.min()) >= 1 and int(k.max()) <= KMAX
        order = torch.cumsum(near, 1) - 1                       # slot number of every near item
        for c in range(1 << int(k.max())):
            sel = (1 << k) > c
            bits = near[sel] & (((c >> order[sel].clamp(min=0)) & 1) == 1)
            flip = bits[:, :self.nc].reshape(-1, *self.q.shape[1:])
            pflip = bits[:, self.nc:].reshape(-1, 3, self.bs, self.bs)
            b = blocks[sel]
            yb, gxb, _, _ = evaluate(self.fam, self.xb[b], self.gyb[b], flip, pflip)
            yield c, sel, yb, gxb

    # ---- the comparison
    def compare(self, y, gx, tol):
        rep = Report(self, tol)
        for which, img, refb, eps in (("y", y, self.yb, tol.eps), ("gx", gx, self.gxb, tol.eps_g * self.gmax)):
            if img is None:
                continue
            assert tuple(img.shape) == self.shape, (tuple(img.shape), self.shape)
            img = img.detach().cpu()
            if which == "gx" and self.fam.zero_grad:
                nz = int((img != 0).sum())
                rep.stats[which] = dict(self.shares(which), eps=0.0, worst_strict=float(img.abs().max()))
                if nz:
                    rep.failures.append("%s: gx must be exactly zero (hard rounding), %d elements are not" % (self.name, nz))
                continue
            err = self.block_err(img, refb)
            k = self.k[which]
            strict, near = k == 0, (k > 0) & (k <= KMAX)
            rep.stats[which] = dict(self.shares(which), eps=eps, worst_strict=float(err[strict].max()) if strict.any() else 0.0)
            for n in (strict & ~(err <= eps)).nonzero().flatten().tolist():
                rep.fail(which, n, img, refb[n], eps, "strict block", [("float64", float(err[n]))])
            blocks = near.nonzero().flatten()
            if len(blocks) == 0:
                continue
            sb = to_blocks(img.double(), self.bs)[blocks]
            best = torch.full((len(blocks),), float("inf"), dtype=torch.float64)
            bestc = torch.zeros(len(blocks), dtype=torch.long)
            tried = [[] for _ in blocks]
            for c, sel, yb, gxb in self.alternates(which, blocks):
                alt = yb if which == "y" else gxb
                d = ((sb[sel] - alt).abs() * self.valid[blocks[sel]]).reshape(int(sel.sum()), -1)
                e = torch.nan_to_num(d, nan=float("inf")).amax(1)
                idx = sel.nonzero().flatten()
                better = e < best[idx]
                best[idx] = torch.where(better, e, best[idx])
                bestc[idx] = torch.where(better, torch.full_like(bestc[idx], c), bestc[idx])
                for i, v in zip(idx.tolist(), e.tolist()):
                    tried[i].append(("alternate %d" % c, v))
            rep.flipped[which] = int((bestc != 0).sum())
            for i in (~(best <= eps)).nonzero().flatten().tolist():
                n = int(blocks[i])
                rep.fail(which, n, img, refb[n], eps, "near block (k=%d)" % int(k[n]), tried[i])
        return rep


class Report:
    def __init__(self, case, tol):
        self.case, self.tol, self.stats, self.failures, self.flipped = case, tol, {}, [], {}

    def fail(self, which, n, img, ref_block, eps, what, tried):
        c = self.case
        b, br, bc = n // (c.nh * c.nw), (n // c.nw) % c.nh, n % c.nw
        blk = to_blocks(img.double(), c.bs)[n]
        d = torch.nan_to_num((blk - ref_block).abs() * c.valid[n], nan=float("inf"))
        ch, yy, xx = [int(v) for v in torch.unravel_index(d.argmax(), d.shape)]
        self.failures.append("%s %s: %s batch %d block row %d column %d: worst pixel channel %d y %d x %d (lane row r = %d) off float64 by %.3e "
                             "(eps %.3e); %d pixels of the block above eps; tried %s"
                             % (c.name, which, what, b, br, bc, ch, br * c.bs + yy, bc * c.bs + xx, yy % 8, float(d.max()), eps, int((d > eps).sum()),
                                ", ".join("%s: %.3e" % t for t in tried)))

    @property
    def ok(self):
        return not self.failures

    def line(self):
        out = [self.case.name]
        for which, s in self.stats.items():
            out.append("%s: strict %d near %d skipped %d of %d, eps %.3e, largest deviation on strict blocks %.3e, near blocks on another side %d"
                       % (which, s["strict"], s["near"], s["skipped"], s["blocks"], s["eps"], s["worst_strict"], self.flipped.get(which, 0)))
        return " | ".join(out)

    def assert_ok(self):
        assert self.case.conditions_ok(), "%s: conditions (skipped <= 0.5 %%, strict >= 70 %%) missed: %s" % (
            self.case.name, {w: self.case.shares(w) for w in ("y", "gx")})
        assert self.ok, "%d blocks fail\n" % len(self.failures) + "\n".join(self.failures[:12])


class Tolerances:
    def __init__(self, delta, eps, eps_g, coef_dev, y_dev, g_dev):
        self.delta, self.eps, self.eps_g = delta, eps, eps_g
        self.coef_dev, self.y_dev, self.g_dev = coef_dev, y_dev, g_dev

    def line(self):
        return ("reference f32 vs f64: max |F32 - F64| %.3e, strict-block max |y32 - y64| %.3e, max |gx32 - gx64| / max |gx64| %.3e -> "
                "delta_F %.3e, eps %.3e, eps_g %.3e (relative)" % (self.coef_dev, self.y_dev, self.g_dev, self.delta, self.eps, self.eps_g))


def measure(cases):
    """delta_F, eps, eps_g of one configuration from the reference alone, over all of its inputs; classifies the cases"""
    coef = max(c.coef_dev for c in cases)
    delta = FACTOR * coef
    devs = [c.classify(delta).ref_dev() for c in cases]
    y_dev, g_dev = max(d[0] for d in devs), max(d[1] for d in devs)
    return Tolerances(delta, FACTOR * y_dev, FACTOR * g_dev, coef, y_dev, g_dev)


def fixed_case(fam, x, gy=None):
    """one fixed input (a fixture's): the case, classified, with tolerances measured on it alone"""
    c = Case(fam, x, gy if gy is not None else torch.zeros_like(x))
    return c, measure([c])


def assert_matches_fixture(case, tol, y, ref, atol, gx=None):
    """for a float32 fixture of the reference under hard rounding, instead of a share of pixels that may differ: y passes the block
    comparison against float64, and every strict block is within atol of the fixture (a block may leave the fixture's side only
    where a coefficient sits within delta_F of a tie)"""
    case.compare(y, gx, tol).assert_ok()
    err = case.block_err(y.detach().cpu().double() - torch.as_tensor(ref).double(), torch.zeros_like(case.yb))
    strict = case.strict("y")
    assert bool((err[strict] <= atol).all()), (case.name, float(err[strict].max()))
    return int((err[~strict] > atol).sum())


def build_cases(fam, specs):
    """specs: [(name, make(seed) -> (x, gy))].  Inputs whose case misses the conditions with the reference alone are drawn again from
    another seed (the conditions stay); returns (cases, Tolerances)."""
    tries = [0] * len(specs)
    mk = lambda i: Case(fam, *specs[i][1](tries[i]), name="%s %s" % (fam.label, specs[i][0]))    # noqa: E731
    cases = [mk(i) for i in range(len(specs))]
    for _ in range(12):
        delta = FACTOR * max(c.coef_dev for c in cases)
        bad = [i for i, c in enumerate(cases) if not c.classify(delta).conditions_ok()]
        if not bad:
            return cases, measure(cases)
        for i in bad:
            tries[i] += 1
            cases[i] = mk(i)
    raise AssertionError("no input found that meets the conditions with the reference alone: %s" % [cases[i].name for i in bad])


# ----------------------------------------------------------------------------------------------------------------- the case list
# shape (B, H, W) -> the path of csrc/jpeg.hip it pins (wave_task, load_rows, store_rows)
BLOCK_SHAPES = [
    ((16, 256, 256), "the benchmark's size"),
    ((1, 8, 8), "one block"), ((1, 1, 1), "one block, all but one pixel padding"), ((1, 7, 5), "one block, partly padding"),
    ((2, 9, 64), "exactly one strip, H one row into the second block row"), ((2, 8, 65), "one pixel into the second strip"),
    ((3, 16, 72), "nine blocks per row"),
    ((2, 24, 520), "nine strips per row, float4 path throughout"),
    ((2, 61, 75), "W % 4 != 0: scalar loads, ragged last block"), ((1, 30, 43), "W % 4 != 0"),
    ((2, 40, 68), "W % 4 == 0, last block has x0 + 8 > W: float4 and scalar lanes in one wave"), ((1, 16, 76), "the same, one block row"),
    ((5, 8, 8), "five waves: idle waves in the last workgroup"), ((3, 24, 40), "nine waves"),
    ((2, 31, 33), "4:2:0 replication across the padding on odd sizes"),
]
BLOCK_QS = (10, 50, 90, 100)
# round / ss x Q x subsample; JpegMask has no tables, so one Q covers it
BLOCK_CONFIGS = [(m, q, s) for m in ("round", "ss") for q in BLOCK_QS for s in (0, 2)] + [("mask", 50, 0), ("mask", 50, 2)]
RAGGED_SHAPES = [(2, 8, 65), (2, 24, 520), (2, 61, 75), (1, 30, 43), (2, 40, 68), (1, 16, 76), (1, 7, 5), (2, 31, 33)]     # the act16 test
DIFF_SHAPES = [(1, 16, 16), (2, 16, 48), (2, 48, 80), (3, 32, 272), (16, 256, 256)]
DIFF_QUALITIES = (10, 50, 75, 90)


def _seed(shape, salt):
    B, H, W = shape
    return 1000 * salt + 7 * B + 31 * H + 131 * W


def uniform_spec(shape, lo=0.0, hi=1.0, tag=""):
    B, H, W = shape

    def make(t):
        s = _seed(shape, t)
        return detgen.uniform((B, 3, H, W), s, lo, hi), detgen.normal((B, 3, H, W), s + 500)
    return ("%dx3x%dx%d%s" % (B, H, W, tag), make)


def constant_spec(shape):
    """a constant image (one value per sample and colour plane): every AC coefficient is zero"""
    B, H, W = shape

    def make(t):
        s = _seed(shape, t) + 77
        return detgen.uniform((B, 3, 1, 1), s).expand(B, 3, H, W).contiguous(), detgen.normal((B, 3, H, W), s + 500)
    return ("%dx3x%dx%d constant" % (B, H, W), make)


def table_multiple_image(shape, Q, seed):
    """an image whose coefficients are integer multiples n t of the tables of Q (subsample 0), so every q = n sits as far from a
    rounding tie, and from |q| = 0.5, as it can: x = rgb2yuv^-1 (IDCT(n t)) / 255 in float64, rounded to float32.  H, W multiples of 8."""
    B, H, W = shape
    assert H % 8 == 0 and W % 8 == 0
    lum, chroma = jpeg_ref.quant_tables(jpeg_ref.scale_factor(Q))
    t = torch.stack([lum, chroma, chroma]).double()
    N = B * (H // 8) * (W // 8)
    g = torch.Generator().manual_seed(seed)
    n = torch.zeros(N, 3, 8, 8, dtype=torch.float64)
    n[:, :, :3, :3] = torch.randint(-1, 2, (N, 3, 3, 3), generator=g).double()
    n[:, 0, 0, 0] = torch.round(1024 / t[0, 0, 0]) + torch.randint(-8, 9, (N,), generator=g).double()
    c = jpeg_ref.dct_matrix().double()
    yuv = torch.matmul(torch.matmul(c.t(), n * t), c)
    eye = torch.eye(3, dtype=torch.float64).reshape(1, 3, 3, 1)
    M = jpeg_ref.rgb2yuv(eye)[0, :, :, 0]                       # [out, in]
    rgb = torch.einsum("oi,nihw->nohw", torch.linalg.inv(M), yuv)
    return from_blocks(rgb / 255, (B, 3, H, W), 8).float().contiguous()


def table_multiple_spec(shape, Q):
    B, H, W = shape

    def make(t):
        s = _seed(shape, t) + 99
        return table_multiple_image(shape, Q, s), detgen.normal((B, 3, H, W), s + 500)
    return ("%dx3x%dx%d table multiples" % (B, H, W), make)


def block_specs(Q, big=True):
    """the inputs of one block-JPEG configuration: every shape of the table with a uniform [0,1) image, and at two of the shapes an
    image outside the nominal range, a constant image and an image of table multiples"""
    specs = [uniform_spec(s) for s, _ in BLOCK_SHAPES if big or s[0] * s[1] * s[2] < 500000]
    for s in ((2, 61, 75), (3, 24, 40)):
        specs += [uniform_spec(s, -0.3, 1.4, " in [-0.3,1.4)"), constant_spec(s)]
    specs += [table_multiple_spec((3, 24, 40), Q), table_multiple_spec((2, 8, 64), Q)]
    return specs


def diff_specs(big=True):
    return [uniform_spec(s) for s in DIFF_SHAPES if big or s[0] * s[1] * s[2] < 500000]
