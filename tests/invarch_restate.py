"""models/modules/Inv_arch.py and Subnet_constructor.DenseBlock of the reference restated for the tests of the HIP modules
(video_watermarking_forgery_detection_amd/models/modules/Inv_arch.py, csrc/invblock.hip).  CPU only, never imports the HIP package.

1. The four modules in torch on the CPU, in any dtype (float64 = the statement), written from their definitions:
     DenseBlock       five 3x3 convolutions over the growing concatenation, LeakyReLU(0.2) after the first four
     HaarDownsampling the +-1 2x2 filters / 4, wavelet-major channel order (k*C + c); rev: the synthesis with the unscaled filters
     InvBlockExp      rev 0: y1 = x1 + F(x2); s = clamp (2 sigmoid(H(y1)) - 1); y2 = x2 exp(s) + G(y1)
                      rev 1: s = clamp (2 sigmoid(H(x1)) - 1); y2 = (x2 - G(x1)) / exp(s); y1 = x1 - F(y2);  jacobian = +-sum(s) / B
     InvRescaleNet    operations forwards then operations_inverse reversed in the opposite direction (AttackNet: the same frame over
                      bare DenseBlocks; its forward cannot run in the reference, only its keys are compared)
   with the reference's state_dict keys, so tests/golden/detgen.fill_f2 fills them exactly as it fills the reference's modules.
   `run_cases` is the one procedure behind the fixture tests/golden/invarch.npz (make_golden_invarch.py runs it on the reference's own
   modules), behind tests/test_cpu_invarch.py (on this restatement) and behind tests/test_gpu_invarch.py (on the HIP modules).

2. A per-element bound model of the two coupling kernels, from tests/gelem_exact.py's pieces, following CouplingCase stage by stage with
   the `+ eps` stage removed (e = ex) and the shift's single rounding added:
     q = 2 sigmoid(h): exp's U ulp through -q*q/2, the sum and the division: 2 roundings;  m = q - 1: 1 rounding on q + 1
     s = clamp * m: |clamp| dm + 1 rounding (none when clamp = 0: s = 0);  ex = exp(s): ex * ds + U ulp
     forward  rev 0: v = ex x + g: |x| dex + 2 roundings on |ex x| + |g|;  rev 1: v = (x - g) / ex: |v| dex / ex + 2 roundings on (|x| + |g|) / ex
     backward de = ex * clamp * 2 * sg * (1 - sg) as CouplingCase;  rev 0: gx = ex go, gg = go, gh = go v de;  rev 1: ge = go / ex, gx = ge,
       gg = -ge, gh = -ge v de (v = the stored output)
     shift    v = x + sign f: 1 rounding on |x| + |f|;  its backward and every pass-through (other, the untouched half of gx): exact
     jac[b]   = sum of s over the sample, summed in double: the per-element ds summed + 1 float32 rounding of the sum
   Padding channels of every input hold SENTINEL (a result that used one is far off); every destination is compared whole, its padding
   channels against exact zeros.
"""
import numpy as np
import torch
import torch.nn as nn

import gelem_exact as GX
from gelem_exact import R, U, Cmp, finish, sigmoid_ref, ulp32  # noqa: F401

SENTINEL = GX.SENTINEL


def cpad(c):
    return (c + 15) // 16 * 16


# ======================================================================================================== 1. the modules
class DenseBlock(nn.Module):
    def __init__(self, channel_in, channel_out, init="xavier", gc=32, bias=True):
        super().__init__()
        for i in range(4):
            setattr(self, "conv%d" % (i + 1), nn.Conv2d(channel_in + i * gc, gc, 3, 1, 1, bias=bias))
        self.conv5 = nn.Conv2d(channel_in + 4 * gc, channel_out, 3, 1, 1, bias=bias)

    def forward(self, x):
        cat = x
        for conv in (self.conv1, self.conv2, self.conv3, self.conv4):
            cat = torch.cat((cat, nn.functional.leaky_relu(conv(cat), 0.2)), 1)
        return self.conv5(cat)


def haar_unscaled(channels):
    w = torch.ones(4, 1, 2, 2)
    w[1, 0, :, 1] = -1
    w[2, 0, 1, :] = -1
    w[3, 0, 1, 0] = -1
    w[3, 0, 0, 1] = -1
    return torch.cat([w] * channels, 0)


class HaarDownsampling(nn.Module):
    def __init__(self, channel_in):
        super().__init__()
        self.channel_in = channel_in
        self.haar_weights = nn.Parameter(haar_unscaled(channel_in), requires_grad=False)

    def forward(self, x, rev=False):
        C = self.channel_in
        if not rev:
            self.last_jac = x.shape[1] * x.shape[2] * x.shape[3] / 4 * np.log(1 / 16.)
            a, b, c, d = x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]
            return torch.cat(((a + b) + (c + d), (a - b) + (c - d), (a + b) - (c + d), (a - b) - (c - d)), 1) / 4.0
        self.last_jac = x.shape[1] * x.shape[2] * x.shape[3] / 4 * np.log(16.)
        k0, k1, k2, k3 = (x[:, k * C:(k + 1) * C] for k in range(4))
        out = x.new_zeros(x.shape[0], C, 2 * x.shape[2], 2 * x.shape[3])
        out[:, :, 0::2, 0::2] = (k0 + k1) + (k2 + k3)
        out[:, :, 0::2, 1::2] = (k0 - k1) + (k2 - k3)
        out[:, :, 1::2, 0::2] = (k0 + k1) - (k2 + k3)
        out[:, :, 1::2, 1::2] = (k0 - k1) - (k2 - k3)
        return out

    def jacobian(self, x, rev=False):
        return self.last_jac


class InvBlockExp(nn.Module):
    def __init__(self, subnet_constructor, channel_num, channel_split_num, clamp=1.):
        super().__init__()
        self.split_len1, self.split_len2, self.clamp = channel_split_num, channel_num - channel_split_num, clamp
        self.F = subnet_constructor(self.split_len2, self.split_len1)
        self.G = subnet_constructor(self.split_len1, self.split_len2)
        self.H = subnet_constructor(self.split_len1, self.split_len2)

    def forward(self, x, rev=False):
        x1, x2 = x[:, :self.split_len1], x[:, self.split_len1:]
        if not rev:
            y1 = x1 + self.F(x2)
            self.s = self.clamp * (2 * torch.sigmoid(self.H(y1)) - 1)
            y2 = x2 * torch.exp(self.s) + self.G(y1)
        else:
            self.s = self.clamp * (2 * torch.sigmoid(self.H(x1)) - 1)
            y2 = (x2 - self.G(x1)) / torch.exp(self.s)
            y1 = x1 - self.F(y2)
        return torch.cat((y1, y2), 1)

    def jacobian(self, x, rev=False):
        return (-self.s.sum() if rev else self.s.sum()) / x.shape[0]


def _frame(channel_in, down_num, blocks):
    ops, c = [], channel_in
    for i in range(down_num):
        ops.append(HaarDownsampling(c))
        c *= 4
        ops.extend(blocks(i, c))
    return nn.ModuleList(ops)


class InvRescaleNet(nn.Module):
    def __init__(self, channel_in=3, channel_out=3, subnet_constructor=None, block_num=(8, 8, 8, 8), down_num=2):
        super().__init__()
        blocks = lambda i, c: [InvBlockExp(subnet_constructor, c, channel_out) for _ in range(block_num[i])]   # noqa: E731
        self.operations = _frame(channel_in, down_num, blocks)
        self.operations_inverse = _frame(channel_in, down_num, blocks)

    def forward(self, x, rev=False, cal_jacobian=False):
        first, second = (self.operations, self.operations_inverse) if not rev else (self.operations_inverse, self.operations)
        out, jac = x, 0
        for op, r in [(op, False) for op in first] + [(op, True) for op in reversed(second)]:
            out = op(out, r)
            if cal_jacobian:
                jac = jac + op.jacobian(out, r)
        return (out, jac) if cal_jacobian else out


class AttackNet(nn.Module):
    def __init__(self, channel_in=3, channel_out=3):
        super().__init__()
        blocks = lambda i, c: [DenseBlock(c, c) for _ in range(4)]   # noqa: E731
        self.operations = _frame(channel_in, 2, blocks)
        self.operations_inverse = _frame(channel_in, 2, blocks)


# ======================================================================================================== the fixture's cases
DB_CIN, DB_COUT, DB_SHAPE = 9, 3, (2, 9, 5, 7)
NET_BLOCKS, NET_DOWN, NET_SHAPE = [1, 1], 2, (2, 3, 8, 12)
DB_GRADS = ("conv1.weight", "conv5.bias")
NET_GRADS = ("operations.1.F.conv1.weight", "operations_inverse.3.H.conv5.bias")
SEED = 9200


def case_inputs():
    """float32 tensors: x, gy of the DenseBlock case; x, y (the reverse's input), the two upstream gradients of the net case"""
    import detgen
    return {"db/x": detgen.normal(DB_SHAPE, SEED), "db/gy": detgen.normal((DB_SHAPE[0], DB_COUT) + DB_SHAPE[2:], SEED + 1),
            "net/x": detgen.normal(NET_SHAPE, SEED + 2, std=0.5), "net/y": detgen.normal(NET_SHAPE, SEED + 3, std=0.5),
            "net/gy_fwd": detgen.normal(NET_SHAPE, SEED + 4), "net/gy_rev": detgen.normal(NET_SHAPE, SEED + 5)}


def _np(t):
    return t.detach().double().cpu().numpy()


def _grads(mod, names):
    p = dict(mod.named_parameters())
    return {k: _np(p[k].grad) for k in names}


def run_cases(db, net, inp, cast, middle):
    """Every stored quantity {name: float64 array} from a filled DenseBlock(9, 3) `db` and InvRescaleNet(3, 3, DenseBlock, [1, 1], 2) `net`
    of ANY implementation (the reference's, this file's, the HIP one).  cast(t): the float32 input as the implementation takes it (dtype,
    device); middle(net, x): the tensor between `operations` and `operations_inverse` of net(x) as NCHW."""
    q = {}
    x = cast(inp["db/x"]).requires_grad_(True)
    out = db(x)
    db.zero_grad()
    (out * cast(inp["db/gy"])).sum().backward()
    q["db/out"], q["db/gx"] = _np(out), _np(x.grad)
    q.update({"db/g/" + k: v for k, v in _grads(db, DB_GRADS).items()})

    x = cast(inp["net/x"]).requires_grad_(True)
    out = net(x)
    net.zero_grad()
    (out * cast(inp["net/gy_fwd"])).sum().backward()
    q["net/fwd"], q["net/fwd_gx"] = _np(out), _np(x.grad)
    q.update({"net/fwd_g/" + k: v for k, v in _grads(net, NET_GRADS).items()})
    with torch.no_grad():
        out2, jac = net(cast(inp["net/x"]), cal_jacobian=True)
        q["net/fwd_with_jac"], q["net/jac"] = _np(out2), _np(torch.as_tensor(jac)).reshape(())
        q["net/mid"] = _np(middle(net, cast(inp["net/x"])))
        q["net/rt"] = _np(net(net(cast(inp["net/x"])), rev=True))
        _, jr = net(cast(inp["net/y"]), rev=True, cal_jacobian=True)
        q["net/rev_jac"] = _np(torch.as_tensor(jr)).reshape(())
    y = cast(inp["net/y"]).requires_grad_(True)
    out = net(y, rev=True)
    net.zero_grad()
    (out * cast(inp["net/gy_rev"])).sum().backward()
    q["net/rev"], q["net/rev_gx"] = _np(out), _np(y.grad)
    q.update({"net/rev_g/" + k: v for k, v in _grads(net, NET_GRADS).items()})
    return q


def middle_nchw(net, x):
    """`middle` of run_cases for NCHW implementations (the reference's and this file's)"""
    out = x
    for op in net.operations:
        out = op(out, False)
    return out


def build(dtype=torch.float64):
    """this file's filled modules in `dtype`: (DenseBlock(9, 3), InvRescaleNet(3, 3, DenseBlock, [1, 1], 2))"""
    import detgen
    db = detgen.fill_f2(DenseBlock(DB_CIN, DB_COUT))
    net = detgen.fill_f2(InvRescaleNet(3, 3, DenseBlock, NET_BLOCKS, NET_DOWN))
    return db.to(dtype), net.to(dtype)


def keys_of(mod):
    return [f"{k}:{tuple(v.shape)}" for k, v in mod.state_dict().items()]


# ======================================================================================================== 2. the kernels' bound model
def _padded(vals, stride, c0=0):
    """[npix, n] float64 -> [npix, stride] with the values at channels [c0, c0 + n) and SENTINEL elsewhere (an input as the kernel gets it)"""
    buf = np.full((vals.shape[0], stride), SENTINEL, dtype=np.float64)
    buf[:, c0:c0 + vals.shape[1]] = vals
    return buf


def _placed(stride, npix, *parts):
    """(reference, bound) [npix, stride]: each part (c0, ref, bound) at its channels, exact zeros elsewhere (an output as it must come back)"""
    ref, b = np.zeros((npix, stride)), np.zeros((npix, stride))
    for c0, r, bb in parts:
        ref[:, c0:c0 + r.shape[1]] = r
        b[:, c0:c0 + r.shape[1]] = bb
    return ref, b


def _data(shape, seed, dt):
    return GX.rnd(GX.normal(shape, seed), dt)


class ShiftCase:
    """wm_invblock_shift and wm_invblock_shift_bwd on npix pixels: inputs as [npix, stride] float64 arrays (values of dtype dt, SENTINEL in
    the padding), every output as (reference, bound) at its full stride"""

    def __init__(self, dt, npix, n1, n2, sign, whole):
        self.dt, self.npix, self.n1, self.n2, self.sign, self.whole = dt, npix, n1, n2, float(sign), bool(whole)
        cp, cp1, cp2 = cpad(n1 + n2), cpad(n1), cpad(n2)
        self.cp, self.cp1, self.cp2 = cp, cp1, cp2
        seed = 9300 + npix + 7 * n2 + (1 if whole else 0)
        x, f, other = _data((npix, n1 + n2), seed, dt), _data((npix, n1), seed + 1, dt), _data((npix, n2), seed + 2, dt)
        self.x, self.f, self.other = _padded(x, cp), _padded(f, cp1), (_padded(other, cp2) if whole else None)
        v = x[:, :n1] + self.sign * f
        bv = R * (np.abs(x[:, :n1]) + np.abs(f))
        parts = [(0, v, bv)] + ([(n1, other, np.zeros_like(other))] if whole else [])
        self.ostride = cp if whole else cp1
        self.out = finish(*_placed(self.ostride, npix, *parts), dt)
        g = _data((npix, n1 + n2 if whole else n1), seed + 3, dt)
        self.g = _padded(g, self.ostride)
        z = np.zeros((npix, n1))
        self.gx = finish(*_placed(cp, npix, (0, g[:, :n1], z)), dt)
        self.gf = finish(*_placed(cp1, npix, (0, self.sign * g[:, :n1], z)), dt)
        self.gother = finish(*_placed(cp2, npix, (0, g[:, n1:], np.zeros((npix, n2)))), dt) if whole else None
        self.label = "invblock_shift %s npix=%d %d/%d sign=%+g %s" % (dt, npix, n1, n2, sign, "whole" if whole else "own")

    def largest_stored(self):
        return float(np.abs(self.out[0]).max())

    def check_fwd(self, out):
        return [Cmp(self.label + " out", out, *self.out)]

    def check_bwd(self, gx, gf, gother):
        c = [Cmp(self.label + " gx", gx, *self.gx), Cmp(self.label + " gf", gf, *self.gf)]
        return c + ([Cmp(self.label + " gother", gother, *self.gother)] if self.whole else [])


class AffineCase:
    """wm_invblock_affine (with jac) and wm_invblock_affine_bwd on B samples of hw pixels.  h starts with 0, 20, -20 (saturation) in
    every channel's first three pixels and mixes a 1/8 grid with normal values after them"""

    def __init__(self, dt, B, hw, n1, n2, rev, whole, clamp):
        self.dt, self.B, self.hw, self.n1, self.n2, self.rev, self.whole = dt, B, hw, n1, n2, int(rev), bool(whole)
        self.clamp = c = float(np.float32(clamp))
        npix = self.npix = B * hw
        cp, cp1, cp2 = cpad(n1 + n2), cpad(n1), cpad(n2)
        self.cp, self.cp1, self.cp2 = cp, cp1, cp2
        seed = 9400 + npix + 7 * n2 + 2 * self.rev + (1 if whole else 0)
        xa, g, other, go = (_data(s, seed + i, dt) for i, s in enumerate(((npix, n1 + n2), (npix, n2), (npix, n1), (npix, n1 + n2))))
        h = GX.grid((npix, n2), seed + 4, 0.125, -2.0, 2.0)
        h[1::2] = GX.rnd(GX.normal(h[1::2].shape, seed + 5, std=2.0), dt)
        h[0], h[1], h[2] = 0.0, 20.0, -20.0
        self.x, self.h, self.g, self.other = _padded(xa, cp), _padded(h, cp2), _padded(g, cp2), (_padded(other, cp1) if whole else None)
        x = xa[:, n1:]
        sg, dsg = sigmoid_ref(h)
        q, dq = 2 * sg, 2 * dsg
        mm = q - 1.0
        dm = dq + R * (q + 1.0)
        s = c * mm
        ds = (abs(c) * dm + R * np.abs(s)) if c != 0 else np.zeros_like(s)
        ex = np.exp(s)
        dex = ex * ds + U["exp"] * ulp32(ex)
        if self.rev:
            v = (x - g) / ex
            bv = np.abs(v) * dex / ex + 2 * R * (np.abs(x) + np.abs(g)) / ex
        else:
            v = ex * x + g
            bv = np.abs(x) * dex + 2 * R * (np.abs(ex * x) + np.abs(g))
        self.ostride, self.vo = (cp, n1) if whole else (cp2, 0)
        parts = [(self.vo, v, bv)] + ([(0, other, np.zeros_like(other))] if whole else [])
        self.out = finish(*_placed(self.ostride, npix, *parts), dt)
        js = s.reshape(B, hw * n2).sum(1)
        self.jac = (js, ds.reshape(B, hw * n2).sum(1) + GX.EPS32 * np.abs(js) + GX.TINY32)
        # ---- backward: the saved tensor is x (rev 0) or the output AS STORED (rev 1), handed to the kernel from here
        if self.rev:
            stored = GX.rnd(v, dt)
            self.v, self.voff, vv = _padded(stored, self.ostride, self.vo), self.vo, stored
        else:
            self.v, self.voff, vv = self.x, n1, x
        gv = go[:, n1:] if whole else go[:, :n2]
        self.gout = _padded(go, cp) if whole else _padded(gv, cp2)
        der = ex * c * 2 * sg * (1 - sg)
        dder = np.abs(c * 2 * sg * (1 - sg)) * dex + np.abs(ex * c * 2) * (dsg * np.abs(1 - 2 * sg) + sg * R * (1 + sg)) + 3 * R * np.abs(der)
        if self.rev:
            ge = gv / ex
            dge = np.abs(ge) * dex / ex + R * np.abs(ge)
            gh = -ge * vv * der
            gx, gg = (ge, dge), (-ge, dge)
            ghb = np.abs(vv * der) * dge + np.abs(ge * vv) * dder + 2 * R * np.abs(gh)
        else:
            gh = gv * vv * der
            gx, gg = (ex * gv, np.abs(gv) * dex + R * np.abs(ex * gv)), (gv, np.zeros_like(gv))
            ghb = np.abs(gv * vv) * dder + 2 * R * np.abs(gh)
        self.gx = finish(*_placed(cp, npix, (n1,) + gx), dt)
        self.gh = finish(*_placed(cp2, npix, (0, gh, ghb)), dt)
        self.gg = finish(*_placed(cp2, npix, (0,) + gg), dt)
        self.gother = finish(*_placed(cp1, npix, (0, go[:, :n1], np.zeros((npix, n1)))), dt) if whole else None
        self.label = "invblock_affine %s B=%d hw=%d %d/%d rev=%d %s clamp=%g" % (dt, B, hw, n1, n2, self.rev, "whole" if whole else "own", clamp)

    def largest_stored(self):
        """the largest |reference| among the outputs stored in the activation type (f16: must stay below 65504)"""
        return float(max(np.abs(t[0]).max() for t in (self.out, self.gx, self.gh, self.gg)))

    def check_fwd(self, out, jac=None):
        c = [Cmp(self.label + " out", out, *self.out)]
        return c + ([Cmp(self.label + " jac", jac, *self.jac)] if jac is not None else [])

    def check_bwd(self, gx, gh, gg, gother):
        c = [Cmp(self.label + " " + k, got, *ref) for k, got, ref in (("gx", gx, self.gx), ("gh", gh, self.gh), ("gg", gg, self.gg))]
        return c + ([Cmp(self.label + " gother", gother, *self.gother)] if self.whole else [])


# n1 / n2.  3 / 9 and 3 / 45 are the reference's; n1 = 4 (f32), 8 (16-bit) and 16 are multiples of the vector, so an operand n1 channels
# off the walk is loaded as vectors at c0 + shift (ld_win's guard i0 >= 0); 19 / 13 has n1 > 16 (two vectors of padding walk) and n2 < n1
SPLITS = ((3, 9), (3, 45), (4, 8), (8, 24), (16, 32), (19, 13))
# (B, hw): 70 pixels = 2 x 5 x 7, no multiple of a block or a vector; 257; B = 5 and 16: jac rows b >= 4 (jac_finalize's b += 4 loop)
PIXELS = ((2, 35), (1, 257), (5, 3), (16, 9))
KERNEL_DTYPES = ("f32", "bf16", "f16")
CLAMPS = (1.0, 0.0)
MAX_F16 = 65504.0
P64_KEY = (1, 5462, 3, 45)              # hw * 48 > 64 * 4096: the jac partial count at its cap of 64
BIG_KEY = (2, 21850, 3, 45)             # 43 700 pixels, f32, misaligned: 43 700 * 48 > 8192 * 256 (a second grid-stride trip of the three
#                                         capped kernels); 21 850 * 48 / 256 > 2048 (the no-jac forward's grid at its cap)


def affine_keys(dt):
    return [(dt, B, hw, n1, n2, rev, whole, clamp) for B, hw in PIXELS for n1, n2 in SPLITS for rev in (0, 1) for whole in (True, False)
            for clamp in CLAMPS]


def shift_keys(dt):
    return [(dt, B * hw, n1, n2, sign, whole) for B, hw in PIXELS for n1, n2 in SPLITS for sign, whole in ((1.0, False), (-1.0, True), (1.0, True), (-1.0, False))]
