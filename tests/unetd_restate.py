"""What tests/test_cpu_unetd.py, tests/test_gpu_unetd.py and tests/golden/make_golden_unetd.py share for the UNetDiscriminator work
(models/networks.py of the reference, :896-1113 and :1387-1421):

  * float64 numpy restatements of nn.ReflectionPad2d and its adjoint, the Bayar constraint (:1059-1061) and the dilated convolution with its
    two gradients.  The adjoint is written in SCATTER form (every padded position is added onto the pixel it mirrors) where the kernel
    (csrc/reflect_pad.hip) gathers, and the convolution as a loop over taps on [B,C,H,W] where the kernel walks NHWC fragments: they share
    no index arithmetic with the code under test;
  * the kernel-level cases and their seeded inputs, the two network cases, their deterministic parameters (detgen, by state_dict key: the
    fixture holds probes of them, not the 330,000 values) and seeded inputs / upstream gradients;
  * the comparison rule: bounds(g, name) and check(label, got, bound).

The rule (as tests/test_gpu_ssim3.py and tests/test_gpu_advloss.py argue it): a quantity's bound is MARGIN = 4 x the
REFERENCE'S OWN float32-vs-float64 deviation of that quantity on the very same inputs, max |f32 - f64| over the whole tensor, stored by the
generator and never calibrated on a kernel: x 2 because the kernels add the same terms in another order than torch's CPU kernels do, x 2
headroom.  Where the stored deviation is (nearly) 0 the bound is at least 2 float32 ulp of the largest |value| of the tensor.
"""
import numpy as np

MARGIN = 4.0

# ----------------------------------------------------------------------------- kernel-level cases
PAD_CASES = {   # name: (B, H, W, CP, p)
    "p2_3x4_c8": (2, 3, 4, 8, 2),      # all three sources of the 3-long axis coincide on its middle pixel
    "p2_3x4_c24": (2, 3, 4, 24, 2),
    "p1_2x5_c8": (2, 2, 5, 8, 1),
    "p1_2x5_c24": (2, 2, 5, 24, 1),
}
CONV_CASES = {  # name: (B, Cin, Cout, IH, IW, pad, dil): 3x3, stride 1
    "c64": (1, 64, 64, 9, 11, 0, 2),   # the ResnetBlock layer: a 5 x 7 map reflection-padded by 2, valid convolution -> 1 x 5 x 7
    "c24_40": (2, 24, 40, 6, 5, 2, 2),  # channel tails on both sides; zero padding 2: taps that fall outside the image -> 2 x 6 x 5
}
BAYAR_CASES = ("pos", "neg")


def _rs(tag, names, name):
    return np.random.RandomState(tag + 10 * sorted(names).index(name))


def pad_inputs(name):
    """x [B,H,W,CP], g [B,H+2p,W+2p,CP] float32"""
    B, H, W, CP, p = PAD_CASES[name]
    rs = _rs(8100, PAD_CASES, name)
    return rs.randn(B, H, W, CP).astype(np.float32), rs.randn(B, H + 2 * p, W + 2 * p, CP).astype(np.float32)


def conv_inputs(name):
    """x [B,Cin,IH,IW], w [Cout,Cin,3,3], g [B,Cout,OH,OW] float32"""
    B, Cin, Cout, IH, IW, pad, dil = CONV_CASES[name]
    OH, OW = IH + 2 * pad - 2 * dil, IW + 2 * pad - 2 * dil
    rs = _rs(8200, CONV_CASES, name)
    x = rs.randn(B, Cin, IH, IW).astype(np.float32)
    w = (rs.randn(Cout, Cin, 3, 3) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    return x, w, rs.randn(B, Cout, OH, OW).astype(np.float32)


def bayar_inputs(name):
    """[3,3,5,5] float32: `pos` every plane sum near +12; `neg` plane (1, 2) negated (sum near -12), plane (2, 0) with mixed signs"""
    rs = _rs(8300, BAYAR_CASES, name)
    w = (rs.rand(3, 3, 5, 5) + 0.5).astype(np.float32)
    if name == "neg":
        w[1, 2] = -w[1, 2]
        w[2, 0, ::2] = -0.25 * w[2, 0, ::2]
    return w


# ----------------------------------------------------------------------------- restatements (float64 unless said otherwise)
def reflect_index(n, p):
    """source index of every padded position of an axis of length n: the edge pixel is not repeated"""
    i = np.arange(-p, n + p)
    return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))


def reflect_pad(x, p):
    """x [B,H,W,C] -> [B,H+2p,W+2p,C]"""
    x = np.asarray(x, np.float64)
    return x[:, reflect_index(x.shape[1], p)][:, :, reflect_index(x.shape[2], p)]


def reflect_pad_adj(g, p):
    """the adjoint, scatter form: g [B,H+2p,W+2p,C] -> [B,H,W,C]"""
    g = np.asarray(g, np.float64)
    H, W = g.shape[1] - 2 * p, g.shape[2] - 2 * p
    out = np.zeros((g.shape[0], H, W, g.shape[3]))
    ry, rx = reflect_index(H, p), reflect_index(W, p)
    for py in range(H + 2 * p):
        for px in range(W + 2 * p):
            out[:, ry[py], rx[px]] += g[:, py, px]
    return out


def pad_terms(n, p):
    """how many padded positions every index of an axis of length n receives from (1..3)"""
    return np.bincount(reflect_index(n, p), minlength=n)


def plane_sums(w25, dtype, order):
    """sums of the rows of w25 [n,25] in `dtype`.  order 'left': plain left to right (np.cumsum: sequential).  order 'torch': what
    torch.sum over the last two axes does for 25 contiguous floats on the CPU (ATen SumKernel.cpp, vectorized_inner_sum with 8-float
    vectors): lane sums l_j = (x[j] + x[j+8]) + x[j+16], then x[24] + l_0 + ... + l_7 from the left"""
    w25 = np.asarray(w25, dtype)
    if order == "left":
        return np.cumsum(w25, axis=1, dtype=dtype)[:, -1]
    lanes = ((w25[:, 0:8] + w25[:, 8:16]).astype(dtype) + w25[:, 16:24]).astype(dtype)
    return np.cumsum(np.concatenate([w25[:, 24:25], lanes], axis=1), axis=1, dtype=dtype)[:, -1]


def bayar(w, dtype=np.float64, order="torch"):
    """the three statements of networks.py:1059-1061 on w [Co,Ci,5,5] in `dtype`: w *= mask; w *= pow(sum(w), -1); w += final; the plane
    sum by plane_sums, the reciprocal rounded, then multiplied"""
    w = np.array(w, dtype).reshape(-1, 25)
    w[:, 12] *= dtype(0)
    s = plane_sums(w, dtype, order)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (w * (dtype(1) / s)).astype(dtype)
    w[:, 12] += dtype(-1)
    return w.reshape(-1, 5, 5)


def _zero_padded(x, pad):
    return np.pad(np.asarray(x, np.float64), [(0, 0), (0, 0), (pad, pad), (pad, pad)])


def dil_conv(x, w, pad, dil):
    """x [B,Cin,IH,IW], w [Cout,Cin,KH,KW] -> [B,Cout,OH,OW], stride 1, zero padding"""
    xp, w = _zero_padded(x, pad), np.asarray(w, np.float64)
    KH, KW = w.shape[2:]
    OH, OW = xp.shape[2] - dil * (KH - 1), xp.shape[3] - dil * (KW - 1)
    out = np.zeros((xp.shape[0], w.shape[0], OH, OW))
    for ky in range(KH):
        for kx in range(KW):
            out += np.einsum("oi,biyx->boyx", w[:, :, ky, kx], xp[:, :, ky * dil:ky * dil + OH, kx * dil:kx * dil + OW])
    return out


def dil_conv_dgrad(g, w, pad, dil, in_hw):
    g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
    KH, KW = w.shape[2:]
    OH, OW = g.shape[2:]
    gp = np.zeros((g.shape[0], w.shape[1], in_hw[0] + 2 * pad, in_hw[1] + 2 * pad))
    for ky in range(KH):
        for kx in range(KW):
            gp[:, :, ky * dil:ky * dil + OH, kx * dil:kx * dil + OW] += np.einsum("oi,boyx->biyx", w[:, :, ky, kx], g)
    return gp[:, :, pad:pad + in_hw[0], pad:pad + in_hw[1]]


def dil_conv_wgrad(g, x, pad, dil, k=3):
    g, xp = np.asarray(g, np.float64), _zero_padded(x, pad)
    OH, OW = g.shape[2:]
    gw = np.zeros((g.shape[1], xp.shape[1], k, k))
    for ky in range(k):
        for kx in range(k):
            gw[:, :, ky, kx] = np.einsum("boyx,biyx->oi", g, xp[:, :, ky * dil:ky * dil + OH, kx * dil:kx * dil + OW])
    return gw


# ----------------------------------------------------------------------------- the network cases
NET_KW = dict(in_channels=3, out_channels=1, residual_blocks=2, use_spectral_norm=True, dim=16, use_sigmoid=True)
NET_CASES = {"srm": dict(use_SRM=True, additional_conv=False), "plain": dict(use_SRM=False, additional_conv=True)}
NET_SHAPE = (2, 3, 20, 28)      # non-square; 1120 output pixels = 17.5 blocks of 64; the bottom level 5 x 7 = 70 pixels, a wave tail, and the
#                                 dilation-2 reflection pad leaves one clear pixel on the axis of 5
BIG = 2048                      # parameter gradients of more elements are stored subsampled
STRIDES = {"e0": 9, "d2": 3, "d1": 9, "x": 1, "gx": 1}     # (coprime with every extent of the tensor: each row, column and channel is visited)


def net_kwargs(name):
    return dict(NET_KW, **NET_CASES[name])


def fill_net(net, name):
    """the case's parameters, by state_dict key (detgen.fill_module: conv weights N(0, 2 / fan_in), biases N(0, 0.1), so the SRM filters are
    random too); spectral-norm u / v normalised as torch leaves them; the Bayar filter 0.04 * (U[0,1) + 0.5): every plane sum near 0.96"""
    import detgen
    import torch
    salt = sorted(NET_CASES).index(name)
    detgen.fill_module(net, salt)
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if k.endswith("weight_u") or k.endswith("weight_v"):
                v.copy_(torch.nn.functional.normalize(v, dim=0, eps=1e-12))
            if k == "BayarConv2D.weight":
                v.copy_(0.04 * (detgen.uniform(tuple(v.shape), detgen.key_seed(k, 7 + salt)) + 0.5))
    return net


def net_inputs(name):
    """(image, upstream gradients of x, d2, d1) float32 torch tensors: the loss of the case is the sum of (output * its gradient).sum()"""
    import detgen
    s = 9500 + 10 * sorted(NET_CASES).index(name)
    B, _, H, W = NET_SHAPE
    dim = NET_KW["dim"]
    return (detgen.uniform(NET_SHAPE, s), detgen.normal((B, NET_KW["out_channels"], H, W), s + 1),
            detgen.normal((B, 2 * dim, H // 2, W // 2), s + 2, std=0.25), detgen.normal((B, dim, H, W), s + 3, std=0.25))


def stride_of(q, numel):
    """the subsampling stride the fixture stores quantity q with (q: 'e0', 'x', 'd2', 'd1', 'gx', 'g/<parameter>', 'after/<buffer>')"""
    if q in STRIDES:
        return STRIDES[q]
    if q.startswith("after/"):
        return 1 if numel <= 256 else 5
    return 1 if numel <= BIG else 61


def conv_stride(numel):
    return 1 if numel <= 8192 else 5


def sub(a, stride):
    return np.asarray(a).reshape(-1)[::stride]


# ----------------------------------------------------------------------------- the comparison rule
def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def bound_of(dev, amax, margin=MARGIN):
    return max(margin * float(dev), 2.0 * ulp32(float(amax)))


def bounds(g, name, kind="dev32"):
    """{quantity: bound} of case `name` from the fixture g: MARGIN x the reference's own deviation (kind 'dev32': float32 against float64;
    'devbf16' / 'devf16': the reference run in that dtype against float64), at least 2 float32 ulp of the tensor's largest |value|"""
    pre = "%s/%s/" % (name, kind)
    return {k[len(pre):]: bound_of(g[k], g["%s/amax/%s" % (name, k[len(pre):])]) for k in g.files if k.startswith(pre)}


def check(label, got, bound):
    """`got` = the largest |difference| found; printed before it is asserted"""
    got = float(got)
    print("%-46s %.3e (bound %.3e, %.2f of it)" % (label, got, bound, got / bound if bound > 0 else float("inf")))
    assert got <= bound, (label, got, bound)
    return got


def maxdiff(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return float(np.max(np.abs(got - want))) if got.size else 0.0
