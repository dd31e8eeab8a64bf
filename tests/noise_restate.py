"""Float64 restatement of the stochastic and JPEG-Drop attack layers (noise_layers/dropout.py, crop.py Dropout, gaussian.py,
gaussian_noise.py, salt_pepper_noise.py, jpeg_compression.py of the reference), each taking its random draws as an input, and a numpy
Philox4x32-10 with the stream layout of csrc/noise.hip.  Used by the CPU tests (against tests/golden/noise.npz, the reference's own
outputs for recorded draws) and the GPU tests (against the kernels, fed the draws of wm_rng_fill).  numpy only."""
import math

import numpy as np

U32 = np.uint64(0xFFFFFFFF)
PH_M0, PH_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PH_W0, PH_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """ctr: uint32 array [..., 4], key: (k0, k1) python ints -> uint32 array [..., 4] (Salmon et al. SC'11, 10 rounds)"""
    c = [ctr[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + PH_W0) & 0xFFFFFFFF, (k1 + PH_W1) & 0xFFFFFFFF
        p0, p1 = PH_M0 * c[0], PH_M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & U32]
    return np.stack(c, axis=-1).astype(np.uint32)


def words(seed, offset, n):
    """the n 32-bit words of elements 0..n-1 at (seed, offset): element i = word i % 4 of the block with counter (i / 4, offset)"""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q & U32, q >> np.uint64(32), np.full_like(q, offset & 0xFFFFFFFF), np.full_like(q, offset >> 32)], axis=-1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]


def uniform(seed, offset, n):
    """float32 in [0,1): (w >> 8) * 2^-24 -- what the kernels draw, bit for bit"""
    return ((words(seed, offset, n) >> 8).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def normal(seed, offset, n):
    """float64 Box-Muller on the word pairs (0,1), (2,3) of each block: the kernels' f32 logf / sincosf agree to a few ulp"""
    m = (n + 3) // 4 * 4
    w = words(seed, offset, m).reshape(-1, 2, 2).astype(np.uint64)
    u1 = ((w[..., 0] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (w[..., 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    t = np.float64(np.float32(2 * math.pi)) * u2
    r = np.sqrt(-2.0 * np.log(u1))
    return np.stack([r * np.cos(t), r * np.sin(t)], axis=-1).reshape(-1)[:n]


def f32(v):
    return float(np.float32(v))


# ----------------------------------------------------------------------------- the layers, draws given
def dropout_keep(u0, keep_min, keep_max):
    """dropout.Dropout's keep ratio from its uniform draw, as the kernel forms it: fma(f32(max - min), u0, f32(min)) rounded once"""
    return np.float32(np.float64(np.float32(keep_min)) + np.float64(np.float32(keep_max - keep_min)) * np.float64(u0))


def dropout(x, cover, mask):
    """dropout.py:20-26: mask [H,W] in {0,1} shared over B and C; returns (y, d y/d x, d y/d cover) -- the two gradients as multipliers"""
    m = np.broadcast_to(mask.astype(np.float64), x.shape)
    y = x.astype(np.float64) * m + cover.astype(np.float64) * (1 - m)
    return y.astype(np.float32), m, 1 - m


def crop_dropout(x, cover, u, prob):
    """crop.py:144-146: where(u > prob, cover, image), prob compared in f32"""
    sel = u > np.float32(prob)
    return np.where(sel, cover, x).astype(np.float32), (~sel).astype(np.float64), sel.astype(np.float64)


def gauss_noise(z, mean, std):
    """the kernels' noise: fma(f32 std, z, f32 mean), one rounding (z the f32 normal draw)"""
    return (np.float64(np.float32(std)) * z.astype(np.float64) + np.float64(np.float32(mean))).astype(np.float32)


def gaussian(x, noise):
    """gaussian.py:12-16: clamp(x + noise, 0, 1); the gradient passes where 0 <= x + noise <= 1"""
    s = (x.astype(np.float64) + noise.astype(np.float64)).astype(np.float32)
    return np.clip(s, 0, 1).astype(np.float32), ((s >= 0) & (s <= 1)).astype(np.float64)


def gn(x, noise):
    """gaussian_noise.py:13-15: x + noise (noise already f32); gradient 1"""
    return (x.astype(np.float64) + noise.astype(np.float64)).astype(np.float32)


def salt_pepper(x, u, prob):
    """salt_pepper_noise.py:10-19, thresholds compared in f32"""
    lo, hi = np.float32(prob / 2), np.float32(1 - prob / 2)
    y = np.where(u > hi, np.float32(0), x)
    y = np.where(u < lo, np.float32(1), y)
    return y.astype(np.float32), ((u <= hi) & (u >= lo)).astype(np.float64)


# ----------------------------------------------------------------------------- JpegCompression
RGB2YUV = np.array([[0.299, 0.587, 0.114], [-0.14713, -0.28886, 0.436], [0.615, -0.51499, -0.10001]])
YUV2RGB = np.array([[1.0, 0.0, 1.13983], [1.0, -0.39465, -0.58060], [1.0, 2.03211, 0.0]])


def dct_mats():
    k, n = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    C = np.cos(np.pi / 8 * (n + 0.5) * k)                               # C[k][n]: coefficient k from sample n (dct_coeff)
    D = ((n == 0) * -0.5 + np.cos(np.pi / 8 * (k + 0.5) * n)) * np.sqrt(1 / 16.0)   # D[k][n]: sample k from coefficient n (idct_coeff)
    return C, D


def zigzag_mask(count):
    order = sorted(((x, y) for x in range(8) for y in range(8)), key=lambda p: (p[0] + p[1], -p[1] if (p[0] + p[1]) % 2 else p[1]))
    m = np.zeros((8, 8))
    for i, j in order[:count]:
        m[i, j] = 1
    return m


def _blocks(x):
    B, Cc, H, W = x.shape
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    p = np.zeros((B, Cc, Hp, Wp))
    p[:, :, :H, :W] = x
    return p.reshape(B, Cc, Hp // 8, 8, Wp // 8, 8), (H, W)


def _unblock(b, hw):
    B, Cc, hb, _, wb, _ = b.shape
    return b.reshape(B, Cc, hb * 8, wb * 8)[:, :, :hw[0], :hw[1]]


def jpeg_compression(x, keep=(25, 9, 9), adjoint=False, absolute=False):
    """jpeg_compression.py:126-159 in float64; adjoint=True: the transpose map; absolute=True: every matrix by its absolute value (the
    magnitude chain |yuv2rgb| |D| |D| mask |C| |C| |rgb2yuv| |x| that bounds the rounding error of an f32 evaluation)"""
    C, D = dct_mats()
    A, Bm = RGB2YUV, YUV2RGB
    if adjoint:
        A, Bm, C, D = YUV2RGB.T, RGB2YUV.T, D.T, C.T
    if absolute:
        A, Bm, C, D = abs(A), abs(Bm), abs(C), abs(D)
    mask = np.stack([zigzag_mask(k) for k in keep])                    # [3, 8, 8], (row frequency, column frequency)
    b, hw = _blocks(np.asarray(x, np.float64))
    v = np.einsum("ij,bjhywx->bihywx", A, b)
    v = np.einsum("ky,bchywx,lx->bchkwl", C, v, C)
    v = v * mask[None, :, None, :, None, :]
    v = np.einsum("ky,bchywx,lx->bchkwl", D, v, D)
    v = np.einsum("ij,bjhywx->bihywx", Bm, v)
    return _unblock(v, hw)


# f32 evaluation of the chain: colour (3 terms) . 8-point transform x 4 (8 terms each) . colour (3 terms) = 38 rounded accumulations on the
# longest path, plus one rounding of each of the 6 matrices to f32 -> |y_f32 - y| <= gamma_44 |chain|(|x|), gamma_n = n u / (1 - n u),
# u = 2^-24.  The reference evaluates each 2-D transform as one 64-tap conv2d (64 + 64 + 3 + 3 = 134 accumulations, + 6): gamma_140 bounds
# either evaluation.
JPEG_GAMMA_N = 140


def jpeg_bound(x, keep=(25, 9, 9), adjoint=False):
    u = 2.0 ** -24
    g = JPEG_GAMMA_N * u / (1 - JPEG_GAMMA_N * u)
    return g * jpeg_compression(np.abs(np.asarray(x, np.float64)), keep, adjoint=adjoint, absolute=True)
