"""The Swin block of the reference's network/SUNet_detail.py restated for the tests of the HIP modules
(video_watermarking_forgery_detection_amd/network/SUNet_detail.py, csrc/swin.hip).  CPU only, never imports the HIP package.

1. The rule the attention kernel computes instead of reading tensors: rel_index_rule(ws) and mask_rule(H, W, ws, shift), written as the
   kernel writes them (per token pair, from window coordinates and region ids of the rolled grid), and token_of(): where window token n lives
   on the un-rolled grid.  tests/test_cpu_swin.py holds them against the reference's buffers stored in the fixture.
2. Float64 numpy statements: layernorm64 / layernorm_bwd64, attention_core64 / attention_core_bwd64 (on the token grid, through the rule).
3. The modules in torch on the CPU in any dtype with the reference's state_dict keys (Mlp, WindowAttention, SwinTransformerBlock,
   BasicLayer), their index and mask buffers made by the rule; `run_cases` is the one procedure behind tests/golden/swin.npz
   (make_golden_swin.py runs it on the reference's own modules), tests/test_cpu_swin.py (this restatement) and tests/test_gpu_swin.py (HIP).
4. Per-element bound models of the kernels (LnCase, AttnCase), built as tests/gelem_exact.py builds them: a float32 result formed with k
   roundings is accepted within R * k * (sum of |terms|), R = FACTOR * 2**-24; expf / logf take U ulps of their result, propagated through
   the expression that uses them; an operand rounded to bf16 / f16 for the MFMA adds half an ulp of that type; a stored value adds its
   store rounding (finish).  Probabilities below the float32 normal range may be flushed: MIN_NORMAL is added to every probability's bound.
   f16 is the same model with half_ulp(., "f16"): 2**-11 relative and never below 2**-25, the half-spacing of the subnormals that P and
   dS reach below 2**-14 as operands; the data keeps every stored value below 65504 (largest_stored(), asserted in tests/test_cpu_swin.py).
   tests/test_cpu_swin.py holds float32 imitations of the kernels that pass these models and named defects that fail them.
"""
import numpy as np
import torch
import torch.nn as nn

import gelem_exact as GX
from gelem_exact import R, U, Cmp, finish, half_ulp, ulp32  # noqa: F401

SENTINEL = GX.SENTINEL
EPS = 1e-5
MIN_NORMAL = 2.0 ** -126


def cpad(c):
    return (c + 15) // 16 * 16


# ======================================================================================================== 1. the kernel's rule
def rel_index_rule(ws):
    """[N, N] int64: (iy - jy + ws - 1) * (2 ws - 1) + (ix - jx + ws - 1)"""
    n = np.arange(ws * ws)
    iy, ix = n // ws, n % ws
    return (iy[:, None] - iy[None, :] + ws - 1) * (2 * ws - 1) + (ix[:, None] - ix[None, :] + ws - 1)


def region_rule(L, ws, shift, pos):
    """region of coordinate `pos` of an axis of length L on the rolled grid: [0, L - ws) -> 0, [L - ws, L - shift) -> 1, the rest -> 2"""
    return np.where(pos < L - ws, 0, np.where(pos < L - shift, 1, 2))


def mask_rule(H, W, ws, shift):
    """[nW, N, N] float64: -100 where the two tokens' region ids differ (zeros for shift 0); windows in row-major order"""
    n = np.arange(ws * ws)
    out = np.zeros((H // ws * (W // ws), ws * ws, ws * ws))
    if shift == 0:
        return out
    for wy in range(H // ws):
        for wx in range(W // ws):
            rid = region_rule(H, ws, shift, wy * ws + n // ws) * 3 + region_rule(W, ws, shift, wx * ws + n % ws)
            out[wy * (W // ws) + wx] = np.where(rid[:, None] != rid[None, :], -100.0, 0.0)
    return out


def token_of(H, W, ws, shift):
    """[nW, N, 2] int: (y, x) on the un-rolled grid of token n of window w of the grid rolled by -shift"""
    n = np.arange(ws * ws)
    out = np.zeros((H // ws * (W // ws), ws * ws, 2), dtype=np.int64)
    for wy in range(H // ws):
        for wx in range(W // ws):
            out[wy * (W // ws) + wx, :, 0] = (wy * ws + n // ws + shift) % H
            out[wy * (W // ws) + wx, :, 1] = (wx * ws + n % ws + shift) % W
    return out


# ======================================================================================================== 2. float64 statements
def layernorm64(x, gamma, beta, eps=EPS):
    """x [T, C] -> (y, xhat, mean, rstd)"""
    x = np.asarray(x, np.float64)
    mean = x.mean(1, keepdims=True)
    var = ((x - mean) ** 2).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean) * rstd
    return xhat * gamma[None] + beta[None], xhat, mean, rstd


def layernorm_bwd64(x, g, gamma, eps=EPS):
    _, xhat, _, rstd = layernorm64(x, gamma, np.zeros_like(gamma), eps)
    gg = g * gamma[None]
    dx = rstd * (gg - gg.mean(1, keepdims=True) - xhat * (gg * xhat).mean(1, keepdims=True))
    return dx, (g * xhat).sum(0), g.sum(0)


def gather_windows(t, H, W, ws, shift, nH):
    """grid [B,H,W,nH*hd] -> [B, nW, nH, N, hd] through token_of"""
    tok = token_of(H, W, ws, shift)
    B = t.shape[0]
    w = t[:, tok[..., 0], tok[..., 1]]                       # [B, nW, N, nH*hd]
    return w.reshape(B, tok.shape[0], ws * ws, nH, -1).transpose(0, 1, 3, 2, 4)


def scatter_windows(w, H, W, ws, shift):
    """[B, nW, nH, N, hd] -> grid [B,H,W,nH*hd]"""
    tok = token_of(H, W, ws, shift)
    B, nW, nH, N, hd = w.shape
    out = np.zeros((B, H, W, nH * hd))
    out[:, tok[..., 0], tok[..., 1]] = w.transpose(0, 1, 3, 2, 4).reshape(B, nW, N, nH * hd)
    return out


def scores64(qkv, table, nH, ws, shift, scale):
    """qkv grid [B,H,W,3C] -> (q, k, v [B,nW,nH,N,hd], S [B,nW,nH,N,N])"""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    q, k, v = (gather_windows(qkv[..., i * C:(i + 1) * C], H, W, ws, shift, nH) for i in range(3))
    bias = table[rel_index_rule(ws)].transpose(2, 0, 1)      # [nH, N, N]
    S = scale * np.einsum("bwhid,bwhjd->bwhij", q, k) + bias[None, None] + mask_rule(H, W, ws, shift)[None, :, None]
    return q, k, v, S


def softmax64(S):
    m = S.max(-1, keepdims=True)
    e = np.exp(S - m)
    return e / e.sum(-1, keepdims=True)


def attention_core64(qkv, table, nH, ws, shift, scale):
    """the attention core on the token grid: qkv [B,H,W,3C] float64 -> out [B,H,W,C]"""
    _, H, W, _ = qkv.shape
    q, k, v, S = scores64(np.asarray(qkv, np.float64), np.asarray(table, np.float64), nH, ws, shift, scale)
    return scatter_windows(np.einsum("bwhij,bwhjd->bwhid", softmax64(S), v), H, W, ws, shift)


def attention_core_bwd64(qkv, table, gout, nH, ws, shift, scale):
    """(g_qkv [B,H,W,3C], g_table [(2ws-1)^2, nH])"""
    B, H, W, C3 = qkv.shape
    q, k, v, S = scores64(np.asarray(qkv, np.float64), np.asarray(table, np.float64), nH, ws, shift, scale)
    P = softmax64(S)
    dO = gather_windows(np.asarray(gout, np.float64), H, W, ws, shift, nH)
    A = np.einsum("bwhid,bwhjd->bwhij", dO, v)
    dS = P * (A - (P * A).sum(-1, keepdims=True))
    dV = np.einsum("bwhij,bwhid->bwhjd", P, dO)
    dQ = scale * np.einsum("bwhij,bwhjd->bwhid", dS, k)
    dK = scale * np.einsum("bwhij,bwhid->bwhjd", dS, q)
    gq = np.concatenate([scatter_windows(t, H, W, ws, shift) for t in (dQ, dK, dV)], -1)
    gt = np.zeros(table.shape)
    np.add.at(gt, rel_index_rule(ws).reshape(-1), dS.sum((0, 1)).transpose(1, 2, 0).reshape(ws ** 4, nH))
    return gq, gt


# ======================================================================================================== 3. the modules
def window_partition(x, ws):
    B, H, W, C = x.shape
    return x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C)


def window_reverse(windows, ws, H, W):
    B = windows.shape[0] // (H * W // ws // ws)
    return windows.view(B, H // ws, W // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)

    def forward(self, x):
        return self.fc2(nn.functional.gelu(self.fc1(x)))


class WindowAttention(nn.Module):
    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None):
        super().__init__()
        self.dim, self.ws, self.num_heads = dim, window_size[0], num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * self.ws - 1) ** 2, num_heads))
        self.register_buffer("relative_position_index", torch.from_numpy(rel_index_rule(self.ws)))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x, mask=None):
        B_, N, C = x.shape
        qkv = self.qkv(x).reshape(B_, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        attn = (qkv[0] * self.scale) @ qkv[1].transpose(-2, -1)
        bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(N, N, -1).permute(2, 0, 1)
        attn = attn + bias.unsqueeze(0)
        if mask is not None:
            nW = mask.shape[0]
            attn = (attn.view(B_ // nW, nW, self.num_heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, self.num_heads, N, N)
        return self.proj((attn.softmax(-1) @ qkv[2]).transpose(1, 2).reshape(B_, N, C))


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, input_resolution, num_heads, window_size=7, shift_size=0, mlp_ratio=4., qkv_bias=True, qk_scale=None):
        super().__init__()
        self.dim, self.input_resolution, self.window_size, self.shift_size = dim, input_resolution, window_size, shift_size
        if min(input_resolution) <= window_size:
            self.shift_size, self.window_size = 0, min(input_resolution)
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, (self.window_size, self.window_size), num_heads, qkv_bias, qk_scale)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))
        H, W = input_resolution
        self.register_buffer("attn_mask", torch.from_numpy(mask_rule(H, W, self.window_size, self.shift_size)).float() if self.shift_size > 0 else None)

    def forward(self, x):
        H, W = self.input_resolution
        B, L, C = x.shape
        s, ws = self.shift_size, self.window_size
        g = self.norm1(x).view(B, H, W, C)
        if s:
            g = torch.roll(g, shifts=(-s, -s), dims=(1, 2))
        a = self.attn(window_partition(g, ws).view(-1, ws * ws, C), mask=self.attn_mask)
        g = window_reverse(a.view(-1, ws, ws, C), ws, H, W)
        if s:
            g = torch.roll(g, shifts=(s, s), dims=(1, 2))
        x = x + g.view(B, H * W, C)
        return x + self.mlp(self.norm2(x))


class BasicLayer(nn.Module):
    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio=4., qkv_bias=True, qk_scale=None):
        super().__init__()
        self.blocks = nn.ModuleList([SwinTransformerBlock(dim, input_resolution, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2,
                                                          mlp_ratio, qkv_bias, qk_scale) for i in range(depth)])

    def forward(self, x):
        for b in self.blocks:
            x = b(x)
        return x


# ======================================================================================================== the fixture's cases
BATCH = 2
SEED = 9600
# name: (kind, constructor keywords); the third block asks for window 8 and shift 3 on a 4 x 4 grid: it collapses to window 4, shift 0
CASES = {
    "blk1": ("block", dict(dim=24, input_resolution=(8, 8), num_heads=2, window_size=4, shift_size=2, qk_scale=8)),
    "blk2": ("block", dict(dim=24, input_resolution=(14, 7), num_heads=2, window_size=7, shift_size=3)),
    "blk3": ("block", dict(dim=16, input_resolution=(4, 4), num_heads=2, window_size=8, shift_size=3)),
    "layer": ("layer", dict(dim=24, input_resolution=(8, 8), depth=2, num_heads=2, window_size=4)),
}
BLOCK_GRADS = ("attn.relative_position_bias_table", "attn.qkv.weight", "norm1.weight", "mlp.fc2.bias")
LAYER_GRADS = ("blocks.1.attn.relative_position_bias_table", "blocks.1.attn.qkv.weight", "blocks.0.norm1.weight", "blocks.0.mlp.fc2.bias")
CORE_CASES = ("blk1", "blk2")       # the blocks whose attention core (qkv -> out on the grid) is stored on its own


def geometry(name):
    """(H, W, C, heads, effective window, effective shift, scale) of a block case"""
    kw = CASES[name][1]
    H, W = kw["input_resolution"]
    ws, s = kw["window_size"], kw.get("shift_size", 0)
    if min(H, W) <= ws:
        ws, s = min(H, W), 0
    hd = kw["dim"] // kw["num_heads"]
    return H, W, kw["dim"], kw["num_heads"], ws, s, kw.get("qk_scale") or hd ** -0.5


@torch.no_grad()
def fill_swin(mod):
    """detgen.fill_module by state_dict key (the bias table is two-dimensional: N(0, sqrt(2 / heads)), far from the reference's std .02),
    the index and mask buffers kept"""
    import detgen
    keep = {k: v.clone() for k, v in mod.state_dict().items() if k.endswith("relative_position_index") or k.endswith("attn_mask")}
    detgen.fill_module(mod)
    sd = mod.state_dict()
    for k, v in keep.items():
        sd[k].copy_(v)
    return mod


def case_inputs():
    import detgen
    out = {}
    for i, (name, (_, kw)) in enumerate(CASES.items()):
        H, W = kw["input_resolution"]
        out[name + "/x"] = detgen.normal((BATCH, H * W, kw["dim"]), SEED + 2 * i)
        out[name + "/gy"] = detgen.normal((BATCH, H * W, kw["dim"]), SEED + 2 * i + 1)
    return out


def _np(t):
    return t.detach().double().cpu().numpy()


def run_cases(mods, inp, cast):
    """every stored quantity {name: float64 array} from filled modules {case: module} of ANY implementation; cast(t): the float32 input as
    the implementation takes it"""
    q = {}
    for name, (kind, _) in CASES.items():
        m = mods[name]
        x = cast(inp[name + "/x"]).requires_grad_(True)
        out = m(x)
        m.zero_grad()
        (out * cast(inp[name + "/gy"])).sum().backward()
        q[name + "/out"], q[name + "/gx"] = _np(out), _np(x.grad)
        p = dict(m.named_parameters())
        for k in (BLOCK_GRADS if kind == "block" else LAYER_GRADS):
            q[name + "/g/" + k] = _np(p[k].grad)
    return q


def build(classes, param_dtype=torch.float64, **extra):
    """{case: filled module} from (SwinTransformerBlock, BasicLayer) classes of any implementation; extra: further constructor keywords"""
    blk, layer = classes
    return {name: fill_swin((blk if kind == "block" else layer)(**kw, **extra)).to(param_dtype) for name, (kind, kw) in CASES.items()}


def keys_of(mod):
    return [f"{k}:{tuple(v.shape)}" for k, v in mod.state_dict().items()]


# ======================================================================================================== 4. the kernels' bound models
def _padded(vals, stride):
    buf = np.full(vals.shape[:-1] + (stride,), SENTINEL, dtype=np.float64)
    buf[..., :vals.shape[-1]] = vals
    return buf


def _placed(ref, bound, stride):
    r, b = np.zeros(ref.shape[:-1] + (stride,)), np.zeros(ref.shape[:-1] + (stride,))
    r[..., :ref.shape[-1]], b[..., :ref.shape[-1]] = ref, bound
    return r, b


def sum_bound(n, absum):
    """any-order float32 sum of n terms"""
    return R * (n + 1) * absum + GX.TINY32


class LnCase:
    """wm_layernorm_fwd / wm_layernorm_bwd on T tokens of C channels: row 0 constant (variance 0), row T - 1 = 1000 + N(0, 1)
    (cancellation) when T > 1; padding channels of every input hold SENTINEL, every output is compared whole (padding: exact zeros)"""

    def __init__(self, dt, T, C):
        self.dt, self.T, self.C, self.cp = dt, T, C, cpad(C)
        seed = 9700 + 13 * T + C
        x = GX.normal((T, C), seed)
        x[0] = 2.5
        if T > 1:
            x[T - 1] += 1000.0
        x, g = GX.rnd(x, dt), GX.rnd(GX.normal((T, C), seed + 1), dt)
        gamma, beta = GX.rnd(GX.normal((C,), seed + 2, std=0.3, mean=1.0), "f32"), GX.rnd(GX.normal((C,), seed + 3, std=0.3), "f32")
        self.x, self.g, self.gamma, self.beta = _padded(x, self.cp), _padded(g, self.cp), gamma, beta
        y, xh, mean, rstd = layernorm64(x, gamma, beta)
        ax = np.abs(x).sum(1, keepdims=True)
        dm = sum_bound(C, ax) / C + R * np.abs(mean)
        d = x - mean
        dd = dm + R * np.abs(d)
        var = (d * d).mean(1, keepdims=True)
        dvar = (2 * (np.abs(d) * dd).sum(1, keepdims=True) + sum_bound(C + 1, (d * d).sum(1, keepdims=True))) / C + R * var
        dr = 0.5 * rstd / (var + EPS) * dvar + 3 * R * rstd
        dxh = dd * rstd + np.abs(d) * dr + R * np.abs(xh)
        self.y = finish(*_placed(y, np.abs(gamma) * dxh + R * (np.abs(xh * gamma) + np.abs(beta)) + GX.TINY32, self.cp), dt)
        self.mean = (mean[:, 0], dm[:, 0])
        self.rstd = (rstd[:, 0], dr[:, 0])
        # backward (mean and rstd as the forward stored them: their bounds plus the store)
        dx, dgam, dbet = layernorm_bwd64(x, g, gamma)
        gg = g * gamma
        agg = np.abs(gg).sum(1, keepdims=True)
        m1, m2 = gg.mean(1, keepdims=True), (gg * xh).mean(1, keepdims=True)
        dm1 = (R * agg + sum_bound(C, agg)) / C + R * np.abs(m1)
        t2 = np.abs(gg * xh).sum(1, keepdims=True)
        dm2 = ((np.abs(gg) * dxh).sum(1, keepdims=True) + 2 * R * t2 + sum_bound(C, t2)) / C + R * np.abs(m2)
        inner = gg - m1 - xh * m2
        dinner = R * np.abs(gg) + dm1 + dxh * np.abs(m2) + np.abs(xh) * dm2 + 3 * R * (np.abs(gg) + np.abs(m1) + np.abs(xh * m2))
        self.dx = finish(*_placed(dx, dr * np.abs(inner) + rstd * dinner + R * np.abs(dx) + GX.TINY32, self.cp), dt)
        self.dgamma = (dgam, (np.abs(g) * dxh).sum(0) + ulp32(dgam) + GX.TINY32)
        self.dbeta = (dbet, ulp32(dbet) + GX.TINY32)
        self.label = "layernorm %s T=%d C=%d" % (dt, T, C)

    def largest_stored(self):
        """the largest |reference| among the outputs stored in the activation type (f16: must stay below 65504)"""
        return float(max(np.abs(self.y[0]).max(), np.abs(self.dx[0]).max()))

    def check(self, y, mean, rstd, dx, dgamma, dbeta):
        return [Cmp(self.label + " " + k, got, *ref) for k, got, ref in (("y", y, self.y), ("mean", mean, self.mean), ("rstd", rstd, self.rstd),
                                                                          ("dx", dx, self.dx), ("dgamma", dgamma, self.dgamma), ("dbeta", dbeta, self.dbeta))]


# C: 16 / 64 no padding and exactly one lane pass, 65 one over; 192 / 384 / 768 the reference's widths (EMB_DIM 96 doubled per stage), 257 /
# 384 / 768 the second and third channel block of the parameter kernel, 768 twelve elements per lane.  T: 4 / 5 a full workgroup and one
# over, 64 / 65 the slice boundary, 130 three slices.  LN_BIG (f32 only): ceil(T / 256) = 65 > 64, the LN_MAX_SLICES branch of ln_slice()
LN_C = (1, 16, 24, 64, 65, 96, 100, 192, 257, 384, 768)
LN_T = (1, 3, 4, 5, 64, 65, 130)
LN_BIG = (16385 + 130, 16)
KERNEL_DTYPES = ("f32", "bf16", "f16")
MAX_F16 = 65504.0
# (ws, hd, heads, shift, H, W); the first six are the cases the kernels arrived with
ATTN_SHAPES = ((4, 12, 2, 2, 8, 8), (7, 24, 2, 3, 14, 7), (8, 96, 1, 4, 8, 16), (8, 12, 8, 0, 8, 8), (1, 4, 1, 0, 2, 2), (2, 5, 3, 1, 4, 4),
               (8, 48, 2, 4, 8, 16),      # the reference's third stage: two chunks, the last 16 wide; head 1 starts at channel 48
               (4, 32, 3, 1, 8, 12),      # an exact chunk; shift 1, several windows along both axes
               (4, 33, 1, 3, 12, 8),      # one channel over a chunk; shift ws - 1
               (2, 64, 1, 1, 4, 6),       # two full chunks
               (3, 5, 3, 1, 6, 9),        # MT / KS = 1 / 1 with padding rows (N = 9)
               (5, 12, 2, 2, 10, 5),      # MT / KS = 2 / 1 (N = 25)
               (6, 24, 1, 5, 12, 12),     # MT / KS = 3 / 2 (N = 36), shift ws - 1
               (8, 96, 2, 7, 16, 8))      # three chunks, two heads, shift ws - 1


def ln_keys(dt):
    """(dt, T, C) of every LayerNorm case of a dtype"""
    return [(dt, T, C) for C in LN_C for T in LN_T] + ([(dt,) + LN_BIG] if dt == "f32" else [])


class AttnCase:
    """wm_winattn_fwd / wm_winattn_bwd, batch 2.  The last token of the grid rolled by -shift (a window that mixes regions when shift > 0)
    has q = a e_0 and one key of ITS window from another region (shift > 0; any other key otherwise) has k = 8 e_0, with scale * a * 8 =
    300: that score beats the row's others by more than 100, so with the mask's -100 it still carries the row (spread, masked_p)"""

    def __init__(self, dt, ws, hd, nH, shift, H, W, qkv=None, table=None, scale=None):
        self.dt, self.ws, self.hd, self.nH, self.shift, self.H, self.W = dt, ws, hd, nH, shift, H, W
        B, C, N = BATCH, nH * hd, ws * ws
        self.B, self.C, self.N, self.cp3, self.cpo = B, C, N, cpad(3 * C), cpad(C)
        self.scale = scale = float(np.float32(scale if scale is not None else (8.0 if (ws, hd) == (4, 12) else hd ** -0.5)))
        seed = 9800 + 7 * ws + hd + 31 * nH + shift
        tok = token_of(H, W, ws, shift)
        if qkv is None:
            qkv = GX.normal((B, H, W, 3 * C), seed, std=0.5)
            table = GX.normal(((2 * ws - 1) ** 2, nH), seed + 1)
            if N > 1:
                rid = mask_rule(H, W, ws, shift)[-1, N - 1]
                j = int(np.argmin(rid[:N - 1])) if shift else 0           # a key of the last window that the mask separates from the last token
                (yi, xi), (yj, xj) = tok[-1, N - 1], tok[-1, j]
                qkv[0, yi, xi, :hd] = 0.0
                qkv[0, yi, xi, 0] = 300.0 / (scale * 8.0)
                qkv[0, yj, xj, C:C + hd] = 0.0
                qkv[0, yj, xj, C] = 8.0
                self.big = (j,)
        qkv, table = GX.rnd(qkv, dt), GX.rnd(table, "f32")
        gout = GX.rnd(GX.normal((B, H, W, C), seed + 2), dt)
        self.qkv, self.table, self.gout = _padded(qkv, self.cp3), table, _padded(gout, self.cpo)
        h16 = dt != "f32"
        q, k, v, S = scores64(qkv, table, nH, ws, shift, scale)
        bias = table[rel_index_rule(ws)].transpose(2, 0, 1)[None, None]
        msk = mask_rule(H, W, ws, shift)[None, :, None]
        aqk = scale * np.einsum("bwhid,bwhjd->bwhij", np.abs(q), np.abs(k))
        # the roundings wa_scores performs: hd products summed (<= hd), per chunk the product with scale and the sum with the chunks
        # before (2 each), all on the dot product's terms; the table entry added once (1 rounding on |s| + |bias|), then the mask's -100
        # added once (1 rounding on |s + bias| + 100): neither is multiplied by the depth of the sum
        nchunk = (hd + 31) // 32
        dS = R * ((hd + 2 * nchunk + 2) * aqk + 2 * np.abs(bias) + np.abs(msk)) + GX.TINY32
        m = S.max(-1, keepdims=True)
        P = softmax64(S)
        self.spread = float((S.max(-1) - S.min(-1)).max())
        self.masked_p = float((P * (msk != 0)).max()) if shift else 0.0
        lse = m + np.log(np.exp(S - m).sum(-1, keepdims=True))
        # forward: p = exp(s - m) / sum
        e = dS + R * np.abs(S - m) + U["exp"] * 2.0 ** -23
        emax = e.max(-1, keepdims=True)
        dP = P * (e + emax + R * (N + 3)) + MIN_NORMAL
        dPo = dP + (half_ulp(P, dt) if h16 else 0.0)
        O = np.einsum("bwhij,bwhjd->bwhid", P, v)
        dO_ = np.einsum("bwhij,bwhjd->bwhid", dPo, np.abs(v)) + R * (N + 1) * np.einsum("bwhij,bwhjd->bwhid", P, np.abs(v)) + GX.TINY32
        self.out = finish(*_placed(scatter_windows(O, H, W, ws, shift), scatter_windows(dO_, H, W, ws, shift), self.cpo), dt)
        dl = emax + R * (N + 1) + U["log"] * ulp32(lse - m) + 2 * R * np.abs(lse)
        self.lse_win, self.dlse_win = lse[..., 0], dl[..., 0]                # [B, nW, nH, N]
        # backward: p = exp(s - lse) with the stored lse
        eb = dS + dl + R * np.abs(S - lse) + U["exp"] * 2.0 ** -23
        dPb = P * eb + MIN_NORMAL
        go = gather_windows(gout, H, W, ws, shift, nH)
        A = np.einsum("bwhid,bwhjd->bwhij", go, v)
        dA = R * (hd + 2) * np.einsum("bwhid,bwhjd->bwhij", np.abs(go), np.abs(v)) + GX.TINY32
        D = (P * A).sum(-1, keepdims=True)
        dD = (dPb * np.abs(A) + P * dA).sum(-1, keepdims=True) + R * (N + 2) * (P * np.abs(A)).sum(-1, keepdims=True)
        Sg = P * (A - D)
        dSg = dPb * np.abs(A - D) + P * (dA + dD + R * (np.abs(A) + np.abs(D))) + R * np.abs(Sg) + GX.TINY32
        dSo = dSg + (half_ulp(Sg, dt) if h16 else 0.0)
        dPbo = dPb + (half_ulp(P, dt) if h16 else 0.0)
        ago = np.abs(go)
        gV = np.einsum("bwhij,bwhid->bwhjd", P, go)
        bV = np.einsum("bwhij,bwhid->bwhjd", dPbo, ago) + R * (N + 1) * np.einsum("bwhij,bwhid->bwhjd", P, ago) + GX.TINY32
        gQ = scale * np.einsum("bwhij,bwhjd->bwhid", Sg, k)
        bQ = scale * (np.einsum("bwhij,bwhjd->bwhid", dSo, np.abs(k)) + R * (N + 2) * np.einsum("bwhij,bwhjd->bwhid", np.abs(Sg), np.abs(k))) + GX.TINY32
        gK = scale * np.einsum("bwhij,bwhid->bwhjd", Sg, q)
        bK = scale * (np.einsum("bwhij,bwhid->bwhjd", dSo, np.abs(q)) + R * (N + 2) * np.einsum("bwhij,bwhid->bwhjd", np.abs(Sg), np.abs(q))) + GX.TINY32
        ref = np.concatenate([scatter_windows(t, H, W, ws, shift) for t in (gQ, gK, gV)], -1)
        bnd = np.concatenate([scatter_windows(t, H, W, ws, shift) for t in (bQ, bK, bV)], -1)
        self.gqkv = finish(*_placed(ref, bnd, self.cp3), dt)
        gt, bt = np.zeros(table.shape), np.zeros(table.shape)
        idx = rel_index_rule(ws).reshape(-1)
        np.add.at(gt, idx, Sg.sum((0, 1)).transpose(1, 2, 0).reshape(N * N, nH))
        np.add.at(bt, idx, (dSg + R * (N + 1) * np.abs(Sg)).sum((0, 1)).transpose(1, 2, 0).reshape(N * N, nH))
        self.gtable = (gt, bt + ulp32(gt) + GX.TINY32)
        self.label = "winattn %s ws=%d hd=%d heads=%d shift=%d %dx%d" % (dt, ws, hd, nH, shift, H, W)

    def largest_stored(self):
        """the largest |reference| among the values stored or used as MFMA operands in the activation type (f16: below 65504)"""
        return float(max(np.abs(self.out[0]).max(), np.abs(self.gqkv[0]).max(), np.abs(self.qkv[..., :3 * self.C]).max()))

    def lse_grid(self):
        """(reference, bound) [B, nH, H, W]"""
        tok = token_of(self.H, self.W, self.ws, self.shift)
        ref, b = np.zeros((self.B, self.nH, self.H, self.W)), np.zeros((self.B, self.nH, self.H, self.W))
        ref[:, :, tok[..., 0], tok[..., 1]] = self.lse_win.transpose(0, 2, 1, 3)
        b[:, :, tok[..., 0], tok[..., 1]] = self.dlse_win.transpose(0, 2, 1, 3)
        return ref, b

    def check_fwd(self, out, lse):
        return [Cmp(self.label + " out", out, *self.out), Cmp(self.label + " lse", lse, *self.lse_grid())]

    def check_bwd(self, gqkv, gtable):
        return [Cmp(self.label + " g_qkv", gqkv, *self.gqkv), Cmp(self.label + " g_table", gtable, *self.gtable)]
