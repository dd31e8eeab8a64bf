"""tests/swin_restate.py against the fixture made from the reference's network/SUNet_detail.py (tests/golden/swin.npz), and the HIP modules'
state_dict surface; then the kernels' bound models (LnCase, AttnCase) against float32 imitations of csrc/swin.hip, faithful and defective.
No GPU: construction and numpy / torch CPU arithmetic only."""
import functools
import os

import numpy as np
import pytest
import torch

import instnorm_restate as NR
import swin_restate as SR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swin.npz")
D53 = 2.0 ** -53


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_restated_modules_match_the_fixture(golden):
    """every stored quantity of the four cases from the restated modules in float64: within the float64 round-off of sums of a few thousand
    terms of the quantity's size (2**-53 x 4096 x amax; the two sides add in different orders)"""
    q = SR.run_cases(SR.build((SR.SwinTransformerBlock, SR.BasicLayer), torch.float64), SR.case_inputs(), lambda t: t.double().clone())
    assert sorted(q) == sorted(k for k in golden if k.split("/")[0] in SR.CASES)
    for k in sorted(q):
        NR.check(k, NR.maxdiff(q[k], golden[k]), 4096 * D53 * max(float(golden["amax/" + k]), 1.0))


@pytest.mark.parametrize("name", SR.CORE_CASES)
def test_restated_core_matches_the_fixture(golden, name):
    """attention_core64 (gather by token_of, the index and mask rule, softmax, scatter) on the reference's own qkv gives the reference's
    attention output, on the token grid"""
    H, W, C, nH, ws, s, scale = SR.geometry(name)
    got = SR.attention_core64(golden["core/%s/qkv" % name], golden["core/%s/table" % name], nH, ws, s, scale)
    want = golden["core/%s/out" % name]
    NR.check(name + " core", NR.maxdiff(got, want), 4096 * D53 * max(float(np.abs(want).max()), 1.0))


def test_core_backward_is_the_gradient_of_the_core():
    """attention_core_bwd64 against torch autograd through the restated float64 forward written in torch (one small shifted case)"""
    ws, hd, nH, s, H, W = 2, 5, 3, 1, 4, 4
    c = SR.AttnCase("f32", ws, hd, nH, s, H, W)
    C = nH * hd
    qkv = torch.from_numpy(c.qkv[..., :3 * C]).requires_grad_(True)
    table = torch.from_numpy(c.table).requires_grad_(True)
    g = torch.roll(qkv, shifts=(-s, -s), dims=(1, 2))
    win = SR.window_partition(g, ws).view(-1, ws * ws, 3, nH, hd).permute(2, 0, 3, 1, 4)
    att = (win[0] * c.scale) @ win[1].transpose(-2, -1)
    att = att + table[torch.from_numpy(SR.rel_index_rule(ws)).view(-1)].view(ws * ws, ws * ws, -1).permute(2, 0, 1).unsqueeze(0)
    mask = torch.from_numpy(SR.mask_rule(H, W, ws, s))
    att = (att.view(-1, mask.shape[0], nH, ws * ws, ws * ws) + mask.unsqueeze(1).unsqueeze(0)).view(-1, nH, ws * ws, ws * ws)
    o = SR.window_reverse((att.softmax(-1) @ win[2]).transpose(1, 2).reshape(-1, ws, ws, C), ws, H, W)
    o = torch.roll(o, shifts=(s, s), dims=(1, 2))
    (o * torch.from_numpy(c.gout[..., :C])).sum().backward()
    gq, gt = SR.attention_core_bwd64(c.qkv[..., :3 * C], c.table, c.gout[..., :C], nH, ws, s, c.scale)
    NR.check("core forward", NR.maxdiff(SR.attention_core64(c.qkv[..., :3 * C], c.table, nH, ws, s, c.scale), o.detach().numpy()), 1e-12 * 300)
    NR.check("g_qkv", NR.maxdiff(gq, qkv.grad.numpy()), 1e-12 * max(1.0, float(np.abs(gq).max())))
    NR.check("g_table", NR.maxdiff(gt, table.grad.numpy()), 1e-12 * max(1.0, float(np.abs(gt).max())))
    assert c.spread > 100 and c.masked_p > 0.5, (c.spread, c.masked_p)


@pytest.mark.parametrize("name", [n for n, (kind, _) in SR.CASES.items() if kind == "block"])
def test_index_and_mask_rule_equal_the_reference_buffers(golden, name):
    """what the kernel computes per token pair equals the buffers the reference builds, exactly"""
    H, W, C, nH, ws, s, _ = SR.geometry(name)
    assert np.array_equal(SR.rel_index_rule(ws), golden["buf/%s/relative_position_index" % name])
    key = "buf/%s/attn_mask" % name
    if s:
        assert np.array_equal(SR.mask_rule(H, W, ws, s), golden[key].astype(np.float64))
    else:
        assert key not in golden and not SR.mask_rule(H, W, ws, s).any()


def test_rule_for_every_kernel_shape():
    """the rule against the reference's construction (written out here from SUNet_detail.py:86-96, 202-221) for the kernel tests' shapes"""
    for ws, _, _, s, H, W in SR.ATTN_SHAPES:
        co = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij")).flatten(1)
        rel = (co[:, :, None] - co[:, None, :]).permute(1, 2, 0).contiguous()
        rel[:, :, 0] += ws - 1
        rel[:, :, 1] += ws - 1
        rel[:, :, 0] *= 2 * ws - 1
        assert np.array_equal(SR.rel_index_rule(ws), rel.sum(-1).numpy())
        if s:
            img = torch.zeros(1, H, W, 1)
            cnt = 0
            for h in (slice(0, -ws), slice(-ws, -s), slice(-s, None)):
                for w in (slice(0, -ws), slice(-ws, -s), slice(-s, None)):
                    img[:, h, w, :] = cnt
                    cnt += 1
            mw = SR.window_partition(img, ws).view(-1, ws * ws)
            am = mw.unsqueeze(1) - mw.unsqueeze(2)
            am = am.masked_fill(am != 0, -100.0).masked_fill(am == 0, 0.0)
            assert np.array_equal(SR.mask_rule(H, W, ws, s), am.double().numpy())


def test_hip_modules_have_the_reference_state_dict(golden):
    """keys, order and shapes of the HIP modules' state_dicts equal the reference's; the buffers carry the reference's values"""
    from video_watermarking_forgery_detection_amd.network import SUNet_detail as D
    for name, (kind, kw) in SR.CASES.items():
        m = (D.SwinTransformerBlock if kind == "block" else D.BasicLayer)(**kw)
        assert SR.keys_of(m) == list(golden["keys/" + name]), name
        if kind == "block":
            assert np.array_equal(m.attn.relative_position_index.numpy(), golden["buf/%s/relative_position_index" % name])
            if m.attn_mask is not None:
                assert np.array_equal(m.attn_mask.numpy(), golden["buf/%s/attn_mask" % name])
            assert (m.window_size, m.shift_size) == SR.geometry(name)[4:6]
    assert SR.keys_of(SR.build((SR.SwinTransformerBlock, SR.BasicLayer))["layer"]) == list(golden["keys/layer"])


def test_limits_raise():
    from video_watermarking_forgery_detection_amd.network import SUNet_detail as D
    with pytest.raises(NotImplementedError):
        D.BasicLayer(24, (8, 8), 2, 2, 4, use_checkpoint=True)
    with pytest.raises(NotImplementedError):
        D.BasicLayer(24, (8, 8), 2, 2, 4, downsample=D.PatchMerging)
    for cls in (D.PatchEmbed, D.PatchMerging, D.UpSample, D.SUNet):
        with pytest.raises(NotImplementedError):
            cls()
    blk = D.SwinTransformerBlock(24, (8, 8), 2, window_size=4, drop_path=0.1)
    with pytest.raises(RuntimeError, match="GPU"):
        blk(torch.zeros(2, 64, 24))
    with pytest.raises(RuntimeError, match="GPU"):
        D.WindowAttention(24, (4, 4), 2)(torch.zeros(4, 16, 24))


# ================================================================================================= the kernels' bound models, without a GPU
# Float32 numpy imitations of csrc/swin.hip's arithmetic as the kernels perform it must pass the bound models of swin_restate.py (LnCase,
# AttnCase) on every key in f32 / bf16 / f16, and each named defect, switched on inside the imitation, must FAIL the unchanged model at
# the case named for it.  So a green tests/test_gpu_swin.py means something.
from layers_exact import TORCH, all_ok, first_bad  # noqa: E402

f32 = np.float32
LN_WAVES, LN_SLICE, LN_MAX_SLICES, WA_HC = 4, 64, 256, 32      # swin.hip's constants


def a32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def stored(v, dt, truncate=False):
    """float32 values -> what a conversion to dtype dt keeps (round to nearest even; truncate: the defect), as float64"""
    v = a32(v)
    if dt == "f32":
        return v.astype(np.float64)
    if not truncate:
        return torch.from_numpy(v).to(TORCH[dt]).double().numpy()
    if dt == "bf16":
        return (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    h = v.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float64)


def must_pass(cmps):
    for c in cmps:
        c.assert_ok()


def must_fail(cmps, what):
    assert not all_ok(cmps), "the defect `%s` passed every comparison" % what


def fma(a, b, c):
    """float32 fused multiply-add: the product of two float32 values is exact in float64, so one rounding of the sum remains"""
    return (a32(a).astype(np.float64) * a32(b).astype(np.float64) + a32(c).astype(np.float64)).astype(f32)


# ---- the dispatch formulas of swin.hip
def ln_slice(tokens):
    c = -(-tokens // LN_MAX_SLICES)
    return c if c > LN_SLICE else LN_SLICE


def ln_slices(tokens):
    return -(-tokens // ln_slice(tokens))


def wa_mt(ws):
    return (ws * ws + 15) // 16


def wa_ks(ws):
    return (ws * ws + 31) // 32


def wa_nchunk(hd):
    return (hd + WA_HC - 1) // WA_HC


# ----------------------------------------------------------------------------------------------------------------- LayerNorm
def wave_sum(lanes):
    """[T, 64] float32 -> [T]: the xor butterfly, offsets 32 .. 1"""
    v, idx = lanes, np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, idx ^ o]
    return v[:, 0]


def lane_sums(terms, acc_fma=None):
    """terms [T, n]: lane l adds its elements l, l + 64, ... in order in float32; acc_fma = (a, b): the term is a * b, fused"""
    T, n = (terms if acc_fma is None else acc_fma[0]).shape
    s = np.zeros((T, 64), dtype=f32)
    for c0 in range(0, n, 64):
        w = min(64, n - c0)
        if acc_fma is None:
            s[:, :w] = s[:, :w] + terms[:, c0:c0 + w]
        else:
            s[:, :w] = fma(acc_fma[0][:, c0:c0 + w], acc_fma[1][:, c0:c0 + w], s[:, :w])
    return wave_sum(s)


def imit_ln(c, defect=None):
    """layernorm_fwd_kernel, layernorm_bwd_dx_kernel, layernorm_bwd_param_kernel + finalise -> (y, mean, rstd, dx, dgamma, dbeta)"""
    T, C, cp, dt = c.T, c.C, c.cp, c.dt
    nread = cp if defect == "padding channels of x read" else C
    x, g = a32(c.x)[:, :nread], a32(c.g)[:, :nread]
    gamma, beta = np.ones(nread, dtype=f32), np.zeros(nread, dtype=f32)
    gamma[:C], beta[:C] = a32(c.gamma), a32(c.beta)
    div = f32(cp if defect == "mean divided by CP" else C)
    m = (lane_sums(x) / div)[:, None]
    if defect == "variance as E[x^2] - mean^2":
        var = lane_sums(None, (x, x))[:, None] / div - m * m
    else:
        d = x - m
        var = lane_sums(None, (d, d))[:, None] / div
    with np.errstate(divide="ignore"):
        r = f32(1) / np.sqrt(var + f32(SR.EPS))
        r_out = f32(1) / np.sqrt(var) if defect == "rstd stored without eps" else r
    found = SR.SENTINEL if defect == "padding channels of y / dx not zeroed" else 0.0
    y = np.full((T, cp), found)
    y[:, :C] = stored(fma((x - m) * r, gamma[None], beta[None])[:, :C], dt)
    # backward: mean and rstd as the forward stored them
    r = r_out
    xh = (x - m) * r
    if defect == "gamma on the first term of dx only":
        gg, mg = g * gamma[None], g
    else:
        gg = mg = g * gamma[None]
    m1 = (lane_sums(mg) / div)[:, None]
    m2 = (lane_sums(None, (mg, xh)) / div)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        dx = np.full((T, cp), found)
        dx[:, :C] = stored((r * fma(-xh, m2, gg - m1))[:, :C], dt)
        # parameters: partial rows in double per slice, added in slice order
        sl = ln_slice(T)
        starts = np.arange(0, T, sl)
        pg = np.add.reduceat(g[:, :C].astype(np.float64) * xh[:, :C].astype(np.float64), starts, axis=0)
        pb = np.add.reduceat(g[:, :C].astype(np.float64), starts, axis=0)
    if defect == "last slice dropped from dgamma":
        pg = pg[:-1]
    dgamma, dbeta = np.zeros(C), np.zeros(C)
    for s in range(pg.shape[0]):
        dgamma += pg[s]
    for s in range(pb.shape[0]):
        dbeta += pb[s]
    if defect == "dgamma of channels >= 256 from channel c - 256":
        dgamma[256:] = dgamma[:C - 256]
    return y, m[:, 0], r_out[:, 0], dx, a32(dgamma), a32(dbeta)


LN_KEYS = [k for dt in SR.KERNEL_DTYPES for k in SR.ln_keys(dt)]


@functools.lru_cache(maxsize=None)
def ln_case(dt, T, C):
    return SR.LnCase(dt, T, C)


def test_layernorm_imitation_passes():
    for key in LN_KEYS:
        c = ln_case(*key)
        must_pass(c.check(*imit_ln(c)))
        assert key[0] != "f16" or c.largest_stored() < SR.MAX_F16, c.label


LN_DEFECTS = [
    ("variance as E[x^2] - mean^2", ("f32", 3, 96)),
    ("variance as E[x^2] - mean^2", ("f16", 130, 192)),
    ("mean divided by CP", ("f32", 4, 100)),
    ("mean divided by CP", ("f16", 5, 65)),
    ("padding channels of x read", ("bf16", 3, 24)),
    ("padding channels of x read", ("f16", 65, 257)),
    ("padding channels of y / dx not zeroed", ("f32", 1, 1)),
    ("padding channels of y / dx not zeroed", ("f16", 64, 100)),
    ("gamma on the first term of dx only", ("f32", 5, 16)),
    ("gamma on the first term of dx only", ("bf16", 130, 768)),
    ("gamma on the first term of dx only", ("f16", 4, 384)),
    ("last slice dropped from dgamma", ("f32", 65, 64)),            # the last slice is one token
    ("last slice dropped from dgamma", ("f16", 130, 96)),
    ("last slice dropped from dgamma", ("f32",) + SR.LN_BIG),
    ("dgamma of channels >= 256 from channel c - 256", ("f32", 3, 257)),
    ("dgamma of channels >= 256 from channel c - 256", ("bf16", 64, 384)),
    ("dgamma of channels >= 256 from channel c - 256", ("f16", 5, 768)),
    ("rstd stored without eps", ("f32", 4, 24)),                    # the constant row: variance 0
    ("rstd stored without eps", ("f16", 1, 192)),
]


@pytest.mark.filterwarnings("ignore::RuntimeWarning")          # a defect may produce inf / nan: that is its failure
@pytest.mark.parametrize("defect,key", LN_DEFECTS)
def test_layernorm_defects_fail(defect, key):
    c = ln_case(*key)
    assert key in LN_KEYS
    must_fail(c.check(*imit_ln(c, defect)), defect)


# ----------------------------------------------------------------------------------------------------------------- window attention
class Grid:
    """a token-grid tensor as the kernel addresses it: a flat array of elements, with a guard of SENTINEL after the last token so that a
    defect's out-of-range address reads something (and its out-of-range store is dropped)"""

    def __init__(self, arr, stride, fill=None):
        self.stride, self.n = stride, arr.size
        self.flat = np.full(arr.size + 4096 * 4, SR.SENTINEL, dtype=np.float64)
        self.flat[:arr.size] = arr.reshape(-1) if fill is None else fill

    def read(self, tok, chan):
        """tok [...], chan [k] -> float32 [..., k]"""
        return a32(self.flat[tok[..., None] * self.stride + chan])

    def write(self, tok, chan, vals):
        idx = (tok[..., None] * self.stride + chan).reshape(-1)
        ok = idx < self.n
        self.flat[idx[ok]] = np.asarray(vals, dtype=np.float64).reshape(-1)[ok]

    def array(self, shape):
        return self.flat[:self.n].reshape(shape)


def wa_geometry(c, defect=None):
    """(tok [B, nW, N] token offsets as wa_token gives them, masked [nW, N, N] bool as wa_region decides, rel [N, N] as wa_rel)"""
    ws, s, H, W, N = c.ws, c.shift, c.H, c.W, c.N
    n = np.arange(N)
    tok = np.zeros((c.B, H // ws * (W // ws), N), dtype=np.int64)
    masked = np.zeros((tok.shape[1], N, N), dtype=bool)
    for wy in range(H // ws):
        for wx in range(W // ws):
            y0, x0 = wy * ws + n // ws, wx * ws + n % ws
            y, x = y0 + s, x0 + s
            y = np.where(y > H if defect == "wrap y > H for y >= H" else y >= H, y - H, y)
            x = np.where(x >= W, x - W, x)
            tok[:, wy * (W // ws) + wx] = (np.arange(c.B)[:, None] * H + y[None]) * W + x[None]
            if defect == "mask from the un-shifted coordinates":
                y0, x0 = (y0 + s) % H, (x0 + s) % W
            if defect == "region bands with <= for <":
                ry = np.where(y0 <= H - ws, 0, np.where(y0 <= H - s, 1, 2))
                rx = np.where(x0 <= W - ws, 0, np.where(x0 <= W - s, 1, 2))
            else:
                ry = np.where(y0 < H - ws, 0, np.where(y0 < H - s, 1, 2))
                rx = np.where(x0 < W - ws, 0, np.where(x0 < W - s, 1, 2))
            rid = ry * 3 + rx
            masked[wy * (W // ws) + wx] = rid[:, None] != rid[None, :]
    if s == 0 or defect == "mask omitted":
        masked[:] = False
    i, j = (n[None, :], n[:, None]) if defect == "relative index with i and j swapped" else (n[:, None], n[None, :])
    rel = (i // ws - j // ws + ws - 1) * (2 * ws - 1) + (i % ws - j % ws + ws - 1)
    return tok, masked, rel


def wa_stage(c, grid, tok, chan0, c0, defect=None):
    """wa_stage: channels [c0, c0 + 32) of a head from channel chan0 on -> float32 [B, nW, N, 32], zeros beyond hd"""
    v = grid.read(tok, chan0 + c0 + np.arange(WA_HC))
    if defect != "last chunk's channels >= hd not zeroed":
        v[..., max(c.hd - c0, 0):] = 0
    return v


def wa_scores(c, q, tok, masked, rel, head, defect=None):
    """S [B, nW, N, N] float32 of one head: scale * Q K^T chunk by chunk, table and mask on the last chunk"""
    S = None
    for ci in range(wa_nchunk(c.hd)):
        if defect == "second chunk dropped" and ci == 1:
            continue
        qc = wa_stage(c, q, tok, 0 * c.C + head * c.hd, ci * WA_HC, defect)
        kc = wa_stage(c, q, tok, 1 * c.C + head * c.hd, ci * WA_HC, defect)
        acc = np.matmul(qc, kc.transpose(0, 1, 3, 2))
        scale = f32(1) if (defect == "scores not scaled on the first chunk" and ci == 0) else f32(c.scale)
        S = scale * acc + (f32(0) if S is None else S)
    nt = (2 * c.ws - 1) ** 2
    tbl = a32(c.table).reshape(-1)
    bias = tbl[head * nt + rel] if defect == "table read as [head][index]" else tbl[rel * c.nH + head]
    S = S + bias[None, None]
    return np.where(masked[None], S + f32(-100), S)


def operand(v, c, defect=None):
    """a float32 LDS value as the MFMA takes it: rounded to the activation type for bf16 / f16, as it is for f32"""
    if c.dt == "f32":
        return a32(v)
    return a32(stored(v, c.dt, truncate=(defect == "P and dS truncated to the 16-bit type")))


def stale(P, c, defect):
    """the [64][65] score tile's columns >= N that the 32 KS deep products read: zeroed by the kernel.  The defect leaves what wa_scores put
    there (exp(0 - max) / sum for columns < 16 MT) and, beyond 16 MT, LDS nobody wrote: modelled as NaN"""
    N, K = c.N, 32 * wa_ks(c.ws)
    out = np.zeros(P.shape[:-1] + (K,), dtype=f32)
    out[..., :N] = P
    if defect == "P columns >= N not zeroed" and K > N:
        out[..., N:] = np.nan
    return out


def imit_attn(c, defect=None):
    """winattn_fwd_kernel, winattn_bwd_kernel and winattn_table_finalize_kernel -> (out, lse, g_qkv, g_table) as float64 arrays"""
    B, H, W, C, nH, hd, N, dt = c.B, c.H, c.W, c.C, c.nH, c.hd, c.N, c.dt
    tok, masked, rel = wa_geometry(c, defect)
    nW, nt = tok.shape[1], (2 * c.ws - 1) ** 2
    found = defect == "padding channels of out / g_qkv left as found"
    qkv, gout = Grid(c.qkv, c.cp3), Grid(c.gout, c.cpo)
    out = Grid(np.empty((B, H, W, c.cpo)), c.cpo, fill=SR.SENTINEL)
    gq = Grid(np.empty((B, H, W, c.cp3)), c.cp3, fill=SR.SENTINEL)
    lse = Grid(np.empty((B, nH, H, W)), 1, fill=SR.SENTINEL)
    per = H * W
    gtable = np.zeros((nt, nH))
    nchunk = wa_nchunk(hd)
    zpad = np.zeros((B, nW, 32 * wa_ks(c.ws) - N, WA_HC), dtype=f32)           # rows >= N of a staged chunk

    def deep(a, bmat):
        """a [.., N, K] (K = 32 KS columns) times a staged chunk [.., N, 32] padded with its zero rows"""
        return np.matmul(a, np.concatenate([bmat, zpad], axis=2))

    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for h in range(nH):
            chq, chk, chv = h * hd, C + h * hd, 2 * C + h * hd
            S = wa_scores(c, qkv, tok, masked, rel, h, defect)
            m = S.max(-1, keepdims=True) if defect != "row maximum not subtracted" else np.zeros(S.shape[:-1] + (1,), dtype=f32)
            e = np.exp(S - m)
            ssum = e.sum(-1, keepdims=True, dtype=f32)
            P = e * (f32(1) / ssum)
            l32 = (m + np.log(ssum))[..., 0]                                  # [B, nW, N]
            ltok = (tok // per) * (nH * per) + h * per + tok % per            # the LSE's [B, nH, H, W] address of a token
            lse.write(ltok, np.arange(1), l32)
            Pk = stale(operand(P, c, defect), c, defect)
            for ci in range(nchunk):
                vc = wa_stage(c, qkv, tok, chv, ci * WA_HC)
                w = min(WA_HC, hd - ci * WA_HC)
                out.write(tok, chq + ci * WA_HC + np.arange(w), stored(deep(Pk, vc)[..., :w], dt))
            # ---- backward: S again, dP = dO V^T over the chunks, P from the stored LSE
            A = None
            for ci in range(nchunk):
                if defect == "second chunk dropped" and ci == 1:
                    continue
                dO = wa_stage(c, gout, tok, h * hd, ci * WA_HC)
                vc = wa_stage(c, qkv, tok, chv, ci * WA_HC)
                acc = np.matmul(dO, vc.transpose(0, 1, 3, 2))
                A = acc if A is None else acc + A
            lrd = ltok - h * per if defect == "LSE of head 0 for every head" else ltok
            lst = a32(lse.flat[lrd])[..., None]
            Pb = np.exp(S - lst)
            rs = (Pb * A).sum(-1, keepdims=True, dtype=f32)
            dS = Pb * (A - rs)
            part = np.zeros((B * nW, nt), dtype=f32)                          # dS by relative index, (i, j) row-major, in float32
            np.add.at(part, (slice(None), rel.reshape(-1)), dS.reshape(B * nW, N * N))
            if defect == "one window's partial table dropped" and B * nW > 1:
                part = np.delete(part, 1, axis=0)
            gtable[:, h] = a32(part.astype(np.float64).sum(0))
            Pt = stale(operand(Pb, c, defect).transpose(0, 1, 3, 2), c, None)
            dSo = operand(dS, c, defect)
            dSk, dSt = stale(dSo, c, None), stale(dSo.transpose(0, 1, 3, 2), c, None)
            if defect == "P columns >= N not zeroed":
                Pt = stale(operand(Pb, c).transpose(0, 1, 3, 2), c, defect)
            for ci in range(nchunk):
                w, d = min(WA_HC, hd - ci * WA_HC), ci * WA_HC + np.arange(min(WA_HC, hd - ci * WA_HC))
                qc, kc = wa_stage(c, qkv, tok, chq, ci * WA_HC), wa_stage(c, qkv, tok, chk, ci * WA_HC)
                dO = wa_stage(c, gout, tok, h * hd, ci * WA_HC)
                sc = f32(c.scale)
                gq.write(tok, chv + d, stored(deep(Pt, dO)[..., :w], dt))
                gq.write(tok, chq + d, stored((sc * deep(dSt if defect == "dQ with dS transposed" else dSk, kc))[..., :w], dt))
                gq.write(tok, chk + d, stored(((f32(1) if defect == "dK without scale" else sc) * deep(dSt, qc))[..., :w], dt))
        if not found:
            if c.cpo > C:
                out.write(tok, np.arange(C, c.cpo), np.zeros(tok.shape + (c.cpo - C,)))
            if c.cp3 > 3 * C:
                gq.write(tok, np.arange(3 * C, c.cp3), np.zeros(tok.shape + (c.cp3 - 3 * C,)))
    return out.array((B, H, W, c.cpo)), lse.array((B, nH, H, W)), gq.array((B, H, W, c.cp3)), gtable


ATTN_KEYS = [(dt,) + s for dt in SR.KERNEL_DTYPES for s in SR.ATTN_SHAPES]


@functools.lru_cache(maxsize=None)
def attn_case(*key):
    return SR.AttnCase(*key)


def check_attn(c, got):
    return c.check_fwd(got[0], got[1]) + c.check_bwd(got[2], got[3])


@pytest.mark.parametrize("key", ATTN_KEYS, ids=lambda k: "%s_ws%d_hd%d_nh%d_s%d_%dx%d" % k)
def test_attention_imitation_passes(key):
    """and the data holds its conditions in every dtype: the planted score still spreads its row over more than 100 and a masked key still
    carries it after q and k are rounded to the type; no reference value is beyond f16's largest"""
    c = attn_case(*key)
    must_pass(check_attn(c, imit_attn(c)))
    if c.N > 1:
        assert c.spread > 100, c.spread
        assert c.shift == 0 or c.masked_p > 0.5, c.masked_p
    assert c.largest_stored() < SR.MAX_F16


S48, S32, S33, S64, S3, S5, S6, S96 = SR.ATTN_SHAPES[6:]
S4, S7 = SR.ATTN_SHAPES[0], SR.ATTN_SHAPES[1]
ATTN_DEFECTS = [
    ("mask omitted", "f32", S32), ("mask omitted", "f16", S6),
    ("mask from the un-shifted coordinates", "f32", S33), ("mask from the un-shifted coordinates", "f16", S32),
    ("region bands with <= for <", "bf16", S3), ("region bands with <= for <", "f16", S96),
    ("wrap y > H for y >= H", "f32", S5), ("wrap y > H for y >= H", "f16", S48),
    ("relative index with i and j swapped", "f32", S3), ("relative index with i and j swapped", "f16", S7),
    ("table read as [head][index]", "bf16", S32), ("table read as [head][index]", "f16", S48),
    ("last chunk's channels >= hd not zeroed", "f32", S48), ("last chunk's channels >= hd not zeroed", "bf16", S33),
    ("last chunk's channels >= hd not zeroed", "f16", S5),
    ("second chunk dropped", "f32", S33), ("second chunk dropped", "bf16", S64), ("second chunk dropped", "f16", S48),
    ("scores not scaled on the first chunk", "f32", S64), ("scores not scaled on the first chunk", "f16", S96),
    ("row maximum not subtracted", "f32", S4), ("row maximum not subtracted", "f16", S6),
    ("LSE of head 0 for every head", "f32", S5), ("LSE of head 0 for every head", "f16", S48),
    ("P columns >= N not zeroed", "f32", S3), ("P columns >= N not zeroed", "bf16", S6), ("P columns >= N not zeroed", "f16", S3),
    # (an operand's half ulp and the stored value's half ulp are most of a 16-bit bound, and a truncation errs by up to one ulp: this
    # defect goes beyond the bound by a factor of 1.1 to 1.2 on a handful of elements of these cases, never by more)
    ("P and dS truncated to the 16-bit type", "bf16", S4), ("P and dS truncated to the 16-bit type", "bf16", S33),
    ("P and dS truncated to the 16-bit type", "f16", S64), ("P and dS truncated to the 16-bit type", "f16", S32),
    ("dK without scale", "f32", S48), ("dK without scale", "f16", S3),
    ("dQ with dS transposed", "f32", S6), ("dQ with dS transposed", "f16", S33),
    ("one window's partial table dropped", "f32", S64), ("one window's partial table dropped", "f16", S5),
    ("padding channels of out / g_qkv left as found", "bf16", S5), ("padding channels of out / g_qkv left as found", "f16", S33),
]


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("defect,dt,shape", ATTN_DEFECTS)
def test_attention_defects_fail(defect, dt, shape):
    c = attn_case(dt, *shape)
    must_fail(check_attn(c, imit_attn(c, defect)), defect)


def test_key_tables_reach_every_path():
    """swin.hip's dispatch formulas restated (ln_slice, ln_slices, the parameter kernel's channel blocks, MT, KS, nchunk) against the key
    tables: every value the GPU tests are meant to visit is visited"""
    # LayerNorm: lane passes, padding, channel blocks of the parameter kernel, workgroup tails, slices
    assert {96, 192, 384, 768} <= set(SR.LN_C)                                      # the reference's widths
    assert {-(-C // 64) for C in SR.LN_C} >= {1, 2, 3, 5, 6, 12} and {16, 64} <= {C for C in SR.LN_C if C == SR.cpad(C) and C <= 64}
    assert {C - 64 for C in SR.LN_C} >= {0, 1} and any(C != SR.cpad(C) for C in SR.LN_C)
    assert {-(-C // 256) for C in SR.LN_C} >= {1, 2, 3} and 257 in SR.LN_C          # grid.x of layernorm_bwd_param_kernel, and its tail
    assert {T % LN_WAVES for T in SR.LN_T} == {0, 1, 2, 3} and {-(-T // LN_WAVES) for T in SR.LN_T} >= {1, 2, 33}
    assert all(ln_slice(T) == LN_SLICE for T in SR.LN_T) and {ln_slices(T) for T in SR.LN_T} >= {1, 2, 3}
    assert {T - LN_SLICE for T in SR.LN_T} >= {0, 1}                                # the slice boundary
    big = SR.LN_BIG[0]
    assert ln_slice(big) == 65 > LN_SLICE and ln_slices(big) <= LN_MAX_SLICES and big % ln_slice(big) != 0
    assert ("f32",) + SR.LN_BIG in LN_KEYS
    # attention: tiles, chunks, heads, shifts
    sh = SR.ATTN_SHAPES
    assert {(wa_mt(s[0]), wa_ks(s[0])) for s in sh} >= {(1, 1), (2, 1), (3, 2), (4, 2)}
    assert {s[0] * s[0] % 16 for s in sh if s[0] in (3, 5, 6)} >= {9, 4}            # padding rows inside the last tile
    assert {wa_mt(s[0]) ** 2 % 4 for s in sh} >= {0, 1} and {wa_mt(s[0]) * 2 % 4 for s in sh} >= {0, 2}   # tiles over the four waves
    assert {12, 24, 48, 96} <= {s[1] for s in sh}                                   # the reference's head dims
    assert {(wa_nchunk(s[1]), s[1] % WA_HC) for s in sh} >= {(1, 0), (2, 1), (2, 16), (2, 0), (3, 0)}
    assert any(s[2] > 1 and wa_nchunk(s[1]) > 1 for s in sh)                        # a second head behind more than one chunk
    assert any((which * s[1] * s[2] + h * s[1]) % 16 and wa_nchunk(s[1]) > 1 for s in sh for which in range(3) for h in range(s[2]))
    several = [s for s in sh if s[4] // s[0] > 1 and s[5] // s[0] > 1 and s[0] > 2]
    assert {1} <= {s[3] for s in several} and any(s[3] == s[0] - 1 for s in several)
    assert any(s[3] == s[0] - 1 and wa_nchunk(s[1]) == 3 and s[2] == 2 for s in sh)
    assert any(SR.cpad(s[1] * s[2]) > s[1] * s[2] for s in sh) and any(SR.cpad(3 * s[1] * s[2]) > 3 * s[1] * s[2] for s in sh)
    assert SR.KERNEL_DTYPES == ("f32", "bf16", "f16")
