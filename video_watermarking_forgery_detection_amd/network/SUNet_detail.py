"""The Swin block of the reference's SUNet localiser (network/SUNet_detail.py) on the HIP layer toolkit: Mlp, WindowAttention,
SwinTransformerBlock and BasicLayer with the reference's names, constructor signatures and state_dict keys (`attn.relative_position_bias_table`,
`attn.relative_position_index`, `attn.qkv.*`, `attn.proj.*`, `norm1.*`, `norm2.*`, `mlp.fc1.*`, `mlp.fc2.*`, `attn_mask`), so a reference
checkpoint loads unchanged.

Inside a block the activation is a token grid [B,H,W,Cp] (glayers): LayerNorm and Linear act per token, so they commute with the cyclic
shift and the window partition, and the attention core (glayers.window_attention, csrc/swin.hip) folds roll, window_partition, the head
split, the bias gather, the mask, the softmax, window_reverse and the reverse roll into one launch each way.  The buffers
`relative_position_index` and `attn_mask` carry the reference's values for checkpoints and callers; the kernel computes both itself.

Not implemented (NotImplementedError): non-zero drop / attn_drop / drop_path in training mode (identity in eval), use_checkpoint=True,
downsample / upsample modules, PatchEmbed, PatchMerging, UpSample and SUNet itself.  A CPU input raises; there is no fallback.
`dtype` (an extra keyword of every module here) is the compute dtype of the activations between the layers (float32 = the parity path).
"""
import torch
import torch.nn as nn

from .. import glayers as G


def to_2tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


def _need_gpu(x):
    if not x.is_cuda:
        raise RuntimeError("the HIP layer toolkit runs on the GPU only; there is no CPU fallback")


def tokens_to_grid(x, H, W, dtype):
    """[B, H*W, C] f32 -> token grid [B,H,W,Cp] of `dtype`"""
    _need_gpu(x)
    B, L, C = x.shape
    if L != H * W:
        raise ValueError(f"input feature has wrong size: {L} tokens for a {H} x {W} grid")
    return G.to_nhwc(x.float().transpose(1, 2).reshape(B, C, H, W).contiguous(), dtype)


def grid_to_tokens(g, C):
    """token grid [B,H,W,Cp] -> [B, H*W, C] f32"""
    B, H, W, _ = g.shape
    return G.to_nchw(g, C).reshape(B, C, H * W).transpose(1, 2).contiguous()


def _no_dropout(mod, **rates):
    for name, p in rates.items():
        if p and mod.training:
            raise NotImplementedError(f"{type(mod).__name__}: {name}={p} in training mode is not implemented (identity in eval)")


class Mlp(nn.Module):
    """:8-24: fc1 -> GELU -> fc2 on a token grid [B,H,W,Cp]"""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        if act_layer is not nn.GELU:
            raise NotImplementedError("Mlp: only act_layer=nn.GELU is implemented")
        self.fc1 = G.Linear(in_features, hidden_features)
        self.act = G.Act("gelu")
        self.fc2 = G.Linear(hidden_features, out_features)
        self.drop = float(drop)

    def forward(self, x):
        _need_gpu(x)
        _no_dropout(self, drop=self.drop)
        return self.fc2(self.act(self.fc1(x)))


def window_partition(x, window_size):
    """host helper (:27-39): [B,H,W,C] -> [num_windows*B, ws, ws, C]"""
    B, H, W, C = x.shape
    x = x.view(B, H // window_size, window_size, W // window_size, window_size, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, window_size, window_size, C)


def window_reverse(windows, window_size, H, W):
    """host helper (:42-56): [num_windows*B, ws, ws, C] -> [B,H,W,C]"""
    B = int(windows.shape[0] / (H * W / window_size / window_size))
    x = windows.view(B, H // window_size, W // window_size, window_size, window_size, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


def relative_position_index(window_size):
    """:86-96: [Wh*Ww, Wh*Ww] int64"""
    wh, ww = window_size
    coords = torch.stack(torch.meshgrid([torch.arange(wh), torch.arange(ww)], indexing="ij"))
    flat = torch.flatten(coords, 1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += wh - 1
    rel[:, :, 1] += ww - 1
    rel[:, :, 0] *= 2 * ww - 1
    return rel.sum(-1)


def shifted_window_mask(H, W, window_size, shift_size):
    """:202-221: [nW, N, N] f32, -100 where two tokens of a window come from different regions of the rolled grid"""
    img_mask = torch.zeros((1, H, W, 1))
    cnt = 0
    for h in (slice(0, -window_size), slice(-window_size, -shift_size), slice(-shift_size, None)):
        for w in (slice(0, -window_size), slice(-window_size, -shift_size), slice(-shift_size, None)):
            img_mask[:, h, w, :] = cnt
            cnt += 1
    mw = window_partition(img_mask, window_size).view(-1, window_size * window_size)
    am = mw.unsqueeze(1) - mw.unsqueeze(2)
    return am.masked_fill(am != 0, float(-100.0)).masked_fill(am == 0, float(0.0))


class WindowAttention(nn.Module):
    """:59-138.  forward(x [num_windows*B, N, C], mask) as the reference; the fused path runs on the grid the owning block told it about
    (set_grid): the windows are put back on that grid and the kernel partitions, shifts and masks by itself.  Without a grid every window is
    its own ws x ws grid and a mask cannot be honoured.  forward_grid(x [B,H,W,Cp]) is what SwinTransformerBlock calls: no host partition."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0., proj_drop=0., dtype=torch.float32):
        super().__init__()
        self.dim, self.window_size, self.num_heads, self.dtype = dim, to_2tuple(window_size), num_heads, dtype
        if self.window_size[0] != self.window_size[1] or not 1 <= self.window_size[0] <= 8:
            raise NotImplementedError(f"WindowAttention: window {self.window_size} (square, 1 to 8 tokens a side)")
        if dim % num_heads or dim // num_heads > 96:
            raise NotImplementedError(f"WindowAttention: {dim} channels over {num_heads} heads (a head has at most 96 channels)")
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        ws = self.window_size[0]
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) * (2 * ws - 1), num_heads))
        self.register_buffer("relative_position_index", relative_position_index(self.window_size))
        self.qkv = G.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = float(attn_drop)
        self.proj = G.Linear(dim, dim)
        self.proj_drop = float(proj_drop)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)
        self._grid = None

    def set_grid(self, H, W, shift):
        self._grid = (int(H), int(W), int(shift))

    def forward_grid(self, x, shift):
        """x: token grid [B,H,W,Cp] (already normalised) -> proj(attention) on the same grid"""
        _need_gpu(x)
        _no_dropout(self, attn_drop=self.attn_drop, proj_drop=self.proj_drop)
        _, H, W, _ = x.shape
        a = G.window_attention(self.qkv(x), self.relative_position_bias_table, self.num_heads, self.window_size[0], shift, self.scale, H, W, dim=self.dim)
        return self.proj(a)

    def forward(self, x, mask=None):
        _need_gpu(x)
        B_, N, C = x.shape
        ws = self.window_size[0]
        if N != ws * ws or C != self.dim:
            raise ValueError(f"WindowAttention expects [num_windows*B, {ws * ws}, {self.dim}], got {tuple(x.shape)}")
        if self._grid is None:
            if mask is not None:
                raise NotImplementedError("WindowAttention: a mask needs the grid it belongs to (set_grid); arbitrary masks are not implemented")
            out = self.forward_grid(tokens_to_grid(x, ws, ws, self.dtype), 0)
            return grid_to_tokens(out, C)
        H, W, shift = self._grid
        if (mask is None) != (shift == 0):
            raise NotImplementedError("WindowAttention: the mask must be the shifted-window mask of the grid (None exactly when shift is 0)")
        if mask is not None and not torch.equal(mask.detach().float().cpu(), shifted_window_mask(H, W, ws, shift)):
            raise NotImplementedError("WindowAttention: only the shifted-window mask of the grid is implemented")
        grid = window_reverse(x.view(-1, ws, ws, C), ws, H, W)
        if shift:
            grid = torch.roll(grid, shifts=(shift, shift), dims=(1, 2))
        out = grid_to_tokens(self.forward_grid(tokens_to_grid(grid.reshape(-1, H * W, C), H, W, self.dtype), shift), C).view(-1, H, W, C)
        if shift:
            out = torch.roll(out, shifts=(-shift, -shift), dims=(1, 2))
        return window_partition(out, ws).view(-1, N, C)

    def extra_repr(self):
        return f'dim={self.dim}, window_size={self.window_size}, num_heads={self.num_heads}'


class SwinTransformerBlock(nn.Module):
    """:157-264.  forward(x [B, L, C] f32) -> [B, L, C] f32; forward_grid(x [B,H,W,Cp]) is the same block between token grids (what
    BasicLayer chains).  fused=False composes the attention from the host partition helpers and torch (tools/bench_swin.py, the tests)."""

    def __init__(self, dim, input_resolution, num_heads, window_size=7, shift_size=0, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0.,
                 attn_drop=0., drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, dtype=torch.float32, fused=True):
        super().__init__()
        if norm_layer is not nn.LayerNorm and norm_layer is not G.LayerNorm:
            raise NotImplementedError("SwinTransformerBlock: only norm_layer=nn.LayerNorm is implemented")
        self.dim, self.input_resolution, self.num_heads = dim, tuple(input_resolution), num_heads
        self.window_size, self.shift_size, self.mlp_ratio = window_size, shift_size, mlp_ratio
        self.dtype, self.fused = dtype, fused
        if min(self.input_resolution) <= self.window_size:
            self.shift_size = 0
            self.window_size = min(self.input_resolution)
        assert 0 <= self.shift_size < self.window_size, "shift_size must in 0-window_size"
        H, W = self.input_resolution
        if H % self.window_size or W % self.window_size:
            raise ValueError(f"SwinTransformerBlock: a {H} x {W} grid is not a multiple of the window {self.window_size}")
        self.norm1 = G.LayerNorm(dim)
        self.attn = WindowAttention(dim, window_size=to_2tuple(self.window_size), num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                    attn_drop=attn_drop, proj_drop=drop, dtype=dtype)
        self.attn.set_grid(H, W, self.shift_size)
        self.drop_path = float(drop_path)
        self.norm2 = G.LayerNorm(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.register_buffer("attn_mask", shifted_window_mask(H, W, self.window_size, self.shift_size) if self.shift_size > 0 else None)

    def _composed_attention(self, xn):
        """the reference's own sequence on torch ops and the host helpers, around the existing Linear layers: roll, window_partition, head
        split, q k^T, bias gather, mask, softmax, attn v, window_reverse, roll (fused=False)"""
        a, C, ws, s, nH = self.attn, self.dim, self.window_size, self.shift_size, self.num_heads
        B, H, W, _ = xn.shape
        qkv = grid_to_tokens(a.qkv(xn), 3 * C).view(B, H, W, 3 * C)
        if s:
            qkv = torch.roll(qkv, shifts=(-s, -s), dims=(1, 2))
        win = window_partition(qkv, ws).view(-1, ws * ws, 3, nH, C // nH).permute(2, 0, 3, 1, 4)
        q, k, v = win[0] * a.scale, win[1], win[2]
        att = q @ k.transpose(-2, -1)
        bias = a.relative_position_bias_table[a.relative_position_index.view(-1)].view(ws * ws, ws * ws, -1).permute(2, 0, 1)
        att = att + bias.unsqueeze(0)
        if self.attn_mask is not None:
            nW = self.attn_mask.shape[0]
            att = (att.view(-1, nW, nH, ws * ws, ws * ws) + self.attn_mask.unsqueeze(1).unsqueeze(0)).view(-1, nH, ws * ws, ws * ws)
        o = (att.softmax(-1) @ v).transpose(1, 2).reshape(-1, ws, ws, C)
        o = window_reverse(o, ws, H, W)
        if s:
            o = torch.roll(o, shifts=(s, s), dims=(1, 2))
        return a.proj(tokens_to_grid(o.reshape(B, H * W, C), H, W, self.dtype))

    def forward_grid(self, x):
        _need_gpu(x)
        _no_dropout(self, drop_path=self.drop_path)
        H, W = self.input_resolution
        if tuple(x.shape[1:3]) != (H, W):
            raise ValueError(f"input feature has wrong size: {tuple(x.shape)} for a {H} x {W} grid")
        xn = self.norm1(x)
        att = self.attn.forward_grid(xn, self.shift_size) if self.fused else self._composed_attention(xn)
        x = G.add(x, att)
        return G.add(x, self.mlp(self.norm2(x)))

    def forward(self, x):
        H, W = self.input_resolution
        return grid_to_tokens(self.forward_grid(tokens_to_grid(x, H, W, self.dtype)), self.dim)

    def extra_repr(self):
        return f"dim={self.dim}, input_resolution={self.input_resolution}, num_heads={self.num_heads}, " \
               f"window_size={self.window_size}, shift_size={self.shift_size}, mlp_ratio={self.mlp_ratio}"


class BasicLayer(nn.Module):
    """:389-445 with downsample=None: depth blocks, shift 0 and window_size // 2 in turn; the token grid is built once and handed through"""

    def __init__(self, dim, input_resolution, depth, num_heads, window_size, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0., norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False, dtype=torch.float32):
        super().__init__()
        if use_checkpoint:
            raise NotImplementedError("BasicLayer: use_checkpoint=True is not implemented")
        if downsample is not None:
            raise NotImplementedError("BasicLayer: downsample modules (PatchMerging) are not implemented")
        self.dim, self.input_resolution, self.depth, self.use_checkpoint, self.dtype = dim, tuple(input_resolution), depth, False, dtype
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, input_resolution=input_resolution, num_heads=num_heads, window_size=window_size,
                                 shift_size=0 if (i % 2 == 0) else window_size // 2, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                 drop=drop, attn_drop=attn_drop, drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                                 norm_layer=norm_layer, dtype=dtype)
            for i in range(depth)])
        self.downsample = None

    def forward(self, x):
        H, W = self.input_resolution
        g = tokens_to_grid(x, H, W, self.dtype)
        for blk in self.blocks:
            g = blk.forward_grid(g)
        return grid_to_tokens(g, self.dim)

    def extra_repr(self):
        return f"dim={self.dim}, input_resolution={self.input_resolution}, depth={self.depth}"


def _not_part(name):
    class _Missing(nn.Module):
        def __init__(self, *a, **kw):
            raise NotImplementedError(f"{name} is not implemented: the Swin block and BasicLayer(downsample=None) are what this module provides")
    _Missing.__name__ = _Missing.__qualname__ = name
    return _Missing


PatchEmbed, PatchMerging, UpSample, BasicLayer_up, SUNet = (_not_part(n) for n in ("PatchEmbed", "PatchMerging", "UpSample", "BasicLayer_up", "SUNet"))
