"""models/networks.py of the reference on the HIP layer toolkit (glayers.py): `Discriminator` (networks.py:631-749),
same constructor, same forward contract (NCHW f32 image in, [B,1,H/32,W/32] f32 out), same state_dict keys
(`init_conv.0.weight_orig`, `.weight_u`, `.weight_v`, ..., `conv5.0.weight`); and the tamper localiser of the reference's trainers,
`UNetDiscriminator` (networks.py:896-1113) with its `ResnetBlock` (:1387-1421), under the same rules; and `define_G` (:13-31), the
factory of the IRN trainers' generator (models/modules/Inv_arch.InvRescaleNet)."""
import torch
import torch.nn as nn

from .. import glayers as G
from .. import ops


def define_G(opt, subnet_type, block_num, dtype=torch.float32):
    """networks.py:13-31: the generator of every IRN trainer from an option file's `network_G` block (`in_nc`, `out_nc`, `scale` ->
    down_num = log2(scale), `init`, default 'xavier'): InvRescaleNet(in_nc, out_nc, subnet, block_num, down_num).  subnet_type 'DBNet'
    (what every option file of the reference names) takes Subnet_constructor.DenseBlock directly -- `subnet('DBNet')` keeps refusing --
    any other name goes through `subnet(subnet_type, init)`."""
    import math

    from .modules.Inv_arch import InvRescaleNet
    from .modules.Subnet_constructor import DenseBlock, subnet

    opt_net = opt["network_G"]
    init = opt_net["init"] if opt_net.get("init") else "xavier"
    down_num = int(math.log(opt_net["scale"], 2))
    if subnet_type == "DBNet":
        def constructor(channel_in, channel_out):
            return DenseBlock(channel_in, channel_out, init) if init == "xavier" else DenseBlock(channel_in, channel_out)
    else:
        constructor = subnet(subnet_type, init)
    return InvRescaleNet(opt_net["in_nc"], opt_net["out_nc"], constructor, block_num, down_num, dtype=dtype)


def spectral_norm_conv(cin, cout, k, stride, padding, use_spectral_norm):
    # networks.py:1381-1385 spectral_norm(nn.Conv2d(.., bias=not use_spectral_norm), use_spectral_norm)
    cls = G.SpectralNormConv2d if use_spectral_norm else G.Conv2d
    return cls(cin, cout, k, stride, padding, bias=not use_spectral_norm)


def _sn(cls_plain, cls_sn, use_spectral_norm, *args, **kw):
    # networks.py:1381-1385 spectral_norm(module, mode): the module itself, biased, when mode is off
    return (cls_sn if use_spectral_norm else cls_plain)(*args, **kw)


def default_srm_weight():
    """The three SRM residual kernels of the steganalysis literature (Fridrich & Kodovsky 2012, in the normalised 5x5 form of
    Zhou et al. 2018): the 3x3 second-order "square" kernel / 4, the 5x5 "square" kernel / 12 and the first-row second derivative / 2, each
    applied to one colour channel: filter 3 f + c reads channel c with kernel f, -> [9,3,5,5].  Every filter sums to 0."""
    k = torch.zeros(3, 5, 5)
    k[0, 1:4, 1:4] = torch.tensor([[-1.0, 2, -1], [2, -4, 2], [-1, 2, -1]]) / 4
    k[1] = torch.tensor([[-1.0, 2, -2, 2, -1], [2, -6, 8, -6, 2], [-2, 8, -12, 8, -2], [2, -6, 8, -6, 2], [-1, 2, -2, 2, -1]]) / 12
    k[2, 2, 1:4] = torch.tensor([1.0, -2, 1]) / 2
    w = torch.zeros(9, 3, 5, 5)
    for f in range(3):
        for c in range(3):
            w[3 * f + c, c] = k[f]
    return w


class BaseNetwork(nn.Module):
    def init_weights(self, init_type="kaiming", gain=0.02):
        """networks.py:104-129.  The reference initialises `m.weight.data`; under spectral norm that is the derived attribute the
        next forward overwrites, so `weight_orig` keeps nn.Conv2d's default initialisation -- as here."""

        def init_func(m):
            if isinstance(m, (G.SpectralNormConv2d, G.SpectralNormConvTranspose2d)) or not isinstance(m, (G.Conv2d, G.Linear, G.ConvTranspose2d)):
                return
            w = m.weight.data
            if init_type == "normal":
                nn.init.normal_(w, 0.0, gain)
            elif init_type == "xavier":
                nn.init.xavier_normal_(w, gain=gain)
            elif init_type == "kaiming":
                nn.init.kaiming_normal_(w, a=0, mode="fan_in")
            elif init_type == "orthogonal":
                nn.init.orthogonal_(w, gain=gain)
            if m.bias is not None:
                nn.init.constant_(m.bias.data, 0.0)

        self.apply(init_func)


class Discriminator(BaseNetwork):
    """networks.py:631-749: five (4x4 stride-2 conv, GELU, 3x3 conv, GELU) stages 3 -> 32 -> 64 -> 128 -> 256 -> 512 under spectral
    norm, a 1x1 conv to one channel, sigmoid.  `in_channels` and `use_SRM` are accepted and, as in the reference, unused (the first
    conv is hard-wired to 3 channels)."""

    def __init__(self, in_channels, use_sigmoid=True, use_spectral_norm=True, init_weights=True, use_SRM=False, dtype=torch.float32):
        super().__init__()
        self.use_sigmoid = use_sigmoid
        self.use_SRM = use_SRM
        self.in_channels = in_channels
        self.dtype = dtype
        dim = 32
        sn = use_spectral_norm

        def stage(cin, cout):
            return G.FusedSequential(spectral_norm_conv(cin, cout, 4, 2, 1, sn), G.Act("gelu"), spectral_norm_conv(cout, cout, 3, 1, 1, sn), G.Act("gelu"))

        self.init_conv = stage(3, dim)
        self.conv1 = stage(dim, dim * 2)
        self.conv2 = stage(dim * 2, dim * 4)
        self.conv3 = stage(dim * 4, dim * 8)
        self.conv4 = stage(dim * 8, dim * 16)
        self.conv5 = nn.Sequential(G.Conv2d(dim * 16, 1, 1, 1, 0, bias=False))
        self._sigmoid = G.Act("sigmoid")
        if init_weights:
            self.init_weights()

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"Discriminator expects [B,3,H,W], got {tuple(x.shape)}")
        h = G.to_nhwc(x, self.dtype)
        for blk in (self.init_conv, self.conv1, self.conv2, self.conv3, self.conv4, self.conv5):
            h = blk(h)
        if self.use_sigmoid:
            h = self._sigmoid(h)
        return G.to_nchw(h, 1)


class ResnetBlock(nn.Module):
    """networks.py:1387-1421, the spectral-norm branch: x + conv_block(x) with conv_block = ReflectionPad2d(dilation), spectral-norm 3x3
    conv with that dilation, GELU, ReflectionPad2d(1), spectral-norm 3x3 conv -- both valid, without bias.  state_dict keys
    `conv_block.1.weight_orig`, `.weight_u`, `.weight_v`, `conv_block.4...`."""

    def __init__(self, dim, dilation=1, use_spectral_norm=False):
        super().__init__()
        if not use_spectral_norm:
            raise NotImplementedError("ResnetBlock(use_spectral_norm=False) needs InstanceNorm2d, which this package has no kernel for")
        self.conv_block = G.FusedSequential(
            G.ReflectionPad2d(dilation),
            G.SpectralNormConv2d(dim, dim, 3, 1, 0, bias=False, dilation=dilation),
            G.Act("gelu"),
            G.ReflectionPad2d(1),
            G.SpectralNormConv2d(dim, dim, 3, 1, 0, bias=False, dilation=1),
        )

    def forward(self, x):
        return G.add(x, self.conv_block(x))


class UNetDiscriminator(BaseNetwork):
    """networks.py:896-1113, the tamper localiser IRN_model.py:147 / IRNp_model.py:162 / IRNcrop_model.py:125 build.

    use_SRM: the noise-residual first block (:1057-1071) -- the Bayar constraint on `BayarConv2D.weight` (in place on the parameter, no
    gradient through it, as the reference writes weight.data), the image symmetrically padded by 2, and ONE valid 5x5 convolution
    in_channels -> dim whose filter is the reference's torch.cat order `init_conv.weight` (dim - 12 rows) | `SRMConv2D.weight` (9, frozen)
    | `BayarConv2D.weight` (3), then GELU; autograd splits the filter's gradient back by rows and drops the frozen ones.  Otherwise two
    spectral-norm 3x3 conv + GELU pairs (:924-930).  Body: two stride-2 encoder stages, `residual_blocks` dilation-2 ResnetBlocks, two
    transposed-convolution decoder stages over skip concatenations, decoder_0, optional sigmoid.

    forward(x [B,in_channels,H,W] f32 on the GPU, H and W multiples of 4 and >= 12) -> (x [B,out_channels,H,W], (d2 [B,2 dim,H/2,W/2],
    d1 [B,dim,H,W])), all NCHW f32.

    `SRMConv2D.weight` is `srm_weight` [9,in_channels,5,5] (the reference reads it from a MantraNetv4.pt outside its tree) or, when None,
    default_srm_weight(); a load_state_dict replaces it.  It is a frozen parameter and, unlike in the reference (whose init_weights
    re-draws it, :1022-1023 after :909), init_weights leaves it alone.  `dtype` is the activations' (float32, bfloat16, float16).

    fused_head (additional_conv=False only, out_channels <= 4): decoder_0, the sigmoid and the NCHW f32 conversion run as ONE launch that reads
    e0 and d1 in place (glayers._Head2Fn) instead of concatenation, padded 1x1 convolution, activation pass and layout pass.  Same parameters
    and state_dict keys; False keeps the separate launches."""

    def __init__(self, in_channels=3, out_channels=3, residual_blocks=8, init_weights=True, use_spectral_norm=True, use_SRM=True,
                 with_attn=False, additional_conv=False, dim=32, use_sigmoid=False, dtype=torch.float32, srm_weight=None, fused_head=False):
        super().__init__()
        if with_attn:
            raise NotImplementedError("UNetDiscriminator(with_attn=True), the QF-conditioned variant, is not implemented")
        if fused_head and additional_conv:
            raise ValueError("UNetDiscriminator(fused_head=True) fuses the 1x1 decoder_0 of additional_conv=False; with additional_conv=True "
                             "decoder_0 starts with a 3x3 convolution")
        if fused_head and not 1 <= out_channels <= 4:
            raise ValueError(f"UNetDiscriminator(fused_head=True) needs 1 <= out_channels <= 4 (the mask head's kernel), got {out_channels}")
        self.fused_head = bool(fused_head)
        self.use_SRM, self.use_sigmoid, self.with_attn, self.additional_conv = use_SRM, use_sigmoid, with_attn, additional_conv
        self.in_channels, self.out_channels, self.dim, self.dtype = in_channels, out_channels, dim, dtype
        sn = use_spectral_norm

        def conv(cin, cout, k, stride, pad):
            return _sn(G.Conv2d, G.SpectralNormConv2d, sn, cin, cout, k, stride, pad)

        def convt(cin, cout):
            return _sn(G.ConvTranspose2d, G.SpectralNormConvTranspose2d, sn, cin, cout, 4, 2, 1)

        if use_SRM:
            if dim <= 12:
                raise ValueError(f"UNetDiscriminator(use_SRM=True) needs dim > 12 (9 SRM + 3 Bayar channels), got {dim}")
            if srm_weight is None:
                if in_channels != 3:
                    raise ValueError(f"the default SRM filters are defined for 3 input channels, got {in_channels}: pass srm_weight")
                srm_weight = default_srm_weight()
            if tuple(srm_weight.shape) != (9, in_channels, 5, 5):
                raise ValueError(f"srm_weight must be [9,{in_channels},5,5], got {tuple(srm_weight.shape)}")
            self.init_conv = G.Conv2d(in_channels, dim - 12, 5, 1, 0, bias=False)
            self.SRMConv2D = G.Conv2d(in_channels, 9, 5, 1, 0, bias=False)
            self.BayarConv2D = G.Conv2d(in_channels, 3, 5, 1, 0, bias=False)
            self.activation = G.Act("gelu")
        else:
            self.init_conv = G.FusedSequential(conv(in_channels, dim, 3, 1, 1), G.Act("gelu"), conv(dim, dim, 3, 1, 1), G.Act("gelu"))
        self.encoder_1 = G.FusedSequential(conv(dim, dim * 2, 4, 2, 1), G.Act("gelu"), conv(dim * 2, dim * 2, 3, 1, 1), G.Act("gelu"))
        self.encoder_2 = G.FusedSequential(conv(dim * 2, dim * 4, 4, 2, 1), G.Act("gelu"), conv(dim * 4, dim * 4, 3, 1, 1), G.Act("gelu"))
        self.middle = nn.Sequential(*[ResnetBlock(dim * 4, dilation=2, use_spectral_norm=sn) for _ in range(residual_blocks)])
        self.decoder_2 = G.FusedSequential(convt(dim * 8, dim * 2), G.Act("gelu"), conv(dim * 2, dim * 2, 3, 1, 1), G.Act("gelu"))
        self.decoder_1 = G.FusedSequential(convt(dim * 4, dim), G.Act("gelu"), conv(dim, dim, 3, 1, 1), G.Act("gelu"))
        if not additional_conv:
            self.decoder_0 = G.FusedSequential(G.Conv2d(dim * 2, out_channels, 1, 1, 0, bias_grad_f64=True))
        else:
            self.decoder_0 = G.FusedSequential(conv(dim * 2, dim, 3, 1, 1), G.Act("gelu"), G.Conv2d(dim, out_channels, 1, 1, 0, bias_grad_f64=True))
        self._sigmoid = G.Act("sigmoid")
        if init_weights:
            self.init_weights()
        if use_SRM:
            with torch.no_grad():
                self.SRMConv2D.weight.copy_(srm_weight)
            self.SRMConv2D.weight.requires_grad_(False)

    def first_block(self, x):
        """e0 as an NHWC activation [B,H,W,cpad(dim)] from the NCHW f32 image"""
        if not self.use_SRM:
            return self.init_conv(G.to_nhwc(x, self.dtype))
        ops.bayar_constrain_(self.BayarConv2D.weight.data, torch_order=True)                # :1059-1061
        xp = G.to_nhwc(x, self.dtype, pads=(2, 2, 2, 2), mode=ops.PAD_SYMMETRIC)            # :1064
        w = torch.cat((self.init_conv.weight, self.SRMConv2D.weight, self.BayarConv2D.weight), 0)   # :1070's order
        return G._ConvActFn.apply(xp, w, None, 1, 0, 1, "gelu")

    def forward(self, x):
        if (x.dim() != 4 or x.shape[1] != self.in_channels or not x.is_cuda or x.shape[2] % 4 or x.shape[3] % 4
                or x.shape[2] < 12 or x.shape[3] < 12):
            raise ValueError(f"UNetDiscriminator expects a GPU tensor [B,{self.in_channels},H,W] with H and W multiples of 4 and >= 12 "
                             f"(the dilation-2 reflection pad at H/4 x W/4), got {tuple(x.shape)} on {x.device}")
        dim = self.dim
        e0 = self.first_block(x)
        e1 = self.encoder_1(e0)
        e2 = self.encoder_2(e1)
        m = self.middle(e2)
        d2 = self.decoder_2(G.chan_cat(e2, dim * 4, m, dim * 4))
        d1 = self.decoder_1(G.chan_cat(e1, dim * 2, d2, dim * 2))
        if self.fused_head:    # decoder_0 + sigmoid + to_nchw in one launch that reads e0 and d1 in place (csrc/mask_head.hip)
            head = self.decoder_0[0]
            y = G._Head2Fn.apply(e0, dim, d1, dim, head.weight, head.bias, 1 if self.use_sigmoid else 0)
            return y, (G.to_nchw(d2, dim * 2), G.to_nchw(d1, dim))
        y = self.decoder_0(G.chan_cat(e0, dim, d1, dim))
        if self.use_sigmoid:
            y = self._sigmoid(y)
        return G.to_nchw(y, self.out_channels), (G.to_nchw(d2, dim * 2), G.to_nchw(d1, dim))
