"""models/modules/Subnet_constructor.py of the reference, the part the invertible embedder's option files name: `subnet('Resnet')` and its
`ResBlock` (:145-179), the instance-normalised coupling subnet ("Use Instance Norm to prevent gradient explosion"), and `DenseBlock`
(:102-127), the LeakyReLU dense block behind `subnet_type: DBNet`, on the HIP layer toolkit (glayers.py; csrc/instnorm.hip,
csrc/gconv.hip, csrc/conv3x3*.hip).  Same constructor arguments and state_dict keys; activations are NHWC tensors of the toolkit, as in
models/invertible_net.py, whose couplings take this ResBlock as `subnet_constructor`; DenseBlock is the subnet of models/modules/Inv_arch.py."""
import torch.nn as nn

from ... import glayers as G


def initialize_weights(net_l, scale=1):
    """:7-24 for the toolkit's Conv2d: kaiming_normal_(a=0, fan_in) * scale, zero bias"""
    for m in (net_l if isinstance(net_l, list) else [net_l]):
        for c in m.modules():
            if isinstance(c, G.Conv2d):
                nn.init.kaiming_normal_(c.weight, a=0, mode="fan_in")
                c.weight.data *= scale
                if c.bias is not None:
                    c.bias.data.zero_()


def initialize_weights_xavier(net_l, scale=1):
    """:27-44 for the toolkit's Conv2d: xavier_normal_ * scale, zero bias"""
    for m in (net_l if isinstance(net_l, list) else [net_l]):
        for c in m.modules():
            if isinstance(c, G.Conv2d):
                nn.init.xavier_normal_(c.weight)
                c.weight.data *= scale
                if c.bias is not None:
                    c.bias.data.zero_()


class DenseBlock(nn.Module):
    """:102-127: five 3x3 convolutions over the growing concatenation (x, x1, ..), LeakyReLU(0.2) after the first four.  Each
    convolution + LeakyReLU pair is one autograd node (glayers._ConvActFn, kind "lrelu").  state_dict keys `conv1.weight` .. `conv5.bias`;
    conv1-4 start from the reference's xavier (init='xavier') or kaiming initialiser scaled by 0.1, conv5 from zero."""

    def __init__(self, channel_in, channel_out, init="xavier", gc=32, bias=True):
        super().__init__()
        self.channel_in, self.channel_out, self.gc = channel_in, channel_out, gc
        self.conv1 = G.Conv2d(channel_in, gc, 3, 1, 1, bias=bias)
        self.conv2 = G.Conv2d(channel_in + gc, gc, 3, 1, 1, bias=bias)
        self.conv3 = G.Conv2d(channel_in + 2 * gc, gc, 3, 1, 1, bias=bias)
        self.conv4 = G.Conv2d(channel_in + 3 * gc, gc, 3, 1, 1, bias=bias)
        self.conv5 = G.Conv2d(channel_in + 4 * gc, channel_out, 3, 1, 1, bias=bias)
        if init == "xavier":
            initialize_weights_xavier([self.conv1, self.conv2, self.conv3, self.conv4], 0.1)
        else:
            initialize_weights([self.conv1, self.conv2, self.conv3, self.conv4], 0.1)
        initialize_weights(self.conv5, 0)

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("the HIP layer toolkit runs on the GPU only; there is no CPU fallback")
        if x.dim() != 4 or x.shape[3] != G.cpad(self.channel_in):
            raise ValueError(f"DenseBlock expects an NHWC activation of {self.channel_in} channels (stride {G.cpad(self.channel_in)}), got {tuple(x.shape)}")
        cat, n = x, self.channel_in
        for conv in (self.conv1, self.conv2, self.conv3, self.conv4):
            y = G._ConvActFn.apply(cat, conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation, "lrelu")
            cat, n = G.chan_cat(cat, n, y, self.gc), n + self.gc
        return self.conv5(cat)


class ResBlock(nn.Module):
    """:145-179: four stages of (3x3 conv to 64, InstanceNorm2d(64), ReLU), then a 3x3 conv of cat(x, features) to channel_out.

    Each stage keeps the reference's nn.Sequential indices: `0` the convolution (`conv1.0.weight`, `conv1.0.bias`, ...), `1` the
    normalisation -- no parameters, no buffers: affine=False, track_running_stats=False -- with the ReLU folded into its kernels
    (glayers.InstanceNorm2d(act="relu")), `2` the place of the reference's nn.ReLU, an identity here.  Parameters start from torch's
    defaults, as the reference's do (it calls no initialiser on this block).

    The reference's forward (:172-179) calls `self.relu1` around every stage, an attribute it never defines (the line that made it is
    commented out, :154), so it cannot run as written.  The contract taken here is its submodules in its order,
    conv5(cat(x, conv4(conv3(conv2(conv1(x)))))): the second ReLU it intends would be the identity on a ReLU's output."""

    def __init__(self, channel_in, channel_out):
        super().__init__()
        feature = 64
        self.channel_in, self.channel_out, self.feature = channel_in, channel_out, feature

        def stage(cin):
            return nn.Sequential(G.Conv2d(cin, feature, 3, 1, 1), G.InstanceNorm2d(feature, track_running_stats=False, act="relu"), nn.Identity())

        self.conv1 = stage(channel_in)
        self.conv2 = stage(feature)
        self.conv3 = stage(feature)
        self.conv4 = stage(feature)
        self.conv5 = G.Conv2d(feature + channel_in, channel_out, 3, 1, 1)

    def forward(self, x):
        r = self.conv4(self.conv3(self.conv2(self.conv1(x))))
        return self.conv5(G.chan_cat(x, self.channel_in, r, self.feature))


def subnet(net_structure, init="xavier"):
    """:130-143: the constructor (channel_in, channel_out) -> subnet that an option file's `subnet_type` selects.  'Resnet' builds ResBlock.
    'DBNet' is the reference's DenseBlock with LeakyReLU(0.2) (:102-127): this function keeps refusing it (NotImplementedError), as it
    did before that block existed here -- take `DenseBlock` itself as the constructor, or build the network with
    models/networks.define_G, which does.  Any other name gives, as in the reference, a constructor that returns None."""
    if net_structure == "DBNet":
        raise NotImplementedError("subnet('DBNet') is not wired here: the LeakyReLU dense block is Subnet_constructor.DenseBlock -- pass it as the "
                                  "subnet constructor or build the generator with models/networks.define_G (models/invertible_net.DenseBlock "
                                  "is the ELU one)")

    def constructor(channel_in, channel_out):
        if net_structure == "Resnet":
            return ResBlock(channel_in, channel_out)
        return None     # not supported

    return constructor
