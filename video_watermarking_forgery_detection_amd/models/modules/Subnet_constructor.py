"""models/modules/Subnet_constructor.py of the reference, the part the invertible embedder's option files name: `subnet('Resnet')` and its
`ResBlock` (:145-179), the instance-normalised coupling subnet ("Use Instance Norm to prevent gradient explosion"), on the HIP layer
toolkit (glayers.py; csrc/instnorm.hip, csrc/gconv.hip, csrc/conv3x3*.hip).  Same constructor arguments and state_dict keys; activations
are NHWC tensors of the toolkit, as in models/invertible_net.py, whose couplings take this ResBlock as `subnet_constructor`."""
import torch.nn as nn

from ... import glayers as G


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
    'DBNet' is the reference's DenseBlock with LeakyReLU(0.2) (:102-127), which this package does not have (models/invertible_net.py's
    DenseBlock is the ELU one): NotImplementedError.  Any other name gives, as in the reference, a constructor that returns None."""
    if net_structure == "DBNet":
        raise NotImplementedError("subnet('DBNet'): the LeakyReLU dense block (Subnet_constructor.DenseBlock) is not implemented; "
                                  "models/invertible_net.DenseBlock is the ELU one")

    def constructor(channel_in, channel_out):
        if net_structure == "Resnet":
            return ResBlock(channel_in, channel_out)
        return None     # not supported

    return constructor
