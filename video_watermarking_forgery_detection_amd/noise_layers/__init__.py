"""Differentiable attack layers on the MI355X kernels -- mirror of the reference's noise_layers/
package: the layers the models instantiate and the stochastic / JPEG-Drop attacks the
reference's trainers construct and its __init__ exports (Dropout = crop.py's, GN, SaltPepper); Hybrid is the per-frame mix of several
of them that the reference's video model feeds its localiser (models/IRNcrop_model.py:347-373)."""
import random


def get_random_float(float_range):
    return random.random() * (float_range[1] - float_range[0]) + float_range[0]


def get_random_int(int_range):
    return random.randint(int_range[0], int_range[1])


from .identity import Identity  # noqa: E402
from .jpeg import Jpeg, JpegSS, JpegMask, JpegBasic  # noqa: E402
from .combined import Combined  # noqa: E402
from .gaussian_blur import GaussianBlur  # noqa: E402
from .middle_filter import MiddleBlur  # noqa: E402
from .resize import Resize  # noqa: E402
from .crop import Crop, Dropout  # noqa: E402
from .gaussian_noise import GN  # noqa: E402
from .salt_pepper_noise import SaltPepper  # noqa: E402
from .gaussian import Gaussian  # noqa: E402
from .jpeg_compression import JpegCompression  # noqa: E402
from .noiser import Noiser  # noqa: E402
from .hybrid import Hybrid  # noqa: E402
