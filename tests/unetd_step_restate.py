"""What tests/golden/make_golden_unetd_step.py, tests/test_gpu_unetd_trainer.py and tests/test_cpu_unetd_trainer.py share: the case, the
seeded inputs of the two training steps, how a quantity is subsampled into the fixture, and its bound (the rule of tests/unetd_restate.py:
MARGIN x the reference's own float32-vs-float64 deviation, at least 2 float32 ulp of the tensor's largest |value|)."""
import numpy as np

import unetd_restate as R

NAME = "srm"
LR = 1e-3


def step_inputs():
    """(image [2,3,20,28] in [0,1), mask [2,1,20,28] of {0,1}) float32 torch tensors"""
    import detgen
    B, _, H, W = R.NET_SHAPE
    return detgen.uniform(R.NET_SHAPE, 9700), (detgen.uniform((B, 1, H, W), 9701) > 0.5).float()


def stride_of(k, numel):
    if k.startswith("p"):
        return 401
    if k.startswith("uv"):
        return 1 if numel <= 256 else 17
    return 1


def stored(k, v):
    """quantity k (whole tensor) as the fixture holds it"""
    v = np.asarray(v)
    return v.reshape(-1)[::stride_of(k, v.size)] if v.ndim else v


GROUPS = ("p1", "p2", "uv1", "uv2")


def unpack(g):
    """{quantity: stored float64 values} of the fixture g"""
    q = {k: g[k] for k in ("loss1", "loss2", "gx1")}
    for grp in GROUPS:
        o = 0
        for name, n in zip(g[grp + "/names"], g[grp + "/sizes"]):
            q[f"{grp}/{name}"] = g[grp][o:o + int(n)]
            o += int(n)
    return q


def bounds(g):
    """{quantity: bound}"""
    return {str(k): R.bound_of(d, a) for k, d, a in zip(g["qnames"], g["dev32"], g["amax"])}
