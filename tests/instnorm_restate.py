"""nn.InstanceNorm2d(C, eps, affine, track_running_stats=False) (+ nn.ReLU) restated in float64 numpy, forward and backward, with the
cases, seeded inputs and the tolerance rule that tests/test_cpu_instnorm.py and tests/test_gpu_instnorm.py share.

The statement (NCHW, statistics over the H*W plane of every (sample, channel)):
    mean = E[x], var = E[(x - mean)^2] (biased), rstd = 1 / sqrt(var + eps), xhat = (x - mean) * rstd
    y = act(xhat * gamma + beta)                       gamma = 1, beta = 0 without affine; act = identity or ReLU
    g = dy * [y > 0] (ReLU) or dy
    dx = gamma * rstd * (g - E[g] - xhat * E[g * xhat]),   dgamma = sum_{b,h,w} g * xhat,   dbeta = sum_{b,h,w} g
tests/test_cpu_instnorm.py shows that this equals torch's own float64 result through autograd on every case.

Tolerance (this project's rule): a device result is held to MARGIN = 4 x the deviation of TORCH'S OWN CPU run in the same dtype (float32,
bfloat16, float16) from float64 on the same inputs -- measured where it is used, never on a kernel -- and, where that deviation is (nearly)
0, to 2 float32 ulp of the tensor's largest |value| (`bound_of`).  Inputs of a 16-bit run are rounded to that dtype first, and gamma / beta
are multiples of 1/16 that both 16-bit formats hold exactly, so every side computes from the same numbers."""
import numpy as np
import torch

EPS = 1e-5
MARGIN = 4.0
# (B, C, H, W): 64 channels on a small plane; padded channels (24 of a stride of 32) on an odd plane; a plane of 1551 pixels, which
# spans several workgroups and ends in a tail; the smallest legal plane
CASES = {"c64_4x4": (2, 64, 4, 4), "c24_5x7": (3, 24, 5, 7), "c16_33x47": (2, 16, 33, 47), "c64_2x1": (1, 64, 2, 1)}
CANCEL_CASE = "c16_33x47"          # x = 1000 + N(0, 1) in float32: the variance is 1e-6 of E[x^2]
CONST_B, CONST_C, CONST_V = 0, 1, 2.5      # inputs(const=True): the plane (sample 0, channel 1) is the constant 2.5: var = 0, xhat = 0, y = beta
CONST_BETA = -0.5                  # beta of that channel: y = -0.5 there, so the ReLU masks the plane and its dx is 0 (with beta > 0 it is not)
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def inputs(name, cancel=False, const=False):
    """(x, dy, gamma, beta) float32 arrays of case `name`, seeded by the shape; gamma, beta are used by the affine runs only.  const: with
    the constant plane -- kept out of the runs that are held to torch's deviation, because torch's own float32 result is not exact there
    (its mean of 2.5s is not 2.5, and rstd = 316 magnifies that) and would widen the bound of the whole tensor"""
    B, C, H, W = CASES[name]
    rs = np.random.RandomState(9000 + 7 * B + 11 * C + 13 * H + 17 * W + (1 if cancel else 0))
    x = rs.randn(B, C, H, W)
    if cancel:
        x = 1000.0 + x
    else:
        x = 1.5 * x + 0.25
    if const:
        x[CONST_B, CONST_C] = CONST_V
    dy = rs.randn(B, C, H, W)
    gamma = 1.0 + rs.randint(-8, 9, C) / 16.0
    beta = rs.randint(-8, 9, C) / 16.0
    if const:
        beta[CONST_C] = CONST_BETA
    return tuple(a.astype(np.float32) for a in (x, dy, gamma, beta))


def rounded(a, tag):
    """float32 array -> the same values after a round trip through dtype `tag` (float32 again)"""
    return torch.from_numpy(a).to(TORCH_DT[tag]).float().numpy()


def forward(x, gamma=None, beta=None, relu=False, eps=EPS):
    """float64 (y, xhat, rstd)"""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=(2, 3), keepdims=True)
    var = ((x - mean) ** 2).mean(axis=(2, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean) * rstd
    y = xhat
    if gamma is not None:
        y = xhat * np.asarray(gamma, np.float64)[None, :, None, None] + np.asarray(beta, np.float64)[None, :, None, None]
    if relu:
        y = np.maximum(y, 0.0)
    return y, xhat, rstd


def backward(x, dy, gamma=None, beta=None, relu=False, eps=EPS):
    """float64 (dx, dgamma, dbeta); dgamma / dbeta None without gamma"""
    y, xhat, rstd = forward(x, gamma, beta, relu, eps)
    g = np.asarray(dy, np.float64)
    if relu:
        g = g * (y > 0)
    k = rstd if gamma is None else rstd * np.asarray(gamma, np.float64)[None, :, None, None]
    dx = k * (g - g.mean(axis=(2, 3), keepdims=True) - xhat * (g * xhat).mean(axis=(2, 3), keepdims=True))
    if gamma is None:
        return dx, None, None
    return dx, (g * xhat).sum(axis=(0, 2, 3)), g.sum(axis=(0, 2, 3))


def restate(x, dy, gamma=None, beta=None, relu=False):
    """{y, dx[, dgamma, dbeta]} float64"""
    y = forward(x, gamma, beta, relu)[0]
    dx, dg, db = backward(x, dy, gamma, beta, relu)
    out = {"y": y, "dx": dx}
    if gamma is not None:
        out.update(dgamma=dg, dbeta=db)
    return out


def torch_run(x, dy, gamma=None, beta=None, relu=False, dtype=torch.float64):
    """torch.nn.InstanceNorm2d (+ nn.ReLU) on the CPU in `dtype`, through autograd: {y, dx[, dgamma, dbeta]} as float64 arrays"""
    C = x.shape[1]
    m = torch.nn.InstanceNorm2d(C, eps=EPS, affine=gamma is not None, track_running_stats=False)
    if gamma is not None:
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(np.asarray(gamma, np.float32)))
            m.bias.copy_(torch.from_numpy(np.asarray(beta, np.float32)))
    m = m.to(dtype)
    xt = torch.from_numpy(np.asarray(x, np.float32)).to(dtype).requires_grad_(True)
    y = m(xt)
    if relu:
        y = torch.nn.functional.relu(y)
    y.backward(torch.from_numpy(np.asarray(dy, np.float32)).to(dtype))
    out = {"y": y, "dx": xt.grad}
    if gamma is not None:
        out.update(dgamma=m.weight.grad, dbeta=m.bias.grad)
    return {k: v.detach().double().numpy() for k, v in out.items()}


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def bound_of(dev, amax, margin=MARGIN):
    return max(margin * float(dev), 2.0 * ulp32(float(amax)))


def maxdiff(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return float(np.max(np.abs(got - want))) if got.size else 0.0


def torch_bounds(x, dy, gamma, beta, relu, tag, want):
    """{quantity: bound}: MARGIN x max |torch's CPU run in dtype `tag` - `want`| (want = the float64 statement on the same inputs), at
    least 2 float32 ulp of the quantity's largest |value|"""
    low = torch_run(x, dy, gamma, beta, relu, TORCH_DT[tag])
    return {k: bound_of(maxdiff(low[k], want[k]), np.max(np.abs(want[k]))) for k in want}


def check(label, got, bound):
    """`got` = the largest |difference| found; printed before it is asserted"""
    got = float(got)
    print("%-58s %.3e (bound %.3e, %.2f of it)" % (label, got, bound, got / bound if bound > 0 else float("inf")))
    assert got <= bound, (label, got, bound)
    return got
