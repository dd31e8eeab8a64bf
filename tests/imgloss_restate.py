"""Torch-CPU restatement of the three image losses the kernels of csrc/imgloss.hip compute, written from their definitions (the reference's
models/modules/loss.py ReconstructionLoss, loss.py ExclusionLoss and GradientLoss).  Dtype-generic: at float64 it is the yardstick of the GPU
tests, and the CPU tests compare it with the reference's recorded float64 results in tests/golden/imgloss.npz.

    recon(x, t, kind, eps)        mean_b sum_chw f(x - t),  f = d^2 (l2) | sqrt(d^2 + eps) (l_char) | d (l1: the signed sum, no abs)
    gradient_loss(a)              mean |a[..., :-1] - a[..., 1:]| + mean |a[..., :-1, :] - a[..., 1:, :]|
    exclusion(img1, img2, level)  per level (2 x 2 average pooling, floor, between levels), direction (0 = gradx, the row difference;
                                  1 = grady, the column difference) and channel pair: mean_{b,y,x}(s1^2 s2^2) ** 0.25 with
                                  s = 2 sigmoid(diff) - 1;  loss = (sum gradx terms + sum grady terms) / (level * 9) / 2
Term k of a (level, direction) is the pair (img1 channel k % C1, img2 channel k // C1): the reference's list order when C1 == C2 (its
loops index the wrong image when the counts differ, and raise).  One deliberate difference, the kernels': a term whose mean is exactly 0
contributes 0 with a ZERO gradient (the reference's autograd gives 0 * inf = NaN there).

`defect=` plants one known mistake (the CPU tests show that the GPU tests' comparisons catch each).  Also here: the seeded input generators
and the fixture's case table.  torch and numpy only."""
import numpy as np
import torch

KINDS = ("l2", "l_char", "l1")
EPS = (1e-6, 1e-3)
# name -> (img1 shape, img2 shape, level): the fixture's exclusion cases; the first four also serve the other two losses
CASES = {
    "e0": ((2, 3, 32, 32), (2, 3, 32, 32), 3),
    "e1": ((1, 3, 30, 43), (1, 3, 30, 43), 3),
    "e2": ((2, 3, 9, 13), (2, 3, 9, 13), 3),
    "e3": ((1, 3, 70, 91), (1, 3, 70, 91), 3),
    "e4": ((1, 1, 8, 8), (1, 2, 8, 8), 3),
    "e0_l1": ((2, 3, 32, 32), (2, 3, 32, 32), 1),
    "e0_l2": ((2, 3, 32, 32), (2, 3, 32, 32), 2),
}
IMAGE_CASES = ("e0", "e1", "e2", "e3")
SEEDS = (0, 1, 2)       # the fixture stores the inputs of seed 0; the deviations' maxima run over all three


def case_seed(name, seed=0):
    return 1000 * seed + 17 * sorted(CASES).index(name.split("_")[0]) + 3


def gen_pair(shape1, shape2, seed):
    """two float32 images, uniform in [0, 1)"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape1, generator=g), torch.rand(shape2, generator=g)


def gen_case(name, seed=0):
    s1, s2, level = CASES[name]
    a, b = gen_pair(s1, s2, case_seed(name, seed))
    return a, b, level


def fixture_case(g, name):
    base = name.split("_")[0]
    return torch.from_numpy(g[base + "_img1"]), torch.from_numpy(g[base + "_img2"]), CASES[name][2]


# ----------------------------------------------------------------------------- reconstruction
def recon(x, t, kind="l_char", eps=1e-6, defect=None):
    d = x - t
    if kind == "l2":
        v = d * d
    elif kind == "l_char":
        v = torch.sqrt(d * d + (0.0 if defect == "eps_ignored" else eps))
    elif kind == "l1":
        v = d.abs() if defect == "l1_abs" else d
    else:
        raise ValueError(kind)
    if defect == "pixel_dropped":
        v = v.clone()
        v.reshape(-1)[v.numel() // 2] = 0
    return v.reshape(v.shape[0], -1).sum(dim=1).mean()


# ----------------------------------------------------------------------------- gradient loss
def gradient_loss(a, defect=None):
    gx = (a[:, :, :, :-1] - a[:, :, :, 1:]).abs()
    gy = (a[:, :, :-1, :] - a[:, :, 1:, :]).abs()
    if defect == "pixel_dropped":
        gx = gx.clone()
        gx[0, 0, gx.shape[2] // 2, gx.shape[3] // 2] = 0
    if defect == "row_dropped":
        gy = gy.clone()
        gy[:, :, _interior4(gy.shape[2])] = 0
    if defect == "swapped":       # each mean over the other direction's count
        return gx.sum() / gy.numel() + gy.sum() / gx.numel()
    return gx.mean() + gy.mean()


def _interior4(n):
    """an interior row index that is a multiple of 4 (a tile seam of the kernels)"""
    r = 4 * max(1, (n // 2) // 4)
    assert 0 < r < n
    return r


# ----------------------------------------------------------------------------- exclusion
def _pool(x, ceil=False):
    return torch.nn.functional.avg_pool2d(x, 2, stride=2, ceil_mode=ceil)


def exclusion_means(img1, img2, level=3, defect=None):
    """[level, 2, C1*C2] means of s1^2 s2^2"""
    C1, C2 = img1.shape[1], img2.shape[1]
    rows = []
    for l in range(level):
        per_dir = []
        for d in range(2):
            if (d == 0) != (defect == "swapped"):
                g1, g2 = img1[:, :, 1:, :] - img1[:, :, :-1, :], img2[:, :, 1:, :] - img2[:, :, :-1, :]
            else:
                g1, g2 = img1[:, :, :, 1:] - img1[:, :, :, :-1], img2[:, :, :, 1:] - img2[:, :, :, :-1]
            if l == 0 and d == 0 and defect == "pixel_dropped":
                g1 = g1.clone()
                g1[0, :, g1.shape[2] // 2, g1.shape[3] // 2] = 0
            if l == 0 and d == 0 and defect == "row_dropped":
                g1 = g1.clone()
                g1[:, :, _interior4(g1.shape[2])] = 0
            s1, s2 = 2 * torch.sigmoid(g1) - 1, 2 * torch.sigmoid(g2) - 1
            per_dir.append(torch.stack([(s1[:, k % C1] ** 2 * s2[:, k // C1] ** 2).mean() for k in range(C1 * C2)]))
        rows.append(torch.stack(per_dir))
        img1, img2 = _pool(img1, defect == "ceil_pool"), _pool(img2, defect == "ceil_pool")
    return torch.stack(rows)


def exclusion_from_means(means, level):
    pos = means > 0
    terms = torch.where(pos, means, torch.ones_like(means)) ** 0.25 * pos      # a vanished term: 0, with a zero gradient
    return (terms[:, 0].sum() + terms[:, 1].sum()) / (level * 9) / 2


def exclusion(img1, img2, level=3, want_terms=False, defect=None):
    means = exclusion_means(img1, img2, level, defect)
    loss = exclusion_from_means(means, level)
    return (loss, means) if want_terms else loss


def grad_of(fn, *xs, wrt=None):
    """gradients of the scalar fn(*xs) wrt xs[i] for i in wrt (default: all), through autograd"""
    xs = [x.detach().clone().requires_grad_(True) for x in xs]
    wrt = range(len(xs)) if wrt is None else wrt
    return torch.autograd.grad(fn(*xs), [xs[i] for i in wrt])


# ----------------------------------------------------------------------------- the comparisons of the GPU tests (CPU-tested on planted defects)
def rel_dev(got, want):
    """max |got - want| / |want| elementwise (float64 numpy in, NaN / inf -> inf)"""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.max(np.abs(got - want) / np.abs(want)))


def grad_dev(got, want):
    """max |got - want| / max |want|"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float("inf")
    m = float(np.max(np.abs(want)))
    assert m > 0
    return float(np.max(np.abs(got - want))) / m


def check_value(what, got, want, bound):
    d = rel_dev(got, want)
    print("%s rel %.3e (bound %.2e)" % (what, d, bound))
    assert d <= bound, (what, d, bound)
    return d


def check_grad(what, got, want, bound):
    d = grad_dev(got, want)
    print("%s grad %.3e of max |grad| (bound %.2e)" % (what, d, bound))
    assert d <= bound, (what, d, bound)
    return d


def bounds(g):
    """4 x the reference's own float32-vs-float64 deviation (the maxima stored in the fixture), per loss family and quantity"""
    return {k[len("dev_"):].replace("_max", ""): 4.0 * float(g[k]) for k in g.files if k.startswith("dev_") and "_max_" in k}
