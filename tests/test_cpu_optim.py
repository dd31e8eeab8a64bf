"""CPU: the host-side training machinery of optim.py that needs no device and launches nothing -- the one slice-and-repoint loop
(flatten_parameters), the graph-capture guard's handling of Python's cyclic collector (no_gc), and the three state_dict layouts
FlatAdam.load_state_dict accepts (torch's, the flat one with lists of tensors, FlatAdamW's flat one with single tensors)."""
import gc

import pytest
import torch
import torch.nn as nn

from video_watermarking_forgery_detection_amd.optim import FlatAdam, flatten_parameters, no_gc


class _Flat:
    """what FlatAdam drives: flat_params, flat_grads, parameters() (an engine.FlatModule network or a FlatParameters on the device)"""

    def __init__(self, net):
        self.params = list(net.parameters())
        self.flat_params, self.flat_grads = flatten_parameters(self.params)

    def parameters(self):
        return iter(self.params)


def _stand_in(seed, n_in=5, n_out=3):
    torch.manual_seed(seed)
    return _Flat(nn.Linear(n_in, n_out))


def test_flatten_parameters_repoints_data_and_grad_at_slices():
    torch.manual_seed(0)
    lin = nn.Linear(5, 3)
    params = list(lin.parameters())
    before = [p.detach().clone() for p in params]
    flat, gflat = flatten_parameters(params)
    assert flat.dtype == torch.float32 and flat.numel() == gflat.numel() == 5 * 3 + 3
    assert int(torch.count_nonzero(gflat)) == 0
    off = 0
    for p, b in zip(params, before):
        assert p.data_ptr() == flat.data_ptr() + 4 * off
        assert p.grad.data_ptr() == gflat.data_ptr() + 4 * off and p.grad.shape == p.shape
        assert torch.equal(p.detach(), b)                                   # bit for bit
        assert torch.equal(flat[off:off + p.numel()].view_as(p), b)
        off += p.numel()
    flat.fill_(2.5)                                                         # writing the buffer changes the parameter ...
    assert all(bool((p == 2.5).all()) for p in params)
    gflat.fill_(-1.0)                                                       # ... and the gradient buffer the .grad
    assert all(bool((p.grad == -1.0).all()) for p in params)
    (lin(torch.ones(2, 5)).sum()).backward()                                # autograd accumulates in place, into the buffer
    assert torch.equal(gflat[15:], torch.full((3,), 1.0))


@pytest.mark.parametrize("start_enabled", [True, False])
@pytest.mark.parametrize("raises", [False, True])
def test_no_gc_switches_the_collector_off_and_puts_it_back(start_enabled, raises):
    was = gc.isenabled()
    try:
        gc.enable() if start_enabled else gc.disable()
        if raises:
            with pytest.raises(KeyError):
                with no_gc():
                    assert not gc.isenabled()
                    raise KeyError("body")
        else:
            with no_gc():
                assert not gc.isenabled()
        assert gc.isenabled() == start_enabled
    finally:
        gc.enable() if was else gc.disable()


def _fill_moments(opt, seed):
    opt._ensure()
    g = torch.Generator().manual_seed(seed)
    for t in opt._m + opt._v:
        t.copy_(torch.rand(t.shape, generator=g))


def test_torch_layout_round_trips():
    a = FlatAdam([_stand_in(1), _stand_in(2, 4, 2)], lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.02, decoupled=True)
    _fill_moments(a, 7)
    a.step_count = 9
    sd = a.state_dict()
    assert set(sd) == {"state", "param_groups"} and len(sd["state"]) == 4
    b = FlatAdam([_stand_in(3), _stand_in(4, 4, 2)])
    b.load_state_dict(sd)
    assert b.step_count == 9 and b.decoupled is True
    assert b.param_groups[0] == a.param_groups[0]
    for x, y in zip(a._m + a._v, b._m + b._v):
        assert torch.equal(x, y)


def test_flat_layouts_load_the_hand_filled_moments():
    group = {"lr": 1e-4, "betas": (0.7, 0.9), "eps": 1e-7, "weight_decay": 0.03}
    src = FlatAdam([_stand_in(1), _stand_in(2, 4, 2)])
    _fill_moments(src, 11)
    # lists of one flat tensor per module
    sd = {"step": 5, "param_groups": [dict(group)], "exp_avg": [t.clone() for t in src._m], "exp_avg_sq": [t.clone() for t in src._v]}
    dst = FlatAdam([_stand_in(3), _stand_in(4, 4, 2)])
    dst.load_state_dict(sd)
    assert dst.step_count == 5 and all(dst.param_groups[0][k] == v for k, v in group.items())
    for x, y in zip(src._m + src._v, dst._m + dst._v):
        assert torch.equal(x, y)
    # single flat tensors (FlatAdamW.state_dict): the one-module case
    one = {"step": 6, "param_groups": [dict(group)], "exp_avg": src._m[0].clone(), "exp_avg_sq": src._v[0].clone()}
    dst1 = FlatAdam([_stand_in(5)])
    dst1.load_state_dict(one)
    assert dst1.step_count == 6 and dst1.param_groups[0]["lr"] == 1e-4
    assert torch.equal(dst1._m[0], src._m[0]) and torch.equal(dst1._v[0], src._v[0])
    # ... refused, with a message, by an optimiser over two modules -- and nothing of it is taken over
    two = FlatAdam([_stand_in(6), _stand_in(7, 4, 2)])
    with pytest.raises(ValueError, match="one module"):
        two.load_state_dict(one)
    assert two.step_count == 0 and two.param_groups[0]["lr"] == 1e-3 and int(torch.count_nonzero(two._m[0])) == 0


@pytest.mark.parametrize("layout", ["single", "list", "torch"])
def test_a_moment_tensor_of_the_wrong_size_is_refused(layout):
    group = {"lr": 1e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0}
    opt = FlatAdam([_stand_in(1)])            # 18 values
    n = opt.modules[0].flat_params.numel()
    good, bad = torch.ones(n), torch.ones(n - 1)
    if layout == "single":
        sds = [{"step": 1, "param_groups": [group], "exp_avg": bad, "exp_avg_sq": good},
               {"step": 1, "param_groups": [group], "exp_avg": good, "exp_avg_sq": bad}]
    elif layout == "list":
        sds = [{"step": 1, "param_groups": [group], "exp_avg": [bad], "exp_avg_sq": [good]},
               {"step": 1, "param_groups": [group], "exp_avg": [good], "exp_avg_sq": [bad]},
               {"step": 1, "param_groups": [group], "exp_avg": [good, good], "exp_avg_sq": [good, good]}]
    else:
        sd = FlatAdam([_stand_in(2, 4, 3)]).state_dict()      # a weight of another shape
        sd["state"] = {i: {"step": torch.tensor(1.0), "exp_avg": torch.ones_like(p), "exp_avg_sq": torch.ones_like(p)}
                       for i, p in enumerate(_stand_in(2, 4, 3).parameters())}
        sds = [sd]
    for sd in sds:
        with pytest.raises(ValueError):
            opt.load_state_dict(sd)
        if layout != "torch":
            assert opt.step_count == 0 and opt.param_groups[0]["lr"] == 1e-3 and int(torch.count_nonzero(opt._m[0])) == 0
