"""CPU: the learning-rate schedules (models/lr_scheduler.py) without a GPU.
  * every case of tests/golden/lr_schedule.npz (recorded from the reference's MultiStepLR_Restart / CosineAnnealingLR_Restart over a
    torch.optim.Adam: make_golden_lr.py) is reproduced EXACTLY (==, no tolerance) on a minimal stand-in optimiser -- an object with
    `param_groups` -- and on torch.optim.Adam: the recurrences are the same Python-float expressions in the same order with the same
    math.cos, so there is nothing to tolerate.  Warm-up is applied by BaseModel.update_learning_rate itself;
  * state_dict() excludes the optimiser and, loaded into a new instance, continues the sequence exactly (cases g_*: the fixture's own
    sequence was resumed mid-run inside the reference);
  * clear_state: reset_state() of an optimiser that has it is called exactly at the restart steps, a torch optimiser's state is emptied;
  * construction: initial_lr set at last_epoch -1 and required otherwise, the initial step; a restart wins over a milestone;
  * a training section shaped like the reference's train_IRNrhi_x4.yml yields the expected class and arguments, an unknown scheme raises
    the reference's NotImplementedError, no scheme gives no scheduler; the C3 multi-step option file parses."""
import json
import os
import pickle
from collections import Counter, defaultdict

import numpy as np
import pytest
import torch

from video_watermarking_forgery_detection_amd.models import lr_scheduler as LS
from video_watermarking_forgery_detection_amd.models.base_model import BaseModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video_watermarking_forgery_detection_amd")
CASES = ("a", "b", "c", "d", "e_multi", "e_cos", "f", "g_multi", "g_cos")


class StandIn:
    """the least an optimiser must be: param_groups"""

    def __init__(self, lrs):
        self.param_groups = [{"lr": lr} for lr in lrs]


class Resettable(StandIn):
    """... with reset_state(): notes the step (`now`, set by the test) of every call"""

    def __init__(self, lrs):
        super().__init__(lrs)
        self.resets, self.now = [], 0

    def reset_state(self):
        self.resets.append(self.now)


def _steps(opt, sch, n):
    lrs = []
    for _ in range(n):
        opt.now = sch.last_epoch + 1
        sch.step()
        lrs.append(opt.param_groups[0]["lr"])
    return lrs


def _adam(lrs):
    return torch.optim.Adam([{"params": [torch.zeros(3, requires_grad=True)], "lr": lr} for lr in lrs], betas=(0.9, 0.99))


def _build(case, opt):
    args = dict(case["args"])
    if case["kind"] == "multistep":
        return LS.MultiStepLR_Restart(opt, args.pop("milestones"), **args)
    return LS.CosineAnnealingLR_Restart(opt, args.pop("T_period"), **args)


def _model(opt, sch):
    m = BaseModel({"gpu_ids": None, "is_train": True})
    m.optimizers, m.schedulers = [opt], [sch]
    return m


def _sequence(case, make_opt, resume=True):
    opt = make_opt(case["lrs"])
    m = _model(opt, _build(case, opt))
    rows = [[g["lr"] for g in opt.param_groups]]
    for i in range(1, case["steps"] + 1):
        m.update_learning_rate(i, warmup_iter=case["warmup"])
        rows.append([g["lr"] for g in opt.param_groups])
        if resume and case["resume_at"] == i:
            state, lrs = m.schedulers[0].state_dict(), [g["lr"] for g in opt.param_groups]
            assert "optimizer" not in state
            state = pickle.loads(pickle.dumps(state))   # plain data: survives a file
            opt = make_opt(case["lrs"])
            m = _model(opt, _build(case, opt))
            m.schedulers[0].load_state_dict(state)
            for g, lr in zip(opt.param_groups, lrs):   # (what optimizer.load_state_dict restores in a real resume)
                g["lr"] = lr
    return rows


@pytest.mark.parametrize("make_opt", [StandIn, _adam], ids=["stand-in", "torch-adam"])
@pytest.mark.parametrize("name", CASES)
def test_sequences_equal_the_reference_exactly(golden, name, make_opt):
    g = golden("lr_schedule")
    case = json.loads(str(g["cases"]))[name]
    want = g[name + "_lr"]
    assert want.dtype == np.float64 and want.shape == (case["steps"] + 1, len(case["lrs"]))
    got = _sequence(case, make_opt)
    for i, (row, ref) in enumerate(zip(got, want.tolist())):
        assert all(type(v) is float for v in row)
        assert row == ref, (name, i, row, ref)          # exact: == on Python floats
    assert len(got) == len(want)
    if case["resume_at"] is not None:                   # ... and the resumed sequence is the uninterrupted one
        assert _sequence(case, make_opt, resume=False) == got


def test_fixture_covers_what_it_must(golden):
    g = golden("lr_schedule")
    cases = json.loads(str(g["cases"]))
    assert set(cases) == set(CASES)
    a = cases["a"]["args"]
    assert max(Counter(a["milestones"]).values()) == 2 and a["gamma"] == 0.5 and "restarts" not in a
    assert cases["b"]["args"]["weights"] == [1, 0.5] and len(cases["b"]["args"]["restarts"]) == 2
    assert set(cases["c"]["args"]["milestones"]) & set(cases["c"]["args"]["restarts"])
    d = cases["d"]["args"]
    assert d == {"T_period": [10, 15, 20], "restarts": [10, 25], "weights": [1, 0.5], "eta_min": 1e-7}
    assert cases["d"]["steps"] > 25 + 1 + 20            # past (t - last_restart - 1 - T_max) % (2 T_max) == 0 at t = 46
    lr = g["d_lr"][:, 0]
    assert lr[45] == pytest.approx(1e-7, abs=1e-12) and lr[46] > lr[45]     # bottom of the last period, then the branch's step up
    assert len(cases["e_multi"]["lrs"]) == 2 and cases["f"]["warmup"] == 5 and cases["f"]["args"] == cases["a"]["args"]
    assert all(40 <= c["steps"] <= 60 for c in cases.values())
    # the repeated milestone applied gamma twice; the warm-up ramps linearly from 0
    assert g["a_lr"][12, 0] == g["a_lr"][11, 0] * 0.5 ** 2
    assert g["f_lr"][1:5, 0].tolist() == [2e-4 / 5 * i for i in range(1, 5)]


def test_state_dict_round_trip_continues_exactly(golden):
    g = golden("lr_schedule")
    for name in ("g_multi", "g_cos"):
        case = json.loads(str(g["cases"]))[name]
        want = g[name + "_lr"].tolist()
        opt = StandIn(case["lrs"])
        sch = _build(case, opt)
        k = case["resume_at"]
        for _ in range(k):
            sch.step()
        state = sch.state_dict()
        assert "optimizer" not in state and state["last_epoch"] == k
        if case["kind"] == "cosine":
            assert state["last_restart"] == 25 and state["T_max"] == 20
        else:
            assert state["milestones"] == Counter(case["args"]["milestones"])
        opt2 = StandIn(case["lrs"])
        sch2 = _build(case, opt2)
        sch2.load_state_dict(state)
        for g2, g1 in zip(opt2.param_groups, opt.param_groups):
            g2["lr"] = g1["lr"]
        assert sch2.state_dict() == state and sch2.optimizer is opt2
        for i in range(k + 1, case["steps"] + 1):
            sch2.step()
            assert [p["lr"] for p in opt2.param_groups] == want[i] == sch2.get_last_lr(), (name, i)


def test_construction_as_torch_base_class_does_it():
    opt = StandIn([2e-4, 1e-3])
    sch = LS.MultiStepLR_Restart(opt, [3], gamma=0.5)
    assert [g["initial_lr"] for g in opt.param_groups] == [2e-4, 1e-3] == sch.base_lrs
    assert sch.last_epoch == 0 and sch.get_last_lr() == [2e-4, 1e-3] and sch.get_lr() == [2e-4, 1e-3]
    assert sch.restarts == [0] and sch.restart_weights == [1] and sch.milestones == Counter([3]) and sch.clear_state is False
    with pytest.raises(KeyError, match="initial_lr"):
        LS.MultiStepLR_Restart(StandIn([1e-3]), [3], last_epoch=4)
    with pytest.raises(KeyError, match="initial_lr"):
        LS.CosineAnnealingLR_Restart(StandIn([1e-3]), [10], last_epoch=4)
    with pytest.raises(AssertionError, match="restarts and their weights do not match"):
        LS.MultiStepLR_Restart(StandIn([1e-3]), [3], restarts=[5, 9], weights=[1])
    # resumed construction: initial_lr given, the initial step lands on last_epoch + 1
    opt = StandIn([1e-3])
    opt.param_groups[0]["initial_lr"] = 4e-3
    sch = LS.MultiStepLR_Restart(opt, [5], gamma=0.5, last_epoch=4)
    assert sch.last_epoch == 5 and opt.param_groups[0]["lr"] == 1e-3 * 0.5 and sch.base_lrs == [4e-3]
    cos = LS.CosineAnnealingLR_Restart(StandIn([1e-3]), [10, 10], restarts=[10], weights=[1], eta_min=1e-7)
    assert (cos.T_period, cos.T_max, cos.eta_min, cos.last_restart, cos.restarts, cos.restart_weights) == ([10, 10], 10, 1e-7, 0, [10], [1])
    assert not isinstance(sch, torch.optim.lr_scheduler.LRScheduler)


def test_clear_state_resets_exactly_at_the_restart_steps():
    opt = Resettable([1e-3])
    sch = LS.MultiStepLR_Restart(opt, [3, 6], restarts=[8, 11], weights=[1, 0.5], gamma=0.5, clear_state=True)
    lrs = _steps(opt, sch, 14)
    assert opt.resets == [8, 11]
    assert lrs[6:11] == [2.5e-4, 1e-3, 1e-3, 1e-3, 5e-4]
    # without clear_state nothing is reset; the default restart at 0 resets at construction only
    opt = Resettable([1e-3])
    _steps(opt, LS.MultiStepLR_Restart(opt, [3], restarts=[8], weights=[1], clear_state=False), 10)
    assert opt.resets == []
    opt = Resettable([1e-3])
    _steps(opt, LS.MultiStepLR_Restart(opt, [3], clear_state=True), 5)
    assert opt.resets == [0]


def test_clear_state_empties_a_torch_optimisers_state():
    p = torch.zeros(3, requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-3)
    sch = LS.MultiStepLR_Restart(opt, [2], restarts=[4], weights=[0.5], clear_state=True)
    for step in range(1, 7):
        sch.step()
        if step == 4:
            assert len(opt.state) == 0 and isinstance(opt.state, defaultdict) and opt.param_groups[0]["lr"] == 5e-4
        p.grad = torch.ones(3)
        opt.step()
        assert float(opt.state[p]["step"]) == (step if step < 4 else step - 3)


def _train_section():
    """the training section of the reference's options/train/train_IRNrhi_x4.yml, as far as the learning rate goes"""
    return {"lr_G": 1e-4, "lr_D": 1e-4, "beta1": 0.9, "beta2": 0.5, "niter": 500000, "warmup_iter": -1, "lr_scheme": "MultiStepLR",
            "lr_steps": [20000, 40000, 60000, 80000, 100000, 120000, 140000, 160000, 180000, 200000], "lr_gamma": 0.5,
            "pixel_criterion_forw": "l2", "manual_seed": 10, "val_freq": 1000.0, "lambda_fit_forw": 16.0, "weight_decay_G": 1e-5,
            "gradient_clipping": 10}


def test_option_parsing():
    from video_watermarking_forgery_detection_amd.options import options
    opts = [StandIn([1e-4]), StandIn([1e-4]), StandIn([2e-4])]
    for section in (_train_section(), options.dict_to_nonedict(_train_section())):
        s = LS.build_schedulers(opts, section)
        assert [type(x) for x in s] == [LS.MultiStepLR_Restart] * 3 and [x.optimizer for x in s] == opts
        for x in s:
            assert x.milestones == Counter(_train_section()["lr_steps"]) and x.gamma == 0.5
            assert x.restarts == [0] and x.restart_weights == [1] and x.clear_state is False
    t = dict(_train_section(), restarts=[250000], restart_weights=[0.5], clear_state=True)
    (x,) = LS.build_schedulers(opts[:1], t)
    assert x.restarts == [250000] and x.restart_weights == [0.5] and x.clear_state is True
    t = dict(_train_section(), lr_scheme="CosineAnnealingLR_Restart", T_period=[250000, 250000], restarts=[250000], restart_weights=[1],
             eta_min=1e-7)
    (x,) = LS.build_schedulers(opts[:1], t)
    assert type(x) is LS.CosineAnnealingLR_Restart
    assert (x.T_period, x.restarts, x.restart_weights, x.eta_min, x.T_max) == ([250000, 250000], [250000], [1], 1e-7, 250000)
    with pytest.raises(NotImplementedError, match="MultiStepLR learning rate scheme is enough."):
        LS.build_schedulers(opts, dict(_train_section(), lr_scheme="StepLR"))
    none = {k: v for k, v in _train_section().items() if k != "lr_scheme"}
    assert LS.build_schedulers(opts, none) == [] == LS.build_schedulers(opts, options.dict_to_nonedict(none)) == LS.build_schedulers(opts, None)


def test_c3_multistep_configuration_parses_and_changes_the_rate():
    from video_watermarking_forgery_detection_amd.options import options
    opt = options.parse(os.path.join(PKG, "options", "train", "train_hidden_c3_multistep.yml"), is_train=True)
    base = options.parse(os.path.join(PKG, "options", "train", "train_hidden_c3.yml"), is_train=True)
    keys = ("lr_scheme", "lr_steps", "lr_gamma", "restarts", "restart_weights", "clear_state", "warmup_iter")
    assert {k: v for k, v in opt["train"].items() if k not in keys} == dict(base["train"]) and opt["datasets"] == base["datasets"]
    assert all(options.dict_to_nonedict(base)["train"][k] is None for k in keys)       # absent there: no scheduler
    o = StandIn([opt["train"]["lr_G"]])
    m = _model(o, *LS.build_schedulers([o], opt["train"]))
    seen = []
    for step in range(1, opt["train"]["niter"] + 1):
        m.update_learning_rate(step, warmup_iter=opt["train"]["warmup_iter"])
        seen.append(m.get_current_learning_rate())
    assert len(opt["train"]["restarts"]) == 1 and len(set(seen)) >= 3
    assert (seen[28], seen[29], seen[39], seen[48], seen[49], seen[59]) == (1e-3, 5e-4, 2.5e-4, 2.5e-4, 1e-3, 5e-4)
