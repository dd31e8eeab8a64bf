#!/usr/bin/env python3
"""Generate tests/golden/lr_schedule.npz from the REFERENCE's models/lr_scheduler.py (imported unmodified; torch and numpy suffice).

Runs only where the reference tree exists, like make_golden_dice.py.  Its two classes, MultiStepLR_Restart and CosineAnnealingLR_Restart,
drive a torch.optim.Adam on the CPU; after construction and after every step() the learning rate of every param group is recorded as
float64 (a Python float, unchanged).  The file holds, per case, `<case>_lr` [steps + 1, groups] (row 0: after construction) and, under
`cases`, one JSON text with every case's settings -- the test builds its schedulers from that text, so fixture and test cannot drift apart:

    kind        'multistep' | 'cosine'
    lrs         the param groups' learning rates
    args        the scheduler's keyword arguments (milestones / T_period, restarts, weights, gamma, eta_min)
    steps       number of step() calls
    warmup      warm-up length w: after step() number i < w every group's rate is set to initial_lr / w * i, the way
                BaseModel.update_learning_rate(i, w) does it (base_model.py:51-61); -1: none
    resume_at   k or null: after step k the scheduler's state_dict() and the groups' rates are taken, a NEW optimiser and scheduler are
                built, given both (optimizer.load_state_dict carries 'lr' in a real run), and the sequence continues on them

Cases: a  milestones with one repeated, gamma 0.5          b  two restarts, weights [1, 0.5]        c  b with a milestone ON a restart step
       d  cosine, T_period [10, 15, 20], restarts [10, 25], weights [1, 0.5], eta_min 1e-7, 60 steps: passes (t - 1 - T) % (2 T) == 0 at 46
       e_multi, e_cos  two param groups with different rates       f  a with a warm-up over the first 5 steps
       g_multi, g_cos  b and d continued from a state_dict() taken mid-run (asserted equal to the uninterrupted sequence here)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lr.py REFERENCE_ROOT
"""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

MULTI_B = dict(milestones=[4, 9, 17, 24, 31], restarts=[15, 30], weights=[1, 0.5], gamma=0.3)
COS_D = dict(T_period=[10, 15, 20], restarts=[10, 25], weights=[1, 0.5], eta_min=1e-7)
CASES = {
    "a": dict(kind="multistep", lrs=[2e-4], args=dict(milestones=[5, 12, 12, 20, 33], gamma=0.5), steps=40, warmup=-1, resume_at=None),
    "b": dict(kind="multistep", lrs=[2e-4], args=MULTI_B, steps=45, warmup=-1, resume_at=None),
    "c": dict(kind="multistep", lrs=[2e-4], args=dict(MULTI_B, milestones=[4, 9, 15, 17, 24, 31]), steps=45, warmup=-1, resume_at=None),
    "d": dict(kind="cosine", lrs=[2e-4], args=COS_D, steps=60, warmup=-1, resume_at=None),
    "e_multi": dict(kind="multistep", lrs=[2e-4, 1e-3], args=MULTI_B, steps=45, warmup=-1, resume_at=None),
    "e_cos": dict(kind="cosine", lrs=[2e-4, 1e-3], args=COS_D, steps=60, warmup=-1, resume_at=None),
    "f": dict(kind="multistep", lrs=[2e-4], args=dict(milestones=[5, 12, 12, 20, 33], gamma=0.5), steps=40, warmup=5, resume_at=None),
    "g_multi": dict(kind="multistep", lrs=[2e-4], args=MULTI_B, steps=45, warmup=-1, resume_at=20),
    "g_cos": dict(kind="cosine", lrs=[2e-4, 1e-3], args=COS_D, steps=60, warmup=-1, resume_at=30),
}


def build(ref, case):
    opt = torch.optim.Adam([{"params": [torch.zeros(3, requires_grad=True)], "lr": lr} for lr in case["lrs"]], betas=(0.9, 0.99))
    args = dict(case["args"])
    if case["kind"] == "multistep":
        return opt, ref.MultiStepLR_Restart(opt, args.pop("milestones"), **args)
    return opt, ref.CosineAnnealingLR_Restart(opt, args.pop("T_period"), **args)


def run(ref, case, resume=True):
    opt, sch = build(ref, case)
    rows = [[g["lr"] for g in opt.param_groups]]
    w = case["warmup"]
    for i in range(1, case["steps"] + 1):
        sch.step()
        if i < w:
            for g in opt.param_groups:
                g["lr"] = g["initial_lr"] / w * i
        rows.append([g["lr"] for g in opt.param_groups])
        if resume and case["resume_at"] == i:
            state, lrs = sch.state_dict(), [g["lr"] for g in opt.param_groups]
            opt, sch = build(ref, case)
            sch.load_state_dict(state)
            for g, lr in zip(opt.param_groups, lrs):
                g["lr"] = lr
    assert all(type(v) is float for r in rows for v in r)
    return np.array(rows, dtype=np.float64)


def main(ref_root):
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_lr_scheduler", os.path.join(ref_root, "models", "lr_scheduler.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    warnings.simplefilter("ignore")   # torch warns that scheduler.step() comes before optimizer.step(): no optimiser step is taken here
    out = {"cases": np.array(json.dumps(CASES, sort_keys=True))}
    for name, case in CASES.items():
        out[name + "_lr"] = run(ref, case)
        if case["resume_at"] is not None:
            assert np.array_equal(out[name + "_lr"], run(ref, case, resume=False)), name
        print(name, out[name + "_lr"].shape, "last", out[name + "_lr"][-1])
    path = os.path.join(HERE, "lr_schedule.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_lr.py REFERENCE_ROOT (the reference repository's checkout)")
    main(sys.argv[1])
