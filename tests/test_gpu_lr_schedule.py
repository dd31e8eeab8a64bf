"""GPU: the learning-rate schedules (models/lr_scheduler.py) through the optimisers' device-side path -- the first client of the
hyperparameter block a replayed step reads (_StepGraph._hyper_refresh, wm_adam_step_dev / wm_adam_step_amp).

One schedule throughout: MultiStepLR_Restart, milestones [3, 6], gamma 0.5, a restart at 8 (weight 1), 12 steps, every scheduler stepped
BEFORE its training step as train.py does (update_learning_rate, then optimize_parameters).  Step s therefore runs at
    s = 1, 2: lr0     3, 4, 5: lr0 / 2     6, 7: lr0 / 4     8 ... 12: lr0   (halving is exact in binary, so the list below is exact)
and a clear_state restart empties Adam's state between steps 7 and 8: step 8 is the fresh optimiser's step 1, step 9 its step 2.

  * eager: after EVERY step the encoder-decoder optimiser's update is replayed on copies of (p, m, v) taken before the step with the core
    kernel wm_adam_step, the scheduled lr and the step's own gradients -- bit for bit;
  * replayed (enable_graph) against eager: every parameter, buffer, gradient, moment and step count equal after step 12; equal to a
    constant-lr run after step 2 and different from it after step 4 (a pure replay: the capture is call 3) -- the replay read the new value;
  * clear_state, eager and replayed, without a recapture: the moments are zero and the count 0 before step 8; after step 8 (p, m, v) are
    wm_adam_step with step 1 on zeroed moments, after step 9 that state stepped once more with step 2 -- bit for bit;
  * the same under f16 with the device-side GradScaler: the scaler's per-optimiser step count restarts too, checked through
    wm_adam_step_amp's bias correction (a reference scaler state with count 0, then 1);
  * resume through the model surface: training state saved at step 5, a new model resumed from it and run to 12 equals the uninterrupted
    run bit for bit, and the logged `lr` follows the schedule on both.

Shapes: 2 x 3 x 32 x 32 in f32 under JpegMask(50), the smallest step tests/test_gpu_graph.py builds and captures; the f16 scaler case runs
at 2 x 3 x 64 x 64 under JpegSS(50), the smallest f16 step that file captures.  No two-rank (gloo) comparison is made: the learning rate
is host arithmetic on the options every rank parses, no collective is involved, and a two-process GPU launcher is not what these tests
are about."""
import functools

import pytest
import torch

import detgen

pytestmark = pytest.mark.gpu

NSTEP, LR0 = 12, 2e-3
SCHEDULE = dict(milestones=[3, 6], gamma=0.5, restarts=[8], weights=[1])
LRS = [None, LR0, LR0, LR0 / 2, LR0 / 2, LR0 / 2, LR0 / 4, LR0 / 4, LR0, LR0, LR0, LR0, LR0]     # LRS[s]: the rate step s runs at
SHAPES = {"f32": (32, 2, torch.float32), "f16": (64, 2, torch.float16)}


@functools.lru_cache(maxsize=None)
def _batch(kind, step):
    S, B, _ = SHAPES[kind]
    return detgen.uniform((B, 3, S, S), 9000 + step).cuda(), detgen.bits((B, 30), 9100 + step).cuda()


def _make(kind, graph=False, scheduled=True, clear_state=False):
    from video_watermarking_forgery_detection_amd import noise_layers as NL, ops
    from video_watermarking_forgery_detection_amd.hidden_models import Hidden
    from video_watermarking_forgery_detection_amd.models.lr_scheduler import MultiStepLR_Restart
    from video_watermarking_forgery_detection_amd.options import HiDDenConfiguration
    S, B, dt = SHAPES[kind]
    amp = ops.AmpState(torch.device("cuda")) if kind == "f16" else None
    noise = NL.JpegMask(50) if kind == "f32" else NL.JpegSS(50)
    h = Hidden(HiDDenConfiguration(H=S, W=S), torch.device("cuda"), noise, None, compute_dtype=dt, amp=amp)
    for m in (h.encoder_decoder.encoder, h.encoder_decoder.decoder, h.discriminator):
        detgen.fill_module(m)
    opts = (h.optimizer_enc_dec, h.optimizer_discrim)
    for o in opts:
        o.param_groups[0].update(lr=LR0, initial_lr=LR0)
    if graph:
        h.enable_graph()
    h.schedulers = [MultiStepLR_Restart(o, SCHEDULE["milestones"], restarts=SCHEDULE["restarts"], weights=SCHEDULE["weights"],
                                        gamma=SCHEDULE["gamma"], clear_state=clear_state) for o in opts] if scheduled else []
    return h


def _step(h, kind, step):
    for s in h.schedulers:      # BaseModel.update_learning_rate without a warm-up
        s.step()
    x, msg = _batch(kind, step)
    return h.train_on_batch([x, msg])


def _state(h):
    out = {}
    for k, m in (("E", h.encoder_decoder.encoder), ("Dec", h.encoder_decoder.decoder), ("D", h.discriminator)):
        for n, t in m.state_dict().items():
            out[f"{k}.{n}"] = t.detach().clone()
        out[f"{k}.grad"] = m.flat_grads.detach().clone()
    for k, o in (("optD", h.optimizer_discrim), ("optED", h.optimizer_enc_dec)):
        for i, (m, v) in enumerate(zip(o._m, o._v)):
            out[f"{k}.m{i}"], out[f"{k}.v{i}"] = m.detach().clone(), v.detach().clone()
        out[f"{k}.steps"] = torch.tensor(o.step_count)
    if h.amp is not None:
        out["amp"] = h.amp.state.detach().clone()
    return out


def _params(h):
    return torch.cat([m.flat_params.detach().clone() for m in (h.encoder_decoder.encoder, h.encoder_decoder.decoder, h.discriminator)])


def _pmv(o):
    """copies of the optimiser's (p, m, v) per module"""
    o._ensure()
    return [(mod.flat_params.detach().clone(), m.detach().clone(), v.detach().clone()) for mod, m, v in zip(o.modules, o._m, o._v)]


def _grads(o):
    return [mod.flat_grads.detach().clone() for mod in o.modules]


def _same(name, got, want, ctx):
    for i, (a, b) in enumerate(zip(got, want)):
        for nm, x, y in zip("pmv", a, b):
            assert torch.equal(x, y), f"{name} {ctx}: {nm} of module {i} differs in {int((x != y).sum())} of {x.numel()} elements"


def _core_step(ops, pmv, grads, group, lr, t):
    """wm_adam_step on the copies: the core kernel with the scheduled lr and step count t"""
    for (p, m, v), g in zip(pmv, grads):
        ops.adam_step(p, g, m, v, lr, group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"], t)
    return pmv


@functools.lru_cache(maxsize=None)
def _eager_reference(clear_state):
    """the eagerly enqueued scheduled f32 run, computed once: its state after step 12, its parameters after steps 2 and 4"""
    h = _make("f32", clear_state=clear_state)
    params = {}
    for step in range(1, NSTEP + 1):
        _step(h, "f32", step)
        if step in (2, 4):
            params[step] = _params(h)
    return _state(h), params


def test_eager_steps_run_at_the_scheduled_rate_bit_for_bit():
    from video_watermarking_forgery_detection_amd import ops
    h = _make("f32")
    o = h.optimizer_enc_dec
    for step in range(1, NSTEP + 1):
        before = _pmv(o)
        _step(h, "f32", step)
        for opt in (o, h.optimizer_discrim):
            assert opt.param_groups[0]["lr"] == LRS[step], (step, opt.param_groups[0]["lr"])
        assert o.step_count == step
        want = _core_step(ops, before, _grads(o), o.param_groups[0], LRS[step], step)
        _same("eager", _pmv(o), want, f"after step {step} at lr {LRS[step]}")
    final, _ = _eager_reference(False)
    got = _state(h)
    for k in final:
        assert torch.equal(final[k], got[k]), k           # (and the run is reproducible: the shared reference is this run)


def test_replayed_steps_follow_the_schedule_and_equal_the_eager_run():
    final, params = _eager_reference(False)
    graph, const = _make("f32", graph=True), _make("f32", scheduled=False)
    for step in range(1, NSTEP + 1):
        _step(graph, "f32", step)
        if step <= 4:
            _step(const, "f32", step)
        if step == 2:
            assert torch.equal(_params(graph), params[2]) and torch.equal(_params(const), params[2])
        if step == 4:      # a replay (the capture is call 3) at lr0 / 2: the constant-lr run has left
            assert torch.equal(_params(graph), params[4])
            assert not torch.equal(_params(const), params[4])
    (g,) = graph._graphs.values()
    assert g.failed is None and g.graph is not None and g.calls == NSTEP
    got = _state(graph)
    assert got.keys() == final.keys()
    for k in final:
        assert torch.equal(final[k], got[k]), k


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "replayed"])
def test_clear_state_restart_starts_adam_again(graph):
    from video_watermarking_forgery_detection_amd import ops
    h = _make("f32", graph=graph, clear_state=True)
    o = h.optimizer_enc_dec
    captured = None
    for step in range(1, NSTEP + 1):
        if step in (8, 9):
            for s in h.schedulers:
                s.step()
            if step == 8:      # the restart has just cleared the state, in place
                captured = next(iter(h._graphs.values())).graph if graph else None
                for opt in (o, h.optimizer_discrim):
                    assert opt.step_count == 0
                    assert all(int(torch.count_nonzero(t)) == 0 for t in opt._m + opt._v)
                ref = _pmv(o)
            else:
                assert o.step_count == 1
                for (p, _, _), (q, _, _) in zip(ref, _pmv(o)):
                    assert torch.equal(p, q)
            h.train_on_batch(list(_batch("f32", step)))
            ref = _core_step(ops, ref, _grads(o), o.param_groups[0], LRS[step], step - 7)     # t = 1, then t = 2
            _same("clear_state", _pmv(o), ref, f"after step {step}")
            assert int(torch.count_nonzero(o._m[0])) > 0
        else:
            _step(h, "f32", step)
    assert o.step_count == NSTEP - 7 == h.optimizer_discrim.step_count
    if graph:
        (g,) = h._graphs.values()
        assert g.failed is None and g.graph is captured and g.calls == NSTEP       # one capture served the restart
    final, _ = _eager_reference(True)
    kept, _ = _eager_reference(False)
    got = _state(h)
    for k in final:
        assert torch.equal(final[k], got[k]), k
    assert not torch.equal(final["optED.m0"], kept["optED.m0"])                    # (the restart is not a no-op)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "replayed"])
def test_clear_state_restart_under_the_scaler_restarts_the_device_step_count(graph):
    from video_watermarking_forgery_detection_amd import ops
    h = _make("f16", graph=graph, clear_state=True)
    o, amp = h.optimizer_enc_dec, h.amp
    k = o.amp_slot
    ref_amp = ops.AmpState(torch.device("cuda"))
    for _ in range(amp.nopt):
        ref_amp.slot()
    taken = 0      # steps a fresh optimiser has taken since the restart (the scaler skips a step whose gradients hold an inf / nan)
    for step in range(1, NSTEP + 1):
        if step not in (8, 9):
            _step(h, "f16", step)
            continue
        counts = [amp.step_count(opt.amp_slot) for opt in (o, h.optimizer_discrim)]
        for s in h.schedulers:
            s.step()
        if step == 8:
            assert min(counts) > 0, counts                    # the scaler let steps through before the restart ...
            assert [amp.step_count(opt.amp_slot) for opt in (o, h.optimizer_discrim)] == [0, 0]     # ... and both counts restart
            assert all(int(torch.count_nonzero(t)) == 0 for t in o._m + o._v)
            ref = _pmv(o)
        scaler_before = amp.state.detach().clone()
        h.train_on_batch(list(_batch("f16", step)))
        # the reference: wm_adam_step_amp under a scaler state that differs from the real one only in holding the count a FRESH optimiser has
        ref_amp.state.copy_(scaler_before)
        ref_amp.state[12 + k] = float(taken)
        grads = _grads(o)
        ref_amp.found_inf(k, grads)
        skipped = float(ref_amp.state[8 + k]) != 0.0
        g = o.param_groups[0]
        for (p, m, v), gr in zip(ref, grads):
            ops.adam_step_amp(p, gr, m, v, LRS[step], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], ref_amp, k)
        taken += 0 if skipped else 1
        print(f"step {step}: scale {float(scaler_before[0])}, skipped {skipped}, device step count {amp.step_count(k)}")
        assert amp.step_count(k) == taken, (step, amp.step_count(k), taken)
        _same("clear_state under the scaler", _pmv(o), ref, f"after step {step}")
    assert taken == 2, "the scaler skipped a step after the restart (inf / nan gradients): the bias-correction comparison needs taken steps"
    if graph:
        (gr,) = h._graphs.values()
        assert gr.failed is None and gr.graph is not None and gr.calls == NSTEP


def test_resumed_run_equals_the_uninterrupted_run(tmp_path):
    import os
    from video_watermarking_forgery_detection_amd.models.IRNrhi_model import IRNrhiModel
    from video_watermarking_forgery_detection_amd.options.options import dict_to_nonedict
    S, B, _ = SHAPES["f32"]

    def make(resume_from=None):
        path = {"models": str(tmp_path / "models"), "training_state": str(tmp_path / "state")}
        if resume_from is not None:
            path.update({"pretrain_model_" + n: os.path.join(path["models"], f"{resume_from}_{n}.pth") for n in ("encoder", "decoder", "discriminator")})
        opt = dict_to_nonedict({"gpu_ids": [0], "dist": False, "is_train": True, "datasets": {"train": {"GT_size": S, "batch_size": B}},
                                "train": {"compute_dtype": "f32", "attacks": ["JpegMask50"], "lr_G": LR0, "manual_seed": 10, "save_interval": 3000,
                                          "localizer": False, "lr_scheme": "MultiStepLR", "lr_steps": SCHEDULE["milestones"],
                                          "lr_gamma": SCHEDULE["gamma"], "restarts": SCHEDULE["restarts"], "restart_weights": SCHEDULE["weights"],
                                          "clear_state": True},
                                "path": path})
        m = IRNrhiModel(opt)
        assert len(m.schedulers) == len(m.optimizers) == 2 and m.hidden._graphs is not None
        if resume_from is None:
            for net in (m.netG.encoder, m.netG.decoder, m.discriminator):
                detgen.fill_module(net)
        for _ in range(2):      # the surface trains once two previous batches exist (IRNrhi_model.py:446)
            m.feed_data(_batch("f32", 0)[0])
            assert m.optimize_parameters(0, None)[0] == []
        return m

    def run(m, first, last, save_at=None):
        for step in range(first, last + 1):
            m.update_learning_rate(step, warmup_iter=-1)
            x, msg = _batch("f32", step)
            m.feed_data(x)
            m.messages = msg
            logs, _ = m.optimize_parameters(step, None)
            assert dict(logs)["lr"] == LRS[step] == m.get_current_learning_rate(), (step, dict(logs)["lr"])
            if step == save_at:
                m.save(step)
                return m.save_training_state(0, step)

    whole = make()
    state_path = run(whole, 1, 5, save_at=5)
    run(whole, 6, NSTEP)
    resumed = make(resume_from=5)
    state = torch.load(state_path, map_location="cpu", weights_only=False)
    assert len(state["schedulers"]) == 2 and state["schedulers"][0]["last_epoch"] == 5 and "optimizer" not in state["schedulers"][0]
    resumed.resume_training(state)
    assert resumed.get_current_learning_rate() == LRS[5] and resumed.schedulers[0].last_epoch == 5
    run(resumed, 6, NSTEP)
    a, b = _state(whole.hidden), _state(resumed.hidden)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert whole.hidden.optimizer_enc_dec.step_count == NSTEP - 7         # (the restart at 8 cleared the resumed run's loaded state too)
