"""What every trainer shares on the host: parameters and gradients in flat f32 buffers (flatten_parameters, FlatParameters, _flat_grad),
the one flat Adam / AdamW (FlatAdam: the only caller of the library's Adam kernels) and hipGraph capture of a step (no_gc, CapturedStep).
Imports ops alone: the layer toolkit (glayers), the engine and the trainers build on this module, never the other way round."""
import contextlib
import gc
import weakref

import torch

from . import ops


def flatten_parameters(params):
    """Move `params` into ONE new flat f32 buffer, in order: each p.data becomes a view of it (values kept bit for bit) and each p.grad a
    view of a second, zeroed buffer.  Returns (flat, gflat)."""
    params = list(params)
    n = sum(p.numel() for p in params)
    dev = params[0].device
    flat = torch.empty(n, device=dev, dtype=torch.float32)
    gflat = torch.zeros(n, device=dev, dtype=torch.float32)
    off = 0
    for p in params:
        k = p.numel()
        v = flat[off:off + k].view_as(p)
        v.copy_(p.data)
        p.data = v
        p.grad = gflat[off:off + k].view_as(p)
        off += k
    return flat, gflat


_FLAT_GRADS = {}      # parameter data_ptr -> (weakref flat parameters, weakref flat gradients, offset, numel) of a live FlatParameters


def _flat_grad(ptr, numel):
    """the slice of a live FlatParameters' gradient buffer that belongs to the parameter at address `ptr` (None if there is none: the
    buffers were collected -- their addresses may have been reused -- or the tensor is not a parameter of one)"""
    e = _FLAT_GRADS.get(ptr)
    if e is None:
        return None
    flat, grad = e[0](), e[1]()
    if flat is None or grad is None or e[3] != numel or flat.data_ptr() + 4 * e[2] != ptr:
        if flat is None or grad is None:
            del _FLAT_GRADS[ptr]
        return None
    return grad[e[2]:e[2] + e[3]]


class FlatParameters:
    """The trainable parameters of an nn.Module of the layer toolkit in ONE flat f32 buffer (`flat_params`; each nn.Parameter becomes a view of
    it) with their gradients in a second (`flat_grads`; each .grad a view of it, autograd accumulates in place), registered so that the
    convolution backward kernels ADD a parameter's gradient straight into the buffer (_flat_grad).  Frozen parameters (requires_grad False:
    UNetDiscriminator's SRMConv2D.weight) stay where they are.  `flat_params`, `flat_grads` and parameters() are what FlatAdam, gradient
    clipping and distributed.GradSync drive; zero_grad() is one memset."""

    def __init__(self, module, who="FlatParameters"):
        ps = [p for p in module.parameters() if p.requires_grad]
        if not ps or not all(p.is_cuda and p.dtype == torch.float32 for p in ps):
            raise RuntimeError(f"{who}: parameters must be float32 CUDA tensors (move the module to the GPU first)")
        self.module = module
        self.params = ps
        self.flat_params, self.flat_grads = flatten_parameters(ps)
        refs = (weakref.ref(self.flat_params), weakref.ref(self.flat_grads))
        for p in ps:
            _FLAT_GRADS[p.data_ptr()] = (*refs, (p.data_ptr() - self.flat_params.data_ptr()) // 4, p.numel())

    def parameters(self):
        return iter(self.params)

    def zero_grad(self):
        self.flat_grads.zero_()


class FlatAdam:
    """torch.optim.Adam defaults (hidden.py:24-25 of the reference), or AdamW with `decoupled`, over flat parameter buffers: `modules` are
    objects with flat_params / flat_grads / parameters() (engine.FlatModule networks, FlatParameters), one kernel launch per module.
    Exposes `param_groups` / `state_dict` enough for BaseModel-style lr handling, the schedulers and checkpoints."""

    def __init__(self, modules, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False):
        self.modules = list(modules)
        # one param group, torch's keys: what BaseModel's learning-rate handling and the schedulers (models/lr_scheduler.py) read and write
        self.param_groups = [{"lr": lr, "initial_lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay}]
        self.decoupled = decoupled
        self.step_count = 0
        self._m = None          # the moment buffers, one per module: allocated on first use by _ensure(), which a captured step's owner
        self._v = None          # calls BEFORE the capture
        self.amp = None         # the device-side scaler this optimiser steps through, and its slot there (attach_amp)
        self.amp_slot = None
        self.capturing = False  # True while a step is being CAPTURED into a hipGraph (_StepGraph): step() leaves step_count to the graph's owner,
        self.hyper_dev = None   # and launches the kernel that reads lr, betas, eps, weight_decay (and, without a scaler, the step-count-dependent
                                # constants) from this [ops.ADAM_HYPER] f32 device tensor, which the owner refreshes before each replay

    def _ensure(self):
        if self._m is None:
            self._m = [torch.zeros_like(m.flat_params) for m in self.modules]
            self._v = [torch.zeros_like(m.flat_params) for m in self.modules]

    def zero_grad(self):
        for m in self.modules:
            m.flat_grads.zero_()

    def attach_amp(self, amp):
        """run under a device-side GradScaler (ops.AmpState): the gradients arrive multiplied by its scale, the step divides it
        out, is skipped when they hold an inf / nan, and takes its bias corrections from the scaler's per-optimiser step count"""
        self.amp, self.amp_slot = amp, amp.slot()

    def step(self, grad_scale=1.0):
        self._ensure()
        if not self.capturing:
            self.step_count += 1
        g = self.param_groups[0]
        hyper = (g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"])
        kw = dict(decoupled=self.decoupled, grad_scale=grad_scale)
        if self.amp is not None:   # scaler.step(optimizer), IRNcrop_model.py:413-414
            self.amp.found_inf(self.amp_slot, [mod.flat_grads for mod in self.modules])
        for mod, m, v in zip(self.modules, self._m, self._v):
            bufs = (mod.flat_params, mod.flat_grads, m, v)
            if self.amp is not None:
                ops.adam_step_amp(*bufs, *hyper, self.amp, self.amp_slot, hyper_dev=self.hyper_dev, **kw)
            elif self.hyper_dev is not None:   # being captured: the numbers of step t come from device memory at replay time
                ops.adam_step_dev(*bufs, self.hyper_dev, **kw)
            else:
                ops.adam_step(*bufs, *hyper, self.step_count, **kw)

    def reset_state(self):
        """Adam from the start again: zero moments, step 0 -- what the reference's schedulers do to a torch optimiser at a restart with
        clear_state (lr_scheduler.py:22-23: `optimizer.state = defaultdict(dict)`).  Memsets on the current stream in the existing buffers,
        no host synchronisation; a captured step needs no recapture (it reads the moments through the same pointers and takes its
        bias corrections from the host's step count at each replay, _StepGraph._hyper_refresh -- under a scaler from the scaler's device-side
        count, zeroed here too)."""
        if self._m is not None:
            for t in self._m + self._v:
                t.zero_()
        self.step_count = 0
        if self.amp is not None:
            self.amp.state[12 + self.amp_slot:13 + self.amp_slot].zero_()

    def hyper(self, step):
        """the current param group and the constants adam_step derives from the step count (host arithmetic): what a captured step's
        replay needs in hyper_dev"""
        g = self.param_groups[0]
        return ops.adam_hyper(g["lr"], g["betas"][0], g["betas"][1], step, g["eps"], g["weight_decay"])

    def _params(self):
        return [p for mod in self.modules for p in mod.parameters()]

    def _slices(self):
        """every (parameter, its slice of the first-moment buffer, of the second), in parameters() order module by module"""
        for mod, m, v in zip(self.modules, self._m, self._v):
            off = 0
            for p in mod.parameters():
                yield p, m[off:off + p.numel()], v[off:off + p.numel()]
                off += p.numel()

    def _steps(self):
        """the steps taken so far: under a scaler its device-side count (a skipped step does not count)"""
        return self.amp.step_count(self.amp_slot) if self.amp is not None else self.step_count

    def state_dict(self):
        """torch.optim.Adam's layout (what the reference's `{iter}.state` files hold, base_model.py:129-150): per-parameter
        {step, exp_avg, exp_avg_sq} sliced out of the flat moment buffers in parameters() order, one param group."""
        self._ensure()
        steps = self._steps()
        state = {i: {"step": torch.tensor(float(steps)), "exp_avg": m.view_as(p).detach().cpu().clone(),
                     "exp_avg_sq": v.view_as(p).detach().cpu().clone()} for i, (p, m, v) in enumerate(self._slices())}
        g = dict(self.param_groups[0])
        group = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": g["weight_decay"], "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": bool(self.decoupled), "initial_lr": g.get("initial_lr", g["lr"]), "params": list(range(len(state)))}
        return {"state": state if steps else {}, "param_groups": [group]}

    def load_state_dict(self, sd):
        """accepts torch.optim.Adam / AdamW state_dicts (the reference's files) and the two flat layouts {step, param_groups, exp_avg,
        exp_avg_sq}: the moments as lists of one flat tensor per module, or (what FlatAdamW.state_dict writes) as single flat tensors for
        an optimiser over one module.  A state of another size is refused before anything is changed."""
        self._ensure()
        if "state" not in sd:
            ms, vs = sd["exp_avg"], sd["exp_avg_sq"]
            if torch.is_tensor(ms):
                if len(self.modules) != 1:
                    raise ValueError(f"optimizer state holds single flat moment tensors (one module), the optimiser has {len(self.modules)} modules")
                ms, vs = [ms], [vs]
            sizes = [t.numel() for t in self._m]
            if [t.numel() for t in ms] != sizes or [t.numel() for t in vs] != sizes:
                raise ValueError(f"optimizer state holds moments of {[t.numel() for t in ms]} / {[t.numel() for t in vs]} values, the modules have {sizes}")
            self._set_steps(int(sd["step"]))
            self._update_group(sd["param_groups"][0])
            for t, src in zip(self._m + self._v, list(ms) + list(vs)):
                t.copy_(src.reshape(-1))
            return
        groups = sd["param_groups"]
        if len(groups) != 1:
            raise ValueError("expected one param group (torch.optim.Adam over one parameter list)")
        for k in ("amsgrad", "maximize"):   # variants the kernel does not run: refused rather than continued as plain Adam
            if groups[0].get(k, False):
                raise ValueError(f"optimizer state uses {k}=True; the flat Adam step implements neither amsgrad nor maximize")
        params = self._params()
        ids = list(groups[0].get("params", range(len(params))))
        if len(ids) != len(params):
            raise ValueError(f"optimizer state has {len(ids)} parameters, the networks have {len(params)}")
        self._update_group(groups[0])
        state = sd["state"]
        steps = set()
        for i, (p, m, v) in enumerate(self._slices()):
            st = state.get(ids[i], state.get(str(ids[i])))
            if st is None:   # torch keeps no entry for a parameter that never received a gradient
                m.zero_(); v.zero_()
                continue
            if tuple(st["exp_avg"].shape) != tuple(p.shape):
                raise ValueError(f"optimizer state of parameter {i} has shape {tuple(st['exp_avg'].shape)}, expected {tuple(p.shape)}")
            m.copy_(st["exp_avg"].reshape(-1))
            v.copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"per-parameter step counts differ ({sorted(steps)}): the fused flat-buffer step keeps one count")
        self._set_steps(steps.pop() if steps else 0)

    def _set_steps(self, n):
        """the loaded step count: on the host, and -- under a scaler -- in the device slot adam_amp_kernel takes its bias correction's t from
        (a resumed f16 run otherwise stepped with t = 1 on warm moments: bc1 = 0.1, bc2 = 0.001 instead of ~1)"""
        self.step_count = n
        if self.amp is not None:
            self.amp.set_step_count(self.amp_slot, n)

    def _update_group(self, g):
        for k in ("lr", "betas", "eps", "weight_decay", "initial_lr"):
            if k in g:
                self.param_groups[0][k] = tuple(g[k]) if k == "betas" else g[k]
        if "decoupled_weight_decay" in g:
            self.decoupled = bool(g["decoupled_weight_decay"])


@contextlib.contextmanager
def no_gc():
    """Keep Python's cyclic collector out of a hipGraph capture: `with no_gc(), torch.cuda.graph(graph): ...`.  Whatever dead cycle the
    collector finds may own device memory, events or another hipGraph, and releasing those calls HIP functions that are illegal while a
    stream captures: the process aborts (seen with the previous test's model in a cycle).  torch 2.10's graph.__enter__ no longer collects
    first, so: collect now, switch the collector off for the block, and put it back as it was -- after an exception too."""
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


class CapturedStep:
    """A launch-bound step (the invertible embedder issues ~20,000 kernels of 3-20 us per forward + reverse + backward) captured ONCE into a
    hipGraph and replayed: `fn()` must be shape-static, read its inputs from tensors that are updated in place (copy_), and not synchronise
    with the host (no .item() / float()).  Gradients land in the parameters' existing .grad tensors (FlatAdamW's flat buffer), so
    zero_grad belongs INSIDE fn and the optimiser step -- whose bias correction depends on the host's step count -- outside:

        step = CapturedStep(lambda: fwd_bwd(x_static))      # two eager warm-up calls on a side stream, then the capture
        for batch in data: x_static.copy_(batch); step.replay(); opt.step()

    step.result holds what fn returned at capture (tensors that every replay overwrites).  Hand results out through that return value, or
    .detach() what fn stores elsewhere: an fn that keeps the autograd graph of its previous call alive (it rebinds an outer name, a dict
    entry, an attribute ... to a tensor that requires grad) is REFUSED with a RuntimeError before anything is captured.  Why: a graph that
    outlives its call keeps the AccumulateGrad node of every parameter it used alive, and the next call's graph picks those nodes up
    again, so they never die -- and a node runs on the stream that was current when it was CREATED.  When the first call ran eagerly on
    the default stream, the captured backward therefore makes the legacy default stream wait on an event of the capturing stream;
    CUDA invalidates such a capture with an error, hipStreamEndCapture on ROCm 7.2 ended it in a segmentation fault
    (round 2; tools/dbg_capture.py).  The check: before the last warm-up call the AccumulateGrad node of every CUDA
    parameter is tagged (Node.metadata); a node with no graph holding it dies with the tag, so a tag that is still there after the call's
    result has been dropped proves a leaked graph."""

    def __init__(self, fn, warmup=2):
        if not torch.cuda.is_available():
            raise RuntimeError("CapturedStep: GPU only")
        warmup = max(int(warmup), 2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        tag, key = object(), "wm_captured_step_probe"
        params = []

        def accumulator(p):
            return torch.autograd.graph.get_gradient_edge(p).node

        with torch.cuda.stream(side):
            for i in range(warmup):
                if i == warmup - 1:
                    gc.collect()
                    params = [o for o in gc.get_objects() if isinstance(o, torch.nn.Parameter) and o.is_cuda and o.requires_grad]
                    for p in params:
                        accumulator(p).metadata[key] = tag
                r = fn()
                del r
            gc.collect()
            leaked = [p for p in params if accumulator(p).metadata.get(key) is tag]
        torch.cuda.current_stream().wait_stream(side)
        if leaked:
            raise RuntimeError(
                f"CapturedStep: fn keeps the autograd graph of its previous call alive (the AccumulateGrad nodes of {len(leaked)} of {len(params)} "
                "parameters survive the call): it stores a tensor that requires grad outside itself (an outer variable, a dict entry, an "
                "attribute).  Return such tensors from fn (step.result) or .detach() them; capturing this fn can crash the process inside "
                "hipStreamEndCapture")
        self.graph = torch.cuda.CUDAGraph()
        with no_gc(), torch.cuda.graph(self.graph):
            self.result = fn()

    def replay(self):
        self.graph.replay()
        return self.result
