"""Hidden -- the GAN training step of the reference's hidden_models/hidden.py:12-118 on the MI355X
kernels: same constructor, `train_on_batch([images, messages])` / `validate_on_batch(...)` returning
(losses dict with the reference's keys, (encoded, noised, decoded)), same order of operations:

    D(cover) -> BCE(1) -> bwd | enc -> noise -> dec | D(enc.detach()) -> BCE(0) -> bwd | Adam(D)
    | D(enc) -> adv*BCE(1) + enc*MSE(enc, img) + dec*MSE(dec, msg) -> bwd | Adam(enc+dec)

The backward is written out (engine.py) instead of traced by autograd, every heavy op is a HIP kernel
behind the C ABI, parameters/gradients/moments of each optimiser live in flat f32 buffers (one fused
Adam launch, one RCCL bucket for data parallel), and the seven logged scalars are fetched with a
single asynchronous copy that the host waits for only when a value is read (StepLosses).
"""
import collections.abc
import itertools

import torch
import torch.nn.functional as F

from .. import engine, ops
from ..noise_layers._device_rng import accepts_cover
from ..optim import FlatAdam, no_gc
from ..options import HiDDenConfiguration
from .discriminator import Discriminator
from .encoder_decoder import EncoderDecoder


LOSS_KEYS = ('loss           ', 'encoder_mse    ', 'dec_mse        ', 'bitwise-error  ', 'adversarial_bce', 'discr_cover_bce',
             'discr_encod_bce')   # hidden.py:105-113


class StepLosses(collections.abc.Mapping):
    """The reference's losses dict (hidden.py:105-113: name -> float), fetched from the device on first access.

    The seven scalars of a step are copied to pinned host memory asynchronously; reading any value (items(), [], ...)
    waits for that copy.  A training loop that logs every step behaves exactly like the reference's; one that only looks
    at the losses now and then (bench.py, print_each) no longer drains the GPU queue once per step."""

    def __init__(self, dev_vals, extra=None):
        self._host = torch.empty(len(LOSS_KEYS), dtype=torch.float32, pin_memory=True)
        self._host.copy_(dev_vals, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record()
        self._vals = None
        self._extra = extra

    def _resolve(self):
        if self._vals is None:
            self._event.synchronize()
            self._vals = dict(zip(LOSS_KEYS, self._host.tolist()))
            if self._extra:
                self._vals['_extra'] = self._extra
            self._host = None
        return self._vals

    def __getitem__(self, k):
        return self._resolve()[k]

    def __iter__(self):
        return iter(self._resolve())

    def __len__(self):
        return len(self._resolve())

    def pop(self, k, *default):
        if k == '_extra' and self._vals is None:   # host-side data: no need to wait for the device
            extra, self._extra = self._extra, None
            if extra:
                return extra
            if default:
                return default[0]
            raise KeyError(k)
        return self._resolve().pop(k, *default)

    def __repr__(self):
        return repr(self._resolve())


def _noise_fwd(noiser, enc, cover):
    """explicit fwd/bwd if the noise layer offers it, autograd otherwise (any nn.Module works)."""
    if hasattr(noiser, "fwd") and hasattr(noiser, "bwd"):
        y, c = noiser.fwd(enc)
        return y, ("explicit", c)
    x = enc.detach().requires_grad_(True)
    with torch.enable_grad():
        out = noiser([x, cover])
        y = out[0] if isinstance(out, (list, tuple)) else out
    return y.detach(), ("autograd", (x, y))


def _noise_bwd(noiser, ctx, g):
    kind, c = ctx
    if kind == "explicit":
        return noiser.bwd(c, g)
    x, y = c
    if not y.requires_grad:
        return torch.zeros_like(g)
    (gx,) = torch.autograd.grad(y, x, g, allow_unused=True)
    return gx if gx is not None else torch.zeros_like(g)


def _noise_bwd_is_zero(noiser, ctx):
    """does the attack layer declare the gradient of THIS forward call identically zero (noise_layers.Jpeg: torch.round)?"""
    kind, c = ctx
    f = getattr(noiser, "bwd_is_zero", None)
    return bool(kind == "explicit" and f is not None and f(c))


def _accepts_id(fn):
    """does fn(image, id=...) exist?  Looked up from the signature (cached per function), never by catching TypeError around
    the call -- that would hide a TypeError raised inside the attack and run it twice."""
    key = getattr(fn, "__func__", fn)
    hit = _ACCEPTS_ID.get(key)
    if hit is None:
        import inspect
        try:
            ps = inspect.signature(fn).parameters
            hit = "id" in ps or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in ps.values())
        except (TypeError, ValueError):
            hit = False
        _ACCEPTS_ID[key] = hit
    return hit


_ACCEPTS_ID = {}


class _StepGraph:
    """One training step of `Hidden` as a hipGraph (the reference runs one Python step per batch per rank, train.py:99-109; here the host's
    ~190 launches per step are enqueued once and replayed).  Exact by construction: the graph holds the very launches of the eager step --
    the step has no autograd and no host synchronisation (engine.py) --, its inputs are static tensors refreshed by copy_, and the only
    host-side numbers a step depends on -- Adam's step count and the param group's lr, betas, eps and weight_decay, which a scheduler or a
    loaded state_dict may change between replays -- reach the kernels through device memory (wm_adam_step_dev / wm_adam_step_amp) that is
    refreshed before each replay; `decoupled`, which selects a code path, is part of the graph's key.  Call k of a shape: k < WARMUP eager
    (real steps; they build the weight-pack plans and settle the allocator),
    k == WARMUP capture + replay, later calls replay.  The tensors a replay returns (encoded, noised, decoded) are the graph's own and are
    overwritten by the next replay of the same graph, as torch.cuda.CUDAGraph documents; the losses are copied out per step."""
    WARMUP = 2

    def __init__(self, hidden):
        import weakref
        self._h = weakref.ref(hidden)   # (no Hidden <-> _StepGraph cycle: a dropped model must die by reference count, taking its hipGraph
                                        # with it THEN -- not whenever the cyclic collector next runs, which may be inside another capture)
        self.calls = 0
        self.graph = None
        self.failed = None   # why the capture failed, if it did: the step then runs eagerly (same launches, same results) and says so once
        self._seen = {}

    @property
    def h(self):
        return self._h()

    def _hyper_refresh(self):
        opts = (self.h.optimizer_discrim, self.h.optimizer_enc_dec)
        # (under the scaler the kernel takes the step count from the device and reads only the hyperparameters of the block)
        vals = [v for o in opts for v in o.hyper(o.step_count + 1)]
        # a FRESH pinned tensor per replay: the copy below is asynchronous, and a host that runs ahead of the GPU (a loop that does not read
        # the losses every step: bench.py) would overwrite a reused staging buffer with the NEXT step's constants before this step's copy
        # has run -- found in round 4 by tools/train_sanity_modes.py (the per-step tests synchronise and never saw it).  The caching host
        # allocator hands a pinned block out again only after the copies that read it have completed.
        host = torch.tensor(vals, dtype=torch.float32).pin_memory()
        self.hyper.copy_(host, non_blocking=True)

    def step(self, images, messages):
        h = self.h
        if self.calls < self.WARMUP or self.failed is not None:
            self.calls += 1
            return h._step_eager(images, messages)
        if self.graph is None:
            dev = images.device
            self.img, self.msg = torch.empty_like(images), torch.empty_like(messages)
            self.hyper = torch.zeros(2 * ops.ADAM_HYPER, device=dev, dtype=torch.float32)
            self.img.copy_(images); self.msg.copy_(messages)
            self._seen = {"img": (images, images._version), "msg": (messages, messages._version)}
            opts = (h.optimizer_discrim, h.optimizer_enc_dec)
            for i, o in enumerate(opts):
                o._ensure()
                o.capturing = True
                o.hyper_dev = self.hyper[ops.ADAM_HYPER * i:ops.ADAM_HYPER * (i + 1)]
            graph = torch.cuda.CUDAGraph()
            try:
                with no_gc(), torch.cuda.graph(graph):
                    self.result = h._step_launches(self.img, self.msg)
            except Exception as e:   # noqa: BLE001 -- whatever stopped the capture (nothing was executed: the model is as it was before)
                import warnings
                self.failed = f"{type(e).__name__}: {e}"
                self.result = None
                warnings.warn("hipGraph capture of the training step failed; this and the following steps are enqueued eagerly (same launches, "
                              "same results, more host time per step): " + self.failed)
            finally:
                for o in opts:
                    o.hyper_dev, o.capturing = None, False
            if self.failed is not None:
                self.calls += 1
                return h._step_eager(images, messages)
            self.graph = graph
        # fresh inputs into the graph's static tensors -- unless the caller hands in the very tensor object of the previous call, unmodified
        # (torch's version counter: every in-place op bumps it, this library's own through ops._wrote): a loop over one resident batch
        for name, src, dst in (("img", images, self.img), ("msg", messages, self.msg)):
            seen = self._seen.get(name)
            if seen is None or seen[0] is not src or seen[1] != src._version:
                dst.copy_(src)
                self._seen[name] = (src, src._version)
        self._hyper_refresh()
        self.graph.replay()
        self.calls += 1
        h.optimizer_discrim.step_count += 1
        h.optimizer_enc_dec.step_count += 1
        vals, extra_logs, outs = self.result
        return h._wrap_losses(vals, extra_logs), outs


class _Step:
    """What the stages of one training step (Hidden._d_cover ... _g_update) hand to one another: the batch, the caller's callables, the networks
    and their gradient dictionaries, and every tensor one stage leaves for a later one.  It lives until the step returns, and the two-chain
    schedule's memory safety rests on that: the caching allocator hands a freed block back to the pool of the stream that allocated it.  Every
    tensor one stream allocates and ANOTHER reads (encoded -- engine.share_image_acts holds its NHWC form --, g_enc, g_from_noise, the encoder's
    activations in cE, the loss scalars) is referenced from here until the chains have been joined, and a side stream is given work only between
    a fork and the next join (Hidden._run) -- so a block that returns to a side stream's pool is not handed out again before the caller's
    stream's readers of it are ordered ahead.  What never leaves its stage is used on one stream only and may be freed with the stage."""
    fidelity = head_logs = extra_logs = ()   # fidelity: [(log name, value, gradient wrt encoded)] of the terms switched on, SSFW, RecFW, SS3FW
    g_from_noise = pending_d = None

    def __init__(self, h, images, messages, extra_encoded_grad, clip, enc_gate):
        ed = h.encoder_decoder
        self.images, self.messages = images, messages
        self.extra_encoded_grad, self.clip, self.enc_gate = extra_encoded_grad, clip, enc_gate
        self.noiser, self.enc_net, self.dec_net, self.D = ed.noiser, ed.encoder, ed.decoder, h.discriminator
        self.gD, self.gE, self.gDec = engine.grad_dict(self.D), engine.grad_dict(self.enc_net), engine.grad_dict(self.dec_net)
        self.fidelity_on = h.ssim_weight > 0 or h.recon_weight > 0 or h.ssim3_weight > 0


# one entry of a schedule: the stage (a Hidden method), the chain it is enqueued on ("A" / "B", None = the caller's stream), the stages of
# OTHER chains it must wait for, and an optional condition (attribute of the _Step, the value it must have for the slot to run)
_Slot = collections.namedtuple("_Slot", "stage chain after when", defaults=(None, (), None))


class Hidden:
    recon_weight, recon_type = 0.0, 'l2'   # (class-level defaults: the graph key and _recon_term read them on any instance)
    ssim3_weight = 0.0                     # (likewise, for _ssim3_term)

    def __init__(self, configuration: HiDDenConfiguration, device: torch.device, noiser, tb_logger=None,
                 compute_dtype=torch.bfloat16, grad_sync=None, amp=None, keep_dead_discriminator_grads=True, ssim_weight=0.0,
                 recon_weight=0.0, recon_type='l2', ssim3_weight=0.0):
        """
        :param configuration: sizes / loss weights (options.HiDDenConfiguration)
        :param device: must be a cuda (ROCm) device -- the step has no CPU path
        :param noiser: attack layer(s): an object with forward([encoded, cover]) -> [noised, cover]
                       (noise_layers.Noiser) or any module of noise_layers
        :param tb_logger: accepted for signature compatibility; unused
        :param compute_dtype: torch.bfloat16 (production) or torch.float32 (parity path)
        :param grad_sync: None or a distributed.GradSync (its interface is required: start / finish / finish_all / scale / average_) --
                          the data-parallel bucket all-reduce started from inside the backward.  A plain callable(flat_grad_tensor) is
                          wrapped into that interface (run once per bucket, synchronously, where the bucket would be waited for)
        :param keep_dead_discriminator_grads: True (default) = the reference's state after a step: g_loss.backward() (hidden.py:101) also
                    accumulates the generator loss's gradients into the DISCRIMINATOR's parameters; nothing ever reads them (no optimiser
                    step uses them, hidden.py:67 zeroes them first thing in the next step).  False: that third pass through the
                    discriminator computes the gradient wrt `encoded` only (no conv weight gradients: 2 body-layer + 1 first-layer
                    weight-gradient GEMMs fewer per step, 9.9 of the step's 249.0 GFLOP per 256x256 frame).  Losses, outputs and every
                    parameter update are identical either way; only the discriminator's .grad left behind after the step differs.
        :param amp: optional ops.AmpState -- torch.cuda.amp.GradScaler semantics on the device (models/IRNcrop_model.py:143,
                    407-416): every loss gradient is multiplied by its scale, both optimisers step through it.  Required in
                    practice with compute_dtype=torch.float16 (the gradients of a 3M-element mean loss underflow f16 otherwise)
        :param ssim_weight: weight w of the structural-similarity fidelity term (models/IRN_model.py:569-570: gen_loss += w * (-ssim(encoded,
                    cover)), w = 0.1 or 0.01 there).  0 (default): no SSIM kernel is launched and the step is the three-term one bit for bit.
                    > 0: the term's gradient is added into the encoded image's gradient, and the value is logged as ('SSFW', ssim) among
                    the step's extra logs.  The logged 'loss' keeps its three-term meaning (adversarial + encoder MSE + decoder MSE) either
                    way.  Also settable afterwards as `hidden.ssim_weight`
        :param recon_weight: weight w of the reference's reconstruction term (models/IRNrhi_model.py:102,153-155: lambda_fit_forw *
                    ReconstructionLoss(encoded, cover, pixel_criterion_forw)), wired exactly as ssim_weight: 0 (default) launches nothing and
                    leaves the step bit for bit; > 0 adds the term's gradient into the encoded image's gradient and logs ('RecFW', value).
                    The term is a per-sample SUM over C*H*W values (196,608 x an MSE at 3 x 256 x 256): size the weight for that
        :param recon_type: 'l2' | 'l1' | 'l_char' (eps 1e-6), the reference's pixel_criterion_forw
        :param ssim3_weight: weight w of the local structure term w * mean(SSIM_Loss()(encoded, cover)) (loss.py:9-39 of the reference: the
                    3 x 3 reflect-padded SSIM map), wired exactly as ssim_weight: 0 (default) launches nothing and leaves the step bit for
                    bit; > 0 adds the term's gradient into the encoded image's gradient and logs ('SS3FW', mean of the map).  Also settable
                    afterwards as `hidden.ssim3_weight`
        """
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("Hidden runs on the MI355X HIP path only (device must be cuda)")
        self.encoder_decoder = EncoderDecoder(configuration, noiser).to(device)
        self.discriminator = Discriminator(configuration).to(device)
        engine.set_compute_dtype(self.encoder_decoder, compute_dtype)
        engine.set_compute_dtype(self.discriminator, compute_dtype)
        enc, dec = self.encoder_decoder.encoder, self.encoder_decoder.decoder
        for m in (enc, dec, self.discriminator):
            m.flatten_parameters_()
        self.optimizer_enc_dec = FlatAdam([enc, dec])
        self.optimizer_discrim = FlatAdam([self.discriminator])
        if configuration.use_vgg:
            raise NotImplementedError("use_vgg: the reference's vgg_loss module is absent from its tree")
        self.vgg_loss = None
        self.config = configuration
        self.device = device
        self.cover_label = 1
        self.encoded_label = 0
        self.tb_logger = tb_logger
        from ..distributed import as_grad_sync
        self.grad_sync = as_grad_sync(grad_sync)
        self.keep_dead_discriminator_grads = bool(keep_dead_discriminator_grads)
        self.ssim_weight = float(ssim_weight)
        if recon_type not in ops.RECON_KINDS:
            raise ValueError("recon_type must be one of %s, got %r" % (", ".join(ops.RECON_KINDS), recon_type))
        self.recon_weight = float(recon_weight)
        self.recon_type = recon_type
        self.ssim3_weight = float(ssim3_weight)
        self.amp = amp
        self.amp_owner = True   # this object calls amp.update() at the end of a step (a wrapping model may take that over)
        if amp is not None:
            self.optimizer_enc_dec.attach_amp(amp)
            self.optimizer_discrim.attach_amp(amp)
        self.noise_id = None  # optional deterministic choice for Combined/Noiser layers
        self.lazy_losses = True  # train_on_batch returns StepLosses (host sync on first read) instead of a plain dict
        self._graphs = None      # enable_graph(): (shapes, attack choice, ...) -> _StepGraph
        # An attack whose backward is identically zero (Jpeg: torch.round) makes the decoder's gradient wrt its input a value nothing depends
        # on: with this switch on (default) the step does not compute it (the decoder's first layer runs its weight gradient alone, the
        # attack's backward and the addition of its zeros are not launched).  Every loss and output is bit-identical either way, and so is
        # every parameter, .grad and optimiser state except ONE tensor's rounding: the decoder's first-layer weight gradient is then summed
        # by the weight-gradient-only kernel instead of the one-pass kernel -- the same sum in another order (tests/test_gpu_graph.py).
        # False = launch it all, as the reference's autograd does
        self.skip_zero_attack_gradient = True
        self.two_streams = False  # the step's two independent chains on two streams (the _TWO_CHAINS schedule); same results bit for bit
        self._streams = None

    MAX_GRAPHS = 32   # captured variants kept per model (shapes x attack variants x ...); calls beyond that run eagerly

    def enable_graph(self, on=True):
        """replay the step from a hipGraph instead of enqueueing its ~190 launches every call (same results bit for bit: _StepGraph).
        Used for plain train_on_batch(batch) calls on one GPU with an attack layer that has an explicit fwd / bwd and declares itself
        `capturable` (the same launches with the same arguments every call: the Jpeg family, GaussianBlur at any size, GF, MiddleBlur, Identity -- not the
        layers that draw their arguments on the host, Resize / Crop / Cropout / Combined) or names the deterministic variant this call runs through
        `capture_key()` (one graph per variant: the model surface's attack cycle, which calls Resize / Crop with fixed arguments and answers None, "run
        this one eagerly", for a layer that says capturable = False: Cropout); a call with
        extra_encoded_grad / clip / enc_gate, with a grad_sync, or while a kernel timer is installed runs eagerly as before."""
        self._graphs = {} if on else None
        return self

    # ------------------------------------------------------------------ helpers
    def _bce_logits(self, logits, target, gscale=1.0):
        """nn.BCEWithLogitsLoss (mean) value ([1] tensor) and gscale * gradient wrt logits, on a [B,1] tensor: one launch."""
        loss, grad = ops.bce_logits(logits, target, gscale, gscale_dev=self._gsd())
        return loss[0], grad.view_as(logits)

    def _gsd(self):
        """the AMP loss scale as a device scalar (None without a scaler): scaler.scale(loss).backward()"""
        return self.amp.scale if self.amp is not None else None

    def _run_noiser(self, enc, cover, n=None):
        n = self.encoder_decoder.noiser if n is None else n
        if hasattr(n, "fwd") and hasattr(n, "bwd"):
            kw = {}
            if _accepts_id(n.fwd):   # Combined / Noiser / the attack cycle take a deterministic choice; single layers do not
                kw["id"] = self.noise_id
            if accepts_cover(n.fwd):   # a layer that mixes in the cover (the Dropouts), or a container that passes it on
                kw["cover"] = cover
            y, c = n.fwd(enc, **kw)
            return y, ("explicit", c)
        return _noise_fwd(n, enc, cover)

    # ------------------------------------------------------------------ the step
    def train_on_batch(self, batch: list, extra_encoded_grad=None, clip=None, enc_gate=None):
        """extra_encoded_grad: optional callable(encoded, images, g_enc) -> [(name, value)] that ADDS its gradient wrt the
        encoded image into g_enc (the tamper-localisation branch of models/IRNrhi_model.py), run after the decoder's backward;
        clip: optional callable(list of flat gradient buffers) applied before each optimiser step -- the buffers of one call
        are clipped TOGETHER by their joint norm (clip_grad_norm_ over netG.parameters(), IRNcrop_model.py:410-412);
        enc_gate: optional callable(encoded, images) -> [2] device tensor (psnr, weight): the PSNR-gated weight of the
        image-fidelity term (IRNcrop_model.py:379-388), multiplied into encoder_loss without a host sync."""
        images, messages = batch
        images = images.to(self.device, torch.float32).contiguous()
        messages = messages.to(self.device, torch.float32).contiguous()
        n = self.encoder_decoder.noiser
        if (self._graphs is not None and extra_encoded_grad is None and clip is None and enc_gate is None and self.grad_sync is None
                and not ops.kernel_timer_installed() and hasattr(n, "fwd") and hasattr(n, "bwd") and not torch.cuda.is_current_stream_capturing()):
            # a layer is capturable as a whole (`capturable`), or says per call which of its deterministic variants this call runs
            # (`capture_key()`: a hashable, or None for "not this time" -- the model surface's attack cycle, whose choice follows the step)
            ck = True if getattr(n, "capturable", False) else (n.capture_key() if hasattr(n, "capture_key") else None)
        else:
            ck = None
        if ck is not None:
            # (the optimisers' numbers are read from device memory at each replay, _StepGraph._hyper_refresh: only `decoupled`, a code path,
            # needs a graph of its own)
            key = self._graph_key(images, messages, ck)
            g = self._graphs.get(key)
            if g is None and len(self._graphs) < self.MAX_GRAPHS:
                g = self._graphs[key] = _StepGraph(self)
            if g is not None:
                return g.step(images, messages)
        return self._step_eager(images, messages, extra_encoded_grad, clip, enc_gate)

    def _graph_key(self, images, messages, ck):
        """what a captured step depends on beside the tensors' contents: shapes, the attack variant and every switch that selects launches"""
        return (tuple(images.shape), tuple(messages.shape), self.noise_id, self.keep_dead_discriminator_grads, self.lazy_losses, self.two_streams,
                self.skip_zero_attack_gradient, self.encoder_decoder.encoder.compute_dtype, ck, self.optimizer_discrim.decoupled,
                self.optimizer_enc_dec.decoupled, float(self.ssim_weight), float(self.recon_weight), self.recon_type,
                float(self.ssim3_weight))

    def _ssim_term(self, encoded, images):
        """the structural-similarity fidelity term ssim_weight * (-SSIM(encoded, cover)): (SSIM value, its gradient wrt encoded in a buffer of
        its own, times the AMP scale) -- two fused launches and a finalise; (None, None) at weight 0"""
        if not self.ssim_weight > 0:
            return None, None
        val, planes = ops.ssim(encoded, images, True, want_grad=True)
        return val, ops.ssim_bwd(planes, encoded, images, gscale=-self.ssim_weight, gscale_dev=self._gsd())

    def _recon_term(self, encoded, images):
        """the reconstruction fidelity term recon_weight * ReconstructionLoss(encoded, cover, recon_type): (its unweighted value, its gradient
        wrt encoded in a buffer of its own, times the AMP scale) -- two launches and a finalise; (None, None) at weight 0"""
        if not self.recon_weight > 0:
            return None, None
        return ops.recon_loss(encoded, images, self.recon_type, 1e-6, want_grad=True, gscale=self.recon_weight, gscale_dev=self._gsd())

    def _ssim3_term(self, encoded, images):
        """the local structure term ssim3_weight * mean(SSIM_Loss()(encoded, cover)): (the mean of the map, its gradient wrt encoded in a buffer
        of its own, times the AMP scale) -- two launches and a finalise, the map itself is never written; (None, None) at weight 0"""
        if not self.ssim3_weight > 0:
            return None, None
        return ops.ssim3_mean(encoded, images, want_grad=True, gscale=self.ssim3_weight, gscale_dev=self._gsd())

    def _step_eager(self, images, messages, extra_encoded_grad=None, clip=None, enc_gate=None):
        vals, extra_logs, outs = self._step_launches(images, messages, extra_encoded_grad, clip, enc_gate)
        return self._wrap_losses(vals, extra_logs), outs

    def _wrap_losses(self, vals, extra_logs):
        if self.lazy_losses:
            return StepLosses(vals, extra_logs)
        losses = dict(zip(LOSS_KEYS, vals.tolist()))
        if extra_logs:
            losses['_extra'] = extra_logs
        return losses

    def _step_launches(self, images, messages, extra_encoded_grad=None, clip=None, enc_gate=None):
        """every launch of one step, no host synchronisation -> ([7] device tensor of the logged scalars, extra logs, (encoded, noised, decoded))"""
        self.encoder_decoder.train()
        self.discriminator.train()
        st = _Step(self, images, messages, extra_encoded_grad, clip, enc_gate)
        two = (self.two_streams and self.grad_sync is None and extra_encoded_grad is None and clip is None and enc_gate is None
               and hasattr(st.noiser, "fwd") and hasattr(st.noiser, "bwd"))
        # packed conv weights: one launch per network here (+ one for D after its optimiser step) instead of one per
        # conv call; valid only inside this step (the parameters are ours to change until it returns)
        nets = (st.enc_net, st.dec_net, st.D)
        try:
            for n in nets:
                n.refresh_packs()
            with engine.defer_bn_counters(), engine.share_image_acts(st.dec_net.compute_dtype):
                self._run(self._TWO_CHAINS if two else self._ONE_STREAM, st)
            return st.vals, st.logs, (st.encoded, st.noised, st.decoded)
        finally:
            for n in nets:
                n.invalidate_packs()

    # ------------------------------------------------------------------ the stages of the step, each written once
    # (issued on whatever stream is current; what later stages read is left on the _Step.  Streams and events are the schedules' business, below)
    def _d_cover(self, st):
        # (fwd_loss: the forward, the loss on its output and the head's share of the backward -- one launch behind the pool instead of four)
        _, st.d_loss_on_cover, c = st.D.fwd_loss(st.images, self.cover_label, 1.0, st.gD, accumulate=False, gscale_dev=self._gsd())
        st.D.bwd(c, None, st.gD, accumulate=False, need_input_grad=False)

    def _share_images(self, st):
        for dt in {st.D.compute_dtype, st.enc_net.compute_dtype}:
            engine.image_to_act(st.images, dt)

    def _encode(self, st):
        st.encoded, st.cE = st.enc_net.fwd(st.images, st.messages)

    def _share_encoded(self, st):
        for dt in {st.D.compute_dtype, st.dec_net.compute_dtype}:
            engine.image_to_act(st.encoded, dt)

    def _fidelity(self, st):
        """the fidelity terms that are switched on, each into a gradient buffer of its own: they need only encoded and the cover"""
        terms = (('SSFW', self._ssim_term), ('RecFW', self._recon_term), ('SS3FW', self._ssim3_term))
        st.fidelity = [t for t in ((name, *term(st.encoded, st.images)) for name, term in terms) if t[2] is not None]

    def _attack(self, st):
        st.noised, st.cN = self._run_noiser(st.encoded, st.images)
        st.zero_attack = bool(self.skip_zero_attack_gradient and _noise_bwd_is_zero(st.noiser, st.cN))

    def _d_encoded(self, st):
        """train the discriminator on the encoded image (hidden.py:76-83)"""
        _, st.d_loss_on_encoded, c = st.D.fwd_loss(st.encoded, self.encoded_label, 1.0, st.gD, accumulate=True, gscale_dev=self._gsd())   # encoded.detach()
        st.D.bwd(c, None, st.gD, accumulate=True, need_input_grad=False)
        # data parallel: the discriminator's bucket travels under the decoder's forward (independent of D; the reference runs it
        # before D(encoded), the results are the same)
        if self.grad_sync is not None:
            st.pending_d = self.grad_sync.start(st.D.flat_grads)

    def _decode(self, st):
        cfg, B = self.config, st.images.shape[0]
        st.decoded, st.msg_out, st.cDec = st.dec_net.fwd_loss(st.noised, st.messages, 2.0 * cfg.decoder_loss / (B * cfg.message_length), st.gDec,
                                                             accumulate=False, gscale_dev=self._gsd())     # mse, bit error, and the head's backward

    def _grad_scale(self, st, flats):
        """what the optimiser multiplies these reduced buffers by: 1 / world -- or 1 after a clip callable, which gets them averaged, and TOGETHER"""
        gs = self.grad_sync
        if st.clip is None:
            return 1.0 if gs is None else gs.scale
        if gs is not None:
            for f in flats:
                gs.average_(f)
        st.clip(flats)
        return 1.0

    def _d_update(self, st):
        if self.grad_sync is not None:
            self.grad_sync.finish(st.pending_d)
        self.optimizer_discrim.step(grad_scale=self._grad_scale(st, [st.D.flat_grads]))
        st.D.refresh_packs()

    def _generator(self, st):
        """train the generator (hidden.py:85-103), down to the gradient wrt the encoded image: adversarial + image fidelity (+ the fidelity terms)"""
        cfg, D, encoded, images = self.config, st.D, st.encoded, st.images
        _, st.g_loss_adv, c = D.fwd_loss(encoded, self.cover_label, cfg.adversarial_loss, st.gD, accumulate=True, gscale_dev=self._gsd())
        # the reference's g_loss.backward() also accumulates into the discriminator's .grad (zeroed at the start of the next step, never
        # read): kept by default so the .grad state matches; keep_dead_discriminator_grads=False computes the image gradient alone
        st.n_img = encoded.numel()
        gate = st.enc_gate(encoded, images) if st.enc_gate is not None else None
        if gate is None:
            # the adversarial term's gradient (NHWC, as the discriminator's first layer wrote it) + the image-fidelity term's, and that
            # term's loss, in one pass
            g_img = D.bwd(c, None, st.gD, accumulate=True, need_input_grad=True, weight_grads=self.keep_dead_discriminator_grads, raw_input_grad=True)
            st.g_enc, st.enc_part = ops.image_grad_mse(g_img, encoded, images, 2.0 * cfg.encoder_loss / st.n_img, gscale_dev=self._gsd())
        else:
            st.g_enc = D.bwd(c, None, st.gD, accumulate=True, need_input_grad=True, weight_grads=self.keep_dead_discriminator_grads)
            st.enc_part, g_mse = ops.mse_fwd_bwd_gated(encoded, images, 2.0 * cfg.encoder_loss / st.n_img, gate[1:2], gscale_dev=self._gsd())
            ops.axpy_(st.g_enc, g_mse)
            st.head_logs = [('PF', gate[0:1])]
        for _, _, g in st.fidelity:
            ops.axpy_(st.g_enc, g)

    def _decode_bwd(self, st):
        st.g_noised = st.dec_net.bwd(st.cDec, None, st.gDec, accumulate=False, need_input_grad=not st.zero_attack)
        # data parallel: the decoder's bucket goes out now and travels while the attack and the encoder run their backward
        if self.grad_sync is not None:
            st.pending = [self.grad_sync.start(st.dec_net.flat_grads)]

    def _attack_bwd(self, st):
        st.g_from_noise = _noise_bwd(st.noiser, st.cN, st.g_noised).contiguous()

    def _encoder_bwd(self, st):
        gs, enc_net = self.grad_sync, st.enc_net
        if st.g_from_noise is not None:
            ops.axpy_(st.g_enc, st.g_from_noise)
        if st.extra_encoded_grad is not None:
            st.extra_logs = st.extra_encoded_grad(st.encoded, st.images, st.g_enc)
        if gs is None:
            enc_net.bwd(st.cE, st.g_enc, st.gE, accumulate=False)
        else:
            # the encoder in two reverse-order buckets: [after_concat, final] leaves under the body layers' backward
            cut = enc_net.body_param_count()
            enc_net.bwd(st.cE, st.g_enc, st.gE, accumulate=False, after_head=lambda: st.pending.append(gs.start(enc_net.flat_grads[cut:])))
            st.pending.append(gs.start(enc_net.flat_grads[:cut]))
            gs.finish_all(st.pending)

    def _g_update(self, st):
        cfg = self.config
        self.optimizer_enc_dec.step(grad_scale=self._grad_scale(st, [st.enc_net.flat_grads, st.dec_net.flat_grads]))
        if self.amp is not None and self.amp_owner:
            self.amp.update()   # scaler.update(), IRNcrop_model.py:416
        # metrics: one host sync for all seven scalars (hidden.py:105-117)
        st.vals = ops.hidden_metrics(st.enc_part, st.n_img, st.msg_out, st.g_loss_adv, st.d_loss_on_cover, st.d_loss_on_encoded,
                                     cfg.adversarial_loss, cfg.encoder_loss, cfg.decoder_loss)
        st.logs = list(st.head_logs) + list(st.extra_logs or ()) + [(name, val.reshape(1)) for name, val, _ in st.fidelity]

    # ------------------------------------------------------------------ the two schedules: the same stages, placed differently
    # One stream: hidden.py:54-118's order on the caller's stream (the fidelity terms before the attack, where both schedules have them).
    _ONE_STREAM = (_Slot(_d_cover), _Slot(_encode), _Slot(_fidelity, when=("fidelity_on", True)), _Slot(_attack), _Slot(_d_encoded), _Slot(_decode),
                   _Slot(_d_update), _Slot(_generator), _Slot(_decode_bwd), _Slot(_attack_bwd, when=("zero_attack", False)), _Slot(_encoder_bwd),
                   _Slot(_g_update))
    # Two chains (Hidden.two_streams; why, and what it measured: DESIGN.md §4): the discriminator's passes (A) beside encoder -> attack ->
    # decoder and back (B), one edge between them (A's second pass waits for encoded) until they join at the encoder's backward.  Listed in
    # host enqueue order, which is behaviour: A's first stage, ALL of B, then the rest of A (a replayed hipGraph ran its branches side by side
    # only when the forked branch was captured first: DESIGN.md §9).
    _TWO_CHAINS = (
        _Slot(_share_images),                                     # converted once, before the fork: both chains read it
        _Slot(_d_cover, "A"),
        _Slot(_encode, "B"),
        _Slot(_share_encoded, "B"),                               # on the producing stream: chain A and -- under an Identity attack -- the decoder read it
        _Slot(_fidelity, "B", when=("fidelity_on", True)),        # in stream order ahead of the attack's kernels, never beside them
        _Slot(_attack, "B"), _Slot(_decode, "B"), _Slot(_decode_bwd, "B"), _Slot(_attack_bwd, "B", when=("zero_attack", False)),
        _Slot(_d_encoded, "A", after=(_share_encoded,)),
        _Slot(_d_update, "A"),
        _Slot(_generator, "A", after=(_fidelity,)),               # (its gradients: before the encoder's backward wherever that runs)
        # an attack that passes back zeros (Jpeg's torch.round, skip_zero_attack_gradient) leaves chain B without a successor in the encoder:
        # the encoder's backward continues chain A, beside the decoder's backward on chain B, and the chains meet only at the optimiser step
        _Slot(_encoder_bwd, "A", when=("zero_attack", True)),
        _Slot(_encoder_bwd, when=("zero_attack", False)),
        _Slot(_g_update))

    def _run(self, schedule, st):
        """Run a schedule's stages in the order listed -- the only stream code of the step.  Slots without a chain run on the caller's stream;
        the first slot on a chain forks A and B from it, the next slot without a chain joins them.  A stage some slot names in `after` gets
        an event recorded behind it, and that slot's stream waits for it (a stage that did not run is not waited for)."""
        caller = torch.cuda.current_stream()
        awaited = {dep for slot in schedule for dep in slot.after}
        side, events = {}, {}
        for chain, slots in itertools.groupby(schedule, key=lambda slot: slot.chain):
            if chain is None:
                for s in side.values():
                    caller.wait_stream(s)
                side = {}
            elif not side:
                if self._streams is None:
                    self._streams = (torch.cuda.Stream(device=self.device), torch.cuda.Stream(device=self.device))
                side = dict(zip("AB", self._streams))
                for s in side.values():
                    s.wait_stream(caller)
            stream = side.get(chain, caller)
            with torch.cuda.stream(side.get(chain)):   # (None on the caller's stream: no switch)
                for slot in slots:
                    if slot.when is not None and getattr(st, slot.when[0]) != slot.when[1]:
                        continue
                    for dep in slot.after:
                        if dep in events:
                            stream.wait_event(events[dep])
                    slot.stage(self, st)
                    if slot.stage in awaited:
                        events[slot.stage] = torch.cuda.Event()
                        events[slot.stage].record(stream)

    def validate_on_batch(self, batch: list):
        """hidden.py:120-182: eval-mode BatchNorm (running statistics), no parameter update."""
        images, messages = batch
        images = images.to(self.device, torch.float32).contiguous()
        messages = messages.to(self.device, torch.float32).contiguous()
        B = images.shape[0]
        cfg = self.config
        ed = self.encoder_decoder
        enc_net, dec_net, D = ed.encoder, ed.decoder, self.discriminator
        ed.eval()
        D.eval()
        with torch.no_grad():
            d_on_cover, _ = D.fwd(images, training=False)
            d_loss_on_cover, _ = self._bce_logits(d_on_cover, self.cover_label)
            encoded, _ = enc_net.fwd(images, messages, training=False)
            noised, _ = self._run_noiser(encoded, images)
            decoded, _ = dec_net.fwd(noised, training=False)
            d_on_encoded, _ = D.fwd(encoded, training=False)
            d_loss_on_encoded, _ = self._bce_logits(d_on_encoded, self.encoded_label)
            g_loss_adv, _ = self._bce_logits(d_on_encoded, self.cover_label)
            g_loss_enc = F.mse_loss(encoded, images)
            g_loss_dec = F.mse_loss(decoded, messages)
            g_loss = cfg.adversarial_loss * g_loss_adv + cfg.encoder_loss * g_loss_enc + cfg.decoder_loss * g_loss_dec
            rounded = decoded.round().clamp(0, 1)
            bit_err = (rounded - messages).abs().sum() / (B * messages.shape[1])
            vals = torch.stack([g_loss, g_loss_enc, g_loss_dec, bit_err, g_loss_adv, d_loss_on_cover,
                                d_loss_on_encoded]).tolist()
        losses = {
            'loss           ': vals[0], 'encoder_mse    ': vals[1], 'dec_mse        ': vals[2],
            'bitwise-error  ': vals[3], 'adversarial_bce': vals[4], 'discr_cover_bce': vals[5],
            'discr_encod_bce': vals[6],
        }
        return losses, (encoded, noised, decoded)

    def evaluate_on_batch(self, batch: list, noisers=None):
        """What a trained model is worth on one batch, read with ONE device -> host copy by the caller: eval-mode BatchNorm and no_grad like
        validate_on_batch.  Returns (values, names): a float32 device tensor and its column names --
            'PSNR', 'SSIM'                       of encoded against cover (metrics.PSNR(1.0), pytorch_ssim.ssim), once per batch;
            'BER/<name>', 'dec_mse/<name>'       per attack layer in `noisers` (default: the configured one): the share of wrong bits of
                                                 round(decoded) clamped to [0, 1], and the decoder's MSE against the message.
        Nothing here synchronises with the host."""
        images, messages = batch
        images = images.to(self.device, torch.float32).contiguous()
        messages = messages.to(self.device, torch.float32).contiguous()
        ed = self.encoder_decoder
        enc_net, dec_net = ed.encoder, ed.decoder
        noisers = [ed.noiser] if noisers is None else list(noisers)
        was = ed.training
        ed.eval()
        try:
            with torch.no_grad():
                encoded, _ = enc_net.fwd(images, messages, training=False)
                vals = [ops.psnr(encoded, images, 1.0), ops.ssim(encoded, images, True).reshape(1)]
                names = ['PSNR', 'SSIM']
                for n in noisers:
                    noised, _ = self._run_noiser(encoded, images, n)
                    decoded, _ = dec_net.fwd(noised.contiguous(), training=False)
                    decoded = decoded.float()
                    vals.append((decoded.round().clamp(0, 1) - messages).abs().mean().reshape(1))
                    vals.append(F.mse_loss(decoded, messages).reshape(1))
                    name = getattr(n, "name", None) or type(n).__name__
                    names += ['BER/' + name, 'dec_mse/' + name]
                return torch.cat(vals), names
        finally:
            ed.train(was)

    def to_stirng(self):
        return '{}\n{}'.format(str(self.encoder_decoder), str(self.discriminator))
