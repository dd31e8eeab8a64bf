"""IRNrhiModel -- the model class whose surface train.py drives (reference
models/IRNrhi_model.py:75,358-395,425-431,690-698,1138-1145; composition of the localisation branch
from models/IRNcrop_model.py:337-416):

    model = IRNrhiModel(opt)
    model.feed_data(batch)
    logs, debug_logs = model.optimize_parameters(step, latest_values)
    progbar.add(len(model.real_H), values=logs)

The step behind it is the HiDDeN-order watermark embed -> attack -> extract GAN step of
hidden_models/hidden.py:54-118 on the HIP kernels (hidden_models.Hidden), optionally followed by the
tamper-localisation branch: STE clamp -> Quantization -> splice with the previous batch by the mask ->
attack -> Quantization -> UNet -> BCEWithLogits on the (sigmoid) mask, whose gradient reaches both the
UNet and, through the attack, the encoder.  train.tamper_cycle alternates that splice with the reference's
other forgery, copy-move within the frame (models/IRNp_model.py:497-499,561-598).

Bookkeeping kept from the reference: `global_step`, input clamp to [0,1] (:430), no work until two
previous batches exist (:446), checkpoint every `save_interval` steps at `step % save_interval == 10`
on rank <= 0 (:691-693), rotation of `previous_images` buffers (:694-697), `logs` as a list of
(name, float).
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from .. import engine, ops
from .. import glayers as G
from ..hidden_models import Hidden
from ..network.UNet import UNet
from ..noise_layers import Combined, Crop, GaussianBlur, Hybrid, Identity, Jpeg, JpegMask, JpegSS, MiddleBlur, Resize
from ..noise_layers._device_rng import call_fwd
from ..noise_layers.crop import Cropout
from ..noise_layers.dropout import Dropout
from ..noise_layers.gaussian import Gaussian
from ..noise_layers.gaussian_filter import GF
from ..noise_layers.jpeg_compression import JpegCompression
from ..noise_layers.salt_pepper_noise import SaltPepper
from ..optim import FlatAdam
from ..options import HiDDenConfiguration
from .base_model import BaseModel
from .lr_scheduler import build_schedulers
from .modules.Quantization import Quantization
from .networks import UNetDiscriminator


def _get(d, *keys, default=None):
    for k in keys:
        if d is None:
            return default
        try:
            d = d[k]
        except (KeyError, TypeError, IndexError):
            return default
    return default if d is None else d


LOCALIZER_ARCHS = ("unet", "unetd")


def localizer_arch(train_opt):
    """train.localizer_arch: 'unet' (the default) or 'unetd'; anything else is a ValueError"""
    arch = _get(train_opt, 'localizer_arch', default='unet')
    if arch not in LOCALIZER_ARCHS:
        raise ValueError(f"train.localizer_arch must be one of {LOCALIZER_ARCHS}, got {arch!r}")
    return arch


TAMPER_KINDS = ("splicing", "copymove")
REFERENCE_TAMPER_CYCLE = ("splicing", "copymove", "splicing")   # IRNp_model.py:499: copy-move where global_step % 3 == 1


def tamper_cycle(train_opt):
    """train.tamper_cycle: the forgeries the localiser is trained on, a list drawn from 'splicing' (the previous batch through the mask,
    IRNcrop_model.py:348) and 'copymove' (the same frame, moved, IRNp_model.py:561-598), indexed by global_step % len.  Absent:
    ['splicing'].  The reference's schedule is REFERENCE_TAMPER_CYCLE.  An unknown name or an empty list is a ValueError"""
    cycle = _get(train_opt, 'tamper_cycle', default=None)
    if cycle is None:
        return ["splicing"]
    cycle = [cycle] if isinstance(cycle, str) else list(cycle)
    if not cycle or any(k not in TAMPER_KINDS for k in cycle):
        raise ValueError(f"train.tamper_cycle must be a non-empty list drawn from {TAMPER_KINDS}, got {cycle!r}")
    return cycle


def draw_copymove_shifts(n_frames, H, W, frac=1.0, per_clip_T=None, rand=np.random.rand):
    """per-frame (sx rows, sy columns) of a copy-move step: int(H * frac * (rand() - 0.5)), then int(W * frac * (rand() - 0.5)) -- the
    reference's order of draws and its truncation towards zero (IRNp_model.py:567-568 with frac 1.0; :1010-1011, copy_move(), is frac 0.25).
    One draw serves the whole batch, as in the reference; per_clip_T = T: one draw per clip of T consecutive frames, so that what was moved
    stays put through a clip."""
    if per_clip_T is None:
        per_clip_T = n_frames
    per_clip_T = int(per_clip_T)
    if n_frames <= 0 or per_clip_T <= 0 or n_frames % per_clip_T:
        raise ValueError(f"draw_copymove_shifts: {n_frames} frames are not whole clips of {per_clip_T}")
    shifts = []
    for _ in range(n_frames // per_clip_T):
        sx = int(H * frac * (rand() - 0.5))
        sy = int(W * frac * (rand() - 0.5))
        shifts += [(sx, sy)] * per_clip_T
    return shifts


def localizer_class(train_opt):
    """the class IRNrhiModel builds its localiser from"""
    return UNetDiscriminator if localizer_arch(train_opt) == "unetd" else UNet


def build_unetd_localizer(device, dtype, dim=16, fused_head=True):
    """the localiser the reference's trainers construct (IRNcrop_model.py:125-126, IRNp_model.py:162, IRN_model.py:147): UNetDiscriminator
    with the SRM / Bayar first block, two dilated residual blocks, one sigmoid mask channel"""
    return UNetDiscriminator(use_sigmoid=True, in_channels=3, residual_blocks=2, out_channels=1, use_spectral_norm=True, dim=int(dim),
                             fused_head=bool(fused_head), dtype=dtype).to(device)


def unetd_localiser_step(net, flat, optimizer, x, mask, weight=1.0, dice_weight=0.0, amp=None, grad_sync=None, clip=None):
    """One training step of a UNetDiscriminator localiser on the batch x [B,3,H,W] with the tamper mask [B,1,H,W] -- what _localise runs once
    the attacked batch exists (IRNcrop_model.py:376-378,391-393,407-416): forward through autograd, weight * BCEWithLogits on the SIGMOID
    output (+ dice_weight * BinaryDiceLoss), both seeded with the scaler's device-side scale; backward through the network into `flat`
    (glayers.FlatParameters of net: the convolution kernels add into it) and into x; all-reduce of the flat gradient (one bucket); joint
    clipping (clip: callable(list of flat gradients)); one step of `optimizer` (FlatAdam over [flat]).
    -> (loss, dice or None, pred [B,1,H,W] detached, the gradient wrt x -- still multiplied by the scaler's scale, like the seeds)"""
    flat.zero_grad()
    x = x.detach().requires_grad_(True)
    pred, _ = net(x)
    p = pred.detach()
    scale_dev = amp.scale if amp is not None else None
    # the reference applies BCEWithLogits to the sigmoid output (:378,391-393): the seed is the gradient wrt that output, the network's own
    # backward (the mask head's kernel, or the sigmoid's) chains the sigmoid
    loss, g_pred = ops.bce_logits_target(p, mask, weight, chain_sigmoid=False, gscale_dev=scale_dev)
    dice = None
    if dice_weight > 0:
        dice, _ = ops.dice_binary(p, mask, 1.0, 2.0, 'mean', want_grad=True, chain_sigmoid=False, gscale=dice_weight, gscale_dev=scale_dev,
                                  grad_out=g_pred)
    pred.backward(g_pred.view_as(pred))
    gscale = 1.0
    if grad_sync is not None:
        grad_sync.finish_all([grad_sync.start(flat.flat_grads)])
        gscale = grad_sync.scale
        if clip is not None:
            grad_sync.average_(flat.flat_grads)
            gscale = 1.0
    if clip is not None:
        clip([flat.flat_grads])
    optimizer.step(grad_scale=gscale)
    return loss, dice, p, x.grad


class DeferredLogs:
    """`logs` of a step whose scalars have not been waited for yet (train.deferred_logs; the reference's list of (name, value) pairs,
    IRNrhi_model.py optimize_parameters -> train.py:109).  Behaves as that list; the first look at it (iteration, len, truth value, indexing,
    comparison) waits for the device.  A loop that looks one step late -- after enqueueing the next step -- never drains the GPU queue."""

    def __init__(self, read):
        self._read, self._logs = read, None

    def resolve(self):
        if self._logs is None:
            self._logs, self._read = self._read(), None
        return self._logs

    def __iter__(self):
        return iter(self.resolve())

    def __len__(self):
        return len(self.resolve())

    def __getitem__(self, i):
        return self.resolve()[i]

    def __eq__(self, other):
        return self.resolve() == (other.resolve() if isinstance(other, DeferredLogs) else other)

    def __repr__(self):
        return repr(self.resolve())


class _AttackCycle:
    """the attack cycles deterministically with the step."""

    def __init__(self, layers):
        self.layers = layers
        self.k = 0
        self.name = "NotChosenYet"

    def _choose(self, id=None, exclude=()):
        i = self.k % len(self.layers) if id is None else id
        layer = self.layers[i]
        for _ in range(len(self.layers)):   # a layer type the caller cannot use (the localiser and Crop): take the next one in the cycle
            if not isinstance(layer, exclude):
                break
            i = (i + 1) % len(self.layers)
            layer = self.layers[i]
        else:
            i, layer = -1, Identity()
        self.name = getattr(layer, "name", type(layer).__name__)
        return i, layer

    def capture_key(self):
        """Hidden.enable_graph: every layer of the cycle runs with fixed arguments here (Resize at 0.7, Crop at a fixed rectangle), so a step
        through layer i launches the same kernels every time -- one captured graph per layer.  (Also names the layer, as fwd does: a
        replayed step does not call fwd.)"""
        i, layer = self._choose()
        if getattr(layer, "capturable", None) is False:
            return None     # a layer that says it draws its arguments on the host per call (Cropout's rectangle): this step runs eagerly
        return ("cycle", i, type(layer).__name__)

    def fwd(self, image, id=None, exclude=(), cover=None):
        i, layer = self._choose(id, exclude)
        if isinstance(layer, Resize):
            y, c = layer.fwd(image, resize_ratio=0.7)
        elif isinstance(layer, Crop):
            H, W = image.shape[2], image.shape[3]
            y, c = layer.fwd(image, apex=(H // 8, H // 8 + int(0.75 * H), W // 8, W // 8 + int(0.75 * W)))
        else:
            y, c = call_fwd(layer, image, cover)   # (the cover reaches the layers that mix it in: Dropout)
        self.name = getattr(layer, "name", type(layer).__name__)   # (a layer may name itself in its forward: the reference's G_Blur -> GaussianBlur)
        return y, (layer, c)

    def bwd(self, ctx, g):
        layer, c = ctx
        return layer.bwd(c, g)


class IRNrhiModel(BaseModel):
    def __init__(self, opt):
        super(IRNrhiModel, self).__init__(opt)
        self.localizer_arch = localizer_arch(opt['train'])      # (an unknown architecture is refused before anything is built)
        # train.tamper_cycle (absent = ['splicing'], today's step): which forgery each step's localiser sees; with the key present the logs
        # also carry ('Tamper', name) and ('Valid', mean of the ground-truth mask).  train.copymove_shift_frac (default 1.0, the inline
        # form's range; 0.25 is copy_move()'s) and train.copymove_per_clip (default false: one draw per batch, as in the reference)
        self.tamper_cycle = tamper_cycle(opt['train'])
        self.log_tamper = _get(opt['train'], 'tamper_cycle', default=None) is not None
        self.copymove_shift_frac = float(_get(opt['train'], 'copymove_shift_frac', default=1.0))
        self.copymove_per_clip = bool(_get(opt['train'], 'copymove_per_clip', default=False))
        self.copymove_rand = np.random.rand     # the shifts' source of draws (tests script it)
        self._clip_T = None                     # frames per clip of the fed batch (feed_data), None for a batch of images
        self._tamper = None                     # (kind, shifts, valid) of the step's forgery (_gate)
        if self.device.type != "cuda":
            raise RuntimeError("IRNrhiModel runs on the MI355X HIP path only (opt['gpu_ids'] must not be None)")
        train_opt = opt['train'] or {}
        self.train_opt = train_opt
        self.rank = torch.distributed.get_rank() if opt['dist'] else -1
        if torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        size = _get(opt, 'datasets', 'train', 'GT_size', default=256)
        self.width_height = size
        self.global_step = 0
        self.real_H = self.mask = None
        self.previous_images = self.previous_previous_images = None
        self.save_interval = _get(train_opt, 'save_interval', default=3000)
        self.gradient_clipping = _get(train_opt, 'gradient_clipping', default=None)
        # train.deferred_logs (default false = the reference's behaviour: every step's scalars are read before optimize_parameters returns):
        # the returned logs wait for the device only when looked at (DeferredLogs)
        self.deferred_logs = bool(_get(train_opt, 'deferred_logs', default=False))
        dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "fp16": torch.float16, "f32": torch.float32,
                 None: torch.bfloat16}[_get(train_opt, 'compute_dtype')]
        # torch.cuda.amp.autocast() + GradScaler() of the reference (IRNcrop_model.py:143,340,407-416): with f16 activations the
        # loss gradients are scaled by a device-side GradScaler (train.amp: true by default for f16, optional for the other dtypes)
        use_amp = _get(train_opt, 'amp', default=(dtype == torch.float16))
        self.amp = ops.AmpState(self.device, init_scale=_get(train_opt, 'amp_init_scale', default=65536.0),
                                growth_interval=_get(train_opt, 'amp_growth_interval', default=2000)) if use_amp else None

        # ---- attacks (IRNrhi_model.py:103-150 / IRNcrop_model.py:85-104) cycled per step
        attacks = _get(train_opt, 'attacks', default=None)
        table = {
            "Jpeg": lambda q: Jpeg(q), "JpegSS": lambda q: JpegSS(q), "JpegMask": lambda q: JpegMask(q),
            "GaussianBlur": lambda q: GaussianBlur(q or 3), "MiddleBlur": lambda q: MiddleBlur(q or 3),
            "Resize": lambda q: Resize(), "Crop": lambda q: Crop(), "Identity": lambda q: Identity(),
            # the stochastic / JPEG-Drop attacks every reference trainer constructs (IRNrhi_model.py:134-136): dropout.Dropout(),
            # Gaussian(), SaltPepper(prob=0.01), JpegCompression; their draws come from the device generator, seeded from torch's
            "Dropout": lambda q: Dropout(), "Gaussian": lambda q: Gaussian(), "SaltPepper": lambda q: SaltPepper(prob=0.01),
            "JpegCompression": lambda q: JpegCompression(self.device),
            # GaussianBlur<k> (above): the k x k blur, k odd in 3..15; GF<k>: the reference's kornia blur (noise_layers/gaussian_filter.py) at
            # sigma 2, kernel k or 7; Cropout: crop.py:121-134 at half the frame each way (its rectangle is drawn per call: such a step runs eagerly)
            "GF": lambda q: GF(sigma=2.0, kernel=q or 7), "Cropout": lambda q: Cropout(0.5, 0.5),
        }
        if attacks is None:
            attacks = ["Jpeg50"]
        layers = []
        for a in attacks:
            kind = "".join(ch for ch in a if not ch.isdigit())
            q = "".join(ch for ch in a if ch.isdigit())
            layers.append(table[kind](int(q) if q else None))
        self.attack = _AttackCycle(layers)
        # train.hybrid_attacks (default false): the localiser sees, per frame, a random convex mix of EVERY layer of the cycle but Crop, clamped and
        # quantised in the same launch (the reference's "HYBRID ATTACKS" block, IRNcrop_model.py:347-373), instead of the step's one layer; the
        # embed -> attack -> extract chain keeps cycling one attack per step
        self.hybrid = None
        if bool(_get(train_opt, 'hybrid_attacks', default=False)):
            usable = [l for l in layers if not isinstance(l, Crop)]
            if not usable:
                raise ValueError("train.hybrid_attacks needs at least one attack other than Crop in train.attacks")
            self.hybrid = Hybrid(usable, quantize=True)
        self.Quantization = Quantization()

        # ---- networks: HiDDeN embedder / extractor / discriminator (+ UNet localiser)
        cfg = HiDDenConfiguration(H=size, W=size, message_length=_get(train_opt, 'message_length', default=30))
        grad_sync = None
        if opt['dist'] and torch.distributed.get_world_size() > 1:
            from ..distributed import GradSync
            grad_sync = GradSync()
        # train.ssim_weight (default 0 = off): the structural-similarity fidelity term w * (-ssim(encoded, cover)) of the reference's trainers
        # (models/IRN_model.py:569-570), logged as SSFW
        # train.lambda_fit_forw (default 0 = off) and train.pixel_criterion_forw (l2 | l1 | l_char, default l2), the reference's own keys
        # (models/IRNrhi_model.py:102,153-155): lambda_fit_forw * ReconstructionLoss(encoded, cover, pixel_criterion_forw), logged as RecFW.
        # The term is a per-sample SUM, 196,608 x an MSE at 3 x 256 x 256
        # train.ssim3_weight (default 0 = off): w * mean(SSIM_Loss()(encoded, cover)), the reference's 3 x 3 reflect-padded structure map
        # (loss.py:9-39), logged as SS3FW
        self.hidden = Hidden(cfg, self.device, self.attack, None, compute_dtype=dtype, grad_sync=grad_sync, amp=self.amp,
                             ssim_weight=float(_get(train_opt, 'ssim_weight', default=0.0) or 0.0),
                             recon_weight=float(_get(train_opt, 'lambda_fit_forw', default=0.0) or 0.0),
                             recon_type=_get(train_opt, 'pixel_criterion_forw', default='l2') or 'l2',
                             ssim3_weight=float(_get(train_opt, 'ssim3_weight', default=0.0) or 0.0))
        # train.eval_metrics (default false): evaluate() appends robustness_report() to its logs
        self.eval_metrics = bool(_get(train_opt, 'eval_metrics', default=False))
        # train.two_streams (default true): the step's two independent chains on two streams wherever a step has them to itself (one GPU, no
        # localisation branch / clipping / PSNR gate: Hidden._TWO_CHAINS); same results bit for bit
        self.hidden.two_streams = bool(_get(train_opt, 'two_streams', default=True))
        # train.graph (default true): a step WITHOUT the localiser branch, gradient clipping and PSNR gate (configuration C3) is replayed from a
        # hipGraph, one graph per layer of the attack cycle (Hidden.enable_graph; same results bit for bit, tests/test_gpu_graph.py); one GPU only
        if grad_sync is None and bool(_get(train_opt, 'graph', default=True)):
            self.hidden.enable_graph()
        self.netG = self.hidden.encoder_decoder
        self.discriminator = self.hidden.discriminator
        lr = _get(train_opt, 'lr_G', default=1e-3)
        betas = (_get(train_opt, 'beta1', default=0.9), _get(train_opt, 'beta2', default=0.999))
        wd = _get(train_opt, 'weight_decay_G', default=0.0) or 0.0
        for o in (self.hidden.optimizer_enc_dec, self.hidden.optimizer_discrim):
            o.param_groups[0].update(lr=lr, initial_lr=lr, betas=betas, weight_decay=wd)
            o.decoupled = bool(_get(train_opt, 'adamw', default=False))
        self.optimizers = [self.hidden.optimizer_enc_dec, self.hidden.optimizer_discrim]
        self.use_localizer = bool(_get(train_opt, 'localizer', default=False))
        self.localizer = None
        # train.localizer_arch (default unet): unet = network.UNet on the fused engine; unetd = the reference trainers' own localiser,
        # models.networks.UNetDiscriminator (IRNcrop_model.py:125-126) of width train.localizer_dim (default 16), trained through autograd on
        # the HIP layer toolkit; train.localizer_fused_head (default true) runs its full-resolution tail as the one mask-head launch
        self.localizer_flat = None
        if self.use_localizer:
            if self.localizer_arch == "unetd":
                self.localizer = build_unetd_localizer(self.device, dtype, _get(train_opt, 'localizer_dim', default=16),
                                                       _get(train_opt, 'localizer_fused_head', default=True))
                # every trainable parameter in one flat buffer (the frozen SRMConv2D.weight stays out): one Adam launch, one clip, one bucket
                self.localizer_flat = G.FlatParameters(self.localizer)
            else:
                self.localizer = UNet(3, 1, 32).to(self.device)
                engine.set_compute_dtype(self.localizer, dtype)
                self.localizer.flatten_parameters_()
            self.optimizer_localizer = FlatAdam([self.localizer_flat or self.localizer], lr=lr, betas=betas, weight_decay=wd)
            if self.amp is not None:
                self.optimizer_localizer.attach_amp(self.amp)
            self.optimizers.append(self.optimizer_localizer)
            self.localizer_weight = _get(train_opt, 'localizer_weight', default=1.0)
            # train.dice_weight (default 0 = off): w * BinaryDiceLoss()(pred, mask) next to the BCE term (the reference's dice_loss.py, the
            # mask-head loss of its tianchi_model.py:48,101); its gradient is added into the BCE gradient by the Dice backward itself; logged as Dice
            self.dice_weight = float(_get(train_opt, 'dice_weight', default=0.0) or 0.0)
        # train.lr_scheme (MultiStepLR | CosineAnnealingLR_Restart, the reference's keys: lr_steps, lr_gamma, restarts, restart_weights,
        # clear_state, T_period, eta_min; IRNrhi_model.py:340-356): one scheduler per optimiser, stepped by update_learning_rate(step,
        # warmup_iter) before each optimize_parameters (train.py).  Absent: no scheduler, lr_G throughout.  A replayed step follows: it reads
        # the param group at every replay, and a clear_state restart zeroes the moments in place (FlatAdam.reset_state)
        self.schedulers = build_schedulers(self.optimizers, train_opt)
        self.psnr_gate = bool(_get(train_opt, 'psnr_gate', default=True))   # IRNcrop_model.py:379-388
        # log side (IRNcrop_model.py:78,399-400: SummaryWriter scalars; :421-437: an image sheet every 500 steps at step % 500 == 10)
        tb_dir = _get(train_opt, 'tensorboard_dir', default=None)
        self.writer = None
        if tb_dir and self.rank <= 0:
            from ..utils import SummaryWriter
            self.writer = SummaryWriter(tb_dir)
        self.image_dump_interval = _get(train_opt, 'image_dump_interval', default=None)
        self.image_dump_dir = _get(self.opt, 'path', 'images', default=None)
        self._loc = None
        self._copy_stream = None
        self.messages = None
        self.keep_outputs = False    # tests / image dumps: keep the step's tensors in self.last_outputs
        self.last_outputs = {}
        if opt['dist']:
            from ..distributed import broadcast_parameters
            nets = [self.netG.encoder, self.netG.decoder, self.discriminator] + ([self.localizer] if self.localizer else [])
            broadcast_parameters(nets)
        self.grad_sync = grad_sync
        self.load()

    # ------------------------------------------------------------------ data
    def feed_data(self, batch):
        """Accepts what the reference's loaders produce for this path: a tensor [B,3,H,W] or clip
        [B,3,T,H,W] in [0,1], optionally with a tamper mask [B,1,(T,)H,W] -- as (imgs, mask), a dict
        {'GT': imgs, 'mask': mask} or the bare tensor.  Clips are folded into the batch (frames are
        independent units, IRNcrop_model.py:357-366)."""
        mask = None
        self.messages = None
        if isinstance(batch, dict):
            imgs, mask = batch.get('GT', batch.get('imgs')), batch.get('mask')
            if batch.get('messages') is not None:   # the watermark bits to embed ([B*T, L]); drawn at random per step when absent
                self.messages = batch['messages'].to(self.device, torch.float32).contiguous()
        elif isinstance(batch, (tuple, list)):
            imgs = batch[0]
            mask = batch[1] if len(batch) > 1 and torch.is_tensor(batch[1]) and batch[1].dim() >= 4 else None
        else:
            imgs = batch
        imgs, mask = self._to_device(imgs), (self._to_device(mask) if mask is not None else None)
        self._clip_T = None
        if imgs.dim() == 5:
            B, C, T, H, W = imgs.shape
            self._clip_T = T
            imgs = imgs.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
            if mask is not None:
                mask = mask.permute(0, 2, 1, 3, 4).reshape(B * T, 1, H, W)
        self.real_H = imgs.contiguous()
        self.mask = mask.contiguous() if mask is not None else None

    def _to_device(self, t):
        """host -> device.  A PINNED source (the training loader's default here, data/__init__.py) is copied on a side stream, so the copy
        runs beside whatever the step's stream still holds -- with train.deferred_logs that is the previous step -- and the step's stream
        only waits for the copy's event; a pageable source is copied in stream order (the host blocks: torch's semantics)."""
        if t.is_cuda or not t.is_pinned():
            return t.to(self.device, torch.float32)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(self.device)
        cur = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(self._copy_stream):
            d = t.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._copy_stream)
        cur.wait_event(ev)
        d.record_stream(cur)
        return d if d.dtype == torch.float32 else d.float()

    # ------------------------------------------------------------------ localisation branch
    def _gate(self, encoded, images):
        """IRNcrop_model.py:344-348,379-388: one pass over the encoded batch forms Q(clamp(encoded)), the spliced (tampered)
        batch for _localise and the PSNR partial sums; the 1.0 / 0.8 forward weight stays on the device.  Where train.tamper_cycle names
        copymove for this step, the one pass is ops.copymove_fwd instead and self._loc carries the moved mask."""
        mask = self.mask
        if mask is None:
            mask = torch.zeros(encoded.shape[0], 1, encoded.shape[2], encoded.shape[3], device=encoded.device)
        kind = self.tamper_cycle[self.global_step % len(self.tamper_cycle)]
        if kind == "copymove":
            # IRNp_model.py:561-598: the masked region is filled with the same frame moved by the drawn shift, and the mask moves with it;
            # from here on the moved mask is the ground truth (the loss target and the gradient's 1 - mask)
            B, _, H, W = encoded.shape
            shifts = draw_copymove_shifts(B, H, W, self.copymove_shift_frac, self._clip_T if self.copymove_per_clip else None,
                                          self.copymove_rand)
            _, tampered, mask, part = ops.copymove_fwd(encoded, mask, shifts, real=images)
            self._tamper = (kind, shifts, ops.copymove_valid(part, B * H * W))
            part = part[0]
        else:
            _, tampered, part = ops.splice_fwd(encoded, real=images, prev=self.previous_images, mask=mask)
            self._tamper = (kind, None, mask.mean() if self.log_tamper else None)
        self._loc = (tampered, mask)
        return ops.psnr_gate(part, encoded.numel(), 33.0, 1.0, 0.8)

    def _localise(self, encoded, images, g_enc):
        """IRNcrop_model.py:344-393 on the HIP kernels: STE clamp -> Quantization -> splice with the previous batch by the
        mask -> attack -> STE clamp -> Quantization -> UNet -> BCEWithLogits on the (sigmoid) mask.  Adds the gradient wrt
        `encoded` into g_enc (the splice passes g*(1-mask); clamp_with_grad and Quantization are identities backwards),
        steps the localiser, returns the logs."""
        net = self.localizer
        if self._loc is None:
            self._gate(encoded, images)
        (tampered, mask), self._loc = self._loc, None
        kind = self.attack.name                                     # the step's attack (set by the embed -> attack -> extract pass)
        if self.hybrid is not None:
            attacked_q, cA = self.hybrid.fwd(tampered, cover=images)    # every layer, mixed per frame, clamped and quantised (:347-373)
        else:
            attacked, cA = self.attack.fwd(tampered, exclude=(Crop,), cover=images)   # the reference's localiser sees no geometric attack (:362-366)
            attacked_q = ops.clamp_quant(attacked)                  # clamp_with_grad + Quantization (:372-373)
        if self.keep_outputs:
            self.last_outputs.update(tampered=tampered, attacked=attacked_q, mask_gt=mask, shifts=self._tamper[1])
        if self.localizer_arch == "unetd":
            loss, dice, pred, g_att = unetd_localiser_step(net, self.localizer_flat, self.optimizer_localizer, attacked_q, mask,
                                                           weight=self.localizer_weight, dice_weight=self.dice_weight, amp=self.amp,
                                                           grad_sync=self.grad_sync, clip=self._clip if self.gradient_clipping else None)
            if self.keep_outputs:
                self.last_outputs["pred"] = pred
            return self._localise_tail(cA, g_att, g_enc, mask, kind, loss, dice)
        net.refresh_packs()   # all conv weights of the localiser packed in one launch, valid until its optimiser step
        try:
            pred, cU = net.fwd(attacked_q)
            if self.keep_outputs:
                self.last_outputs["pred"] = pred
            # the reference applies BCEWithLogits to the sigmoid output (:378,391-393); the kernel chains sigmoid'
            loss, g_logit = ops.bce_logits_target(pred, mask, self.localizer_weight, chain_sigmoid=True,
                                                  gscale_dev=self.amp.scale if self.amp is not None else None)
            dice = None
            if self.dice_weight > 0:   # three launches: sums, finalise, backward accumulated into g_logit (the same loss scale, on the device)
                dice, _ = ops.dice_binary(pred, mask, 1.0, 2.0, 'mean', want_grad=True, chain_sigmoid=True, gscale=self.dice_weight,
                                          gscale_dev=self.amp.scale if self.amp is not None else None, grad_out=g_logit)
            grads = engine.grad_dict(net)
            # data parallel: the localiser's 31 MB of gradients leave in four reverse-order buckets from inside its backward
            gs, pending = self.grad_sync, []
            ready = (lambda lo, hi: pending.append(gs.start(net.flat_grads[lo:hi]))) if gs is not None else None
            g_att = net.bwd(cU, g_logit.view_as(pred), grads, accumulate=False, need_input_grad=True, g_is_logit=True, bucket_ready=ready)
        finally:
            net.invalidate_packs()
        gscale = 1.0
        if gs is not None:
            gs.finish_all(pending)
            gscale = gs.scale
            if self.gradient_clipping:
                gs.average_(net.flat_grads)
                gscale = 1.0
        self._clip([net.flat_grads])
        self.optimizer_localizer.step(grad_scale=gscale)
        return self._localise_tail(cA, g_att, g_enc, mask, kind, loss, dice)

    def _localise_tail(self, cA, g_att, g_enc, mask, kind, loss, dice):
        """the localiser's input gradient back through the attack and the splice into g_enc; the step's logs"""
        g_tamp = self.hybrid.bwd(cA, g_att) if self.hybrid is not None else self.attack.bwd(cA, g_att)
        ops.masked_axpy_(g_enc, g_tamp.contiguous(), mask)
        loc_kind = self.hybrid.name if self.hybrid is not None else self.attack.name
        logs = [('lB', loss), ('CE', loss)] + ([('Dice', dice)] if dice is not None else []) + [('Kind', kind), ('LocKind', loc_kind)]
        if self.log_tamper:
            logs += [('Tamper', self._tamper[0]), ('Valid', self._tamper[2])]
        return logs

    @torch.no_grad()
    def tamper(self, images, mask, kind, shifts=None, source=None):
        """The step's forgery on a batch of one's own, for evaluation scripts: images [B,C,H,W] (clamped and quantised as the step does),
        mask [B,1,H,W] -> (tampered, mask_gt).  kind 'copymove': shifts = B (sx, sy) pairs or an int32 [B,2] device tensor (default: drawn
        as the step draws them, one draw for the batch); mask_gt is the moved mask.  kind 'splicing': source = the batch spliced in
        (default: the previous batch); mask_gt is the mask."""
        if kind not in TAMPER_KINDS:
            raise ValueError(f"tamper: kind must be one of {TAMPER_KINDS}, got {kind!r}")
        images = images.to(self.device, torch.float32).contiguous()
        mask = mask.to(self.device, torch.float32).contiguous()
        if kind == "copymove":
            if shifts is None:
                shifts = draw_copymove_shifts(images.shape[0], images.shape[2], images.shape[3], self.copymove_shift_frac, None, self.copymove_rand)
            _, tampered, mask_gt, _ = ops.copymove_fwd(images, mask, shifts)
            return tampered, mask_gt
        source = self.previous_images if source is None else source
        if source is None:
            raise RuntimeError("tamper: splicing needs a source batch (none given and no previous batch fed yet)")
        _, tampered, _ = ops.splice_fwd(images, prev=source.to(self.device, torch.float32), mask=mask)
        return tampered, mask

    def _clip(self, flats):
        if self.gradient_clipping:
            ops.clip_grad_norm_(flats, self.gradient_clipping)   # joint norm, clip coefficient stays on the device

    @torch.no_grad()
    def localise_mask(self, images, threshold=0.5):
        """integer tamper mask of a batch: the localiser in eval mode (running BatchNorm statistics), sigmoid output > threshold,
        uint8 [B,1,H,W]"""
        if self.localizer is None:
            raise RuntimeError("this model was built without the localiser (train.localizer)")
        x = images.to(self.device, torch.float32).contiguous()
        was = self.localizer.training
        self.localizer.eval()
        try:
            if self.localizer_arch == "unetd":
                pred, _ = self.localizer(x)      # (eval mode: no power iteration, weight_u / weight_v untouched)
            else:
                pred, _ = self.localizer.fwd(x, training=False)
        finally:
            self.localizer.train(was)
        return ops.mask_threshold(pred, threshold)

    # ------------------------------------------------------------------ the step
    def optimize_parameters(self, step, latest_values=None, train=True, eval_dir=None):
        self.global_step = self.global_step + 1
        logs, debug_logs = [], []
        self.real_H = torch.clamp(self.real_H, 0, 1)
        ready = self.previous_images is not None and self.previous_previous_images is not None
        if ready and train:
            B = self.real_H.shape[0]
            L = self.hidden.config.message_length
            messages = self.messages if self.messages is not None else torch.randint(0, 2, (B, L), device=self.device).float()
            self.attack.k = step
            extra = self._localise if self.use_localizer else None
            gate = self._gate if (self.use_localizer and self.psnr_gate) else None
            self._loc = None
            dump = bool(self.image_dump_interval and self.image_dump_dir and step % self.image_dump_interval == 10 % self.image_dump_interval)
            keep, self.keep_outputs = self.keep_outputs, self.keep_outputs or dump
            if self.keep_outputs:
                self.last_outputs = {}
            losses, outs = self.hidden.train_on_batch([self.real_H, messages], extra_encoded_grad=extra,
                                                      clip=self._clip if self.gradient_clipping else None, enc_gate=gate)
            if self.keep_outputs:
                self.last_outputs.update(encoded=outs[0], noised=outs[1], decoded=outs[2])
            self.keep_outputs = keep
            extra_logs = losses.pop('_extra', [])
            lr = self.get_current_learning_rate()

            def read_logs():   # waits for the step's scalars (the reference's .item() calls)
                out = [(k.strip(), v) for k, v in losses.items()]
                for name, v in extra_logs:
                    out.append((name, v.item() if torch.is_tensor(v) else v))
                out.append(('lr', lr))
                return out
            if self.deferred_logs and self.writer is None and not dump:
                logs = DeferredLogs(read_logs)   # train.deferred_logs: read when the caller first looks at them (train.py: one step later)
            else:
                logs = read_logs()
                self._log_side(step, logs)
        elif ready:
            L = self.hidden.config.message_length
            messages = torch.randint(0, 2, (self.real_H.shape[0], L), device=self.device).float()
            losses, _ = self.hidden.validate_on_batch([self.real_H, messages])
            logs = [(k.strip(), v) for k, v in losses.items()]
            if self.eval_metrics:
                logs += self.robustness_report(messages)
        # ---- finally (IRNrhi_model.py:690-698)
        if step % self.save_interval == 10 and self.rank <= 0 and train:
            self.save(self.global_step)
        if self.real_H is not None:
            if self.previous_images is not None:
                self.previous_previous_images = self.previous_images
            self.previous_images = self.real_H.clone().detach()
        return logs, debug_logs

    def _log_side(self, step, logs):
        """TensorBoard scalars of every float in `logs` and, every image_dump_interval steps, the stitched sheet
        input | watermarked | 10 x |difference| | attacked | predicted mask | mask (IRNcrop_model.py:399-400,421-437)"""
        if self.writer is not None:
            for name, v in logs:
                if isinstance(v, float):
                    self.writer.add_scalar(name, v, global_step=self.global_step)
            self.writer.flush()
        n = self.image_dump_interval
        if n and self.image_dump_dir and self.rank <= 0 and step % n == 10 % n and self.last_outputs.get("encoded") is not None:
            from ..utils import postprocess, stitch_images
            o = self.last_outputs
            x, enc = self.real_H[:4], o["encoded"][:4].clamp(0, 1)
            cols = [postprocess(enc), postprocess((10 * (x - enc).abs()).clamp(0, 1))]
            if o.get("attacked") is not None:
                cols += [postprocess(o["attacked"][:4].clamp(0, 1)), postprocess(o["pred"][:4].expand(-1, 3, -1, -1)),
                         postprocess(self.mask[:4].expand(-1, 3, -1, -1))]
            else:
                cols.append(postprocess(o["noised"][:4].clamp(0, 1)))
            sheet = stitch_images(postprocess(x), *cols, img_per_row=1)
            os.makedirs(self.image_dump_dir, exist_ok=True)
            sheet.save(os.path.join(self.image_dump_dir, str(step).zfill(5) + ".png"))

    @torch.no_grad()
    def robustness_report(self, messages=None):
        """How good the model is on the fed batch, in Progbar format [(name, float)]: ('PSNR', .), ('SSIM', .) of the watermarked batch, and per
        layer of the attack cycle ('BER/<layer>', .), ('dec_mse/<layer>', .) (Hidden.evaluate_on_batch).  With train.localizer and a fed mask:
        the tampered batch is built as in training (_gate: quantised encoded spliced with the previous batch by the mask), every non-geometric
        attack runs on it, and the localiser's thresholded mask is scored against self.mask: ('F1/<layer>', .), ('precision/<layer>', .),
        ('recall/<layer>', .).  Everything is computed on the device and read with one copy at the end."""
        if self.real_H is None:
            raise RuntimeError("robustness_report: feed_data first")
        images = torch.clamp(self.real_H, 0, 1)
        B = images.shape[0]
        if messages is None:
            messages = self.messages if self.messages is not None else torch.randint(0, 2, (B, self.hidden.config.message_length),
                                                                                     device=self.device).float()
        layers = self.attack.layers or [Identity()]
        names_of = [getattr(l, "name", None) or type(l).__name__ for l in layers]

        class _Fixed:   # one layer of the cycle with the cycle's fixed arguments (Resize 0.7, the Crop rectangle)
            def __init__(self, cycle, i, name):
                self.cycle, self.i, self.name = cycle, i, name

            def fwd(self, image, cover=None):
                out = self.cycle.fwd(image, id=self.i, cover=cover)
                self.name = self.cycle.name   # (a layer may name itself in its forward: G_Blur -> GaussianBlur)
                return out

            def bwd(self, ctx, g):
                return self.cycle.bwd(ctx, g)
        noisers = [_Fixed(self.attack, i, n) for i, n in enumerate(names_of)] if self.attack.layers else [Identity()]
        vals, names = self.hidden.evaluate_on_batch([images, messages], noisers)
        vals, names = [vals], list(names)
        if self.localizer is not None and self.mask is not None and self.previous_images is not None:
            from .. import metrics
            enc_net = self.netG.encoder
            was = self.netG.training
            self.netG.eval()
            try:
                encoded, _ = enc_net.fwd(images, messages.to(self.device, torch.float32).contiguous(), training=False)
            finally:
                self.netG.train(was)
            _, tampered, _ = ops.splice_fwd(encoded, real=images, prev=self.previous_images, mask=self.mask)
            for i, (layer, lname) in enumerate(zip(layers, names_of)):
                if isinstance(layer, (Crop, Resize)):   # the localiser sees no geometric attack (IRNcrop_model.py:362-366)
                    continue
                attacked, _ = self.attack.fwd(tampered, id=i, cover=images)
                lname = self.attack.name
                pred = self.localise_mask(ops.clamp_quant(attacked.contiguous()))
                c = ops.confusion_counts(pred, self.mask, 0.5, 0.5)[0]
                sc = metrics.scores_from_counts(c)
                tp, fp, fn = sc["TP"].double(), sc["FP"].double(), sc["FN"].double()
                vals.append(torch.stack([sc["F1"], tp / (tp + fp), tp / (tp + fn)]).float())
                names += ['F1/' + lname, 'precision/' + lname, 'recall/' + lname]
        host = torch.cat(vals).tolist()   # the one device -> host read
        return list(zip(names, host))

    def evaluate(self, *args, **kwargs):
        return self.optimize_parameters(self.global_step, train=False)

    # ------------------------------------------------------------------ checkpoints
    def _nets(self):
        nets = [(self.netG.encoder, 'encoder'), (self.netG.decoder, 'decoder'), (self.discriminator, 'discriminator')]
        if self.localizer is not None:
            nets.append((self.localizer, 'localizer'))
        return nets

    def save(self, iter_label):
        path = _get(self.opt, 'path', 'models', default=None)
        if path is None:
            return []
        return [self.save_network(net, label, iter_label, model_path=path) for net, label in self._nets()]

    def load(self):
        for net, label in self._nets():
            p = _get(self.opt, 'path', 'pretrain_model_' + label, default=None)
            if p and os.path.exists(p):
                self.load_network(p, net, _get(self.opt, 'path', 'strict_load', default=True))
