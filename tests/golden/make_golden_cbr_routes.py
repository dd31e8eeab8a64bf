#!/usr/bin/env python3
"""Record tests/golden/cbr_routes.json: the launch trace of engine.cbr_backward and Encoder.bwd, case by case, on the CPU.

The backward dispatcher is host code: which kernel a layer gets, with which arguments, and what it hands to the next layer is decided
before anything is launched.  This recorder replaces every LAUNCHING ops function the backward calls by a spy that appends a record
and returns empty CPU (or meta) tensors of the shapes the real function returns (partial-sum rows: 2); the `*_supported` queries,
`conv3x3_bwd_fused_gvec_max_batch` and `fin_rider_enabled` are host functions of the built library and stay the real ones.

A record holds the op's name and every argument under its parameter name: scalars as they are, a tensor as a LABEL that says which tensor
it is (the case's `g`, `gvec`, `y`, `x.t`, `x.scale`, `stats`, a parameter, `grad(parameter)`, `j.op[k]` = result k of call j; small
int32 tensors -- the permutations -- by content), a rider (`fin`) as a dict of the same; a callable `fin` is called with the spy's partial
rows and recorded as what it returned.  After the calls of a case: the label of the returned tensor, its sweep and premasked attributes,
and whether sums were left on the layer's input (and whether that record's coef is None).

tests/test_cpu_cbr_routes.py replays the same cases against the working tree and compares record for record, so the fixture is recorded
ONCE from the code whose behaviour is to be kept and never regenerated from code that restructures the dispatcher:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cbr_routes.py

Run against an engine that has the route table (engine.select_bwd_route), it writes nothing: it checks the coverage condition on that code
and compares its trace with the fixture.

Recording also asserts the coverage condition: every `return` statement of engine.cbr_backward (and of select_bwd_route, where the
engine has it) is the exit of at least one case, and every case's first launching op is the one it names --
the first behind the prelude every route shares (the BatchNorm-backward coefficients and the filter pack, whose order depends on
nothing but argument evaluation), since that is the op that tells the routes apart; None: the prelude is all there is.
"""
import ast
import inspect
import json
import os
import sys
import textwrap
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "cbr_routes.json")
BF16, F32 = "bfloat16", "float32"


def _case(first, x="cbr", Cout=64, dtype=BF16, H=16, W=16, B=2, dev="cpu", g="dense", gvec=False, g_rev=None, g_masked=False, sums=None,
          perm=False, pool_stats=False, coef_pre=False, unsupported=(), **kw):
    """first: the first launching op the case must record (behind the PRELUDE).  x: what feeds the layer -- 'image' (16 channels, 3 real), 'cbr' (a ConvBNRelu
    output), 'cbr_nosrc' (one that does not know its BatchNorm), 'cbr_strided' (a channel slice of a wider tensor), 'plain64' (64 channels,
    no BatchNorm in front: a pooled tensor), 'cat' (the encoder's 112-channel concat).  g: 'dense' | 'wide' (more channels than y) | None.
    sums: None | 'raw' | 'coef' -- what the consumer left on this layer's output for g.  kw: cbr_backward's keyword arguments."""
    return dict(first=first, x=x, Cout=Cout, dtype=dtype, H=H, W=W, B=B, dev=dev, g=g, gvec=gvec, g_rev=g_rev, g_masked=g_masked, sums=sums,
                perm=perm, pool_stats=pool_stats, coef_pre=coef_pre, unsupported=list(unsupported), kw=kw)


PRELUDE = ("bn_bwd_coef", "bn_bwd_coef_raw", "bn_bwd_coef_pooled", "pack_w3x3")
GV = dict(g=None, gvec=True)
CASES = {
    # 1. image-fed first layer, no input gradient
    "first_layer_weights_only": _case("conv3x3_wgrad_bnfused", x="image", need_input_grad=False, accumulate=True),
    # 2. weight_grads=False
    "no_wgrad_no_dx": _case(None, weight_grads=False, need_input_grad=False),
    "no_wgrad_gvec_feed": _case("conv3x3_dgrad_bwdstats", weight_grads=False, **GV),
    "no_wgrad_dense_feed": _case("conv3x3_dgrad_applyfused", weight_grads=False, g_rev=False, sums="raw"),
    "no_wgrad_dense_rows32": _case("conv3x3_dgrad_applyfused", x="image", weight_grads=False, g_rev=True),
    "no_wgrad_f32": _case("bn_bwd", dtype=F32, weight_grads=False),
    # 3. pooled last layer
    "pooled_onepass": _case("conv3x3_bwd_fused", H=8, accumulate=True, **GV),
    "pooled_over_batch_limit": _case("conv3x3_dgrad_bwdstats", H=8, B="max_batch+1", dev="meta", **GV),
    "pooled_64_to_30": _case("conv3x3_dgrad_bwdstats", Cout=30, **GV),
    "pooled_feeder_without_bn": _case("conv3x3_bwd_fused", x="cbr_nosrc", **GV),
    "pooled_feeder_strided": _case("conv3x3_wgrad_gvfused", x="cbr_strided", **GV),
    "pooled_image_fed": _case("bn_bwd", x="image", **GV),
    "pooled_pool_stats": _case("conv3x3_bwd_fused", pool_stats=True, **GV),
    "pooled_coef_pre": _case("conv3x3_bwd_fused", pool_stats=True, coef_pre=True, **GV),
    # 4. image-fed first layer with input gradient
    "first_layer_dx": _case("conv3x3_bwd_fused16", x="image", g_rev=False, g_masked=True),
    "first_layer_dx_premasked": _case("conv3x3_bwd_fused16", x="image", g_rev=True, g_masked=True, sums="raw", accumulate=True),
    "first_layer_dx_12x20": _case("conv3x3_dgrad_applyfused", x="image", H=12, W=20),
    "first_layer_dx_32_channels": _case("conv3x3_dgrad_applyfused", x="image", dgrad_channels=32),
    # 5. ordinary 64 -> 64 layer (7.: the three ways the coefficients resolve when sums were left or not)
    "body_onepass": _case("conv3x3_bwd_fused", g_rev=False),
    "body_onepass_premasked": _case("conv3x3_bwd_fused", g_rev=True, g_masked=True, sums="raw", accumulate=True),
    "body_onepass_rider_coef": _case("conv3x3_bwd_fused", g_masked=True, sums="coef"),
    "body_onepass_sums_unmasked": _case("conv3x3_bwd_fused", sums="raw"),
    "body_onepass_8x16": _case("conv3x3_bwd_fused", H=8),
    "body_two_kernels": _case("conv3x3_dgrad_applyfused", g_rev=False, unsupported=["conv3x3_bwd_fused_supported"]),
    "body_feeder_without_bn": _case("conv3x3_dgrad_applyfused", x="cbr_nosrc", unsupported=["conv3x3_bwd_fused_supported"]),
    "body_plain_input": _case("conv3x3_dgrad_applyfused", x="plain64", g_rev=True),
    # 6. the generic route
    "generic_f32": _case("bn_bwd", dtype=F32),
    "generic_f32_weights_only": _case("bn_bwd", dtype=F32, need_input_grad=False, accumulate=True),
    "generic_f32_perm": _case("bn_bwd", x="cat", dtype=F32, perm=True, dgrad_channels=64),
    "generic_f32_perm_weights_only": _case("bn_bwd", x="cat", dtype=F32, perm=True, dgrad_channels=64, need_input_grad=False),
    "generic_bf16_perm": _case("bn_bwd", x="cat", perm=True, dgrad_channels=64, sums="raw"),
    "generic_wide_g_feed": _case("bn_bwd", g="wide"),
    "generic_f32_sums_left": _case("bn_bwd", dtype=F32, sums="raw"),
}
ENCODER_CASES = {   # 8. Encoder.bwd end to end on a ctx built by hand
    "encoder_split": dict(first="conv1x1_head_bwd", split=True, dtype=BF16),   # (the head's backward comes before any prelude)
    "encoder_unsplit": dict(first="conv1x1_head_bwd", split=False, dtype=BF16),
    "encoder_unsplit_f32": dict(first="conv1x1_head_bwd", split=False, dtype=F32),
}


# ------------------------------------------------------------------------------------------------ the trace
class Trace:
    def __init__(self):
        self.calls, self.by_id, self.by_key, self.keep = [], {}, {}, []

    @staticmethod
    def _key(t):
        return None if t.device.type == "meta" else (t.data_ptr(), t.numel(), t.dtype)

    def name(self, t, label):
        """`t` (and every tensor over the same memory, such as a fresh `.data` alias or a reshaping view) is called `label`"""
        self.keep.append(t)
        self.by_id[id(t)] = label
        if self._key(t) is not None:
            self.by_key.setdefault(self._key(t), label)
        return t

    def label(self, t, where):
        if id(t) in self.by_id:
            return self.by_id[id(t)]
        if self._key(t) in self.by_key:
            return self.by_key[self._key(t)]
        if t.dtype == torch.int32 and t.device.type == "cpu" and t.numel() <= 4096:
            return "i32[%d]#%08x" % (t.numel(), zlib.crc32(repr(t.tolist()).encode()))
        return self.by_id[id(self.name(t, where))]      # a tensor the code under test made itself: named after where it first shows

    def enc(self, v, where):
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, torch.dtype):
            return str(v)
        if isinstance(v, torch.Tensor):
            return self.label(v, where)
        if isinstance(v, dict):
            return {k: self.enc(v[k], where + "." + k) for k in sorted(v)}
        if isinstance(v, (tuple, list, torch.Size)):
            if all(isinstance(e, int) for e in v):
                return list(v) if len(v) <= 8 else "ints[%d]#%08x" % (len(v), zlib.crc32(repr(list(v)).encode()))
            return [self.enc(e, "%s[%d]" % (where, i)) for i, e in enumerate(v)]
        raise TypeError("cannot record %r (%s)" % (v, where))


def _f32(dev, *shape):
    return torch.empty(*shape, device=dev, dtype=torch.float32)


def _coef(a):
    return _f32(a["y"].device, 3, a["y"].shape[-1])


def _rider_coef(fin, dev):
    return None if fin is None else _f32(dev, 3, fin["y_shape"][-1])


def _nhwc(like, C):
    return torch.empty(*like.shape[:3], C, device=like.device, dtype=like.dtype)


def _masked(t):
    t._wm_masked = True     # as ops.conv3x3_dgrad_bwdstats / conv3x3_dgrad_applyfused / conv3x3_bwd_fused tag their input gradient
    return t


def _r_conv3x3_fwd(a):
    x, wp = a["x"], a["wp"]
    return _nhwc(x, wp.shape[1]), (_f32(x.device, 2, 2, wp.shape[1]) if a["want_stats"] else None)


def _r_pack(a):
    shape = (9, a["CinP"], a["CoutP"]) if a["transpose"] else (9, a["CoutP"], a["CinP"])
    return torch.empty(shape, device=a["w"].device, dtype=a["dtype"])


def _r_dgrad_bwdstats(a):
    CinP = a["wpt"].shape[1]
    return _masked(_nhwc(a["src"], CinP)), _f32(a["src"].device, 2, 2, CinP)


def _r_dgrad_applyfused(a):
    y, feed = a["y"], a["ry"] is not None
    dx = _nhwc(y, a["wpt"].shape[1])
    return torch.empty_like(y) if a["want_dy"] else None, _masked(dx) if feed else dx, _f32(y.device, 2, 2, 64) if feed else None


def _r_bwd_fused(a):
    y = a["y"]
    part = _f32(y.device, 2, 2, 64)
    if callable(a["fin"]):
        a["fin"] = a["fin"](part)
    return _masked(torch.empty_like(y)), part, _rider_coef(a["fin"], y.device)


def _r_head_bwd(a):
    y = a["y"]
    g = torch.empty_like(y)
    if not a["want_bn_partials"]:
        return g
    return g, (_f32(y.device, 2, 2, y.shape[-1]) if a["scale"] is not None else None)


RESULTS = {
    "bn_bwd_coef": _coef, "bn_bwd_coef_raw": _coef, "bn_bwd_coef_pooled": _coef,
    "bn_bwd": lambda a: torch.empty_like(a["y"]),
    "conv3x3_fwd": _r_conv3x3_fwd,
    "conv3x3_wgrad": lambda a: _rider_coef(a["fin"], a["x"].device),
    "conv3x3_wgrad_bnfused": lambda a: None,
    "conv3x3_wgrad_gvfused": lambda a: _rider_coef(a["fin"], a["x"].device),
    "conv3x3_dgrad_gvfused": lambda a: _nhwc(a["y"], a["wpt"].shape[1]),
    "conv3x3_dgrad_bwdstats": _r_dgrad_bwdstats,
    "conv3x3_dgrad_applyfused": _r_dgrad_applyfused,
    "conv3x3_bwd_fused": _r_bwd_fused,
    "conv3x3_bwd_fused16": lambda a: _nhwc(a["y"], 16),
    "pack_w3x3": _r_pack,
    "conv1x1_head_bwd": _r_head_bwd,
    "nchw_to_nhwc": lambda a: a["out"],
    "concat_side_msg_wgrad": lambda a: None,
}


class spies:
    """with spies(ops, trace, unsupported): the launching ops functions record into `trace`; the named `*_supported` queries answer False"""

    def __init__(self, ops, tr, unsupported=()):
        self.ops, self.tr, self.unsupported, self.saved = ops, tr, unsupported, {}

    def _spy(self, name):
        sig, result, tr = inspect.signature(getattr(self.ops, name)), RESULTS[name], self.tr

        def spy(*args, **kwargs):
            b = sig.bind(*args, **kwargs)
            b.apply_defaults()
            a = dict(b.arguments)
            j = len(tr.calls)
            rec = {"op": name}
            tr.calls.append(rec)
            out = result(a)
            for k, t in enumerate(out if isinstance(out, tuple) else (out,)):
                if t is not None and id(t) not in tr.by_id:
                    tr.name(t, "%d.%s[%d]" % (j, name, k))
            rec["args"] = {k: tr.enc(v, "%d.%s:%s" % (j, name, k)) for k, v in a.items()}
            return out
        return spy

    def __enter__(self):
        for name in RESULTS:
            self.saved[name] = getattr(self.ops, name)
            setattr(self.ops, name, self._spy(name))
        for name in self.unsupported:
            self.saved[name] = getattr(self.ops, name)
            setattr(self.ops, name, lambda *a, **k: False)
        return self

    def __exit__(self, *exc):
        for name, f in self.saved.items():
            setattr(self.ops, name, f)


# ------------------------------------------------------------------------------------------------ building a case
def _leave(engine, act, g, part, coef):
    """what a consumer's input-gradient kernel leaves on `act` for the tensor g it returned"""
    if hasattr(engine, "leave_bn_sums"):
        engine.leave_bn_sums(act, g, part, coef)
    else:
        act.bwd = (g, part, coef, g._version)


def _params(tr, grads, prefix, mod):
    for n, p in mod.named_parameters():
        tr.name(p.data, prefix + n)
        grads[p] = tr.name(torch.zeros_like(p.data), "grad(%s%s)" % (prefix, n))


def _input(engine, tr, grads, kind, B, H, W, dt, dev):
    if kind == "image":
        return engine.Act(tr.name(torch.empty(B, H, W, 16, device=dev, dtype=dt), "x.t"), 3)
    if kind == "plain64":
        return engine.Act(tr.name(torch.empty(B, H, W, 64, device=dev, dtype=dt), "x.t"), 64)
    if kind == "cat":
        return engine.Act(tr.name(torch.empty(B, H, W, 112, device=dev, dtype=dt), "x.t"), 97)
    pbn = torch.nn.BatchNorm2d(64)
    _params(tr, grads, "pbn.", pbn)
    pstats = tr.name(_f32(dev, 4, 64), "x.stats")
    t = torch.empty(B, H, W, 128, device=dev, dtype=dt)[..., :64] if kind == "cbr_strided" else torch.empty(B, H, W, 64, device=dev, dtype=dt)
    return engine.Act(tr.name(t, "x.t"), 64, tr.name(pstats[0], "x.scale"), tr.name(pstats[1], "x.shift"),
                      src=None if kind == "cbr_nosrc" else (pbn, pstats))


def _ctx(engine, tr, tag, bn, x, Cout, B, H, W, dt, dev, perm=None):
    CoutP = engine.round_up(Cout, 32)
    ctx = engine.CBRCtx()
    ctx.x, ctx.perm, ctx.training = x, perm, True
    ctx.y = tr.name(torch.empty(B, H, W, CoutP, device=dev, dtype=dt), tag + "y")
    ctx.stats = tr.name(_f32(dev, 4, CoutP), tag + "stats")
    ctx.out = engine.Act(ctx.y, Cout, tr.name(ctx.stats[0], tag + "scale"), tr.name(ctx.stats[1], tag + "shift"), rev=False, src=(bn, ctx.stats))
    return ctx


def build_cbr_case(engine, ops, case, tr):
    """-> (conv, bn, ctx, grads, keyword arguments of cbr_backward) of one CASES entry, every tensor named in `tr`"""
    torch.manual_seed(0)
    dt, dev, H, W = getattr(torch, case["dtype"]), case["dev"], case["H"], case["W"]
    B = ops.conv3x3_bwd_fused_gvec_max_batch() + 1 if case["B"] == "max_batch+1" else case["B"]
    grads = {}
    x = _input(engine, tr, grads, case["x"], B, H, W, dt, dev)
    conv, bn = torch.nn.Conv2d(x.C, case["Cout"], 3, padding=1), torch.nn.BatchNorm2d(case["Cout"])
    _params(tr, grads, "conv.", conv)
    _params(tr, grads, "bn.", bn)
    perm = list(range(30, 94)) + list(range(30)) + [94, 95, 96] if case["perm"] else None
    ctx = _ctx(engine, tr, "", bn, x, case["Cout"], B, H, W, dt, dev, perm)
    CoutP = ctx.y.shape[-1]
    kw = dict(case["kw"])
    if case["g"] is not None:
        g = kw["g"] = tr.name(torch.empty(B, H, W, CoutP * (2 if case["g"] == "wide" else 1), device=dev, dtype=dt), "g")
        if case["g_rev"] is not None:
            g._wm_rev = case["g_rev"]
        if case["g_masked"]:
            g._wm_masked = True
        if case["sums"] is not None:
            _leave(engine, ctx.out, g, tr.name(_f32(dev, 2, 2, CoutP), "sums.partials"),
                   tr.name(_f32(dev, 3, CoutP), "sums.coef") if case["sums"] == "coef" else None)
    if case["gvec"]:
        kw["gvec"] = tr.name(_f32(dev, B, CoutP), "gvec")
    if case["pool_stats"]:
        kw["pool_stats"] = (tr.name(_f32(dev, B, CoutP), "pool.npos"), tr.name(_f32(dev, B, CoutP), "pool.ysum"))
    if case["coef_pre"]:
        kw["coef_pre"] = tr.name(_f32(dev, 3, CoutP), "coef_pre")
    if case["perm"]:
        kw["perm_dev"] = torch.tensor(perm, dtype=torch.int32)
    return conv, bn, ctx, grads, kw


def _after(tr, ret, x):
    left = x.bwd
    return {"ret": None if ret is None else tr.label(ret, "ret"), "ret_rev": getattr(ret, "_wm_rev", None), "ret_masked": getattr(ret, "_wm_masked", None),
            "sums_left": left is not None, "sums_g": None if left is None else tr.label(left[0], "left.g"),
            "sums_partials": None if left is None else tr.label(left[1], "left.partials"),
            "sums_coef": None if left is None or left[2] is None else tr.label(left[2], "left.coef"),
            "sums_version_current": None if left is None else left[3] == left[0]._version}


def run_cbr_case(engine, ops, case):
    tr = Trace()
    conv, bn, ctx, grads, kw = build_cbr_case(engine, ops, case, tr)
    with spies(ops, tr, case["unsupported"]):
        ret = engine.cbr_backward(conv, bn, ctx, grads, **kw)
    assert ctx.out.bwd is None      # whatever was left for this layer is taken
    return {"calls": tr.calls, "after": _after(tr, ret, ctx.x)}


def build_encoder_case(engine, encoder_mod, case, tr):
    """-> (Encoder, its ctx built by hand, grads, g_enc): 2 x 16 x 16, four body layers, 30 message bits"""
    from video_watermarking_forgery_detection_amd.options import HiDDenConfiguration
    torch.manual_seed(0)
    B, H, W, dt, dev = 2, 16, 16, getattr(torch, case["dtype"]), "cpu"
    enc = encoder_mod.Encoder(HiDDenConfiguration(H=H, W=W))
    grads = {}
    _params(tr, grads, "", enc)
    ctx = encoder_mod.EncCtx()
    ctx.B, ctx.H, ctx.W, ctx.split, ctx.layers = B, H, W, case["split"], []
    a = engine.Act(tr.name(torch.empty(B, H, W, 16, device=dev, dtype=dt), "image16"), 3)
    for i, blk in enumerate(enc.conv_layers):
        ctx.layers.append(_ctx(engine, tr, "L%d." % i, blk.layers[1], a, 64, B, H, W, dt, dev))
        a = ctx.layers[-1].out
    bn = enc.after_concat_layer.layers[1]
    if case["split"]:
        ctx.cat_ctx = _ctx(engine, tr, "cat.", bn, a, 64, B, H, W, dt, dev)
        ctx.message, ctx.image = tr.name(_f32(dev, B, 30), "message"), tr.name(_f32(dev, B, 3, H, W), "image")
    else:
        cat = engine.Act(tr.name(torch.empty(B, H, W, enc._cat_ld, device=dev, dtype=dt), "cat.x.t"), 97)
        ctx.cat_ctx = _ctx(engine, tr, "cat.", bn, cat, 64, B, H, W, dt, dev, perm=enc._perm)
    ctx.final_in = ctx.cat_ctx.out
    return enc, ctx, grads, tr.name(_f32(dev, B, 3, H, W), "g_enc")


def run_encoder_case(engine, ops, encoder_mod, case):
    tr = Trace()
    enc, ctx, grads, g_enc = build_encoder_case(engine, encoder_mod, case, tr)
    with spies(ops, tr, case.get("unsupported", ())):
        ret = enc.bwd(ctx, g_enc, grads, accumulate=False)
    assert ret is None and all(c.out.bwd is None for c in ctx.layers + [ctx.cat_ctx])
    return {"calls": tr.calls, "after": _after(tr, None, ctx.cat_ctx.x)}


def first_op(rec):
    return next((c["op"] for c in rec["calls"] if c["op"] not in PRELUDE), None)


def run_all(engine, ops, encoder_mod):
    out = {name: run_cbr_case(engine, ops, case) for name, case in CASES.items()}
    out.update((name, run_encoder_case(engine, ops, encoder_mod, case)) for name, case in ENCODER_CASES.items())
    for name, rec in out.items():
        first = (CASES.get(name) or ENCODER_CASES[name])["first"]
        assert first_op(rec) == first, (name, first_op(rec), first)
    return json.loads(json.dumps(out))      # tuples -> lists: what a reader of the fixture gets


# ------------------------------------------------------------------------------------------------ the coverage condition
class ExitCoverage:
    """which `return` statements of the given functions were the exit of a call (nested helpers are not counted)"""

    def __init__(self, funcs):
        self.returns, self.hit, self.codes = {}, set(), {}
        for f in funcs:
            src, first = inspect.getsourcelines(f)
            fn = ast.parse(textwrap.dedent("".join(src))).body[0]
            todo, lines = list(fn.body), set()
            while todo:
                n = todo.pop()
                if isinstance(n, (ast.FunctionDef, ast.Lambda)):
                    continue
                if isinstance(n, ast.Return):
                    lines.add(first + n.lineno - 1)
                todo.extend(ast.iter_child_nodes(n))
            self.codes[f.__code__] = f.__name__
            self.returns[f.__name__] = lines

    def _trace(self, frame, event, arg):
        if event == "call":
            return self._trace if frame.f_code in self.codes else None
        if event == "return":
            self.hit.add((self.codes[frame.f_code], frame.f_lineno))
        return self._trace

    def __enter__(self):
        sys.settrace(self._trace)
        return self

    def __exit__(self, *exc):
        sys.settrace(None)

    def missed(self):
        return sorted((n, ln) for n, lines in self.returns.items() for ln in lines if (n, ln) not in self.hit)


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, ROOT)
    from video_watermarking_forgery_detection_amd import engine, ops
    from video_watermarking_forgery_detection_amd.hidden_models import encoder as encoder_mod
    split = hasattr(engine, "select_bwd_route")     # the dispatcher is a route table already: this is the code under test, not the record
    funcs = [engine.cbr_backward] + ([engine.select_bwd_route] if split else [])
    with ExitCoverage(funcs) as cov:
        out = run_all(engine, ops, encoder_mod)
    n = sum(len(v) for v in cov.returns.values())
    assert not cov.missed(), "return statements no case leaves through: %s" % cov.missed()
    if split:
        with open(FIXTURE) as f:
            same = json.load(f) == out
        print("the fixture is recorded from the dispatcher before the split and is not rewritten from this one;", len(out), "cases leave through all",
              n, "return statements; the trace", "equals the fixture" if same else "DIFFERS from the fixture")
        sys.exit(0 if same else 1)
    with open(FIXTURE, "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes;", len(out), "cases leave through all", n, "return statements of",
          ", ".join(cov.returns))


if __name__ == "__main__":
    main()
