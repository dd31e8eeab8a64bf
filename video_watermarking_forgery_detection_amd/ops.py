"""Thin Python bindings over the C ABI (include/wm_hip.h): argument checking,
output allocation by torch (device memory + streams are torch's job), raw
pointers into libwm_hip.so.  Every function here launches HIP kernels; none has
a CPU or PyTorch fallback.  Every call goes through _lib.checked(): a status
function that fails raises RuntimeError under its own name, so no call site
looks at a return code.
"""
import ctypes

import torch

from . import _lib

WM_F32, WM_BF16, WM_F16 = 0, 1, 2
_DT = {torch.float32: WM_F32, torch.bfloat16: WM_BF16, torch.float16: WM_F16}


def dt_id(dtype):
    """torch dtype -> WM_F32 / WM_BF16 / WM_F16"""
    try:
        return _DT[dtype]
    except KeyError:
        raise TypeError(f"unsupported activation dtype {dtype} (float32, bfloat16 or float16)") from None


JPEG_ROUND, JPEG_SS, JPEG_MASK = 0, 1, 2


def dtype_id(t):
    return dt_id(t.dtype)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("wm ops run on the GPU only (tensor is on %s); there is no CPU fallback" % t.device)


def _wrote(*ts):
    """a kernel of this library wrote these tensors in place through their raw pointers: bump torch's version counter of each, so that
    every check built on `_version` (engine.cbr_backward's "is this still the tensor my consumer produced", PackPlan's stale-pack test,
    autograd's saved-tensor check) sees the write as it sees torch's own in-place ops.  The counter is shared by a tensor and the views
    torch made of it (a flat buffer and its slices); a parameter whose `.data` was pointed at such a view keeps a counter of its own."""
    for t in ts:
        if t is not None:
            torch.autograd.graph.increment_version(t)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _host_floats(vals):
    arr = (ctypes.c_float * len(vals))(*[float(v) for v in vals])
    return arr


# ----------------------------------------------------------------------------- block JPEG
def jpeg_fwd(x, mode, tables, subsample=0, act16_dtype=None):
    """x [B,3,H,W] f32 cuda; tables: 128 python floats (lum, chroma) or None for mask.  act16_dtype: -> (y, the same image as the
    [B,H,W,16] zero-padded NHWC tensor of that dtype: engine.image_to_act's result without its launch)"""
    _need_cuda(x)
    assert x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32
    x = x.contiguous()
    y = torch.empty_like(x)
    B, _, H, W = x.shape
    a16 = torch.empty(B, H, W, 16, device=x.device, dtype=act16_dtype) if act16_dtype is not None else None
    tb = _host_floats(tables) if tables is not None else None
    _timed("jpeg_fwd", None, lambda: _lib.checked().wm_jpeg_fwd_act(_p(x), _p(y), _p(a16), dt_id(act16_dtype) if a16 is not None else WM_F32, B, H,
                                                                    W, mode, tb, subsample, _stream()))
    return (y, a16) if act16_dtype is not None else y


def jpeg_bwd(x, gy, mode, tables, subsample=0):
    _need_cuda(gy)
    gy = gy.contiguous()
    gx = torch.empty_like(gy)
    B, _, H, W = gy.shape
    tb = _host_floats(tables) if tables is not None else None
    xx = x.contiguous() if x is not None else None
    _timed("jpeg_bwd", None, lambda: _lib.checked().wm_jpeg_bwd(_p(xx), _p(gy), _p(gx), B, H, W, mode, tb, subsample, _stream()))
    return gx


# ----------------------------------------------------------------------------- layout
def _host_ints(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def nchw_to_nhwc(x, out, C_off=0, zero_tail=0):
    """x [B,C,H,W] f32 -> out[B,H,W,ld] (bf16|f32) channels [C_off, C_off+C), zero tail after."""
    _need_cuda(x, out)
    x = x.contiguous()
    B, C, H, W = x.shape
    _lib.checked().wm_nchw_to_nhwc(_p(x), _p(out), B, C, H, W, out.shape[-1], C_off, zero_tail, dtype_id(out), _stream())
    return out


def u8_hwc_to_planes(x, scale=1.0 / 255.0):
    """decoded frames uint8 [N,H,W,C] (cuda) -> float32 planes [N,C,H,W] * scale"""
    _need_cuda(x)
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[-1] <= 4
    x = x.contiguous()
    N, H, W, C = x.shape
    y = torch.empty(N, C, H, W, device=x.device, dtype=torch.float32)
    _lib.checked().wm_u8_hwc_to_planes(_p(x), _p(y), N, H, W, C, scale, _stream())
    return y


def nhwc_to_nchw(x, C, C_off=0):
    _need_cuda(x)
    B, H, W, ld = x.shape
    y = torch.empty(B, C, H, W, device=x.device, dtype=torch.float32)
    _lib.checked().wm_nhwc_to_nchw(_p(x), _p(y), B, C, H, W, ld, C_off, dtype_id(x), _stream())
    return y


def broadcast_to_nhwc(v, out, C_off):
    _need_cuda(v, out)
    v = v.contiguous().float()
    B, H, W, ld = out.shape
    _lib.checked().wm_broadcast_to_nhwc(_p(v), _p(out), B, v.shape[1], H, W, ld, C_off, dtype_id(out), _stream())
    return out


def concat_tail(msg, img, out, C_off):
    """out[..., C_off:] = [msg | img | 0]  (encoder concat tail, one vectorised pass)"""
    _need_cuda(msg, img, out)
    B, H, W, ld = out.shape
    msg = msg.contiguous().float(); img = img.contiguous().float()
    _lib.checked().wm_concat_tail(_p(msg), _p(img), _p(out), B, msg.shape[1], H, W, ld, C_off, ld - C_off, dtype_id(out), _stream())
    return out


def concat_full(x, scale, shift, msg, img, out, C):
    """out = [relu(scale*x+shift)[:C] | msg | img | 0]  (the encoder concat row, one pass, full-line writes)"""
    _need_cuda(x, msg, img, out)
    B, H, W, ld = out.shape
    msg = msg.contiguous().float(); img = img.contiguous().float()
    _lib.checked().wm_concat_full(_p(x), x.shape[-1], _p(scale), _p(shift), _p(msg), _p(img), _p(out), B, C, msg.shape[1], H, W, ld, dtype_id(out),
                                  _stream())
    return out


def bnrelu_copy(x, scale, shift, out, C_off, C):
    B, H, W, ldx = x.shape
    _lib.checked().wm_bnrelu_copy(_p(x), ldx, _p(scale), _p(shift), _p(out), out.shape[-1], C_off, B * H * W, C, dtype_id(x), _stream())
    return out


def pack_w3x3(w, CoutP, CinP, dtype, perm=None, transpose=False):
    """w [Cout,Cin,3,3] f32 -> [9,CoutP,CinP] (or [9,CinP,CoutP] transposed/flipped for dgrad)."""
    _need_cuda(w)
    Cout, Cin = w.shape[0], w.shape[1]
    shape = (9, CinP, CoutP) if transpose else (9, CoutP, CinP)
    wp = torch.empty(shape, device=w.device, dtype=dtype)
    pa = _host_ints(perm) if perm is not None else None
    _lib.checked().wm_pack_w3x3(_p(w), _p(wp), Cout, Cin, CoutP, CinP, pa, 1 if transpose else 0, dtype_id(wp), _stream())
    return wp


class PackPlan:
    """All packed conv weights of one network, refreshed by ONE launch (wm_pack_w3x3_batch).

    Requests are registered lazily (`get` packs one-off with wm_pack_w3x3 while the plan is not valid and remembers the
    request); `refresh()` (re)packs every registered request from the current parameter values and marks the plan valid;
    `invalidate()` must be called whenever the parameters may have changed (optimiser step, state_dict load)."""

    def __init__(self):
        self.req = {}        # key -> (w, CoutP, CinP, dtype, perm tuple | None, transpose)
        self.packed = {}     # key -> packed tensor (stable storage, rewritten by refresh)
        self.jobs = None
        self.njobs = 0
        self.valid = False
        self.max_elems = 0
        self._perm_dev = {}
        self.ver = {}        # key -> the weight tensor's version counter at the last refresh.  What this catches: an in-place write -- torch's or,
                             # through ops._wrote, this library's -- to the very tensor OBJECT handed to get() (or a torch view sharing its
                             # counter).  What it cannot catch: writes through another alias of the storage (`p.data` makes a fresh counter
                             # every time; a parameter pointed at a slice of a flat buffer does not share the buffer's): the owner of
                             # the parameters calls invalidate() / refresh() for those (FlatModule: optimiser step, load_state_dict,
                             # broadcast_parameters)

    @staticmethod
    def key(w, CoutP, CinP, dtype, perm, transpose):
        return (w.data_ptr(), tuple(w.shape), CoutP, CinP, dtype, None if perm is None else tuple(int(v) for v in perm), bool(transpose))

    def get(self, w, CoutP, CinP, dtype, perm=None, transpose=False):
        k = self.key(w, CoutP, CinP, dtype, perm, transpose)
        if self.valid and k in self.packed and self.jobs is not None and self.ver.get(k) == w._version:
            return self.packed[k]
        if k not in self.req:
            self.req[k] = (w, CoutP, CinP, dtype, perm, transpose)
            self.jobs = None           # the job table has to be rebuilt
        return pack_w3x3(w, CoutP, CinP, dtype, perm=perm, transpose=transpose)

    def invalidate(self):
        self.valid = False

    def _build(self):
        import struct
        recs = []
        self.max_elems = 0
        dts = set()
        for k, (w, CoutP, CinP, dtype, perm, transpose) in self.req.items():
            if k not in self.packed:
                shape = (9, CinP, CoutP) if transpose else (9, CoutP, CinP)
                self.packed[k] = torch.empty(shape, device=w.device, dtype=dtype)
            pd = 0
            if perm is not None:
                pk = tuple(int(v) for v in perm)
                if pk not in self._perm_dev:
                    self._perm_dev[pk] = torch.tensor(pk, dtype=torch.int32, device=w.device)
                pd = self._perm_dev[pk].data_ptr()
            recs.append(struct.pack("<QQQiiiiii", w.data_ptr(), self.packed[k].data_ptr(), pd, w.shape[0], w.shape[1],
                                    CoutP, CinP, 1 if transpose else 0, 0))
            self.max_elems = max(self.max_elems, 9 * CoutP * CinP)
            dts.add(dtype)
        assert len(dts) == 1, "one compute dtype per plan"
        self.dtype = dts.pop()
        dev = next(iter(self.req.values()))[0].device
        raw = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8)
        self.jobs = raw.to(dev)
        self.njobs = len(recs)

    def refresh(self):
        if not self.req:
            return
        if self.jobs is None:
            self._build()
        _lib.checked().wm_pack_w3x3_batch(_p(self.jobs), self.njobs, self.max_elems, dt_id(self.dtype), _stream())
        for k, req in self.req.items():
            self.ver[k] = req[0]._version
        self.valid = True


# ----------------------------------------------------------------------------- conv / bn
def conv3x3_nparts(B, H, W, Cin, CoutP, dtype):
    return _lib.checked().wm_conv3x3_nparts(B, H, W, Cin, CoutP, dt_id(dtype))


class _WmBnBwdFin(ctypes.Structure):   # include/wm_hip.h: WmBnBwdFin
    _fields_ = [("partials", ctypes.c_void_p), ("nparts", ctypes.c_int), ("C", ctypes.c_int), ("CP", ctypes.c_int), ("count", ctypes.c_double),
                ("gamma", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("invstd", ctypes.c_void_p), ("dgamma", ctypes.c_void_p),
                ("dbeta", ctypes.c_void_p), ("accumulate", ctypes.c_int), ("coef", ctypes.c_void_p)]


def fin_rider_enabled():
    return bool(_lib.checked().wm_fin_rider_enabled())


def _fin_rider(fin):
    """fin: None or dict(partials [n,2,CP], y_shape, stats [4,CP], C, gamma, dgamma, dbeta, accumulate) -- the BatchNorm-backward
    finalisation (bn_bwd_coef_raw) of ANOTHER layer, carried by this launch's slab reduction.  -> (ctypes struct or None, coef or None)"""
    if fin is None:
        return None, None
    part, stats = fin["partials"], fin["stats"]
    B, H, W, CP = fin["y_shape"]
    assert part.shape[0] <= 256 and part.shape[2] == CP and part.is_contiguous()
    coef = torch.empty(3, CP, device=part.device, dtype=torch.float32)
    st = _WmBnBwdFin(partials=part.data_ptr(), nparts=part.shape[0], C=fin["C"], CP=CP, count=float(B * H * W), gamma=fin["gamma"].data_ptr(),
                     mean=stats[2].data_ptr(), invstd=stats[3].data_ptr(), dgamma=fin["dgamma"].data_ptr(), dbeta=fin["dbeta"].data_ptr(),
                     accumulate=1 if fin["accumulate"] else 0, coef=coef.data_ptr())
    return st, coef


def _sweep(reverse):
    """sweep_reverse argument of the conv / dgrad / wgrad entry points: walk the tiles backwards (start where the producer of the
    input stopped -- its last tiles are still in the Infinity Cache)"""
    return 1 if reverse else 0


def conv3x3_fwd(x, wp, bias, in_scale, in_shift, want_stats, Cin=None, reverse=False):
    """x [B,H,W,ld]; wp [9,CoutP,Cin]; returns y [B,H,W,CoutP] and stat partials (or None)."""
    _need_cuda(x, wp)
    B, H, W, ldx = x.shape
    CoutP, CinW = wp.shape[1], wp.shape[2]
    Cin = CinW if Cin is None else Cin
    assert Cin == CinW and Cin <= ldx
    y = torch.empty(B, H, W, CoutP, device=x.device, dtype=x.dtype)
    st = torch.empty(conv3x3_nparts(B, H, W, Cin, CoutP, x.dtype), 2, CoutP, device=x.device, dtype=torch.float32) if want_stats else None
    info = {"B": B, "H": H, "W": W, "Cin": Cin, "CoutP": CoutP, "xform": in_scale is not None, "dtype": x.dtype}
    _timed("conv3x3_fwd", info, lambda: _lib.checked().wm_conv3x3_fwd(
        _p(x), ldx, _p(wp), _p(bias), 0 if bias is None else bias.numel(), _p(in_scale), _p(in_shift), _p(y), CoutP, _p(st), B, H, W, Cin, CoutP,
        dtype_id(x), _sweep(reverse), _stream()))
    return y, st


def conv3x3_fwd_addin(x, wp, in_scale, in_shift, addend, reverse=False):
    """dense 64 -> 64 forward conv (16-bit dtypes) whose epilogue adds `addend` [B,H,W,64] before the BatchNorm statistics:
    y = conv3x3(relu(in_scale*x + in_shift), wp) + addend.  Returns (y, stat partials)."""
    _need_cuda(x, wp, addend)
    B, H, W, C = x.shape
    assert C == 64 and tuple(wp.shape) == (9, 64, 64) and addend.shape == x.shape and addend.dtype == x.dtype and x.is_contiguous() and addend.is_contiguous()
    y = torch.empty_like(x)
    st = torch.empty(conv3x3_nparts(B, H, W, 64, 64, x.dtype), 2, 64, device=x.device, dtype=torch.float32)
    info = {"B": B, "H": H, "W": W, "Cin": 64, "CoutP": 64, "xform": True, "dtype": x.dtype, "addin": True}
    _timed("conv3x3_fwd", info, lambda: _lib.checked().wm_conv3x3_fwd_addin(_p(x), _p(wp), _p(in_scale), _p(in_shift), _p(addend), _p(y), _p(st), B,
                                                                            H, W, dtype_id(x), _sweep(reverse), _stream()))
    return y, st


def concat_side_fwd(img, w, bias, msg, dtype, c_msg, L, c_img):
    """P [B,H,W,64] = conv3(image channels of w) + bias + the message term (hidden_models/encoder.py:34-41 without the concat):
    img [B,3,H,W] f32, w [64,Cin,3,3] f32, msg [B,L] f32."""
    _need_cuda(img, w, msg)
    B, _, H, W = img.shape
    Cin = w.shape[1]
    assert w.shape[0] == 64 and img.shape[1] == 3 and img.dtype == torch.float32 and img.is_contiguous() and w.is_contiguous()
    msg = msg.contiguous().float()
    P = torch.empty(B, H, W, 64, device=img.device, dtype=dtype)
    wside = torch.empty(64 * 32, device=img.device, dtype=dtype)
    mbias = torch.empty(B, 9, 64, device=img.device, dtype=torch.float32)
    _lib.checked().wm_concat_side_fwd(_p(img), _p(w), _p(bias), _p(msg), _p(wside), _p(mbias), _p(P), B, H, W, Cin, c_msg, L, c_img, dt_id(dtype),
                                      _stream())
    return P


def concat_side_msg_wgrad(dy, msg, dw, accumulate, c_msg, L):
    """dw[:, c_msg + l, tap] (+)= sum_b msg[b,l] * (sum of dy[b] over the pixels for which the tap lies inside the image)"""
    B, H, W, C = dy.shape
    assert C == 64 and dy.is_contiguous() and dw.is_contiguous() and dw.shape[0] == 64
    msg = msg.contiguous().float()
    partial = torch.empty(B, _lib.checked().wm_concat_side_partial_rows(), 64, device=dy.device, dtype=torch.float32)
    S = torch.empty(B, 9, 64, device=dy.device, dtype=torch.float32)
    _lib.checked().wm_concat_side_msg_wgrad(_p(dy), _p(msg), _p(partial), _p(S), _p(dw), 1 if accumulate else 0, B, H, W, dw.shape[1], c_msg, L,
                                            dtype_id(dy), _stream())


def bn_finalize(partials, C, CP, count, gamma, beta, running_mean, running_var, momentum, eps):
    dev = partials.device
    out = torch.empty(4, CP, device=dev, dtype=torch.float32)  # scale, shift, mean, invstd
    _lib.checked().wm_bn_finalize(_p(partials), partials.shape[0], C, CP, count, _p(gamma), _p(beta), _p(running_mean), _p(running_var), momentum,
                                  eps, _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _stream())
    return out


def bn_bwd_coef(g, gvec, y, stats, C, gamma, dgamma, dbeta, accumulate):
    """first half of the ReLU+BN backward: the reduce pass + finalisation.  Writes dgamma / dbeta, returns coef [3,CP]
    (gamma*invstd, mean(gz), mean(gz*xhat)) for the apply pass."""
    B, H, W, CP = y.shape
    hw = H * W
    L = _lib.checked()
    nparts = L.wm_bn_bwd_nparts(B * hw)
    dev = y.device
    part = torch.empty(nparts, 2, CP, device=dev, dtype=torch.float32)
    ldg = 0 if g is None else g.shape[-1]
    L.wm_bn_bwd_reduce(_p(g), ldg, _p(gvec), _p(y), CP, _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(stats[3]), _p(part), B, hw, CP, dtype_id(y),
                       _stream())
    coef = torch.empty(3, CP, device=dev, dtype=torch.float32)
    L.wm_bn_bwd_finalize(_p(part), nparts, C, CP, B * hw, _p(gamma), _p(stats[3]), _p(dgamma), _p(dbeta), 1 if accumulate else 0, _p(coef),
                         _stream())
    return coef


def bn_bwd_coef_raw(partials, y, stats, C, gamma, dgamma, dbeta, accumulate):
    """bn_bwd_coef from partial rows [n,2,CP] = sum(gz), sum(gz*y) already reduced by the dgrad that produced g
    (conv3x3_dgrad_bwdstats): no pass over (g, y)."""
    B, H, W, CP = y.shape
    coef = torch.empty(3, CP, device=y.device, dtype=torch.float32)
    _lib.checked().wm_bn_bwd_finalize_raw(_p(partials), partials.shape[0], C, CP, B * H * W, _p(gamma), _p(stats[2]), _p(stats[3]), _p(dgamma),
                                          _p(dbeta), 1 if accumulate else 0, _p(coef), _stream())
    return coef


def bn_bwd(g, gvec, y, stats, C, gamma, dgamma, dbeta, accumulate, dbias, coef=None):
    """ReLU+BN backward.  g [B,H,W,ld] or None with gvec [B,CP]; y raw conv output [B,H,W,CP];
    stats = [4,CP] (scale, shift, mean, invstd).  Returns dy [B,H,W,CP]; writes dgamma/dbeta/dbias.
    coef: the result of bn_bwd_coef / bn_bwd_coef_raw when the reduce pass already ran (dgamma / dbeta written there)."""
    B, H, W, CP = y.shape
    hw = H * W
    L = _lib.checked()
    dev = y.device
    if coef is None:
        coef = bn_bwd_coef(g, gvec, y, stats, C, gamma, dgamma, dbeta, accumulate)
    nparts = L.wm_bn_bwd_nparts(B * hw)
    ldg = 0 if g is None else g.shape[-1]
    dy = torch.empty_like(y)
    bpart = torch.empty(nparts, CP, device=dev, dtype=torch.float32) if dbias is not None else None
    L.wm_bn_bwd_apply(_p(g), ldg, _p(gvec), _p(y), CP, _p(stats[0]), _p(stats[1]), _p(stats[2]), _p(stats[3]), _p(coef), _p(dy), CP, _p(bpart),
                      B, hw, CP, dtype_id(y), _stream())
    if dbias is not None:
        colsum(bpart, dbias.numel(), CP, dbias, accumulate)
    return dy


def conv3x3_wgrad_bnfused_supported(CinX, CoutY, dtype):
    return bool(_lib.checked().wm_conv3x3_wgrad_bnfused_supported(CinX, CoutY, dt_id(dtype)))


def conv3x3_wgrad_bnfused(x, g, y, stats, coef, dw, accumulate):
    """weight gradient of an image-fed first layer with the BatchNorm-backward apply pass fused: dy is formed from
    (g, y, stats [4,CP] contiguous, coef [3,CP]) while the tile is staged and never written to memory."""
    B, H, W, ldx = x.shape
    CoutY = y.shape[-1]
    L = _lib.checked()
    nbytes = L.wm_conv3x3_wgrad_ws_bytes(B, H, W, ldx, CoutY)
    ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32)
    Cout, Cin = dw.shape[0], dw.shape[1]
    assert dw.is_contiguous() and stats.is_contiguous() and coef.is_contiguous()
    L.wm_conv3x3_wgrad_bnfused(_p(x), ldx, ldx, _p(g), g.shape[-1], _p(y), CoutY, CoutY, _p(stats), _p(coef), _p(ws), _p(dw),
                               1 if accumulate else 0, B, H, W, Cin, Cout, dtype_id(x), _stream())


def conv3x3_gvfused_supported(CinX, CoutY, dtype):
    return bool(_lib.checked().wm_conv3x3_gvfused_supported(CinX, CoutY, dt_id(dtype)))


def conv3x3_wgrad_gvfused(x, in_scale, in_shift, gvec, y, stats, coef, dw, accumulate, fin=None):
    """weight gradient of a globally pooled ConvBNRelu with the BatchNorm-backward apply pass fused: dy is formed from
    (gvec [B,CP], y, stats [4,CP] contiguous, coef [3,CP]) while the tile is staged."""
    B, H, W, ldx = x.shape
    CoutY = y.shape[-1]
    L = _lib.checked()
    nbytes = L.wm_conv3x3_wgrad_ws_bytes(B, H, W, ldx, CoutY)
    ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32)
    Cout, Cin = dw.shape[0], dw.shape[1]
    assert dw.is_contiguous() and stats.is_contiguous() and coef.is_contiguous() and gvec.is_contiguous() and gvec.shape[-1] == CoutY
    fst, fcoef = _fin_rider(fin)
    L.wm_conv3x3_wgrad_gvfused_fin(_p(x), ldx, ldx, _p(in_scale), _p(in_shift), _p(gvec), _p(y), CoutY, CoutY, _p(stats), _p(coef), _p(ws),
                                   _p(dw), 1 if accumulate else 0, B, H, W, Cin, Cout, dtype_id(x),
                                   ctypes.byref(fst) if fst is not None else None, _stream())
    return fcoef


def conv3x3_dgrad_gvfused(y, wpt, gvec, stats, coef):
    """input gradient of the same layer: conv3x3 of the on-the-fly dy with the transposed packed filter wpt [9,CinP,CoutY]"""
    B, H, W, CoutY = y.shape
    CinP = wpt.shape[1]
    assert wpt.shape[2] == CoutY and stats.is_contiguous() and coef.is_contiguous() and gvec.is_contiguous()
    dx = torch.empty(B, H, W, CinP, device=y.device, dtype=y.dtype)
    _lib.checked().wm_conv3x3_dgrad_gvfused(_p(y), CoutY, CoutY, _p(wpt), _p(gvec), _p(stats), _p(coef), _p(dx), B, H, W, CinP, dtype_id(y),
                                            _stream())
    return dx


def _premasked(dx):
    """tag an input gradient whose kernel wrote gz = g * [z > 0] of the feeding layer (what the premasked staging of conv3x3_bwd_fused /
    conv3x3_bwd_fused16 expects); read by engine.is_premasked"""
    dx._wm_masked = True
    return dx


def conv3x3_dgrad_bwdstats_supported(CoutY, CinP, dtype):
    return bool(_lib.checked().wm_conv3x3_dgrad_bwdstats_supported(CoutY, CinP, dt_id(dtype)))


def conv3x3_dgrad_bwdstats(src, wpt, ry, r_scale, r_shift, gvec=None, stats=None, coef=None, reverse=False):
    """input gradient dx = conv3x3(dy, wpt) whose epilogue also reduces the BatchNorm-backward sums of the layer that feeds
    this one (raw output ry, constants r_scale / r_shift).  src = dy, or (with gvec, stats, coef) this layer's raw output
    with the apply pass fused.  Returns (dx, partials [n,2,64])."""
    B, H, W, lds = src.shape
    CinP, CoutY = wpt.shape[1], wpt.shape[2]
    assert ry.shape == (B, H, W, CinP) and ry.is_contiguous() and CoutY <= lds
    assert (gvec is None) == (stats is None) == (coef is None)
    dx = torch.empty(B, H, W, CinP, device=src.device, dtype=src.dtype)
    part = torch.empty(conv3x3_nparts(B, H, W, CoutY, CinP, src.dtype), 2, CinP, device=src.device, dtype=torch.float32)
    _lib.checked().wm_conv3x3_dgrad_bwdstats(_p(src), lds, CoutY, _p(wpt), _p(gvec), _p(stats), _p(coef), _p(ry), _p(r_scale), _p(r_shift), _p(dx),
                                             _p(part), B, H, W, CinP, dtype_id(src), _sweep(reverse), _stream())
    return _premasked(dx), part


def conv3x3_dgrad_applyfused_supported(CoutY, CinP, dtype):
    return bool(_lib.checked().wm_conv3x3_dgrad_applyfused_supported(CoutY, CinP, dt_id(dtype)))


def conv3x3_dgrad_applyfused(g, y, stats, coef, wpt, ry=None, r_scale=None, r_shift=None, reverse=False, want_dy=True):
    """64 -> 64 layer, gradient g a dense tensor: the BatchNorm-backward apply pass inside the input-gradient kernel.
    Returns (dy, dx, partials or None): dy for the weight gradient, dx = conv3x3(dy, wpt), partials = the feeding layer's
    BatchNorm-backward sums when its raw output ry (+ r_scale, r_shift) is given."""
    B, H, W, C = y.shape
    CinP = wpt.shape[1]
    assert C == 64 and g.shape == y.shape and g.is_contiguous() and y.is_contiguous() and tuple(wpt.shape) == (9, CinP, 64) and CinP in (64, 32)
    assert stats.is_contiguous() and coef.is_contiguous() and (ry is None or (CinP == 64 and ry.shape == y.shape and ry.is_contiguous()))
    dy = torch.empty_like(y) if want_dy else None     # want_dy False: the input gradient alone (no weight gradient will read dy)
    dx = torch.empty(B, H, W, CinP, device=y.device, dtype=y.dtype)
    part = torch.empty(conv3x3_nparts(B, H, W, 64, 64, y.dtype), 2, 64, device=y.device, dtype=torch.float32) if ry is not None else None
    info = {"B": B, "H": H, "W": W, "feed": ry is not None, "dtype": y.dtype}
    _timed("conv3x3_dgrad_applyfused", info, lambda: _lib.checked().wm_conv3x3_dgrad_applyfused(
        _p(g), _p(y), _p(stats), _p(coef), _p(wpt), _p(dy), _p(dx), _p(ry), _p(r_scale), _p(r_shift), _p(part), B, H, W, CinP, dtype_id(y),
        _sweep(reverse), _stream()))
    return dy, _premasked(dx) if ry is not None else dx, part


def conv3x3_bwd_fused_supported(dtype, shape=None):
    """the one-kernel backward exists for this dtype (and, given y's shape [B,H,W,64], the tensor fits its 32-bit offsets)"""
    if shape is None:
        return bool(_lib.checked().wm_conv3x3_bwd_fused_supported(dt_id(dtype)))
    return bool(_lib.checked().wm_conv3x3_bwd_fused_supported_shape(shape[0], shape[1], shape[2], dt_id(dtype)))


def conv3x3_bwd_fused_gvec_max_batch():
    return int(_lib.checked().wm_conv3x3_bwd_fused_gvec_max_batch())


def conv3x3_bwd_fused(g, y, stats, coef, wpt, xr, in_scale, in_shift, dw, accumulate, reverse=False, fin=None, premasked=False, gvec=None):
    """The whole backward of a 64 -> 64 body layer fed by another ConvBNRelu in one pass (csrc/bwd_ws.hip): returns
    (dx -- multiplied by the feeding layer's ReLU mask --, partials [nwg,2,64] = the feeding layer's BatchNorm-backward sums, the
    rider's coef or None); dw is written in place by the slab reduction that follows the kernel.  gvec [B,64] f32 instead of g: the
    layer's output was globally pooled (one gradient row per sample)."""
    B, H, W, C = y.shape
    if (g is None) == (gvec is None):
        raise RuntimeError("conv3x3_bwd_fused: exactly one of g (a tensor) and gvec (one row per sample) is given")
    assert C == 64 and xr.shape == y.shape and y.is_contiguous() and xr.is_contiguous()
    assert (g.shape == y.shape and g.is_contiguous()) if g is not None else (tuple(gvec.shape) == (B, 64) and gvec.is_contiguous() and gvec.dtype == torch.float32)
    assert tuple(wpt.shape) == (9, 64, 64) and stats.is_contiguous() and coef.is_contiguous() and dw.is_contiguous()
    L = _lib.checked()
    nwg = L.wm_conv3x3_bwd_fused_nwg(B, H, W)
    dx = torch.empty_like(y)
    part = torch.empty(nwg, 2, 64, device=y.device, dtype=torch.float32)
    fst, fcoef = _fin_rider(fin(part) if callable(fin) else fin)     # fin: a rider dict, or a function of the partial rows this call produces
    ws = torch.empty(nwg * 9 * 64 * 64, device=y.device, dtype=torch.float32)
    Cout, Cin = dw.shape[0], dw.shape[1]
    info = {"B": B, "H": H, "W": W, "dtype": y.dtype, "gvec": gvec is not None}
    _timed("conv3x3_bwd_fused", info, lambda: L.wm_conv3x3_bwd_fused(
        _p(g), _p(gvec), _p(y), _p(stats), _p(coef), _p(wpt), _p(xr), _p(in_scale), _p(in_shift), _p(dx), _p(part), _p(ws), B, H, W, dtype_id(y),
        1 if premasked else 0, _sweep(reverse), _stream()))
    L.wm_conv3x3_bwd_fused_reduce(_p(ws), _p(dw), 1 if accumulate else 0, B, H, W, Cin, Cout, ctypes.byref(fst) if fst is not None else None,
                                  _stream())
    return _premasked(dx), part, fcoef


def conv3x3_bwd_fused16_supported(shape, dtype):
    """the one-kernel backward of an image-fed first layer exists for y's shape [B,H,W,64] (whole 8x16 tiles) and dtype"""
    return bool(_lib.checked().wm_conv3x3_bwd_fused16_supported(shape[0], shape[1], shape[2], dt_id(dtype)))


def conv3x3_bwd_fused16(g, y, stats, coef, wpt, x, dw, accumulate, reverse=False, premasked=False):
    """The whole backward of an image-fed first ConvBNRelu in one pass (csrc/bwd_ws16.hip): returns dx [B,H,W,16] (gradient wrt the 16-channel
    image tensor x); dw [Cout,Cin<=16,3,3] is written in place by the slab reduction that follows the kernel."""
    B, H, W, C = y.shape
    assert C == 64 and g.shape == y.shape and g.is_contiguous() and y.is_contiguous() and tuple(x.shape) == (B, H, W, 16) and x.is_contiguous()
    assert tuple(wpt.shape) == (9, 16, 64) and stats.is_contiguous() and coef.is_contiguous() and dw.is_contiguous() and dw.shape[0] <= 64 and dw.shape[1] <= 16
    L = _lib.checked()
    nwg = L.wm_conv3x3_bwd_fused16_nwg(B, H, W)
    dx = torch.empty(B, H, W, 16, device=y.device, dtype=y.dtype)
    ws = torch.empty(nwg * 9 * 16 * 64, device=y.device, dtype=torch.float32)
    info = {"B": B, "H": H, "W": W, "dtype": y.dtype}
    _timed("conv3x3_bwd_fused16", info, lambda: L.wm_conv3x3_bwd_fused16(
        _p(g), _p(y), _p(stats), _p(coef), _p(wpt), _p(x), _p(dx), _p(ws), _p(dw), 1 if accumulate else 0, B, H, W, dw.shape[1], dw.shape[0],
        dtype_id(y), 1 if premasked else 0, _sweep(reverse), _stream()))
    return dx


def linear_head_fwd(pooled, w, bias, I):
    """pooled [B,ldp] f32 (first I columns used), w [O,I], bias [O] -> [B,O]"""
    _need_cuda(pooled, w)
    B, ldp = pooled.shape
    O = w.shape[0]
    out = torch.empty(B, O, device=pooled.device, dtype=torch.float32)
    _lib.checked().wm_linear_head_fwd(_p(pooled), ldp, _p(w), _p(bias), _p(out), B, I, O, _stream())
    return out


def linear_head_bwd(pooled, w, g_out, dw, db, accumulate, CP, inv_hw):
    """writes dw [O,I], db [O]; returns gvec [B,CP] = (g_out @ w) * inv_hw (zero padded)"""
    _need_cuda(pooled, w, g_out)
    B, ldp = pooled.shape
    O, I = w.shape
    g = g_out.contiguous().float()
    gvec = torch.empty(B, CP, device=pooled.device, dtype=torch.float32)
    _lib.checked().wm_linear_head_bwd(_p(pooled), ldp, _p(w), _p(g), _p(dw), _p(db), 1 if accumulate else 0, _p(gvec), CP, inv_hw, B, I, O,
                                      _stream())
    return gvec


def pooled_head_supported(B, CP, I, O):
    return bool(_lib.checked().wm_pooled_head_supported(B, CP, I, O))


def pooled_head(out3, I, w, bias, kind, target, messages, gscale, gscale_dev, dw, db, accumulate, inv_hw, C, count, gamma, stats, dgamma, dbeta):
    """linear_head_fwd + the loss (kind 0: bce_logits vs the constant `target`; kind 1: message_loss vs messages [B,O]) + linear_head_bwd +
    bn_bwd_coef_pooled as ONE launch.  out3 [3,B,CP] = bnrelu_avgpool_stats' buffer (pooled, N+, S+); stats [4,CP] of the pooled
    ConvBNRelu.  -> (logits [B,O], loss [1] or [2], gvec [B,CP], coef [3,CP]); dw, db, dgamma, dbeta written in place."""
    _, B, CP = out3.shape
    O = w.shape[0]
    assert out3.is_contiguous() and out3.dtype == torch.float32 and tuple(w.shape) == (O, I) and w.is_contiguous() and dw.is_contiguous()
    dev = out3.device
    logits = torch.empty(B, O, device=dev, dtype=torch.float32)
    loss = torch.empty(2 if kind == 1 else 1, device=dev, dtype=torch.float32)
    gvec = torch.empty(B, CP, device=dev, dtype=torch.float32)
    coef = torch.empty(3, CP, device=dev, dtype=torch.float32)
    msg = messages.contiguous().float() if messages is not None else None
    _lib.checked().wm_pooled_head(_p(out3), B, CP, I, O, _p(w), _p(bias), kind, float(target), _p(msg), float(gscale), _p(gscale_dev), _p(logits),
                                  _p(loss), _p(dw), _p(db), 1 if accumulate else 0, _p(gvec), inv_hw, C, float(count), _p(gamma), _p(stats[2]),
                                  _p(stats[3]), _p(dgamma), _p(dbeta), _p(coef), _stream())
    return logits, loss, gvec, coef


def bce_logits(logits, target, gscale=1.0, want_grad=True, gscale_dev=None):
    """BCEWithLogitsLoss(mean) against a constant label: (loss [1] tensor, gscale * d loss / d logits or None).
    gscale_dev (here and in the other loss ops): optional device scalar multiplied into gscale (the AMP loss scale)."""
    _need_cuda(logits)
    x = logits.contiguous().float()
    loss = torch.empty(1, device=x.device, dtype=torch.float32)
    grad = torch.empty_like(x) if want_grad else None
    _lib.checked().wm_bce_logits(_p(x), float(target), x.numel(), float(gscale), _p(gscale_dev), _p(loss), _p(grad), _stream())
    return loss, grad


def message_loss(decoded, messages, gscale, want_grad=True, gscale_dev=None):
    """(out [2] = [mean squared error, bitwise error], gscale * (decoded - messages) or None)."""
    _need_cuda(decoded, messages)
    d = decoded.contiguous().float(); m = messages.contiguous().float()
    out = torch.empty(2, device=d.device, dtype=torch.float32)
    grad = torch.empty_like(d) if want_grad else None
    _lib.checked().wm_message_loss(_p(d), _p(m), d.numel(), float(gscale), _p(gscale_dev), _p(out), _p(grad), _stream())
    return out, grad


def hidden_metrics(enc_partials, n_img, msg2, adv, d_cover, d_enc, w_adv, w_enc, w_dec):
    """[7] f32: loss, encoder mse, decoder mse, bitwise error, adversarial bce, D(cover) bce, D(encoded) bce (one launch)"""
    out = torch.empty(7, device=enc_partials.device, dtype=torch.float32)
    _lib.checked().wm_hidden_metrics(_p(enc_partials), enc_partials.numel(), float(n_img), _p(msg2), _p(adv), _p(d_cover), _p(d_enc), w_adv, w_enc,
                                     w_dec, _p(out), _stream())
    return out


def colsum(partials, C, ldp, out, accumulate):
    _lib.checked().wm_colsum_finalize(_p(partials), partials.shape[0], C, ldp, _p(out), 1 if accumulate else 0, _stream())


def conv3x3_wgrad(x, CinX, in_scale, in_shift, dy, dw, accumulate, perm_dev=None, reverse=False, fin=None):
    """dw [Cout,Cin,3,3] f32 view (written in place).  fin: see _fin_rider; then the rider's coef [3,CP] is returned."""
    fst, fcoef = _fin_rider(fin)
    B, H, W, ldx = x.shape
    CoutY = dy.shape[-1]
    L = _lib.checked()
    nbytes = L.wm_conv3x3_wgrad_ws_bytes(B, H, W, CinX, CoutY)
    ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32)
    Cout, Cin = dw.shape[0], dw.shape[1]
    assert dw.is_contiguous()
    L.wm_conv3x3_wgrad_fin(_p(x), ldx, CinX, _p(in_scale), _p(in_shift), _p(dy), CoutY, CoutY, _p(ws), _p(dw), 1 if accumulate else 0, B, H, W,
                           Cin, Cout, _p(perm_dev), dtype_id(x), ctypes.byref(fst) if fst is not None else None, _sweep(reverse), _stream())
    return fcoef


def conv3x3_fwd_elu_supported(Cin, CoutP, dtype):
    return bool(_lib.checked().wm_conv3x3_fwd_elu_supported(Cin, CoutP, dt_id(dtype)))


def conv3x3_fwd_elu(x, wp, bias):
    """out [B,H,W,64] = elu(conv3x3(x, wp) + bias) in one launch (16-bit dtypes; the pre-activation is not stored)"""
    _need_cuda(x, wp)
    B, H, W, ldx = x.shape
    Cin = wp.shape[2]
    assert wp.shape[1] == 64 and Cin <= ldx
    out = torch.empty(B, H, W, 64, device=x.device, dtype=x.dtype)
    _lib.checked().wm_conv3x3_fwd_elu(_p(x), ldx, _p(wp), _p(bias), 0 if bias is None else bias.numel(), _p(out), B, H, W, Cin, dtype_id(x), 0,
                                      _stream())
    return out


def conv3x3_dgrad_elufused_supported(CinP, dtype):
    return bool(_lib.checked().wm_conv3x3_dgrad_elufused_supported(CinP, dt_id(dtype)))


def conv3x3_dgrad_elufused(g, out, wpt, want_gz=True, dx_stride=None):
    """backward of a conv + ELU layer, input-gradient half: gz = g * (out > 0 ? 1 : out + 1) formed while staging; returns
    (dx [B,H,W,CinP], gz [B,H,W,64] or None, bias_partials f32 [nparts,64]).  dx_stride = 16: wpt packed to 32 rows (upper 16 zero),
    dx [B,H,W,16]"""
    _need_cuda(g, out, wpt)
    B, H, W, C = g.shape
    CinP = wpt.shape[1] if dx_stride is None else dx_stride
    assert C == 64 and out.shape == g.shape and out.dtype == g.dtype and g.is_contiguous() and out.is_contiguous() and wpt.shape[2] == 64
    assert CinP == wpt.shape[1] or (CinP == 16 and wpt.shape[1] == 32)
    L = _lib.checked()
    dx = torch.empty(B, H, W, CinP, device=g.device, dtype=g.dtype)
    gz = torch.empty_like(g) if want_gz else None
    part = torch.empty(L.wm_conv3x3_dgrad_elufused_nparts(B, H, W), 64, device=g.device, dtype=torch.float32)
    L.wm_conv3x3_dgrad_elufused(_p(g), _p(out), _p(wpt), _p(dx), _p(gz), _p(part), B, H, W, CinP, dtype_id(g), 0, _stream())
    return dx, gz, part


def conv3x3_wgrad_bias(x, gz, dw, accumulate, bias_partials, db, db_accumulate):
    """dw [Cout,Cin,3,3] (+)= the weight gradient from (x, gz); db [Cout] (+)= the column sums of bias_partials, in the same reduction launch"""
    B, H, W, ldx = x.shape
    CoutY = gz.shape[-1]
    L = _lib.checked()
    ws = torch.empty(L.wm_conv3x3_wgrad_ws_bytes(B, H, W, ldx, CoutY) // 4, device=x.device, dtype=torch.float32)
    Cout, Cin = dw.shape[0], dw.shape[1]
    assert dw.is_contiguous() and db.is_contiguous() and db.numel() == Cout and bias_partials.is_contiguous() and bias_partials.shape[1] == CoutY
    L.wm_conv3x3_wgrad_bias(_p(x), ldx, ldx, _p(gz), CoutY, CoutY, _p(ws), _p(dw), 1 if accumulate else 0, B, H, W, Cin, Cout, dtype_id(x),
                            _p(bias_partials), bias_partials.shape[0], _p(db), 1 if db_accumulate else 0, _stream())


# ----------------------------------------------------------------------------- heads
def bnrelu_avgpool_stats(y, scale, shift):
    """global average pool of relu(scale*y+shift) plus, per (sample, channel), the active-pixel count N+ and the sum S+ of y over
    the active pixels.  Returns (pooled [B,CP], (N+ [B,CP], S+ [B,CP]))."""
    B, H, W, CP = y.shape
    L = _lib.checked()
    S = L.wm_avgpool_slices(H * W)
    ws = torch.empty(B * S * 3 * CP, device=y.device, dtype=torch.float32)
    out3 = torch.empty(3, B, CP, device=y.device, dtype=torch.float32)
    L.wm_bnrelu_avgpool_stats(_p(y), CP, _p(scale), _p(shift), _p(out3), _p(ws), B, H * W, CP, dtype_id(y), _stream())
    return out3[0], (out3[1], out3[2])


def pooled_bwd_rows(gvec, pool_stats):
    """partial rows [B,2,CP] = (gvec*N+, gvec*S+) for bn_bwd_coef_raw: the pooled layer's BatchNorm-backward sums without a pass over y"""
    B, CP = gvec.shape
    npos, ysum = pool_stats
    assert gvec.is_contiguous() and npos.is_contiguous() and ysum.is_contiguous() and npos.shape == gvec.shape
    rows = torch.empty(B, 2, CP, device=gvec.device, dtype=torch.float32)
    _lib.checked().wm_pooled_bn_bwd_rows(_p(gvec), _p(npos), _p(ysum), B, CP, _p(rows), _stream())
    return rows


def bn_bwd_coef_pooled(gvec, pool_stats, y, stats, C, gamma, dgamma, dbeta, accumulate):
    """bn_bwd_coef of a globally pooled layer from the forward pool's (N+, S+): one small launch, no pass over y"""
    B, H, W, CP = y.shape
    npos, ysum = pool_stats
    assert gvec.is_contiguous() and npos.is_contiguous() and ysum.is_contiguous() and tuple(gvec.shape) == (B, CP) == tuple(npos.shape)
    coef = torch.empty(3, CP, device=y.device, dtype=torch.float32)
    _lib.checked().wm_bn_bwd_finalize_pooled(_p(gvec), _p(npos), _p(ysum), B, C, CP, B * H * W, _p(gamma), _p(stats[2]), _p(stats[3]), _p(dgamma),
                                             _p(dbeta), 1 if accumulate else 0, _p(coef), _stream())
    return coef


def bnrelu_avgpool(y, scale, shift):
    B, H, W, CP = y.shape
    L = _lib.checked()
    S = L.wm_avgpool_slices(H * W)
    ws = torch.empty(B * S * CP, device=y.device, dtype=torch.float32)
    out = torch.empty(B, CP, device=y.device, dtype=torch.float32)
    L.wm_bnrelu_avgpool(_p(y), CP, _p(scale), _p(shift), _p(out), _p(ws), B, H * W, CP, dtype_id(y), _stream())
    return out


def conv1x1_head_fwd(y, scale, shift, w, bias, act=0, want_act16=False):
    """y [B,H,W,Cin]; w [Cout,Cin(,1,1)] f32; -> out [B,Cout,H,W] f32; want_act16: -> (out, the same image as the [B,H,W,16] zero-padded
    NHWC tensor of y's dtype that the image-fed first layers read: engine.image_to_act's result without its launch)"""
    B, H, W, Cin = y.shape
    Cout = w.shape[0]
    out = torch.empty(B, Cout, H, W, device=y.device, dtype=torch.float32)
    a16 = torch.empty(B, H, W, 16, device=y.device, dtype=y.dtype) if want_act16 else None
    _lib.checked().wm_conv1x1_head_fwd_act(_p(y), Cin, _p(scale), _p(shift), _p(w), _p(bias), _p(out), _p(a16), B, H * W, Cin, Cout, act,
                                           dtype_id(y), _stream())
    return (out, a16) if want_act16 else out


def conv1x1_head_bwd(y, scale, shift, w, gout, dw, dbias, accumulate, want_bn_partials=False):
    """-> g (gradient wrt the ReLU output feeding the head); with want_bn_partials: (g, rows [n,2,Cin] of sum(gz), sum(gz*y) of the
    ConvBNRelu that produced y, for bn_bwd_coef_raw: that layer then needs no reduce pass over (g, y))"""
    B, H, W, Cin = y.shape
    Cout = w.shape[0]
    L = _lib.checked()
    nparts = L.wm_conv1x1_head_nparts(B * H * W)
    part = torch.empty(nparts, Cout * (Cin + 1), device=y.device, dtype=torch.float32)
    bnp = torch.empty(nparts, 2, Cin, device=y.device, dtype=torch.float32) if want_bn_partials and scale is not None else None
    g = torch.empty_like(y)
    gout = gout.contiguous()
    L.wm_conv1x1_head_bwd(_p(y), Cin, _p(scale), _p(shift), _p(w), _p(gout), _p(g), Cin, _p(part), _p(bnp), B, H * W, Cin, Cout, dtype_id(y),
                          _stream())
    ldp = Cout * (Cin + 1)
    colsum(part, Cout * Cin, ldp, dw, accumulate)
    # the first call folded the rows in place to <= 64 (wm_colsum_finalize treats partials as scratch)
    colsum(part[:(nparts if nparts <= 256 else 64), Cout * Cin:], Cout, ldp, dbias, accumulate)
    if want_bn_partials:
        return g, bnp
    return g


def _head2_args(name, a, na, b, nb, w, bias):
    _need_cuda(a, b, w, bias)
    if (a.dim() != 4 or b.dim() != 4 or a.shape[:3] != b.shape[:3] or a.dtype != b.dtype or not a.is_contiguous() or not b.is_contiguous()
            or not 0 < na <= a.shape[3] or not 0 < nb <= b.shape[3]):
        raise ValueError(f"{name}: a and b must be contiguous NHWC tensors of one dtype over the same pixels with 0 < na, nb <= their channel "
                         f"strides, got {tuple(a.shape)} {a.dtype} / {tuple(b.shape)} {b.dtype}, na = {na}, nb = {nb}")
    Cout = w.shape[0]
    if w.dtype != torch.float32 or not w.is_contiguous() or w.numel() != Cout * (na + nb) or not 1 <= Cout <= 4:
        raise ValueError(f"{name}: w must be contiguous f32 [Cout <= 4, {na + nb}(,1,1)], got {tuple(w.shape)} {w.dtype}")
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() != Cout):
        raise ValueError(f"{name}: bias must be contiguous f32 [{Cout}]")
    return Cout


def head2_fwd(a, na, b, nb, w, bias, act=0):
    """act(conv1x1(cat(a[..., :na], b[..., :nb]), w, bias)) as NCHW f32 [B,Cout,H,W], read from the two NHWC sources in place (wm_head2_fwd);
    w [Cout, na+nb(,1,1)] f32, Cout <= 4; act 0 none, 1 sigmoid"""
    Cout = _head2_args("head2_fwd", a, na, b, nb, w, bias)
    B, H, W, lda = a.shape
    out = torch.empty(B, Cout, H, W, device=a.device, dtype=torch.float32)
    _lib.checked().wm_head2_fwd(_p(a), lda, na, _p(b), b.shape[3], nb, _p(w), _p(bias), _p(out), B, H * W, Cout, int(act), dtype_id(a), _stream())
    return out


def head2_bwd(a, na, b, nb, w, gout, out=None, dw_acc=None, db_acc=None):
    """-> (ga, gb, dw [Cout, na+nb], dbias [Cout]) of head2_fwd for gout f32 [B,Cout,H,W].  out: the saved forward result of act = 1 -- gout is
    then the gradient wrt the sigmoid output; None: gout is the gradient wrt the logits.  dw_acc AND db_acc: contiguous f32 tensors the two
    parameter gradients are ADDED to (the old values join the double sum before its one rounding)"""
    Cout = _head2_args("head2_bwd", a, na, b, nb, w, None)
    B, H, W, lda = a.shape
    _need_cuda(gout, out)
    if gout.dtype != torch.float32 or tuple(gout.shape) != (B, Cout, H, W) or (out is not None and (out.dtype != torch.float32 or out.shape != gout.shape)):
        raise ValueError(f"head2_bwd: gout (and out) must be f32 [{B},{Cout},{H},{W}], got {tuple(gout.shape)} {gout.dtype}")
    if (dw_acc is None) != (db_acc is None):
        raise ValueError("head2_bwd: dw_acc and db_acc come together")
    acc = dw_acc is not None
    if acc and (not dw_acc.is_contiguous() or dw_acc.numel() != Cout * (na + nb) or dw_acc.dtype != torch.float32
                or not db_acc.is_contiguous() or db_acc.numel() != Cout or db_acc.dtype != torch.float32):
        raise ValueError("head2_bwd: accumulation targets do not match the gradients")
    gout = gout.contiguous()
    out = out.contiguous() if out is not None else None
    L = _lib.checked()
    nparts = L.wm_head2_nparts(B * H * W)
    part = torch.empty(nparts, Cout * (na + nb + 1), device=a.device, dtype=torch.float64)
    ga, gb = torch.empty_like(a), torch.empty_like(b)
    L.wm_head2_bwd(_p(a), lda, na, _p(b), b.shape[3], nb, _p(w), _p(gout), _p(out), 0 if out is None else 1, _p(ga), lda, _p(gb), b.shape[3],
                   _p(part), B, H * W, Cout, dtype_id(a), _stream())
    dw = dw_acc if acc else torch.empty(Cout, na + nb, device=a.device, dtype=torch.float32)
    db = db_acc if acc else torch.empty(Cout, device=a.device, dtype=torch.float32)
    L.wm_head2_finalize(_p(part), nparts, Cout, na + nb, _p(dw), _p(db), 1 if acc else 0, _stream())
    return ga, gb, dw, db


# ----------------------------------------------------------------------------- losses / optimiser
def mse_fwd_bwd(a, b, gscale, want_grad=True, gscale_dev=None):
    """returns (sum of squared differences partials [nparts], grad = gscale*(a-b))"""
    a = a.contiguous(); b = b.contiguous()
    n = a.numel()
    nparts = max(1, min(1024, (n + 4095) // 4096))
    part = torch.empty(nparts, device=a.device, dtype=torch.float32)
    grad = torch.empty_like(a) if want_grad else None
    _lib.checked().wm_mse_fwd_bwd(_p(a), _p(b), _p(grad), gscale, _p(gscale_dev), _p(part), nparts, n, _stream())
    return part, grad


def image_grad_mse(g, a, b, gscale, C=3, C_off=0, gscale_dev=None):
    """(out [B,C,H,W] f32 = nhwc_to_nchw(g)[:, :C] + gscale * (a - b), partials of sum (a - b)^2): the discriminator's input gradient, the
    image-fidelity term's gradient and its loss in one pass (nhwc_to_nchw + mse_fwd_bwd + axpy_ before)"""
    _need_cuda(g, a, b)
    B, H, W, ld = g.shape
    assert a.shape == (B, C, H, W) and b.shape == a.shape and a.dtype == torch.float32 and b.dtype == torch.float32 and g.is_contiguous()
    a = a.contiguous(); b = b.contiguous()
    n = a.numel()
    nparts = max(1, min(1024, (n + 4095) // 4096))
    out = torch.empty_like(a)
    part = torch.empty(nparts, device=a.device, dtype=torch.float32)
    _lib.checked().wm_image_grad_mse(_p(g), ld, C_off, _p(a), _p(b), _p(out), gscale, _p(gscale_dev), _p(part), nparts, B, C, H, W, dtype_id(g),
                                     _stream())
    return out, part


def axpy_(a, b, s=1.0):
    assert a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel()
    _lib.checked().wm_axpy(_p(a), _p(b), s, a.numel(), _stream())
    _wrote(a)
    return a


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, decoupled=False, grad_scale=1.0):
    _lib.checked().wm_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, 1 if decoupled else 0, step, grad_scale,
                                _stream())
    _wrote(p, m, v)


ADAM_HYPER = 8   # WM_ADAM_HYPER


def adam_hyper(lr, beta1, beta2, step, eps, weight_decay):
    """the WM_ADAM_HYPER floats a replayed step reads (host arithmetic, no launch): (lr / (1 - beta1^step), sqrt(1 - beta2^step), lr, beta1,
    beta2, eps, weight_decay, 0) -- the first two exactly as wm_adam_step derives them, the rest rounded to f32 as its arguments are"""
    out = (ctypes.c_float * ADAM_HYPER)()
    _lib.checked().wm_adam_hyper(lr, beta1, beta2, eps, weight_decay, step, out)
    return tuple(float(x) for x in out)


def adam_step_dev(p, g, m, v, hyper_dev, decoupled=False, grad_scale=1.0):
    """adam_step with every number but `decoupled` read from the device tensor hyper_dev [ADAM_HYPER] f32 (adam_hyper's block): what a
    captured step launches -- the caller refreshes hyper_dev before each replay"""
    assert hyper_dev.is_cuda and hyper_dev.dtype == torch.float32 and hyper_dev.numel() >= ADAM_HYPER and hyper_dev.is_contiguous()
    _lib.checked().wm_adam_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), 1 if decoupled else 0, _p(hyper_dev), grad_scale, _stream())
    _wrote(p, m, v)


class AmpState:
    """torch.cuda.amp.GradScaler (IRNcrop_model.py:143,407-416) with its state on the device: see include/wm_hip.h (wm_amp_*).
    `scale` is the device scalar the loss kernels multiply their gradient seeds by."""
    N = 16

    def __init__(self, device, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        st = torch.zeros(self.N, dtype=torch.float32)
        st[0], st[2], st[3], st[4] = init_scale, growth_factor, backoff_factor, growth_interval
        self.state = st.to(device)
        self.scale = self.state[0:1]
        self.nopt = 0

    def slot(self):
        """index of a new optimiser under this scaler (<= 4)"""
        k = self.nopt
        if k >= 4:
            raise ValueError("at most four optimisers per scaler")
        self.nopt += 1
        return k

    def found_inf(self, k, grads):
        """found_inf[k]: does any of optimiser k's flat gradient buffers hold an inf / nan (GradScaler's per-element check)"""
        parts = [nonfinite(g) for g in grads]
        arr = (ctypes.c_void_p * len(parts))(*[p.data_ptr() for p in parts])
        ns = (ctypes.c_int * len(parts))(*[p.numel() for p in parts])
        _lib.checked().wm_amp_found_inf(arr, ns, len(parts), _p(self.state), k, _stream())

    def update(self):
        _lib.checked().wm_amp_update(_p(self.state), max(1, self.nopt), _stream())

    def get_scale(self):
        return float(self.state[0].item())

    def step_count(self, k):
        return int(self.state[12 + k].item())

    def set_step_count(self, k, n):
        """restore optimiser k's step count (the t of Adam's bias correction under the scaler lives on the device, not on the host)"""
        self.state[12 + k] = float(n)

    def state_dict(self):
        """torch.amp.GradScaler.state_dict()'s keys (scale, growth_factor, backoff_factor, growth_interval, _growth_tracker)"""
        st = self.state.detach().cpu()
        return {"scale": float(st[0]), "growth_factor": float(st[2]), "backoff_factor": float(st[3]), "growth_interval": int(st[4]),
                "_growth_tracker": int(st[1])}

    def load_state_dict(self, sd):
        st = self.state.detach().cpu()
        st[0], st[1], st[2], st[3], st[4] = float(sd["scale"]), float(sd.get("_growth_tracker", 0)), float(sd["growth_factor"]), \
            float(sd["backoff_factor"]), float(sd["growth_interval"])
        st[8:12] = 0.0
        self.state.copy_(st)


def adam_step_amp(p, g, m, v, lr, beta1, beta2, eps, weight_decay, amp, k, decoupled=False, grad_scale=1.0, hyper_dev=None):
    """the step under the device scaler; hyper_dev (a captured step): adam_hyper's block on the device, whose lr, betas, eps and weight_decay
    replace the arguments at each replay"""
    if hyper_dev is not None:
        assert hyper_dev.is_cuda and hyper_dev.dtype == torch.float32 and hyper_dev.numel() >= ADAM_HYPER and hyper_dev.is_contiguous()
    _lib.checked().wm_adam_step_amp(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, 1 if decoupled else 0, grad_scale,
                                    _p(amp.state), k, _p(hyper_dev), _stream())
    _wrote(p, m, v)


def sumsq(x):
    n = x.numel()
    nparts = max(1, min(1024, (n + 4095) // 4096))
    part = torch.empty(nparts, device=x.device, dtype=torch.float32)
    _lib.checked().wm_sumsq(_p(x), n, _p(part), nparts, _stream())
    return part


def nonfinite(x):
    """per-block flags (1.0: the block saw an inf / nan in x) -- the rows AmpState.found_inf reduces"""
    n = x.numel()
    nparts = max(1, min(1024, (n + 4095) // 4096))
    part = torch.empty(nparts, device=x.device, dtype=torch.float32)
    _lib.checked().wm_nonfinite(_p(x), n, _p(part), nparts, _stream())
    return part


# ----------------------------------------------------------------------------- tamper-localisation branch
def clamp_quant(x):
    """round(255*clamp(x,0,1))/255: clamp_with_grad + Quantization (IRNcrop_model.py:320-322,344-345,372-373); backward = identity"""
    _need_cuda(x)
    x = x.contiguous().float()
    y = torch.empty_like(x)
    _lib.checked().wm_clamp_quant_fwd(_p(x), _p(y), x.numel(), _stream())
    return y


MIX_MAX_K = 8


def _mix_args(name, ts, w, K):
    """the checks shared by mix_fwd / mix_bwd: `ts` f32 tensors [N, ...] of one shape, w [N, K] f32, 1 <= K <= 8 (ValueError), all on the GPU
    (RuntimeError: there is no CPU path) -> (contiguous ts, contiguous w, N, frame)"""
    if not 1 <= K <= MIX_MAX_K:
        raise ValueError(f"{name}: K = {K} inputs (1..{MIX_MAX_K})")
    t0 = ts[0]
    if t0.dim() < 1 or t0.numel() == 0:
        raise ValueError(f"{name}: tensors must be [N, ...] and not empty, got {tuple(t0.shape)}")
    for t in ts:
        if t.shape != t0.shape:
            raise ValueError(f"{name}: tensors of different shapes {tuple(t.shape)} and {tuple(t0.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: float32 tensors only, got {t.dtype}")
    N = t0.shape[0]
    if tuple(w.shape) != (N, K) or w.dtype != torch.float32:
        raise ValueError(f"{name}: weights must be float32 [{N}, {K}], got {w.dtype} {tuple(w.shape)}")
    for t in list(ts) + [w]:
        if not t.is_cuda:
            raise RuntimeError(f"{name} runs on the HIP path only: move the tensors to cuda")
    return [t.contiguous() for t in ts], w.contiguous(), N, t0.numel() // N


def mix_fwd(xs, w, quant=False):
    """y[n] = sum_k w[n, k] * xs[k][n] per frame n, accumulated with fma in the order k = 0..K-1 from 0 (IRNcrop_model.py:347-371, the hybrid
    attack mix); quant: then clamp_quant, in the same launch.  xs: 1..8 f32 tensors [N, ...] of one shape; w [N, K] f32, used as given."""
    xs = list(xs)
    xs, w, N, frame = _mix_args("mix_fwd", xs, w, len(xs))
    y = torch.empty_like(xs[0])
    ptrs = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    _lib.checked().wm_mix_fwd(ptrs, len(xs), _p(w), _p(y), N, frame, 1 if quant else 0, _stream())
    return y


def mix_bwd(g, w, K, needs=None, out=None):
    """the mix's backward in one launch: [w[:, k] * g per frame for k < K], None where needs[k] is false (that input's gradient is not
    stored).  out: K tensors like g to write into instead of fresh ones (a slot whose needs[k] is false is left untouched)."""
    needs = [True] * K if needs is None else [bool(v) for v in needs]
    if len(needs) != K or (out is not None and len(out) != K):
        raise ValueError(f"mix_bwd: needs / out must have K = {K} entries")
    outs_in = [o for o, nd in zip(out, needs) if nd] if out is not None else []
    for o in outs_in:
        if not o.is_contiguous():
            raise ValueError("mix_bwd: out tensors must be contiguous")
    ts, w, N, frame = _mix_args("mix_bwd", [g] + outs_in, w, K)
    g = ts[0]
    gxs = [(out[k] if out is not None else torch.empty_like(g)) if needs[k] else None for k in range(K)]
    ptrs = (ctypes.c_void_p * K)(*[_p(t) for t in gxs])
    _lib.checked().wm_mix_bwd(_p(g), _p(w), ptrs, K, N, frame, _stream())
    _wrote(*outs_in)
    return gxs


def splice_fwd(enc, real=None, prev=None, mask=None, want_fwd=False):
    """q = clamp_quant(enc); tampered = q*(1-mask) + prev*mask (IRNcrop_model.py:344-348); with `real`, also the partial sums of
    the squared difference of the int-truncated images for the PSNR.  Returns (fwd_q or None, tampered or None, psnr partials or None)."""
    _need_cuda(enc)
    enc = enc.contiguous()
    B, C, H, W = enc.shape
    L = _lib.checked()
    fwd = torch.empty_like(enc) if want_fwd else None
    tam = torch.empty_like(enc) if prev is not None else None
    part = None
    if real is not None:
        part = torch.empty(L.wm_splice_nparts(enc.numel()), device=enc.device, dtype=torch.float64)
        real = real.contiguous()
    if prev is not None:
        prev = prev.contiguous(); mask = mask.contiguous()
        assert prev.shape == enc.shape and tuple(mask.shape) == (B, 1, H, W) and mask.dtype == torch.float32
    L.wm_splice_fwd(_p(enc), _p(real), _p(prev), _p(mask), _p(fwd), _p(tam), _p(part), B, C, H * W, _stream())
    return fwd, tam, part


COPYMOVE_MAX_SHIFT = 2 ** 20   # host-side shifts: a larger magnitude is a mistake (the kernel clamps to the frame's size anyway)


def _copymove_shifts(shifts, B):
    """the checked per-frame (sx rows, sy columns) as an int32 [B, 2] tensor: a tensor is returned as given; a host sequence of B pairs
    becomes a FRESH host tensor, which copymove_fwd copies into a fresh device tensor on every call -- a reused staging buffer could be
    rewritten by the next call while an enqueued launch still has to read it"""
    if torch.is_tensor(shifts):
        if shifts.dtype != torch.int32 or tuple(shifts.shape) != (B, 2):
            raise ValueError(f"copymove_fwd: shifts must be int32 [{B}, 2], got {shifts.dtype} {tuple(shifts.shape)}")
        return shifts
    pairs = [tuple(p) for p in shifts]
    if len(pairs) != B or any(len(p) != 2 for p in pairs):
        raise ValueError(f"copymove_fwd: shifts must be {B} (sx, sy) pairs, got {pairs!r}")
    flat = []
    for sx, sy in pairs:
        for s in (sx, sy):
            if isinstance(s, bool) or int(s) != s:
                raise ValueError(f"copymove_fwd: shifts are integers, got {s!r}")
            if abs(int(s)) > COPYMOVE_MAX_SHIFT:
                raise ValueError(f"copymove_fwd: shift {s} exceeds 2**20 in magnitude")
            flat.append(int(s))
    return torch.tensor(flat, dtype=torch.int32).view(B, 2)


def copymove_fwd(enc, mask, shifts, real=None, want_fwd=False):
    """The copy-move forgery (IRNp_model.py:561-598, :1007-1037) in one launch: q = clamp_quant(enc);
    mask_shifted[b,0,i,j] = clamp01(mask[b,0,i-sx_b,j-sy_b]), t[b,c,i,j] = q[b,c,i-sx_b,j-sy_b] (0 where the source lies outside the frame);
    tampered = q*(1-mask_shifted) + t*mask_shifted.  shifts: int32 [B,2] device tensor or a host sequence of B (sx, sy) pairs.
    Returns (fwd_q or None, tampered, mask_shifted, partials): partials f64 [2, wm_splice_nparts(enc.numel())], row 0 the PSNR sums of
    splice_fwd (zeros without `real`; psnr_gate takes partials[0]), row 1 the sums of mask_shifted (copymove_valid)."""
    if enc.dim() != 4 or enc.dtype != torch.float32:
        raise ValueError(f"copymove_fwd: enc must be float32 [B,C,H,W], got {enc.dtype} {tuple(enc.shape)}")
    B, C, H, W = enc.shape
    if tuple(mask.shape) != (B, 1, H, W) or mask.dtype != torch.float32:
        raise ValueError(f"copymove_fwd: mask must be float32 [{B},1,{H},{W}], got {mask.dtype} {tuple(mask.shape)}")
    if real is not None and (real.shape != enc.shape or real.dtype != torch.float32):
        raise ValueError(f"copymove_fwd: real must be float32 {tuple(enc.shape)}, got {real.dtype} {tuple(real.shape)}")
    sh = _copymove_shifts(shifts, B)
    for t in (enc, mask, real, shifts if torch.is_tensor(shifts) else None):
        if t is not None and not t.is_cuda:
            raise RuntimeError("copymove_fwd runs on the HIP path only: move the tensors to cuda (shifts: or pass a host sequence of pairs)")
    sh = sh.contiguous() if sh.is_cuda else sh.to(enc.device)
    enc = enc.contiguous(); mask = mask.contiguous()
    real = real.contiguous() if real is not None else None
    L = _lib.checked()
    fwd = torch.empty_like(enc) if want_fwd else None
    tam = torch.empty_like(enc)
    ms = torch.empty_like(mask)
    part = torch.empty(2, L.wm_splice_nparts(enc.numel()), device=enc.device, dtype=torch.float64)
    L.wm_copymove_fwd(_p(enc), _p(real), _p(mask), _p(sh), _p(fwd), _p(tam), _p(ms), _p(part), B, C, H, W, _stream())
    return fwd, tam, ms, part


def copymove_valid(partials, count):
    """[1] f32 device tensor: mean of the shifted mask over count = B*H*W pixels (IRNp_model.py:592) from copymove_fwd's partials; no host sync"""
    _need_cuda(partials)
    if partials.dim() != 2 or partials.shape[0] != 2 or partials.dtype != torch.float64 or not partials.is_contiguous() or count <= 0:
        raise ValueError("copymove_valid: contiguous float64 partials [2, nparts] of copymove_fwd and a positive count expected")
    out = torch.empty(1, device=partials.device, dtype=torch.float32)
    _lib.checked().wm_copymove_valid(_p(partials), partials.shape[1], float(count), _p(out), _stream())
    return out


def psnr_gate(partials, n, threshold=33.0, w_below=1.0, w_above=0.8):
    """[2] f32 device tensor: (PSNR, forward-loss weight) -- IRNcrop_model.py:379-388, no host sync"""
    out = torch.empty(2, device=partials.device, dtype=torch.float32)
    _lib.checked().wm_psnr_gate(_p(partials), partials.numel(), float(n), threshold, w_below, w_above, _p(out), _stream())
    return out


def mse_fwd_bwd_gated(a, b, gscale, gate, gscale_dev=None):
    """mse_fwd_bwd with the gradient scale multiplied by the device scalar gate[0]"""
    _need_cuda(a, b, gate, gscale_dev)
    if a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError(f"mse_fwd_bwd_gated: float32 tensors of one shape expected, got {tuple(a.shape)} {a.dtype} and {tuple(b.shape)} {b.dtype}")
    if gate.dtype != torch.float32 or gate.numel() < 1 or (gscale_dev is not None and (gscale_dev.dtype != torch.float32 or gscale_dev.numel() < 1)):
        raise ValueError("mse_fwd_bwd_gated: gate and gscale_dev are float32 device scalars")
    a = a.contiguous(); b = b.contiguous()
    n = a.numel()
    nparts = max(1, min(1024, (n + 4095) // 4096))
    part = torch.empty(nparts, device=a.device, dtype=torch.float32)
    grad = torch.empty_like(a)
    _lib.checked().wm_mse_fwd_bwd_gated(_p(a), _p(b), _p(grad), gscale, _p(gate), _p(gscale_dev), _p(part), nparts, n, _stream())
    return part, grad


def bce_logits_target(p, target, gscale=1.0, want_grad=True, chain_sigmoid=False, gscale_dev=None):
    """BCEWithLogitsLoss(mean)(p, target) for tensors: (loss [1] device tensor, gscale * d loss / d p or None).
    chain_sigmoid: p is a sigmoid output s(z) and the gradient returned is wrt z."""
    _need_cuda(p, target)
    p = p.contiguous().float(); target = target.contiguous().float()
    assert p.numel() == target.numel()
    n = p.numel()
    nparts = max(1, min(1024, (n + 4095) // 4096))
    part = torch.empty(nparts, device=p.device, dtype=torch.float32)
    loss = torch.empty(1, device=p.device, dtype=torch.float32)
    grad = torch.empty_like(p) if want_grad else None
    _lib.checked().wm_bce_logits_target(_p(p), _p(target), n, gscale, _p(gscale_dev), _p(part), nparts, _p(loss), _p(grad),
                                        1 if chain_sigmoid else 0, _stream())
    return loss, grad


def masked_axpy_(a, g, mask):
    """a += g * (1 - mask), mask [B,1,H,W] broadcast over channels"""
    _need_cuda(a, g, mask)
    if a.dim() != 4 or g.shape != a.shape or tuple(mask.shape) != (a.shape[0], 1, a.shape[2], a.shape[3]):
        raise ValueError(f"masked_axpy_: a, g [B,C,H,W] and mask [B,1,H,W] expected, got {tuple(a.shape)}, {tuple(g.shape)}, {tuple(mask.shape)}")
    if not (a.dtype == g.dtype == mask.dtype == torch.float32) or not (a.is_contiguous() and g.is_contiguous() and mask.is_contiguous()):
        raise ValueError("masked_axpy_: contiguous float32 tensors expected (a is updated in place)")
    B, C, H, W = a.shape
    _lib.checked().wm_masked_axpy(_p(a), _p(g), _p(mask), B, C, H * W, _stream())
    _wrote(a)
    return a


def mask_threshold(p, threshold=0.5):
    """uint8 tamper mask: p > threshold"""
    _need_cuda(p)
    p = p.contiguous().float()
    out = torch.empty(p.shape, device=p.device, dtype=torch.uint8)
    _lib.checked().wm_mask_threshold(_p(p), threshold, _p(out), p.numel(), _stream())
    return out


def clip_grad_norm_(flats, max_norm, parts=None):
    """nn.utils.clip_grad_norm_ over the parameters of SEVERAL flat gradient buffers taken together (IRNcrop_model.py:410-412:
    netG.parameters() is one group), without a host sync.  Returns the [2] device tensor (clip coefficient, total norm)."""
    assert 1 <= len(flats) <= 4
    parts = parts if parts is not None else [sumsq(f) for f in flats]
    arr = (ctypes.c_void_p * len(parts))(*[p.data_ptr() for p in parts])
    ns = (ctypes.c_int * len(parts))(*[p.numel() for p in parts])
    out = torch.empty(2, device=flats[0].device, dtype=torch.float32)
    L = _lib.checked()
    L.wm_clip_coef(arr, ns, len(parts), float(max_norm), _p(out), _stream())
    for f in flats:
        L.wm_scale_dev(_p(f), f.numel(), _p(out), _stream())
    return out


# ----------------------------------------------------------------------------- per-kernel timing hook
# bench.py brackets launches of one named kernel family with events on the launch stream
# (torch's current stream == the hipStream_t handed to the C ABI).
_TIMER = None


class KernelTimer:
    def __init__(self, match):
        self.match = match  # callable(name, info) -> bool
        self.pairs = []     # (name, start event, end event)

    def elapsed_ms(self, name=None):
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for n, a, b in self.pairs if name is None or n == name]


def set_kernel_timer(timer):
    global _TIMER
    _TIMER = timer


def kernel_timer_installed():
    return _TIMER is not None


def _timed(name, info, launch):
    t = _TIMER
    if t is None or not t.match(name, info):
        return launch()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    r = launch()
    b.record()
    t.pairs.append((name, a, b))
    return r


# ----------------------------------------------------------------------------- stencil / resample attacks
BILINEAR, BICUBIC = 0, 1


def _planes(x):
    _need_cuda(x)
    assert x.dim() == 4 and x.dtype == torch.float32
    x = x.contiguous()
    B, C, H, W = x.shape
    return x, B * C, H, W


def stencil3(x, w9):
    x, N, H, W = _planes(x)
    y = torch.empty_like(x)
    _lib.checked().wm_stencil3_fwd(_p(x), _p(y), N, H, W, _host_floats(w9), _stream())
    return y


BORDER_ZERO, BORDER_REFLECT = 0, 1
GAUSS_SEP_MAX_K = 15
GAUSS_SEP_TILE = (32, 64)       # (rows, columns) of the output tile a workgroup of csrc/gauss_sep.hip owns: the tests put planes on its seams


def _gauss_sep_out(x, out):
    if out is None:
        return torch.empty_like(x)
    _need_cuda(out)
    if out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("gauss_sep: out must be a contiguous float32 tensor of the input's shape")
    return out


def gauss_sep(x, taps, border=BORDER_ZERO, out=None):
    """separable blur of x [B,C,H,W] with outer(taps, taps), len(taps) odd in 3..15; border: BORDER_ZERO | BORDER_REFLECT"""
    x, N, H, W = _planes(x)
    y = _gauss_sep_out(x, out)
    _lib.checked().wm_gauss_sep_fwd(_p(x), _p(y), N, H, W, _host_floats(taps), len(taps), border, _stream())
    return y


def gauss_sep_bwd(gy, taps, border=BORDER_ZERO, out=None):
    """the transpose of gauss_sep (same taps, not reversed by the caller)"""
    gy, N, H, W = _planes(gy)
    gx = _gauss_sep_out(gy, out)
    _lib.checked().wm_gauss_sep_bwd(_p(gy), _p(gx), N, H, W, _host_floats(taps), len(taps), border, _stream())
    return gx


def cropout_fwd(x, cover, rect):
    """rect = (h0, h1, w0, w1): x inside [h0,h1) x [w0,w1), cover elsewhere; a fresh tensor, cover is only read"""
    x, N, H, W = _planes(x)
    _need_cuda(cover)
    if cover.shape != x.shape or cover.dtype != torch.float32:
        raise ValueError("cropout_fwd: cover must be a float32 tensor of the image's shape")
    cover = cover.contiguous()
    h0, h1, w0, w1 = (int(v) for v in rect)
    y = torch.empty_like(x)
    _lib.checked().wm_cropout_fwd(_p(x), _p(cover), _p(y), N, H, W, h0, h1, w0, w1, _stream())
    return y


def cropout_bwd(g, rect, want_cover=False):
    """-> (gx, gcover or None): g inside the rectangle and 0 outside; 0 inside and g outside"""
    g, N, H, W = _planes(g)
    h0, h1, w0, w1 = (int(v) for v in rect)
    gx = torch.empty_like(g)
    gc = torch.empty_like(g) if want_cover else None
    _lib.checked().wm_cropout_bwd(_p(g), _p(gx), _p(gc), N, H, W, h0, h1, w0, w1, _stream())
    return gx, gc


def median_fwd(x, k, want_idx=True):
    x, N, H, W = _planes(x)
    y = torch.empty_like(x)
    idx = torch.empty(x.shape, device=x.device, dtype=torch.int8) if want_idx else None
    _lib.checked().wm_median_fwd(_p(x), _p(y), _p(idx), N, H, W, k, _stream())
    return y, idx


def median_bwd(gy, idx, k):
    gy, N, H, W = _planes(gy)
    gx = torch.empty_like(gy)
    _lib.checked().wm_median_bwd(_p(gy), _p(idx), _p(gx), N, H, W, k, _stream())
    return gx


def resample_fwd(x, rect, out_hw, kind, clamp01=False):
    """rect = (h0, hs, w0, ws) sub-rectangle of x resampled to out_hw."""
    x, N, H, W = _planes(x)
    h0, hs, w0, ws = rect
    OH, OW = out_hw
    y = torch.empty(x.shape[0], x.shape[1], OH, OW, device=x.device, dtype=torch.float32)
    _lib.checked().wm_resample_fwd(_p(x), _p(y), N, H, W, h0, hs, w0, ws, OH, OW, kind, 1 if clamp01 else 0, _stream())
    return y


def resample_bwd(gy, y_clamped, in_hw, rect, kind, separable=True):
    """the transpose of resample_fwd: separable (default) = two passes through a workspace [N,OH,W] (wm_resample_bwd_sep, 3x faster at the
    Resize attack's ratios); separable=False = the one-kernel gather form (wm_resample_bwd)"""
    gy, N, OH, OW = _planes(gy)
    H, W = in_hw
    h0, hs, w0, ws = rect
    gx = torch.empty(gy.shape[0], gy.shape[1], H, W, device=gy.device, dtype=torch.float32)
    yc = y_clamped.contiguous() if y_clamped is not None else None
    if separable:
        tmp = torch.empty(N, OH, W, device=gy.device, dtype=torch.float32)
        _lib.checked().wm_resample_bwd_sep(_p(gy), _p(yc), _p(gx), _p(tmp), N, H, W, h0, hs, w0, ws, OH, OW, kind, _stream())
        return gx
    _lib.checked().wm_resample_bwd(_p(gy), _p(yc), _p(gx), N, H, W, h0, hs, w0, ws, OH, OW, kind, _stream())
    return gx


def quant(x):
    _need_cuda(x)
    x = x.contiguous().float()
    y = torch.empty_like(x)
    _lib.checked().wm_quant_fwd(_p(x), _p(y), x.numel(), _stream())
    return y


# ----------------------------------------------------------------------------- UNet pieces
def bnrelu_maxpool2(y, scale, shift, C, act_out=None, act_c0=0):
    """y [B,H,W,ld] raw conv output -> pooled activated [B,H/2,W/2,C]; optionally writes the activated
    full-resolution map into act_out[..., act_c0:act_c0+C] (the skip half of a concat buffer)."""
    B, H, W, ld = y.shape
    pooled = torch.empty(B, H // 2, W // 2, C, device=y.device, dtype=y.dtype)
    _lib.checked().wm_bnrelu_maxpool2(_p(y), ld, _p(scale), _p(shift), _p(pooled), C, _p(act_out), 0 if act_out is None else act_out.shape[-1],
                                      act_c0, B, H, W, C, dtype_id(y), _stream())
    return pooled


def maxpool2_bwd(y, scale, shift, gpooled, g_skip, g_skip_c0, C):
    """gradient wrt the activated full-resolution map: skip gradient (slice of a concat gradient) + pooled path."""
    B, H, W, ld = y.shape
    g = torch.empty(B, H, W, C, device=y.device, dtype=y.dtype)
    gs_ptr = None
    ldgs = 0
    if g_skip is not None:
        ldgs = g_skip.shape[-1]
        gs_ptr = g_skip.data_ptr() + g_skip_c0 * g_skip.element_size()
    _lib.checked().wm_maxpool2_bwd(_p(y), ld, _p(scale), _p(shift), _p(gpooled), gpooled.shape[-1], gs_ptr, ldgs, _p(g), C, B, H, W, C, dtype_id(y),
                                   _stream())
    return g


def upconv2x2_mfma_supported(Cin, Cout, dtype):
    return bool(_lib.checked().wm_upconv2x2_mfma_supported(Cin, Cout, dt_id(dtype)))


def upconv2x2_pack(w, dtype=torch.bfloat16):
    """w [Cin,Cout,2,2] f32 -> (wf [4*Cout, Cin] rows (ij, co), wb [Cin, 4*Cout] columns (ij, co)) in the 16-bit activation dtype: the MFMA operands"""
    Cin, Cout = w.shape[0], w.shape[1]
    wf = torch.empty(4 * Cout, Cin, device=w.device, dtype=dtype)
    wb = torch.empty(Cin, 4 * Cout, device=w.device, dtype=dtype)
    _lib.checked().wm_upconv2x2_pack(_p(w), _p(wf), _p(wb), Cin, Cout, dt_id(dtype), _stream())
    return wf, wb


def upconv2x2_fwd(x, scale, shift, w, bias, out, c0):
    """x [B,H,W,Cin] (raw + pending BN/ReLU) ; w [Cin,Cout,2,2] f32 -> writes out[B,2H,2W,ld] channels [c0,c0+Cout)."""
    B, H, W, ldx = x.shape
    Cin, Cout = w.shape[0], w.shape[1]
    if upconv2x2_mfma_supported(Cin, Cout, x.dtype):
        wf, _ = upconv2x2_pack(w, x.dtype)
        _lib.checked().wm_upconv2x2_fwd_mfma(_p(x), ldx, _p(scale), _p(shift), _p(wf), _p(bias), _p(out), out.shape[-1], c0, B, H, W, Cin, Cout,
                                             dtype_id(x), _stream())
        return out
    _lib.checked().wm_upconv2x2_fwd(_p(x), ldx, _p(scale), _p(shift), _p(w), _p(bias), _p(out), out.shape[-1], c0, B, H, W, Cin, Cout, dtype_id(x),
                                    _stream())
    return out


def upconv2x2_bwd(x, scale, shift, w, gy, c0, dw, dbias, accumulate):
    """returns gx [B,H,W,Cin]; writes dw [Cin,Cout,2,2], dbias [Cout]."""
    B, H, W, ldx = x.shape
    Cin, Cout = w.shape[0], w.shape[1]
    L = _lib.checked()
    if upconv2x2_mfma_supported(Cin, Cout, x.dtype):
        _, wb = upconv2x2_pack(w, x.dtype)
        gx = torch.empty(B, H, W, Cin, device=x.device, dtype=x.dtype)
        L.wm_upconv2x2_dgrad_mfma(_p(gy), gy.shape[-1], c0, _p(wb), _p(gx), Cin, B, H, W, Cin, Cout, dtype_id(x), _stream())
        ns = L.wm_upconv2x2_wgrad_nsplit(B, H, W, Cin, Cout)
        part = torch.empty(ns, Cin, 4 * Cout, device=x.device, dtype=torch.float32)
        bpart = torch.empty(ns, 4 * Cout, device=x.device, dtype=torch.float32)
        L.wm_upconv2x2_wgrad_mfma(_p(x), ldx, _p(scale), _p(shift), _p(gy), gy.shape[-1], c0, _p(part), _p(bpart), _p(dw), _p(dbias),
                                  1 if accumulate else 0, B, H, W, Cin, Cout, dtype_id(x), _stream())
        return gx
    chunks = L.wm_upconv2x2_dw_chunks(B, H, W)
    N = 4 * Cout
    part = torch.empty(chunks, (Cin + 1) * N, device=x.device, dtype=torch.float32)
    w_t = w.permute(2, 3, 1, 0).reshape(N, Cin).contiguous()
    gx = torch.empty(B, H, W, Cin, device=x.device, dtype=x.dtype)
    L.wm_upconv2x2_bwd(_p(x), ldx, _p(scale), _p(shift), _p(w_t), _p(gy), gy.shape[-1], c0, _p(gx), Cin, _p(part), B, H, W, Cin, Cout,
                       dtype_id(x), _stream())
    red = torch.empty((Cin + 1) * N, device=x.device, dtype=torch.float32)
    colsum(part, (Cin + 1) * N, (Cin + 1) * N, red, False)
    gw = red[:Cin * N].view(Cin, Cout, 2, 2)
    gb = red[Cin * N:].view(Cout, 4).sum(1)
    if accumulate:
        dw += gw
        dbias += gb
    else:
        dw.copy_(gw)
        dbias.copy_(gb)
    return gx


# ----------------------------------------------------------------------------- DiffJPEG
ROUND, ROUND_ONLY_AT_0, DIFF_ROUND = 0, 1, 2


def diffjpeg_fwd(x, rounding, factor):
    _need_cuda(x)
    assert x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32
    x = x.contiguous()
    y = torch.empty_like(x)
    B, _, H, W = x.shape
    _lib.checked().wm_diffjpeg_fwd(_p(x), _p(y), B, H, W, rounding, factor, _stream())
    return y


def diffjpeg_bwd(x, gy, rounding, factor):
    _need_cuda(x, gy)
    x = x.contiguous(); gy = gy.contiguous()
    gx = torch.empty_like(gy)
    B, _, H, W = x.shape
    _lib.checked().wm_diffjpeg_bwd(_p(x), _p(gy), _p(gx), B, H, W, rounding, factor, _stream())
    return gx


# ----------------------------------------------------------------------------- general layer family (include/wm_hip.h)
ACT_KINDS = {"relu": 0, "lrelu": 1, "gelu": 2, "elu": 3, "sigmoid": 4, "tanh": 5}
ACT_BWD_KINDS = dict(ACT_KINDS, elu_out=6)   # backward only: the ELU derivative from the layer's output (conv3x3_fwd_elu keeps no pre-activation)


def cpad(c):
    """channel stride of an NHWC activation with c real channels"""
    return (int(c) + 15) // 16 * 16


def _nhwc(x):
    _need_cuda(x)
    if x.dim() != 4 or not x.is_contiguous() or x.shape[3] % 16:
        raise ValueError(f"expected a contiguous NHWC tensor with a channel stride that is a multiple of 16, got {tuple(x.shape)}")
    return x


def gconv_pack(w, rows, cols, transpose, dtype):
    """w [Cout,Cin,KH,KW] f32 -> [KH*KW][rows][cols] of dtype (rows = Cout / cols = Cin, or swapped with transpose)"""
    _need_cuda(w)
    assert w.dim() == 4 and w.dtype == torch.float32
    w = w.contiguous()
    Cout, Cin, KH, KW = w.shape
    wp = torch.empty(KH * KW, rows, cols, device=w.device, dtype=dtype)
    _lib.checked().wm_gconv_pack(_p(w), _p(wp), Cout, Cin, KH, KW, rows, cols, 1 if transpose else 0, dt_id(dtype), _stream())
    return wp


def gconv_fwd(x, wp, bias, out_hw, KH, KW, stride, pad, dgrad=False, dilation=1):
    """x [B,IH,IW,KC]; wp [taps][NC][KC] (gconv_pack); bias f32 [NC] or None; -> [B,OH,OW,NC].  dilation 1 is the undilated entry
    point; any other value goes to wm_gconv_dil_fwd (gconv_dil_fwd below takes 1 as well)"""
    if dilation != 1:
        return gconv_dil_fwd(x, wp, bias, out_hw, KH, KW, stride, pad, dilation, dgrad)
    x = _nhwc(x)
    B, IH, IW, KC = x.shape
    taps, NC, KC2 = wp.shape
    if taps != KH * KW or KC2 != KC or wp.dtype != x.dtype:
        raise ValueError(f"packed filter {tuple(wp.shape)} {wp.dtype} does not fit the input {tuple(x.shape)} {x.dtype} / {KH}x{KW}")
    if bias is not None and (bias.numel() != NC or bias.dtype != torch.float32):
        raise ValueError("bias must be f32 with one entry per (padded) output channel")
    OH, OW = out_hw
    out = torch.empty(B, OH, OW, NC, device=x.device, dtype=x.dtype)
    _lib.checked().wm_gconv_fwd(_p(x), _p(wp), _p(bias), _p(out), B, IH, IW, KC, OH, OW, NC, KH, KW, stride, pad, 1 if dgrad else 0, dt_id(x.dtype),
                                _stream())
    return out


def gconv_dil_fwd(x, wp, bias, out_hw, KH, KW, stride, pad, dilation, dgrad=False):
    """gconv_fwd through wm_gconv_dil_fwd: tap (ky, kx) reads ky * dilation, kx * dilation pixels away (stride 1 when dilation > 1)"""
    x = _nhwc(x)
    B, IH, IW, KC = x.shape
    taps, NC, KC2 = wp.shape
    if taps != KH * KW or KC2 != KC or wp.dtype != x.dtype:
        raise ValueError(f"packed filter {tuple(wp.shape)} {wp.dtype} does not fit the input {tuple(x.shape)} {x.dtype} / {KH}x{KW}")
    if bias is not None and (bias.numel() != NC or bias.dtype != torch.float32):
        raise ValueError("bias must be f32 with one entry per (padded) output channel")
    OH, OW = out_hw
    out = torch.empty(B, OH, OW, NC, device=x.device, dtype=x.dtype)
    _lib.checked().wm_gconv_dil_fwd(_p(x), _p(wp), _p(bias), _p(out), B, IH, IW, KC, OH, OW, NC, KH, KW, stride, pad, int(dilation),
                                    1 if dgrad else 0, dt_id(x.dtype), _stream())
    return out


def gconv_wgrad(dout, x, Cout, Cin, KH, KW, stride, pad, want_bias=True, dw_acc=None, db_acc=None, dilation=1, dil_entry=False):
    """dw [Cout,Cin,KH,KW] f32, dbias [Cout] f32 (or None) of the conv x [B,IH,IW,KC] -> dout [B,OH,OW,NC].
    dw_acc (and db_acc when a bias gradient is wanted): contiguous f32 tensors of those shapes the results are ADDED to instead.
    dilation != 1 (or dil_entry, which sends dilation 1 there too) runs wm_gconv_dil_wgrad"""
    dout, x = _nhwc(dout), _nhwc(x)
    B, OH, OW, NC = dout.shape
    _, IH, IW, KC = x.shape
    if x.shape[0] != B or x.dtype != dout.dtype:
        raise ValueError("gconv_wgrad: operands disagree")
    L = _lib.checked()
    partial = torch.empty(L.wm_gconv_wgrad_scratch_floats(B, OH, OW, KC, NC, KH, KW), device=x.device,
                          dtype=torch.float32)
    acc = dw_acc is not None
    if acc and (not dw_acc.is_contiguous() or dw_acc.numel() != Cout * Cin * KH * KW or dw_acc.dtype != torch.float32 or
                (want_bias and (db_acc is None or not db_acc.is_contiguous() or db_acc.numel() != Cout or db_acc.dtype != torch.float32))):
        raise ValueError("gconv_wgrad: accumulation targets do not match the gradients")
    dw = dw_acc if acc else torch.empty(Cout, Cin, KH, KW, device=x.device, dtype=torch.float32)
    db = (db_acc if acc else torch.empty(Cout, device=x.device, dtype=torch.float32)) if want_bias else None
    if dilation != 1 or dil_entry:
        L.wm_gconv_dil_wgrad(_p(dout), _p(x), _p(partial), _p(dw), _p(db), 1 if acc else 0, B, IH, IW, KC, OH, OW, NC, KH, KW, stride, pad,
                             int(dilation), Cout, Cin, dt_id(x.dtype), _stream())
        return dw, db
    _lib.checked().wm_gconv_wgrad(_p(dout), _p(x), _p(partial), _p(dw), _p(db), 1 if acc else 0, B, IH, IW, KC, OH, OW, NC, KH, KW, stride, pad,
                                  Cout, Cin, dt_id(x.dtype), _stream())
    return dw, db


def gcolsum(x, creal, out_acc=None, f64=False):
    """column sums [creal] f32 of x [.., C]; out_acc: a contiguous f32 [creal] tensor they are ADDED to instead.  f64: accumulated in
    double and rounded once (wm_gcolsum_f64)"""
    x = _nhwc(x)
    C = x.shape[3]
    if out_acc is not None and (not out_acc.is_contiguous() or out_acc.numel() != creal or out_acc.dtype != torch.float32):
        raise ValueError("gcolsum: accumulation target does not match")
    out = out_acc if out_acc is not None else torch.empty(creal, device=x.device, dtype=torch.float32)
    L = _lib.checked()
    if f64:
        L.wm_gcolsum_f64(_p(x), x.numel() // C, C, _p(out), creal, 0 if out_acc is None else 1, dt_id(x.dtype), _stream())
        return out
    scratch = torch.empty(L.wm_gcolsum_scratch_floats(x.numel() // C, C), device=x.device, dtype=torch.float32)
    L.wm_gcolsum(_p(x), x.numel() // C, C, _p(out), creal, 0 if out_acc is None else 1, _p(scratch), dt_id(x.dtype), _stream())
    return out


def unary_fwd(x, kind):
    _need_cuda(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    _lib.checked().wm_unary_fwd(_p(x), _p(y), x.numel(), ACT_KINDS[kind], dt_id(x.dtype), _stream())
    return y


def unary_bwd(x, gy, kind):
    _need_cuda(x, gy)
    gy = gy.contiguous()
    gx = torch.empty_like(x)
    _lib.checked().wm_unary_bwd(_p(x), _p(gy), _p(gx), x.numel(), ACT_KINDS[kind], dt_id(x.dtype), _stream())
    return gx


def unary_bwd_colsum(x, gy, kind, creal, db_acc=None):
    """(gx, db): gx = gy * act'(x) and db [creal] = the column sums of gx (the bias gradient of the convolution under the activation)
    in one pass over the data (csrc/gelem.hip); NHWC, channel stride a multiple of 16.  db_acc: added to instead (contiguous f32 [creal])"""
    _need_cuda(x, gy)
    x, gy = _nhwc(x), gy.contiguous()
    C = x.shape[3]
    npix = x.numel() // C
    gx = torch.empty_like(x)
    if db_acc is not None and (not db_acc.is_contiguous() or db_acc.numel() != creal or db_acc.dtype != torch.float32):
        raise ValueError("unary_bwd_colsum: accumulation target does not match")
    db = db_acc if db_acc is not None else torch.empty(creal, device=x.device, dtype=torch.float32)
    L = _lib.checked()
    part = torch.empty(L.wm_unary_bwd_colsum_scratch_floats(npix, C), device=x.device, dtype=torch.float32)
    L.wm_unary_bwd_colsum(_p(x), _p(gy), _p(gx), npix, C, ACT_BWD_KINDS[kind], _p(part), _p(db), creal, 0 if db_acc is None else 1,
                          dt_id(x.dtype), _stream())
    return gx, db


def add_scaled(a, b, alpha=1.0):
    _need_cuda(a, b)
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError("add_scaled: operands disagree")
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty_like(a)
    _lib.checked().wm_add_scaled(_p(a), _p(b), _p(out), a.numel(), alpha, dt_id(a.dtype), _stream())
    return out


def qfatt_fwd(x, res, gamma, beta):
    """x + gamma[b,c] * res + beta[b,c]; gamma / beta f32 [B, >= C]"""
    x, res = _nhwc(x), _nhwc(res)
    B, H, W, C = x.shape
    gamma, beta = gamma.contiguous(), beta.contiguous()
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.shape == beta.shape and gamma.shape[0] == B
    out = torch.empty_like(x)
    _lib.checked().wm_qfatt_fwd(_p(x), _p(res), _p(gamma), _p(beta), _p(out), B, H * W, C, gamma.shape[1], dt_id(x.dtype), _stream())
    return out


def qfatt_bwd(g, res, gamma):
    g, res = _nhwc(g.contiguous()), _nhwc(res)
    B, H, W, C = g.shape
    gamma = gamma.contiguous()
    gres = torch.empty_like(g)
    gg = torch.zeros_like(gamma)
    gb = torch.zeros_like(gamma)
    L = _lib.checked()
    scratch = torch.empty(L.wm_qfatt_bwd_scratch_floats(B, H * W, gamma.shape[1]), device=g.device, dtype=torch.float32)
    L.wm_qfatt_bwd(_p(g), _p(res), _p(gamma), _p(gres), _p(gg), _p(gb), _p(scratch), B, H * W, C, gamma.shape[1], dt_id(g.dtype), _stream())
    return gres, gg, gb


def gpool_fwd(x):
    x = _nhwc(x)
    B, H, W, C = x.shape
    out = torch.empty(B, C, device=x.device, dtype=torch.float32)
    _lib.checked().wm_gpool_fwd(_p(x), _p(out), B, H * W, C, dt_id(x.dtype), _stream())
    return out


def gpool_bwd(g, shape, dtype):
    _need_cuda(g)
    B, H, W, C = shape
    g = g.contiguous().float()
    gx = torch.empty(B, H, W, C, device=g.device, dtype=dtype)
    _lib.checked().wm_gpool_bwd(_p(g), _p(gx), B, H * W, C, dt_id(dtype), _stream())
    return gx


PAD_SYMMETRIC, PAD_REPLICATE = 0, 1


def pad_nchw_to_nhwc(x, pads, mode, dtype):
    """x [B,C,H,W] f32 -> [B,H+top+bottom,W+left+right,cpad(C)] of dtype; pads = (left, right, top, bottom)"""
    _need_cuda(x)
    x = x.contiguous().float()
    B, C, H, W = x.shape
    l, r, t, b = pads
    out = torch.empty(B, H + t + b, W + l + r, cpad(C), device=x.device, dtype=dtype)
    _lib.checked().wm_pad_nchw_to_nhwc(_p(x), _p(out), B, C, H, W, l, r, t, b, mode, out.shape[3], dt_id(dtype), _stream())
    return out


def pad_nchw_to_nhwc_bwd(gp, shape, pads, mode):
    gp = _nhwc(gp.contiguous())
    B, C, H, W = shape
    l, r, t, b = pads
    gx = torch.empty(B, C, H, W, device=gp.device, dtype=torch.float32)
    _lib.checked().wm_pad_nchw_to_nhwc_bwd(_p(gp), _p(gx), B, C, H, W, l, r, t, b, mode, gp.shape[3], dt_id(gp.dtype), _stream())
    return gx


def gunpack_nchw(x, C, H, W):
    x = _nhwc(x)
    B, PH, PW, CP = x.shape
    out = torch.empty(B, C, H, W, device=x.device, dtype=torch.float32)
    _lib.checked().wm_gunpack_nchw(_p(x), _p(out), B, C, H, W, PH, PW, CP, dt_id(x.dtype), _stream())
    return out


def gunpack_nchw_bwd(g, shape, dtype):
    _need_cuda(g)
    g = g.contiguous().float()
    B, C, H, W = g.shape
    _, PH, PW, CP = shape
    gx = torch.empty(B, PH, PW, CP, device=g.device, dtype=dtype)
    _lib.checked().wm_gunpack_nchw_bwd(_p(g), _p(gx), B, C, H, W, PH, PW, CP, dt_id(dtype), _stream())
    return gx


def spectral_norm_fwd(w, u, v, do_iter):
    """w [Cout, ...] f32; u [Cout], v [N] updated in place when do_iter; -> (w / sigma, sigma [1])"""
    _need_cuda(w, u, v)
    w = w.contiguous()
    M, N = w.shape[0], w.numel() // w.shape[0]
    assert u.numel() == M and v.numel() == N and u.is_contiguous() and v.is_contiguous() and u.dtype == torch.float32 and v.dtype == torch.float32
    sigma = torch.empty(1, device=w.device, dtype=torch.float32)
    wsn = torch.empty_like(w)
    L = _lib.checked()
    scratch = torch.empty(L.wm_spectral_norm_scratch_floats(M, N), device=w.device, dtype=torch.float32)
    L.wm_spectral_norm_fwd(_p(w), _p(u), _p(v), _p(sigma), _p(wsn), _p(scratch), M, N, 1 if do_iter else 0, _stream())
    return wsn, sigma


def spectral_norm_bwd(g, wsn, u, v, sigma):
    _need_cuda(g)
    g = g.contiguous()
    M, N = g.shape[0], g.numel() // g.shape[0]
    partial = torch.empty(256, device=g.device, dtype=torch.float32)
    gw = torch.empty_like(g)
    _lib.checked().wm_spectral_norm_bwd(_p(g), _p(wsn), _p(u), _p(v), _p(sigma), _p(partial), _p(gw), M, N, 0, _stream())
    return gw


def bayar_constrain_(w, torch_order=False):
    """the Bayar constraint on w [Co,Ci,5,5] in place (conditional_jpeg_generator.py:814-817, networks.py:1059-1061).  torch_order: the
    plane sums in the order torch.sum takes on the CPU instead of left to right (the reference's float32 result bit for bit)"""
    _need_cuda(w)
    assert w.dtype == torch.float32 and w.is_contiguous() and w.shape[-2:] == (5, 5)
    L = _lib.checked()
    constrain = L.wm_bayar_constrain_torch_order if torch_order else L.wm_bayar_constrain
    constrain(_p(w), w.shape[0] * w.shape[1], _stream())
    return w


def _nhwc16b(x):
    _need_cuda(x)
    if x.dim() != 4 or not x.is_contiguous() or (x.shape[3] * x.element_size()) % 16:
        raise ValueError(f"expected a contiguous NHWC tensor whose channel stride is a multiple of 16 bytes, got {tuple(x.shape)} {x.dtype}")
    return x


def reflect_pad_fwd(x, pad):
    """nn.ReflectionPad2d(pad) on NHWC: x [B,H,W,CP] -> [B,H+2pad,W+2pad,CP]; pad <= min(H, W) - 1; CP a multiple of 16 bytes"""
    x = _nhwc16b(x)
    B, H, W, CP = x.shape
    pad = int(pad)
    if pad < 0 or pad > min(H, W) - 1:
        raise ValueError(f"reflect_pad_fwd: pad {pad} needs min(H, W) - 1 >= pad, got {tuple(x.shape)}")
    out = torch.empty(B, H + 2 * pad, W + 2 * pad, CP, device=x.device, dtype=x.dtype)
    _lib.checked().wm_reflect_pad_fwd(_p(x), _p(out), B, H, W, CP, pad, dt_id(x.dtype), _stream())
    return out


def reflect_pad_bwd(g, pad):
    """the adjoint of reflect_pad_fwd: g [B,H+2pad,W+2pad,CP] -> [B,H,W,CP], every padded position added onto the pixel it mirrors"""
    g = _nhwc16b(g)
    B, PH, PW, CP = g.shape
    pad = int(pad)
    H, W = PH - 2 * pad, PW - 2 * pad
    if pad < 0 or H < 1 or W < 1 or pad > min(H, W) - 1:
        raise ValueError(f"reflect_pad_bwd: {tuple(g.shape)} is no reflection-padded tensor of pad {pad}")
    gx = torch.empty(B, H, W, CP, device=g.device, dtype=g.dtype)
    _lib.checked().wm_reflect_pad_bwd(_p(g), _p(gx), B, H, W, CP, pad, dt_id(g.dtype), _stream())
    return gx


# ----------------------------------------------------------------------------- invertible embedder pieces
def haar(x, C, fac, up, by_wavelet=False):
    """up False: [B,2H,2W,cpad(C)] -> [B,H,W,cpad(4C)] (analysis); up True: [B,H,W,cpad(4C)] -> [B,2H,2W,cpad(C)] (synthesis).
    by_wavelet: the 4C channels in wavelet-major order k*C + c (HaarDownsampling(order_by_wavelet=True)) instead of 4*c + k"""
    x = _nhwc(x)
    B, XH, XW, CPin = x.shape
    if up:
        if CPin < 4 * C:
            raise ValueError(f"haar synthesis of {C} channels needs {4 * C} input channels, stride is {CPin}")
        H, W = XH, XW
        out = torch.empty(B, 2 * H, 2 * W, cpad(C), device=x.device, dtype=x.dtype)
    else:
        if XH % 2 or XW % 2 or CPin < C:
            raise ValueError(f"haar analysis needs even height / width and {C} channels, got {tuple(x.shape)}")
        H, W = XH // 2, XW // 2
        out = torch.empty(B, H, W, cpad(4 * C), device=x.device, dtype=x.dtype)
    _lib.checked().wm_haar(_p(x), _p(out), B, H, W, C, CPin, out.shape[3], fac, (1 if up else 0) | (2 if by_wavelet else 0), dt_id(x.dtype),
                           _stream())
    return out


def chan_copy_(dst, doff, src, soff, n):
    """dst[..., doff:doff+n] = src[..., soff:soff+n] (NHWC, same pixel grid)"""
    dst, src = _nhwc(dst), _nhwc(src)
    if dst.shape[:3] != src.shape[:3] or dst.dtype != src.dtype:
        raise ValueError("chan_copy_: pixel grids / dtypes disagree")
    npix = dst.shape[0] * dst.shape[1] * dst.shape[2]
    _lib.checked().wm_chan_copy(_p(src), _p(dst), npix, src.shape[3], soff, dst.shape[3], doff, n, dt_id(dst.dtype), _stream())
    return dst


def chan_place(dstride, a, aoff, adst, na, b=None, boff=0, bdst=0, nb=0):
    """a new NHWC tensor [.., dstride], written whole by one launch: a[..., aoff:aoff+na] at channel adst, b[..., boff:boff+nb] (optional)
    at bdst, zero elsewhere"""
    a = _nhwc(a)
    if b is not None:
        b = _nhwc(b)
        if b.shape[:3] != a.shape[:3] or b.dtype != a.dtype:
            raise ValueError("chan_place: pixel grids / dtypes disagree")
    if dstride % 16:
        raise ValueError("chan_place: the channel stride must be a multiple of 16")
    out = torch.empty(*a.shape[:3], dstride, device=a.device, dtype=a.dtype)
    npix = a.shape[0] * a.shape[1] * a.shape[2]
    _lib.checked().wm_chan_place(_p(a), a.shape[3], aoff, adst, na, _p(b), b.shape[3] if b is not None else 0, boff, bdst, nb, _p(out), dstride,
                                 npix, dt_id(a.dtype), _stream())
    return out


def coupling_fwd(x, s, t, clamp, eps, rev):
    _need_cuda(x, s, t)
    if not (x.shape == s.shape == t.shape and x.dtype == s.dtype == t.dtype):
        raise ValueError("coupling_fwd: operands disagree")
    x, s, t = x.contiguous(), s.contiguous(), t.contiguous()
    y = torch.empty_like(x)
    _lib.checked().wm_coupling_fwd(_p(x), _p(s), _p(t), _p(y), x.numel(), clamp, eps, 1 if rev else 0, dt_id(x.dtype), _stream())
    return y


def coupling_bwd(g, v, s, clamp, eps, rev):
    _need_cuda(g, v, s)
    g = g.contiguous()
    gx, gs, gt = torch.empty_like(g), torch.empty_like(g), torch.empty_like(g)
    _lib.checked().wm_coupling_bwd(_p(g), _p(v), _p(s), _p(gx), _p(gs), _p(gt), g.numel(), clamp, eps, 1 if rev else 0, dt_id(g.dtype), _stream())
    return gx, gs, gt


# ----------------------------------------------------------------------------- InvBlockExp couplings (csrc/invblock.hip)
def _invblock_args(name, x, n1, n2, **tensors):
    """x [B,H,W,>= n1+n2] and every named tensor [B,H,W,stride] of x's pixel grid and dtype, contiguous -> (x, the tensors, npix)"""
    x = _nhwc(x)
    if n1 < 1 or n2 < 1 or n1 + n2 > x.shape[3]:
        raise ValueError(f"{name}: channels [0,{n1 + n2}) do not fit the stride {x.shape[3]}")
    out = []
    for k, (t, stride) in tensors.items():
        if t is not None:
            t = _nhwc(t)
            if t.shape[:3] != x.shape[:3] or t.dtype != x.dtype or t.shape[3] != stride:
                raise ValueError(f"{name}: {k} {tuple(t.shape)} {t.dtype} is not [{', '.join(map(str, x.shape[:3]))}, {stride}] {x.dtype}")
        out.append(t)
    return x, out, x.shape[0] * x.shape[1] * x.shape[2]


def invblock_shift_fwd(x, f, n1, n2, sign, other=None):
    """x[..., :n1] + sign * f as its own tensor [.., cpad(n1)], or, with other [.., cpad(n2)], as cat(that, other[..., :n2]) [.., cpad(n1+n2)]"""
    x, (f, other), npix = _invblock_args("invblock_shift_fwd", x, n1, n2, f=(f, cpad(n1)), other=(other, cpad(n2)))
    out = torch.empty(*x.shape[:3], cpad(n1 + n2) if other is not None else cpad(n1), device=x.device, dtype=x.dtype)
    _lib.checked().wm_invblock_shift(_p(x), x.shape[3], _p(f), _p(other), _p(out), npix, n1, n2, float(sign), dt_id(x.dtype), _stream())
    return out


def invblock_shift_bwd(g, n1, n2, sign, whole, xstride):
    """g = dL/dout of invblock_shift_fwd (whole: it had `other`) -> (gx [.., xstride], gf [.., cpad(n1)], gother [.., cpad(n2)] or None)"""
    g = _nhwc(g)
    if g.shape[3] != (cpad(n1 + n2) if whole else cpad(n1)) or n1 + n2 > xstride:
        raise ValueError(f"invblock_shift_bwd: gradient stride {g.shape[3]} / x stride {xstride} do not match splits {n1}, {n2}")
    new = lambda c: torch.empty(*g.shape[:3], c, device=g.device, dtype=g.dtype)       # noqa: E731
    gx, gf, gother = new(xstride), new(cpad(n1)), (new(cpad(n2)) if whole else None)
    _lib.checked().wm_invblock_shift_bwd(_p(g), 1 if whole else 0, _p(gx), xstride, _p(gf), _p(gother), g.shape[0] * g.shape[1] * g.shape[2],
                                         n1, n2, float(sign), dt_id(g.dtype), _stream())
    return gx, gf, gother


def invblock_affine_fwd(x, h, g, n1, n2, clamp, rev, other=None, want_jac=False):
    """s = clamp * (2 sigmoid(h) - 1); v = x[..., n1:n1+n2] * exp(s) + g (rev: (.. - g) / exp(s)) as its own tensor [.., cpad(n2)], or, with
    other [.., cpad(n1)], as cat(other[..., :n1], v) [.., cpad(n1+n2)].  -> (out, jac): jac f32 [B] = sum of s per sample (None unless
    want_jac), summed in double in a fixed order"""
    x, (h, g, other), npix = _invblock_args("invblock_affine_fwd", x, n1, n2, h=(h, cpad(n2)), g=(g, cpad(n2)), other=(other, cpad(n1)))
    B, hw = x.shape[0], x.shape[1] * x.shape[2]
    out = torch.empty(*x.shape[:3], cpad(n1 + n2) if other is not None else cpad(n2), device=x.device, dtype=x.dtype)
    jac = scratch = None
    if want_jac:
        jac = torch.empty(B, device=x.device, dtype=torch.float32)
        scratch = torch.empty(max(int(_lib.checked().wm_invblock_scratch_doubles(B, hw, n1, n2)), 1), device=x.device, dtype=torch.float64)
    _lib.checked().wm_invblock_affine(_p(x), x.shape[3], _p(h), _p(g), _p(other), _p(out), _p(jac), _p(scratch), B, hw, n1, n2, float(clamp),
                                      1 if rev else 0, dt_id(x.dtype), _stream())
    return out, jac


def invblock_affine_bwd(gout, v, voff, h, n1, n2, clamp, rev, whole, xstride):
    """gout = dL/dout of invblock_affine_fwd (whole: it had `other`); v = x (rev False, voff = n1) or the forward's output (rev True, voff =
    n1 if whole else 0) -> (gx [.., xstride], gh, gg [.., cpad(n2)], gother [.., cpad(n1)] or None)"""
    gout, v, h = _nhwc(gout), _nhwc(v), _nhwc(h)
    if gout.shape[3] != (cpad(n1 + n2) if whole else cpad(n2)) or h.shape[3] != cpad(n2) or n1 + n2 > xstride or voff + n2 > v.shape[3] \
            or not (gout.shape[:3] == v.shape[:3] == h.shape[:3]) or not (gout.dtype == v.dtype == h.dtype):
        raise ValueError("invblock_affine_bwd: operands disagree with the splits %d, %d" % (n1, n2))
    new = lambda c: torch.empty(*gout.shape[:3], c, device=gout.device, dtype=gout.dtype)       # noqa: E731
    gx, gh, gg, gother = new(xstride), new(cpad(n2)), new(cpad(n2)), (new(cpad(n1)) if whole else None)
    _lib.checked().wm_invblock_affine_bwd(_p(gout), 1 if whole else 0, _p(v), v.shape[3], voff, _p(h), _p(gx), xstride, _p(gh), _p(gg), _p(gother),
                                          gout.shape[0] * gout.shape[1] * gout.shape[2], n1, n2, float(clamp), 1 if rev else 0,
                                          dt_id(gout.dtype), _stream())
    return gx, gh, gg, gother


# ----------------------------------------------------------------------------- instance normalisation (csrc/instnorm.hip)
INSTNORM_ACTS = {None: 0, "relu": 1}


def _instnorm_args(name, x, C, gamma, beta, act):
    x = _nhwc(x)
    _need_cuda(gamma, beta)
    if act not in INSTNORM_ACTS:
        raise ValueError(f"{name}: act {act!r} (None or 'relu')")
    if not 0 < C <= x.shape[3]:
        raise ValueError(f"{name}: {C} channels in a stride of {x.shape[3]}")
    if (gamma is None) != (beta is None):
        raise ValueError(f"{name}: gamma and beta come together")
    for t in (gamma, beta):
        if t is not None and (t.dtype != torch.float32 or t.numel() != C or not t.is_contiguous()):
            raise ValueError(f"{name}: gamma / beta must be contiguous float32 [{C}]")
    return x


def instnorm_stats(x, C, eps=1e-5):
    """(mean, rstd) f32 [B, Cp] of every (sample, channel) plane of x [B,H,W,Cp]: biased variance, rstd = 1 / sqrt(max(var, 0) + eps),
    zeros in the padding channels; sums in double, fixed order"""
    x = _instnorm_args("instnorm_stats", x, C, None, None, None)
    B, H, W, CP = x.shape
    L = _lib.checked()
    part = torch.empty(L.wm_instnorm_scratch_doubles(B, H * W, CP), device=x.device, dtype=torch.float64)
    mean = torch.empty(B, CP, device=x.device, dtype=torch.float32)
    rstd = torch.empty(B, CP, device=x.device, dtype=torch.float32)
    L.wm_instnorm_stats(_p(x), _p(part), _p(mean), _p(rstd), B, H * W, C, CP, float(eps), dt_id(x.dtype), _stream())
    return mean, rstd


def instnorm_apply(x, C, mean, rstd, gamma=None, beta=None, act=None):
    """act((x - mean) * rstd * gamma + beta); padding channels written as zeros"""
    x = _instnorm_args("instnorm_apply", x, C, gamma, beta, act)
    B, H, W, CP = x.shape
    y = torch.empty_like(x)
    _lib.checked().wm_instnorm_apply(_p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(y), B, H * W, C, CP, INSTNORM_ACTS[act], dt_id(x.dtype),
                                     _stream())
    return y


def instnorm_fwd(x, C, eps=1e-5, gamma=None, beta=None, act=None):
    """nn.InstanceNorm2d(C, eps, affine = gamma is not None)(x) (+ ReLU) -> (y, mean, rstd): two launches, three when a plane spans
    several workgroups (ops.instnorm_splits)"""
    mean, rstd = instnorm_stats(x, C, eps)
    return instnorm_apply(x, C, mean, rstd, gamma, beta, act), mean, rstd


def instnorm_bwd(x, dy, C, mean, rstd, gamma=None, beta=None, act=None, want_params=True):
    """(dx, dgamma, dbeta) of instnorm_fwd for the output gradient dy; xhat and the ReLU mask are recomputed from x.  dgamma / dbeta f32 [C],
    None without gamma or with want_params False"""
    x = _instnorm_args("instnorm_bwd", x, C, gamma, beta, act)
    _need_cuda(dy)
    dy = dy.contiguous()
    if dy.shape != x.shape or dy.dtype != x.dtype:
        raise ValueError("instnorm_bwd: the output gradient does not match the input")
    B, H, W, CP = x.shape
    L = _lib.checked()
    part = torch.empty(L.wm_instnorm_scratch_doubles(B, H * W, CP), device=x.device, dtype=torch.float64)
    mg = torch.empty(B, CP, device=x.device, dtype=torch.float32)
    mgx = torch.empty(B, CP, device=x.device, dtype=torch.float32)
    dgamma = dbeta = None
    if gamma is not None and want_params:
        dgamma = torch.empty(C, device=x.device, dtype=torch.float32)
        dbeta = torch.empty(C, device=x.device, dtype=torch.float32)
    act_id, dt = INSTNORM_ACTS[act], dt_id(x.dtype)
    L.wm_instnorm_bwd_sums(_p(x), _p(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(part), _p(mg), _p(mgx), _p(dgamma), _p(dbeta), B, H * W, C,
                           CP, act_id, dt, _stream())
    dx = torch.empty_like(x)
    L.wm_instnorm_bwd_apply(_p(x), _p(dy), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(mg), _p(mgx), _p(dx), B, H * W, C, CP, act_id, dt, _stream())
    return dx, dgamma, dbeta


def instnorm_splits(hw):
    """workgroups that share one (sample) plane of hw pixels in the instance-norm kernels"""
    return _lib.checked().wm_instnorm_splits(hw)


# ----------------------------------------------------------------------------- LayerNorm and Swin window attention (csrc/swin.hip)
def _layernorm_args(name, x, C, gamma, beta):
    x = _nhwc(x)
    _need_cuda(gamma, beta)
    if not 0 < C <= x.shape[3]:
        raise ValueError(f"{name}: {C} channels in a stride of {x.shape[3]}")
    for t in (gamma, beta):
        if t is not None and (t.dtype != torch.float32 or t.numel() != C or not t.is_contiguous()):
            raise ValueError(f"{name}: gamma / beta must be contiguous float32 [{C}]")
    return x


def layernorm_fwd(x, C, gamma, beta, eps=1e-5):
    """nn.LayerNorm(C, eps)(x) over the C channels of every token of x [B,H,W,Cp] -> (y, mean, rstd); mean, rstd f32 [B*H*W]; padding
    channels of y written as zeros"""
    x = _layernorm_args("layernorm_fwd", x, C, gamma, beta)
    B, H, W, CP = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(B * H * W, device=x.device, dtype=torch.float32)
    rstd = torch.empty(B * H * W, device=x.device, dtype=torch.float32)
    _lib.checked().wm_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), B * H * W, C, CP, float(eps), dt_id(x.dtype), _stream())
    return y, mean, rstd


def layernorm_bwd(x, dy, C, gamma, mean, rstd, want_params=True):
    """(dx, dgamma, dbeta) of layernorm_fwd for the output gradient dy; xhat is recomputed from x.  dgamma / dbeta f32 [C] (None with
    want_params False): partial rows in double added in a fixed order, so two calls give the same bits"""
    x = _layernorm_args("layernorm_bwd", x, C, gamma, None)
    _need_cuda(dy, mean, rstd)
    dy = dy.contiguous()
    if dy.shape != x.shape or dy.dtype != x.dtype:
        raise ValueError("layernorm_bwd: the output gradient does not match the input")
    B, H, W, CP = x.shape
    L = _lib.checked()
    dx = torch.empty_like(x)
    dgamma = dbeta = part = None
    if want_params:
        part = torch.empty(L.wm_layernorm_scratch_doubles(B * H * W, C), device=x.device, dtype=torch.float64)
        dgamma = torch.empty(C, device=x.device, dtype=torch.float32)
        dbeta = torch.empty(C, device=x.device, dtype=torch.float32)
    L.wm_layernorm_bwd(_p(x), _p(dy), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dgamma), _p(dbeta), _p(part), B * H * W, C, CP, dt_id(x.dtype),
                       _stream())
    return dx, dgamma, dbeta


def _winattn_args(name, qkv, table, C, num_heads, ws):
    qkv = _nhwc(qkv)
    _need_cuda(table)
    if C % num_heads or qkv.shape[3] != cpad(3 * C):
        raise ValueError(f"{name}: qkv of stride {qkv.shape[3]} for 3 x {C} channels in {num_heads} heads (expected stride {cpad(3 * C)})")
    if table.dtype != torch.float32 or not table.is_contiguous() or tuple(table.shape) != ((2 * ws - 1) ** 2, num_heads):
        raise ValueError(f"{name}: the bias table must be contiguous float32 [{(2 * ws - 1) ** 2}, {num_heads}], got {tuple(table.shape)} {table.dtype}")
    return qkv


def winattn_fwd(qkv, table, C, num_heads, ws, shift, scale):
    """the (shifted-)window attention core on the token grid: qkv [B,H,W,cpad(3C)] (channel = (q|k|v)*C + head*hd + d) -> (out [B,H,W,cpad(C)],
    lse f32 [B,nH,H,W]).  Roll, window partition, head split, bias gather, mask, softmax and their reverses are one launch"""
    qkv = _winattn_args("winattn_fwd", qkv, table, C, num_heads, ws)
    B, H, W, CP3 = qkv.shape
    out = torch.empty(B, H, W, cpad(C), device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty(B, num_heads, H, W, device=qkv.device, dtype=torch.float32)
    _lib.checked().wm_winattn_fwd(_p(qkv), _p(table), _p(out), _p(lse), B, H, W, C, num_heads, ws, shift, float(scale), CP3, cpad(C), dt_id(qkv.dtype),
                                  _stream())
    return out, lse


def winattn_bwd(g_out, qkv, table, lse, C, num_heads, ws, shift, scale):
    """(g_qkv [B,H,W,cpad(3C)], g_table f32 [(2ws-1)^2, nH]) of winattn_fwd; the probabilities are recomputed from qkv and lse.  g_table is
    summed from per-workgroup partial tables in a fixed order: two calls give the same bits"""
    qkv = _winattn_args("winattn_bwd", qkv, table, C, num_heads, ws)
    _need_cuda(g_out, lse)
    g_out = g_out.contiguous()
    B, H, W, CP3 = qkv.shape
    if tuple(g_out.shape) != (B, H, W, cpad(C)) or g_out.dtype != qkv.dtype:
        raise ValueError("winattn_bwd: the output gradient does not match the forward's output")
    L = _lib.checked()
    g_qkv = torch.empty_like(qkv)
    g_table = torch.empty_like(table)
    scratch = torch.empty(L.wm_winattn_scratch_floats(B, H, W, num_heads, ws), device=qkv.device, dtype=torch.float32)
    L.wm_winattn_bwd(_p(g_out), _p(qkv), _p(table), _p(lse), _p(g_qkv), _p(g_table), _p(scratch), B, H, W, C, num_heads, ws, shift, float(scale),
                     CP3, cpad(C), dt_id(qkv.dtype), _stream())
    return g_qkv, g_table


# ----------------------------------------------------------------------------- losses of the literal IRNrhi step
def _nparts(n):
    return max(1, min(1024, (n + 4095) // 4096))


def smooth_l1(a, b, beta=1.0, want_grad=True):
    """nn.SmoothL1Loss()(a, b) -> (loss [1] device scalar, d loss / d a or None)"""
    _need_cuda(a, b)
    a, b = a.contiguous().float(), b.contiguous().float()
    if a.shape != b.shape:
        raise ValueError("smooth_l1: shapes disagree")
    n = a.numel()
    part = torch.empty(_nparts(n), device=a.device, dtype=torch.float32)
    loss = torch.empty(1, device=a.device, dtype=torch.float32)
    grad = torch.empty_like(a) if want_grad else None
    _lib.checked().wm_smooth_l1(_p(a), _p(b), n, beta, _p(part), part.numel(), _p(loss), _p(grad), _stream())
    return loss, grad


def bce_prob(p, target, want_grad=True):
    """nn.BCELoss()(p, full_like(p, target)) -> (loss [1], d loss / d p or None)"""
    _need_cuda(p)
    p = p.contiguous().float()
    n = p.numel()
    part = torch.empty(_nparts(n), device=p.device, dtype=torch.float32)
    loss = torch.empty(1, device=p.device, dtype=torch.float32)
    grad = torch.empty_like(p) if want_grad else None
    _lib.checked().wm_bce_prob(_p(p), target, n, _p(part), part.numel(), _p(loss), _p(grad), _stream())
    return loss, grad


def cross_entropy(logits, labels, want_grad=True):
    """nn.CrossEntropyLoss()(logits [B,K] f32, labels [B] int64) -> (loss [1], d loss / d logits or None)"""
    _need_cuda(logits, labels)
    logits = logits.contiguous().float()
    labels = labels.contiguous()
    if logits.dim() != 2 or labels.dtype != torch.int64 or labels.numel() != logits.shape[0]:
        raise ValueError("cross_entropy: logits [B,K] f32 and labels [B] int64 expected")
    B, K = logits.shape
    loss = torch.empty(1, device=logits.device, dtype=torch.float32)
    grad = torch.empty_like(logits) if want_grad else None
    _lib.checked().wm_cross_entropy(_p(logits), _p(labels), B, K, K, _p(loss), _p(grad), _stream())
    return loss, grad


def clamp01_fwd(x):
    _need_cuda(x)
    x = x.contiguous().float()
    y = torch.empty_like(x)
    _lib.checked().wm_clamp01_fwd(_p(x), _p(y), x.numel(), _stream())
    return y


def clamp01_bwd(x, g):
    _need_cuda(x, g)
    if x.shape != g.shape:
        raise ValueError(f"clamp01_bwd: x {tuple(x.shape)} and g {tuple(g.shape)} disagree")
    x = x.contiguous().float()          # (the kernel walks both flat: a view's storage is not its elements)
    g = g.contiguous().float()
    gx = torch.empty_like(g)
    _lib.checked().wm_clamp01_bwd(_p(x), _p(g), _p(gx), g.numel(), _stream())
    return gx


def psnr255(a, b):
    """PSNR of int(255 a) against int(255 b) (metrics.py:30-46 on postprocess()ed images) -> [1] device scalar (0 when equal)"""
    _need_cuda(a, b)
    a, b = a.contiguous().float(), b.contiguous().float()
    n = a.numel()
    part = torch.empty(_nparts(n), device=a.device, dtype=torch.float64)
    _lib.checked().wm_psnr255_partials(_p(a), _p(b), n, _p(part), part.numel(), _stream())
    return psnr_gate(part, n)[0:1]


# ----------------------------------------------------------------------------- image-quality and mask metrics (csrc/ssim.hip)
_SSIM_WIN = None


def ssim_window():
    """the 11 taps of the reference's window (pytorch_ssim/__init__.py:7-9): Gaussian, sigma 1.5, gauss / gauss.sum() evaluated in float32"""
    global _SSIM_WIN
    if _SSIM_WIN is None:
        import math
        g = torch.tensor([math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
        _SSIM_WIN = _host_floats((g / g.sum()).tolist())
    return _SSIM_WIN


def _ssim_args(a, b):
    _need_cuda(a, b)
    if a.dim() != 4 or a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError("ssim: two float32 [B,C,H,W] images of one shape expected")
    return a.contiguous(), b.contiguous()


def ssim(a, b, size_average=True, want_grad=False):
    """pytorch_ssim._ssim(a, b) with the 11 x 11 window: a 0-dim device tensor (size_average) or the [B] per-image means, no host sync.
    want_grad: -> (value, dplanes [3,B,C,H,W]), the derivative planes ssim_bwd(dplanes, a, b, ...) turns into the gradient wrt a"""
    a, b = _ssim_args(a, b)
    B, C, H, W = a.shape
    L = _lib.checked()
    part = torch.empty(B * L.wm_ssim_nparts(C, H, W), device=a.device, dtype=torch.float64)
    dpl = torch.empty((3,) + tuple(a.shape), device=a.device, dtype=torch.float32) if want_grad else None
    out = torch.empty(1 + B, device=a.device, dtype=torch.float32)
    _timed("ssim_fwd", None, lambda: L.wm_ssim_fwd(_p(a), _p(b), B, C, H, W, ssim_window(), _p(part), _p(dpl), _stream()))
    L.wm_ssim_finalize(_p(part), B, C, H, W, _p(out), _stream())
    val = out[0] if size_average else out[1:]
    return (val, dpl) if want_grad else val


def ssim_bwd(dplanes, a, b, gout=None, per_image=False, gscale=1.0, gscale_dev=None, out=None, accumulate=False):
    """gradient wrt a of gscale * gscale_dev[0] * sum(gout * ssim(a, b)), from the planes ssim(a, b, want_grad=True) wrote.  gout: device
    f32, one element (the mean's upstream gradient) or [B] with per_image (size_average=False); None = 1.  out: the buffer to write, or
    with accumulate to add into (one launch, no axpy)"""
    a, b = _ssim_args(a, b)
    _need_cuda(dplanes)
    B, C, H, W = a.shape
    assert dplanes.shape == (3,) + tuple(a.shape) and dplanes.is_contiguous() and dplanes.dtype == torch.float32
    gout, out = _loss_bwd_args("ssim_bwd", a, gout, gscale_dev, out, accumulate, B if per_image else 1)
    _timed("ssim_bwd", None, lambda: _lib.checked().wm_ssim_bwd(_p(dplanes), _p(a), _p(b), _p(out), B, C, H, W, ssim_window(), _p(gout),
                                                                1 if per_image else 0, gscale, _p(gscale_dev), 1 if accumulate else 0, _stream()))
    _wrote(out)
    return out


def psnr(a, b, max_val):
    """metrics.PSNR(max_val)(a, b) on float images -> [1] device scalar (0 when equal), no host sync"""
    _need_cuda(a, b)
    a, b = a.contiguous().float(), b.contiguous().float()
    if a.shape != b.shape:
        raise ValueError("psnr: shapes disagree")
    n = a.numel()
    part = torch.empty(_nparts(n), device=a.device, dtype=torch.float64)
    out = torch.empty(1, device=a.device, dtype=torch.float32)
    L = _lib.checked()
    _timed("psnr", None, lambda: L.wm_psnr_partials(_p(a), _p(b), n, _p(part), part.numel(), _stream()))
    L.wm_psnr_finalize(_p(part), part.numel(), float(n), float(max_val), _p(out), _stream())
    return out


def confusion_counts(pred, gt, thr_pred, thr_gt):
    """pred, gt: masks [B, ...] (float32 or uint8) of one shape -> int64 [1 + B, 4] device tensor: row 0 the totals, row 1 + b image b's
    (TN, TP, FN, FP) of pred > thr_pred against gt > thr_gt (calculate_f1.py:5-20), exact"""
    _need_cuda(pred, gt)
    if pred.shape != gt.shape or pred.dim() < 1 or pred.numel() == 0:
        raise ValueError("confusion_counts: two non-empty masks of one shape expected")
    for t in (pred, gt):
        if t.dtype not in (torch.float32, torch.uint8):
            raise TypeError("confusion_counts: float32 or uint8 masks")
    pred, gt = pred.contiguous(), gt.contiguous()
    B = pred.shape[0]
    per = pred.numel() // B
    L = _lib.checked()
    part = torch.empty(B * L.wm_confusion_nparts(per) * 4, device=pred.device, dtype=torch.int64)
    out = torch.empty(1 + B, 4, device=pred.device, dtype=torch.int64)
    _timed("confusion_counts", None, lambda: L.wm_confusion_counts(_p(pred), int(pred.dtype == torch.uint8), _p(gt), int(gt.dtype == torch.uint8),
                                                                   thr_pred, thr_gt, B, per, _p(part), _p(out), _stream()))
    return out


def scale_dev_(x, scale_dev):
    """x *= scale_dev[0] (a device scalar)"""
    _need_cuda(x, scale_dev)
    assert x.is_contiguous() and x.dtype == torch.float32 and scale_dev.dtype == torch.float32
    _lib.checked().wm_scale_dev(_p(x), x.numel(), _p(scale_dev), _stream())
    _wrote(x)
    return x


def _loss_bwd_args(name, x, gout, gscale_dev, out, accumulate, n_gout=1, same_shape=True):
    """(gout contiguous, the gradient buffer) of a loss backward.  n_gout: the elements gout must have; same_shape: a given buffer must have
    x's shape (False: x's size -- the Dice backwards take any view of it)"""
    _need_cuda(gout, gscale_dev, out)
    if gout is not None:
        gout = gout.contiguous()
        assert gout.dtype == torch.float32 and gout.numel() == n_gout
    if out is None:
        if accumulate:
            raise ValueError(name + ": accumulate needs the buffer to add into (out=)")
        out = torch.empty_like(x)
    assert (out.shape == x.shape if same_shape else out.numel() == x.numel()) and out.is_contiguous() and out.dtype == torch.float32
    return gout, out


def _loss_bwd_args2(name, xs, want, out, gout, gscale_dev, accumulate):
    """_loss_bwd_args of a loss with two inputs xs: (gout contiguous, [the gradient buffer of each side that want names, None for the other])"""
    g = []
    for x, w, o in zip(xs, want, out):
        if w:
            gout, o = _loss_bwd_args(name, x, gout, gscale_dev, o, accumulate)
        g.append(o if w else None)
    return gout, g


# ----------------------------------------------------------------------------- Dice loss (csrc/dice.hip)
DICE_REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}    # WM_DICE_MEAN / WM_DICE_SUM / WM_DICE_NONE


def _dice_reduction(reduction):
    try:
        return DICE_REDUCTIONS[reduction]
    except (KeyError, TypeError):
        raise Exception('Unexpected reduction {}'.format(reduction)) from None   # the reference's exception (dice_loss.py:61)


def _dice_pair(name, a, b):
    _need_cuda(a, b)
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise TypeError(name + ": float32 tensors expected")
    return a.contiguous(), b.contiguous()


def _dice_finalize(L, part, B, C, per, smooth, red, ignore_index, weight, device):
    coef = torch.empty(B * C, 2, device=device, dtype=torch.float64)
    loss = torch.empty(B if red == DICE_REDUCTIONS["none"] else 1, device=device, dtype=torch.float32)
    L.wm_dice_finalize(_p(part), B, C, per, float(smooth), red, -1 if ignore_index is None else int(ignore_index), _p(weight), _p(coef),
                       _p(loss), _stream())
    return loss, coef


def dice_binary_fwd(p, target, smooth=1.0, pw=2.0, reduction="mean"):
    """BinaryDiceLoss(smooth, pw, reduction)(p, target) for float32 [B, ...] tensors -> (loss, coef): loss a [1] device tensor (mean, sum) or
    [B] (none); coef [B,2] float64 = (num, den) per sample, what dice_binary_bwd reads.  Two launches, no host sync"""
    red = _dice_reduction(reduction)
    p, target = _dice_pair("dice_binary", p, target)
    B = p.shape[0]
    if B == 0 or p.numel() != target.numel() or p.numel() == 0:
        raise ValueError("dice_binary: two non-empty tensors of one size expected")
    per = p.numel() // B
    L = _lib.checked()
    part = torch.empty(B * L.wm_dice_nparts(per) * 3, device=p.device, dtype=torch.float64)
    _timed("dice_sums", None, lambda: L.wm_dice_sums(_p(p), _p(target), B, per, float(pw), _p(part), _stream()))
    return _dice_finalize(L, part, B, 1, per, smooth, red, None, None, p.device)


def dice_binary_bwd(p, target, coef, pw=2.0, reduction="mean", gout=None, gscale=1.0, gscale_dev=None, chain_sigmoid=False, out=None,
                    accumulate=False):
    """gradient wrt p of gscale * gscale_dev[0] * sum(gout * loss) from the coef dice_binary_fwd wrote; chain_sigmoid: p is a sigmoid
    output s(z) and the gradient is wrt z.  gout: device f32, one element or [B] with reduction none; None = 1.  out: the buffer to write,
    or with accumulate to add into (one launch, no axpy)"""
    red = _dice_reduction(reduction)
    p, target = _dice_pair("dice_binary_bwd", p, target)
    B = p.shape[0]
    gout, out = _loss_bwd_args("dice_binary_bwd", p, gout, gscale_dev, out, accumulate, B if red == DICE_REDUCTIONS["none"] else 1, same_shape=False)
    _timed("dice_bwd", None, lambda: _lib.checked().wm_dice_bwd(_p(p), _p(target), _p(coef), _p(out), B, p.numel() // B, float(pw), red, _p(gout),
                                                                gscale, _p(gscale_dev), 1 if chain_sigmoid else 0, 1 if accumulate else 0, _stream()))
    _wrote(out)
    return out


def dice_binary(p, target, smooth=1.0, pw=2.0, reduction="mean", want_grad=True, chain_sigmoid=False, gscale=1.0, gscale_dev=None, grad_out=None):
    """the binary Dice loss and its gradient: (loss, grad or None), loss UNSCALED, grad = gscale * gscale_dev[0] * d loss / d p (wrt the
    pre-sigmoid input with chain_sigmoid).  grad_out: an existing gradient buffer of p's size the result is ADDED into (and returned)"""
    loss, coef = dice_binary_fwd(p, target, smooth, pw, reduction)
    if not want_grad:
        return loss, None
    return loss, dice_binary_bwd(p, target, coef, pw, reduction, None, gscale, gscale_dev, chain_sigmoid, grad_out, grad_out is not None)


def _dice_softmax_args(logits, target, weight):
    logits, target = _dice_pair("dice_softmax", logits, target)
    if logits.dim() < 2 or logits.shape != target.shape or logits.numel() == 0:
        raise ValueError("dice_softmax: two non-empty float32 [B,C,...] tensors of one shape expected")
    B, C = logits.shape[0], logits.shape[1]
    if weight is not None:
        _need_cuda(weight)
        weight = weight.contiguous()
        assert weight.dtype == torch.float32 and weight.numel() == C
    return logits, target, weight, B, C, logits.numel() // (B * C)


def dice_softmax_fwd(logits, target, smooth=1.0, pw=2.0, reduction="mean", ignore_index=None, weight=None):
    """DiceLoss(weight, ignore_index, smooth=, p=, reduction=)(logits, target) on float32 [B,C,...] logits and one-hot targets, C <= 32 ->
    (loss, coef [B*C,2] float64).  The softmax over the classes is formed inside the kernel and never written"""
    red = _dice_reduction(reduction)
    logits, target, weight, B, C, HW = _dice_softmax_args(logits, target, weight)
    L = _lib.checked()
    part = torch.empty(B * C * L.wm_dice_nparts(HW) * 3, device=logits.device, dtype=torch.float64)
    _timed("dice_softmax_sums", None, lambda: L.wm_dice_softmax_sums(_p(logits), _p(target), B, C, HW, float(pw), _p(part), _stream()))
    return _dice_finalize(L, part, B, C, HW, smooth, red, ignore_index, weight, logits.device)


def dice_softmax_bwd(logits, target, coef, pw=2.0, reduction="mean", ignore_index=None, weight=None, gout=None, gscale=1.0, gscale_dev=None,
                     out=None, accumulate=False):
    """gradient wrt the logits of gscale * gscale_dev[0] * sum(gout * loss), from the coef dice_softmax_fwd wrote (same ignore_index, weight)"""
    red = _dice_reduction(reduction)
    logits, target, weight, B, C, HW = _dice_softmax_args(logits, target, weight)
    gout, out = _loss_bwd_args("dice_softmax_bwd", logits, gout, gscale_dev, out, accumulate, B if red == DICE_REDUCTIONS["none"] else 1, same_shape=False)
    _timed("dice_softmax_bwd", None, lambda: _lib.checked().wm_dice_softmax_bwd(
        _p(logits), _p(target), _p(coef), _p(out), B, C, HW, float(pw), red, -1 if ignore_index is None else int(ignore_index), _p(weight), _p(gout),
        gscale, _p(gscale_dev), 1 if accumulate else 0, _stream()))
    _wrote(out)
    return out


def dice_softmax(logits, target, smooth=1.0, pw=2.0, reduction="mean", want_grad=True, ignore_index=None, weight=None, gscale=1.0,
                 gscale_dev=None, grad_out=None):
    """the multi-class Dice loss and its gradient wrt the logits: (loss, grad or None), as dice_binary"""
    loss, coef = dice_softmax_fwd(logits, target, smooth, pw, reduction, ignore_index, weight)
    if not want_grad:
        return loss, None
    return loss, dice_softmax_bwd(logits, target, coef, pw, reduction, ignore_index, weight, None, gscale, gscale_dev, grad_out, grad_out is not None)


# ----------------------------------------------------------------------------- pixel- and gradient-domain image losses (csrc/imgloss.hip)
RECON_KINDS = {"l2": 0, "l_char": 1, "l1": 2}    # WM_RECON_L2 / WM_RECON_LCHAR / WM_RECON_L1


def _f32_cuda(name, *ts):
    _need_cuda(*ts)
    for t in ts:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError(name + ": contiguous float32 tensors expected")


def _recon_args(name, x, t, kind):
    if kind not in RECON_KINDS:
        raise ValueError("%s: kind must be one of %s, got %r" % (name, ", ".join(RECON_KINDS), kind))
    _f32_cuda(name, x, t)
    if x.dim() < 1 or x.shape != t.shape or x.numel() == 0:
        raise ValueError(name + ": two non-empty tensors of one shape expected")
    return x.shape[0], x.numel() // x.shape[0], RECON_KINDS[kind]


def recon_loss_fwd(x, t, kind="l_char", eps=1e-6):
    """ReconstructionLoss(eps=eps)(x, t, kind): mean over the batch of the per-sample SUM of f(x - t), f = d^2 (l2), sqrt(d^2 + eps)
    (l_char) or d (l1: the reference's signed sum, without abs) -> a [1] device tensor.  Two launches, no host sync"""
    B, per, k = _recon_args("recon_loss", x, t, kind)
    L = _lib.checked()
    part = torch.empty(B * L.wm_recon_nparts(per), device=x.device, dtype=torch.float64)
    loss = torch.empty(1, device=x.device, dtype=torch.float32)
    _timed("recon_sums", None, lambda: L.wm_recon_sums(_p(x), _p(t), B, per, k, float(eps), _p(part), _stream()))
    L.wm_recon_finalize(_p(part), B, per, _p(loss), _stream())
    return loss


def recon_loss_bwd(x, t, kind="l_char", eps=1e-6, gout=None, gscale=1.0, gscale_dev=None, out=None, accumulate=False):
    """gradient wrt x of gscale * gscale_dev[0] * gout[0] * recon_loss(x, t); a negative gscale gives the gradient wrt t.  out: the buffer to
    write, or with accumulate to add into (one launch, no axpy)"""
    B, per, k = _recon_args("recon_loss_bwd", x, t, kind)
    gout, out = _loss_bwd_args("recon_loss_bwd", x, gout, gscale_dev, out, accumulate)
    _timed("recon_bwd", None, lambda: _lib.checked().wm_recon_bwd(_p(x), _p(t), _p(out), B, per, k, float(eps), _p(gout), gscale, _p(gscale_dev),
                                                                  1 if accumulate else 0, _stream()))
    _wrote(out)
    return out


def recon_loss(x, t, kind="l_char", eps=1e-6, want_grad=False, gscale=1.0, gscale_dev=None, grad_out=None):
    """the reconstruction loss, and with want_grad its gradient wrt x: a [1] device tensor, or (loss, grad) with loss UNSCALED and
    grad = gscale * gscale_dev[0] * d loss / dx.  grad_out: an existing gradient buffer the result is ADDED into (and returned)"""
    loss = recon_loss_fwd(x, t, kind, eps)
    if not want_grad:
        return loss
    return loss, recon_loss_bwd(x, t, kind, eps, None, gscale, gscale_dev, grad_out, grad_out is not None)


def _gradloss_args(name, a):
    _f32_cuda(name, a)
    if a.dim() != 4 or a.numel() == 0:
        raise ValueError(name + ": a non-empty [B,C,H,W] tensor expected")
    return a.shape[0] * a.shape[1], a.shape[2], a.shape[3]


def gradient_loss(a):
    """GradientLoss()(a): mean |a[..., :-1] - a[..., 1:]| + mean |a[..., :-1, :] - a[..., 1:, :]| -> a [1] device tensor; H, W >= 2"""
    N, H, W = _gradloss_args("gradient_loss", a)
    L = _lib.checked()
    part = torch.empty(N * max(1, L.wm_gradloss_nparts(H, W)) * 2, device=a.device, dtype=torch.float64)
    loss = torch.empty(1, device=a.device, dtype=torch.float32)
    _timed("gradloss_sums", None, lambda: L.wm_gradloss_sums(_p(a), N, H, W, _p(part), _stream()))
    L.wm_gradloss_finalize(_p(part), N, H, W, _p(loss), _stream())
    return loss


def gradient_loss_bwd(a, gout=None, gscale=1.0, gscale_dev=None, out=None, accumulate=False):
    """gradient wrt a of gscale * gscale_dev[0] * gout[0] * gradient_loss(a); the subgradient of |.| at 0 is 0, as torch's"""
    N, H, W = _gradloss_args("gradient_loss_bwd", a)
    gout, out = _loss_bwd_args("gradient_loss_bwd", a, gout, gscale_dev, out, accumulate)
    _timed("gradloss_bwd", None, lambda: _lib.checked().wm_gradloss_bwd(_p(a), _p(out), N, H, W, _p(gout), gscale, _p(gscale_dev),
                                                                        1 if accumulate else 0, _stream()))
    _wrote(out)
    return out


def _excl_args(name, img1, img2, level):
    _f32_cuda(name, img1, img2)
    if img1.dim() != 4 or img2.dim() != 4 or img1.shape[0] != img2.shape[0] or img1.shape[2:] != img2.shape[2:] or img1.numel() == 0:
        raise ValueError(name + ": two non-empty [B,C,H,W] tensors of one batch and image size expected")
    return img1.shape[0], img1.shape[1], img2.shape[1], img1.shape[2], img1.shape[3], int(level)


def exclusion_fwd(img1, img2, level=3):
    """ExclusionLoss(level)(img1, img2) -> (loss [1] f32, means [level, 2, C1*C2] f64, coef [level, 2, C1*C2] f64 -- what exclusion_bwd reads).
    means[l, d, i2*C1 + i1] = mean of s1^2 s2^2 over level l's differences in direction d (0 = gradx, 1 = grady) of img1's channel i1 and
    img2's i2.  1 <= level <= 3, 1 <= C1, C2 <= 4, H and W >= 2 << (level - 1) (the library refuses anything else).  Two launches, no host sync"""
    B, C1, C2, H, W, level = _excl_args("exclusion", img1, img2, level)
    L = _lib.checked()
    n = max(1, level) * 2 * C1 * C2
    part = torch.empty(n * max(1, L.wm_excl_nparts(B, H, W)), device=img1.device, dtype=torch.float64)
    _timed("excl_fwd", None, lambda: L.wm_excl_fwd(_p(img1), _p(img2), B, C1, C2, H, W, level, _p(part), _stream()))
    means = torch.empty(level, 2, C1 * C2, device=img1.device, dtype=torch.float64)
    coef = torch.empty_like(means)
    loss = torch.empty(1, device=img1.device, dtype=torch.float32)
    L.wm_excl_finalize(_p(part), B, C1, C2, H, W, level, _p(means), _p(coef), _p(loss), _stream())
    return loss, means, coef


def exclusion(img1, img2, level=3, want_terms=False):
    """the exclusion loss as a [1] device tensor; want_terms: (loss, the [level, 2, C1*C2] float64 means under the fourth roots)"""
    loss, means, _ = exclusion_fwd(img1, img2, level)
    return (loss, means) if want_terms else loss


def exclusion_bwd(img1, img2, coef, level=3, want=(True, True), gout=None, gscale=1.0, gscale_dev=None, out=(None, None), accumulate=False):
    """gradients of gscale * gscale_dev[0] * gout[0] * exclusion(img1, img2, level) from the coef exclusion_fwd wrote -> (grad1, grad2), None
    where want[i] is false.  out: buffers to write, or with accumulate to add into.  One launch.  A term whose mean is exactly 0 (a constant
    image) contributes a zero gradient (the reference: NaN)"""
    B, C1, C2, H, W, level = _excl_args("exclusion_bwd", img1, img2, level)
    if not (want[0] or want[1]):
        return None, None
    _need_cuda(coef)
    assert coef.dtype == torch.float64 and coef.is_contiguous() and coef.numel() == level * 2 * C1 * C2
    gout, g = _loss_bwd_args2("exclusion_bwd", (img1, img2), want, out, gout, gscale_dev, accumulate)
    _timed("excl_bwd", None, lambda: _lib.checked().wm_excl_bwd(_p(img1), _p(img2), _p(coef), _p(g[0]), _p(g[1]), B, C1, C2, H, W, level, _p(gout),
                                                                gscale, _p(gscale_dev), 1 if accumulate else 0, _stream()))
    _wrote(*g)
    return g[0], g[1]


# ----------------------------------------------------------------------------- local structure loss, mask and gray losses (csrc/ssim3.hip)
def _ssim3_args(name, x, y):
    _f32_cuda(name, x, y)
    if x.dim() != 4 or x.shape != y.shape or x.numel() == 0:
        raise ValueError(name + ": two non-empty [B,C,H,W] tensors of one shape expected")
    if x.shape[2] < 2 or x.shape[3] < 2:
        raise ValueError(name + ": H and W must be at least 2 (the reflection padding needs two pixels)")
    return x.shape[0] * x.shape[1], x.shape[2], x.shape[3]


def ssim3_map_fwd(x, y):
    """SSIM_Loss()(x, y): the [B,C,H,W] map clamp((1 - SSIM_n / SSIM_d) / 2, 0, 1) from reflect-padded 3 x 3 box statistics.  One launch"""
    N, H, W = _ssim3_args("ssim3_map_fwd", x, y)
    out = torch.empty_like(x)
    _timed("ssim3_fwd", None, lambda: _lib.checked().wm_ssim3_fwd(_p(x), _p(y), _p(out), None, N, H, W, _stream()))
    return out


def _ssim3_bwd(name, x, y, g, want, gout, gscale, gscale_dev, out, accumulate):
    N, H, W = _ssim3_args(name, x, y)
    if not (want[0] or want[1]):
        return None, None
    gout, res = _loss_bwd_args2(name, (x, y), want, out, gout, gscale_dev, accumulate)
    _timed("ssim3_bwd", None, lambda: _lib.checked().wm_ssim3_bwd(_p(x), _p(y), _p(g), _p(res[0]), _p(res[1]), N, H, W, _p(gout), gscale,
                                                                  _p(gscale_dev), 1 if accumulate else 0, _stream()))
    _wrote(*res)
    return res[0], res[1]


def ssim3_map_bwd(x, y, g, want=(True, True), gscale=1.0, gscale_dev=None, out=(None, None), accumulate=False):
    """gradients wrt x and y of gscale * gscale_dev[0] * sum(g * ssim3_map_fwd(x, y)) for an upstream map g of x's shape -> (gx, gy), None where
    want[i] is false.  The clamp passes the gradient where the unclamped value lies in [0, 1], bounds included (torch.clamp).  One launch"""
    _f32_cuda("ssim3_map_bwd", g)
    if g.shape != x.shape:
        raise ValueError("ssim3_map_bwd: the upstream gradient must have the inputs' shape")
    return _ssim3_bwd("ssim3_map_bwd", x, y, g, want, None, gscale, gscale_dev, out, accumulate)


def ssim3_mean_fwd(x, y):
    """mean(SSIM_Loss()(x, y)) -> a [1] device tensor; the map is never written.  Two launches, no host sync"""
    N, H, W = _ssim3_args("ssim3_mean", x, y)
    L = _lib.checked()
    part = torch.empty(max(1, L.wm_ssim3_nparts(N, H, W)), device=x.device, dtype=torch.float64)
    loss = torch.empty(1, device=x.device, dtype=torch.float32)
    _timed("ssim3_fwd", None, lambda: L.wm_ssim3_fwd(_p(x), _p(y), None, _p(part), N, H, W, _stream()))
    L.wm_ssim3_finalize(_p(part), N, H, W, _p(loss), _stream())
    return loss


def ssim3_mean_bwd(x, y, want=(True, False), gout=None, gscale=1.0, gscale_dev=None, out=(None, None), accumulate=False):
    """gradients wrt x and y of gscale * gscale_dev[0] * gout[0] * mean(SSIM_Loss()(x, y)) -> (gx, gy).  One launch, the kernel of
    ssim3_map_bwd with one weight for every pixel"""
    return _ssim3_bwd("ssim3_mean_bwd", x, y, None, want, gout, gscale, gscale_dev, out, accumulate)


def ssim3_mean(x, y, want_grad=False, gscale=1.0, gscale_dev=None, grad_out=None):
    """mean(SSIM_Loss()(x, y)) as a [1] device tensor, and with want_grad its gradient wrt x: (loss, grad) with loss UNSCALED and
    grad = gscale * gscale_dev[0] * d loss / dx.  grad_out: an existing gradient buffer the result is ADDED into (and returned)"""
    loss = ssim3_mean_fwd(x, y)
    if not want_grad:
        return loss
    return loss, ssim3_mean_bwd(x, y, (True, False), None, gscale, gscale_dev, (grad_out, None), grad_out is not None)[0]


PIXLOSS_KINDS = {"masked_l1": 0, "non_blurry": 1, "gray": 2}    # WM_PIXLOSS_MASKL1 / NONBLURRY / GRAY


def _pixloss_fwd(name, kind, a, b=None, mask=None):
    _f32_cuda(name, a, b, mask)
    if a.numel() == 0 or any(t is not None and t.shape != a.shape for t in (b, mask)):
        raise ValueError(name + ": non-empty tensors of one shape expected")
    L, n = _lib.checked(), a.numel()
    part = torch.empty(2 * L.wm_pixloss_nparts(n), device=a.device, dtype=torch.float64)
    coef = torch.empty(2, device=a.device, dtype=torch.float64)
    loss = torch.empty(1, device=a.device, dtype=torch.float32)
    k = PIXLOSS_KINDS[kind]
    _timed("pixloss_sums", None, lambda: L.wm_pixloss_sums(k, _p(a), _p(b), _p(mask), n, _p(part), _stream()))
    L.wm_pixloss_finalize(k, _p(part), n, _p(coef), _p(loss), _stream())
    return loss, coef


def _pixloss_bwd(name, kind, a, b, mask, coef, want, gout, gscale, gscale_dev, accumulate, out):
    _f32_cuda(name, a, b, mask)
    _need_cuda(coef)
    assert coef.dtype == torch.float64 and coef.is_contiguous() and coef.numel() == 2
    gout, res = _loss_bwd_args2(name, (a, a), want, out, gout, gscale_dev, accumulate)
    if res[0] is None and res[1] is None:
        return None, None
    _timed("pixloss_bwd", None, lambda: _lib.checked().wm_pixloss_bwd(PIXLOSS_KINDS[kind], _p(a), _p(b), _p(mask), _p(coef), _p(res[0]), _p(res[1]),
                                                                      a.numel(), _p(gout), gscale, _p(gscale_dev), 1 if accumulate else 0, _stream()))
    _wrote(*res)
    return res[0], res[1]


def extended_l1_fwd(a, b, mask):
    """ExtendedL1Loss()(a, b, mask) = mean |mask*a - mask*b| / mean |mask| -> (loss [1] f32, coef [2] f64 -- what extended_l1_bwd reads).
    Three tensors of one shape.  A zero mask gives NaN (0 / 0), as the reference: unguarded.  Two launches, no host sync"""
    return _pixloss_fwd("extended_l1", "masked_l1", a, b, mask)


def extended_l1_bwd(a, b, mask, coef, want=(True, True), gout=None, gscale=1.0, gscale_dev=None, out=(None, None), accumulate=False):
    """gradients wrt a and b of gscale * gscale_dev[0] * gout[0] * extended_l1 -> (ga, gb); sign(0) = 0, as torch's L1Loss.  One launch"""
    return _pixloss_bwd("extended_l1_bwd", "masked_l1", a, b, mask, coef, want, gout, gscale, gscale_dev, accumulate, out)


def non_blurry_fwd(x):
    """NonBlurryLoss()(x) = 1 - mean (x - 1/2)^2 -> (loss [1] f32, coef [2] f64)"""
    return _pixloss_fwd("non_blurry", "non_blurry", x)


def non_blurry_bwd(x, coef, gout=None, gscale=1.0, gscale_dev=None, out=None, accumulate=False):
    return _pixloss_bwd("non_blurry_bwd", "non_blurry", x, None, None, coef, (True, False), gout, gscale, gscale_dev, accumulate, (out, None))[0]


def gray_loss_fwd(x):
    """GrayLoss()(x) = 1 / mean |x - 1/2| -> (loss [1] f32, coef [2] f64 -- coef[0] is the mean gray_loss_bwd reads)"""
    return _pixloss_fwd("gray_loss", "gray", x)


def gray_loss_bwd(x, coef, gout=None, gscale=1.0, gscale_dev=None, out=None, accumulate=False):
    return _pixloss_bwd("gray_loss_bwd", "gray", x, None, None, coef, (True, False), gout, gscale, gscale_dev, accumulate, (out, None))[0]


# ----------------------------------------------------------------------------- GAN objectives (csrc/advloss.hip)
ADV_OBJECTIVES = {"bce_prob": 0, "bce_logits": 1, "mse": 2, "hinge_disc": 3, "neg_mean": 4, "pos_mean": 5}    # WM_ADV_*
_ADV_LABELLED = ("bce_prob", "bce_logits", "mse")


def _adv_args(name, x, objective, label, mask):
    if objective not in ADV_OBJECTIVES:
        raise ValueError("%s: objective must be one of %s, got %r" % (name, ", ".join(ADV_OBJECTIVES), objective))
    _f32_cuda(name, x, mask)
    if x.numel() == 0:
        raise ValueError(name + ": a non-empty tensor expected")
    dims = (0,) * 7
    if objective == "hinge_disc":
        if mask is not None or label is None or float(label) not in (-1.0, 1.0):
            raise ValueError(name + ": hinge_disc takes the sign of relu(1 + s x) as label: -1 (real) or +1 (fake), and no mask")
    elif objective not in _ADV_LABELLED:
        if label is not None or mask is not None:
            raise ValueError(name + ": %s takes neither a label nor a mask" % objective)
    elif mask is not None:
        if label is not None:
            raise ValueError(name + ": a scalar label or a mask, not both (the masked labels are real_label * (1 - mask))")
        if x.dim() != 4 or mask.dim() != 4 or mask.shape[0] != x.shape[0] or mask.shape[1] not in (1, x.shape[1]) or mask.numel() == 0:
            raise ValueError(name + ": masked labels need x [B,C,H,W] and mask [B,1,Hm,Wm] or [B,C,Hm,Wm]")
        dims = tuple(x.shape) + tuple(mask.shape[1:])
    elif label is None:
        raise ValueError(name + ": %s needs a scalar label or a mask" % objective)
    return ADV_OBJECTIVES[objective], 0.0 if label is None else float(label), dims


def adv_loss(x, objective, label=None, mask=None, real_label=1.0, want_grad=False, gscale=1.0, gscale_dev=None, grad_out=None, gout=None):
    """one GAN objective as a mean over every element of x (any shape) -> a [1] device tensor, or with want_grad (loss, grad) with loss
    UNSCALED and grad = gscale * gscale_dev[0] * gout[0] * d loss / dx, both from the SAME streaming launch (two launches in all, no host
    sync).  grad_out: an existing gradient buffer the result is ADDED into (and returned).  objective:
        bce_prob    nn.BCELoss()(x, t) on probabilities (AdversarialLoss nsgan): logs clamped at -100, backward over max(x (1 - x), 1e-12)
        bce_logits  nn.BCEWithLogitsLoss()(x, t) (GANLoss gan / ragan), any label value
        mse         (x - t)^2 (lsgan)
        hinge_disc  relu(1 + s x), s = label = -1 (real) or +1 (fake); the subgradient at 0 is 0
        neg_mean / pos_mean   -+mean(x) (the hinge generator term, wgan-gp); no label
    t is the scalar `label`, or with mask ([B,1,Hm,Wm] or [B,C,Hm,Wm], x [B,C,H,W]) the masked labels real_label * (1 - mask_down), mask_down
    the mask resized to x's H x W bilinearly (align_corners=False, no antialiasing) -- sampled inside the loss kernel, never written.  No
    gradient flows to the mask: it is data"""
    obj, lab, dims = _adv_args("adv_loss", x, objective, label, mask)
    L = _lib.checked()
    n = x.numel()
    part = torch.empty(L.wm_advloss_nparts(n), device=x.device, dtype=torch.float64)
    loss = torch.empty(1, device=x.device, dtype=torch.float32)
    grad = None
    if want_grad:
        gout, grad = _loss_bwd_args("adv_loss", x, gout, gscale_dev, grad_out, grad_out is not None)
    elif grad_out is not None or gout is not None:
        raise ValueError("adv_loss: grad_out / gout need want_grad=True")
    _timed("advloss_elem", None, lambda: L.wm_advloss_elem(obj, _p(x), n, lab, _p(mask), *dims, float(real_label), _p(part), _p(grad), _p(gout),
                                                           float(gscale), _p(gscale_dev), 1 if grad_out is not None else 0, _stream()))
    L.wm_advloss_finalize(_p(part), n, _p(loss), _stream())
    if not want_grad:
        return loss
    _wrote(grad)
    return loss, grad


def cw_margin(logits, target, is_targeted, kappa=0.0, want_grad=False, gscale=1.0, gscale_dev=None, grad_out=None, gout=None, check_target=False):
    """CWLoss()(logits, target, is_targeted, K, kappa): sum over the rows of max(other - real, kappa) (targeted) or max(real - other, kappa),
    real = logits[b, target_b], other = the largest of the row with the target's slot replaced by -10000 -> a [1] device tensor, or with
    want_grad (loss, grad [B,K]) as adv_loss.  Two launches, no host sync.  logits [B,K] float32, K >= 2; target [B] int64.
    A target outside [0, K) is checked ON THE DEVICE: it is never used as an index, and it turns the loss and that row of the gradient into
    NaN.  check_target=True validates on the host first (one synchronisation, so not inside a captured step) and raises ValueError"""
    _f32_cuda("cw_margin", logits)
    _need_cuda(target)
    if logits.dim() != 2 or logits.shape[0] == 0:
        raise ValueError("cw_margin: logits [B,K] expected")
    B, K = logits.shape
    if K < 2:
        raise ValueError("cw_margin: K >= 2 classes expected (with one class there is no other logit)")
    if target.dtype != torch.int64 or not target.is_contiguous() or target.shape != (B,):
        raise TypeError("cw_margin: target must be a contiguous int64 tensor [B]")
    if check_target and bool(((target < 0) | (target >= K)).any()):
        raise ValueError("cw_margin: target outside [0, %d)" % K)
    L = _lib.checked()
    terms = torch.empty(B, device=logits.device, dtype=torch.float64)
    loss = torch.empty(1, device=logits.device, dtype=torch.float32)
    grad = None
    if want_grad:
        gout, grad = _loss_bwd_args("cw_margin", logits, gout, gscale_dev, grad_out, grad_out is not None)
    elif grad_out is not None or gout is not None:
        raise ValueError("cw_margin: grad_out / gout need want_grad=True")
    _timed("cw_margin", None, lambda: L.wm_cw_margin(_p(logits), _p(target), B, K, 1 if is_targeted else 0, float(kappa), _p(terms), _p(loss),
                                                     _p(grad), _p(gout), float(gscale), _p(gscale_dev), 1 if grad_out is not None else 0,
                                                     _stream()))
    if not want_grad:
        return loss
    _wrote(grad)
    return loss, grad


# ----------------------------------------------------------------------------- device RNG and the stochastic / JPEG-Drop attacks (csrc/noise.hip,
# csrc/jpeg_drop.hip).  `state` is a layer's int64[RNG_STATE_WORDS] device tensor {seed, offset, ...}; a forward returns, beside its output,
# rec = int64[2] {seed, offset} of the call, from which the backward regenerates the same draws
RNG_STATE_WORDS = 4
RNG_UNIFORM, RNG_NORMAL = 0, 1
NOISE_DROP, NOISE_GAUSS, NOISE_GN, NOISE_SP = 0, 1, 2, 3


def rng_state(seed, device, offset=0):
    """a fresh generator state {seed, offset, 0, 0} on `device` (seed: a 64-bit integer, stored two's complement)"""
    seed = int(seed) & (2 ** 64 - 1)
    if seed >= 2 ** 63:
        seed -= 2 ** 64
    return torch.tensor([seed, int(offset), 0, 0], dtype=torch.int64).to(device)


def rng_fill(state, n, dist=RNG_UNIFORM):
    """the n draws a kernel consumes for element indices 0..n-1 at (state[0], state[1]); reads the state (or a rec) only"""
    _need_cuda(state)
    assert state.dtype == torch.int64 and state.numel() >= 2
    out = torch.empty(int(n), device=state.device, dtype=torch.float32)
    _lib.checked().wm_rng_fill(_p(state), _p(out), int(n), dist, _stream())
    return out


def _rng_args(x, state):
    _need_cuda(x, state)
    assert state.dtype == torch.int64 and state.numel() == RNG_STATE_WORDS and state.device == x.device
    rec = torch.empty(2, device=x.device, dtype=torch.int64)
    return rec


def noise_fwd(op, x, a, b, state, cover=None):
    """per-element attack (NOISE_DROP needs `cover`) -> (y, rec); advances `state` by one counter block in stream order"""
    _need_cuda(x, cover)
    x = x.contiguous().float()
    if cover is not None:
        cover = cover.contiguous().float()
        assert cover.shape == x.shape
    rec = _rng_args(x, state)
    y = torch.empty_like(x)
    _lib.checked().wm_noise_fwd(op, _p(x), _p(cover), _p(y), x.numel(), a, b, _p(state), _p(rec), _stream())
    _wrote(state)
    return y, rec


def noise_bwd(op, g, a, b, rec, x=None, want_cover=False):
    """-> (gradient wrt the image, gradient wrt the cover or None); x = the forward's input (NOISE_GAUSS)"""
    _need_cuda(g, rec, x)
    g = g.contiguous().float()
    if op == NOISE_GN:
        return g, None
    if x is not None:
        x = x.contiguous().float()
    gx = torch.empty_like(g)
    gc = torch.empty_like(g) if want_cover and op == NOISE_DROP else None
    _lib.checked().wm_noise_bwd(op, _p(x), _p(g), _p(gx), _p(gc), g.numel(), a, b, _p(rec), _stream())
    return gx, gc


def dropout_fwd(x, cover, keep_min, keep_span, state):
    """dropout.Dropout: one keep mask over H x W shared by every plane -> (y, rec); advances `state` by two counter blocks"""
    _need_cuda(cover)
    x, N, H, W = _planes(x)
    cover = cover.contiguous().float()
    assert cover.shape == x.shape
    rec = _rng_args(x, state)
    y = torch.empty_like(x)
    _lib.checked().wm_dropout_fwd(_p(x), _p(cover), _p(y), N, H, W, keep_min, keep_span, _p(state), _p(rec), _stream())
    _wrote(state)
    return y, rec


def dropout_bwd(g, keep_min, keep_span, rec, want_cover=False):
    g, N, H, W = _planes(g)
    gx = torch.empty_like(g)
    gc = torch.empty_like(g) if want_cover else None
    _lib.checked().wm_dropout_bwd(_p(g), _p(gx), _p(gc), N, H, W, keep_min, keep_span, _p(rec), _stream())
    return gx, gc


def _jpeg_drop(name, x, keep):
    _need_cuda(x)
    assert x.dim() == 4 and x.shape[1] == 3, "JpegCompression takes [B,3,H,W] images"
    x = x.contiguous().float()
    y = torch.empty_like(x)
    k = _host_ints(keep)
    getattr(_lib.checked(), name)(_p(x), _p(y), x.shape[0], x.shape[2], x.shape[3], k, _stream())
    return y


def jpeg_drop_fwd(x, keep=(25, 9, 9)):
    """JpegCompression forward (keep = coefficients kept in Y, U, V)"""
    return _jpeg_drop("wm_jpeg_drop_fwd", x, keep)


def jpeg_drop_bwd(g, keep=(25, 9, 9)):
    """the exact transpose of jpeg_drop_fwd"""
    return _jpeg_drop("wm_jpeg_drop_bwd", g, keep)
