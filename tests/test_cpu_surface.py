"""CPU: host-side surface checks that need no GPU -- state_dict keys equal the reference's
(through the oracle restatement, itself pinned to the reference by test_oracle_golden), the C-ABI
library exports exactly the symbols include/wm_hip.h declares and is bound with their signatures, and
the product path refuses to run without a GPU instead of falling back."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from oracle import hidden_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_keys_match_reference_names():
    from video_watermarking_forgery_detection_amd.hidden_models import Encoder, Decoder, Discriminator
    from video_watermarking_forgery_detection_amd.options import HiDDenConfiguration
    cfg = HiDDenConfiguration(H=32, W=32)
    rc = hidden_ref.HiDDenConfiguration(H=32, W=32)
    for mine, ref in ((Encoder(cfg), hidden_ref.Encoder(rc)), (Decoder(cfg), hidden_ref.Decoder(rc)),
                      (Discriminator(cfg), hidden_ref.Discriminator(rc))):
        a, b = mine.state_dict(), ref.state_dict()
        assert list(a.keys()) == list(b.keys())
        assert all(a[k].shape == b[k].shape for k in a)
        ref.load_state_dict(a)  # checkpoints interchange


def _built():
    from video_watermarking_forgery_detection_amd import _lib
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.DEBUG_LIB_PATH)):
        from video_watermarking_forgery_detection_amd import build
        build.build(verbose=False)
    return _lib


def _exported_functions(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(f[2] for f in (ln.split() for ln in nm.splitlines()) if len(f) == 3 and f[1] == "T")


def test_library_exports_every_declared_symbol():
    """the header IS the boundary: the release library exports exactly the functions include/wm_hip.h declares -- no C++ internals --
    and the -DWM_DEBUG twin those plus its wm_debug_* switches"""
    _lib = _built()
    hdr = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(wm_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 20 and names == sorted(_lib.signatures())
    exported = _exported_functions(_lib.LIB_PATH)
    assert not [n for n in exported if n.startswith("_Z")]
    assert exported == names
    assert len(_lib.debug_setters()) >= 1
    assert _exported_functions(_lib.DEBUG_LIB_PATH) == sorted(names + _lib.debug_setters())
    assert ctypes.CDLL(_lib.LIB_PATH).wm_abi_version() >= 1


def test_loaded_handles_carry_the_header_signatures():
    """every declared function of both handles has the header's argtypes and restype (the debug handle: and its setters take one int);
    the type map is closed -- a type it does not know is an error, not an untyped argument"""
    _lib = _built()
    sigs = _lib.signatures()
    for h in (_lib.lib(), _lib.debug_lib()):
        for n, (restype, argtypes) in sigs.items():
            f = getattr(h, n)
            assert list(f.argtypes) == argtypes and f.restype is restype, n
    for n in _lib.debug_setters():
        f = getattr(_lib.debug_lib(), n)
        assert list(f.argtypes) == [ctypes.c_int] and f.restype is None, n
    assert sigs["wm_last_error_string"] == (ctypes.c_char_p, [])
    assert sigs["wm_conv3x3_wgrad_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    assert sigs["wm_bn_finalize"][1][4] is ctypes.c_double and sigs["wm_bn_finalize"][1][9] is ctypes.c_float
    assert sigs["wm_amp_found_inf"][1][:2] == [ctypes.c_void_p] * 2           # const float* const*, const int*
    assert sigs["wm_conv3x3_wgrad_fin"][1][-3:] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]   # const WmBnBwdFin*, sweep_reverse, stream
    for bad in ("int wm_a(long n);", "void wm_b(int n);", "int* wm_c(int n);", "int wm_d(unsigned n);", "int wm_e(int);"):
        with pytest.raises(RuntimeError):
            _lib.parse_header(bad)
    assert _lib.parse_header("int wm_g(void);\nsize_t wm_h(const unsigned char* p, double d /* x */, float f);") == {
        "wm_g": (ctypes.c_int, []), "wm_h": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_double, ctypes.c_float])}


def test_checked_handles_raise_from_the_status_functions_only():
    """checked(), for both builds: every declared function typed as the header says, an errcheck on exactly status_functions() -- and none
    on any function of the raw handles, whose callers assert the return codes"""
    _lib = _built()
    sigs, status = _lib.signatures(), _lib.status_functions()
    release = _lib.checked()
    with _lib.use_debug_library() as raw_debug:
        debug = _lib.checked()
        assert raw_debug is _lib.debug_lib() and _lib.checked() is debug      # created once
    assert _lib.checked() is release and len({id(h) for h in (release, debug, _lib.lib(), _lib.debug_lib())}) == 4
    for h in (release, debug):
        for n, (restype, argtypes) in sigs.items():
            f = getattr(h, n)
            assert list(f.argtypes) == argtypes and f.restype is restype, n
        assert {n for n in sigs if getattr(h, n).errcheck is not None} == status
    for n in _lib.debug_setters():
        f = getattr(debug, n)
        assert list(f.argtypes) == [ctypes.c_int] and f.restype is None and f.errcheck is None, n
    for h in (_lib.lib(), _lib.debug_lib()):
        assert not [n for n in list(sigs) + _lib.debug_setters() if hasattr(h, n) and getattr(h, n).errcheck is not None]


def test_status_functions_are_the_int_functions_that_take_a_pointer():
    """the header's rule (Conventions): what can fail takes a pointer; an int function of scalars only is a query and its int the answer"""
    from video_watermarking_forgery_detection_amd import _lib
    sigs, status = _lib.signatures(), _lib.status_functions()
    assert {"wm_adam_hyper", "wm_jpeg_fwd_act", "wm_pack_w3x3_batch"} <= status
    assert not status & {"wm_abi_version", "wm_fin_rider_enabled", "wm_conv3x3_nparts", "wm_conv3x3_bwd_fused_kernel"}
    assert not [n for n in status if sigs[n][0] in (ctypes.c_size_t, ctypes.c_char_p)]
    assert any(r is ctypes.c_size_t for r, _ in sigs.values()) and sigs["wm_last_error_string"][0] is ctypes.c_char_p
    ints = {n for n, (r, _) in sigs.items() if r is ctypes.c_int}
    assert status and status < ints
    assert all(ctypes.c_void_p in sigs[n][1] for n in status) and not [n for n in ints - status if ctypes.c_void_p in sigs[n][1]]


def test_checked_handle_raises_where_the_raw_one_returns_the_code():
    """wm_adam_hyper is host arithmetic (no GPU): step 0 is refused -- the checked handle raises with the function's name and the library's
    text, the raw one returns WM_E_BADARG; step 1 is served by both with the same eight floats.  Inside use_debug_library() checked() is the
    debug build's twin, after it the release build's again"""
    _lib = _built()
    args = (1e-3, 0.9, 0.999, 1e-8, 0.01)

    def refused(raw, chk):
        out = (ctypes.c_float * 8)()
        with pytest.raises(RuntimeError, match=r"wm_adam_hyper failed \(rc=-1\)") as e:
            chk.wm_adam_hyper(*args, 0, out)
        assert str(e.value).endswith(": " + raw.wm_last_error_string().decode()) and "wm_adam_hyper: bad arguments" in str(e.value)
        assert raw.wm_adam_hyper(*args, 0, out) == -1
        a, b = (ctypes.c_float * 8)(), (ctypes.c_float * 8)()
        assert raw.wm_adam_hyper(*args, 1, a) == 0 and chk.wm_adam_hyper(*args, 1, b) == 0
        assert list(a) == list(b) and a[2] == ctypes.c_float(1e-3).value and a[0] > 0
    release = _lib.checked()
    refused(_lib.lib(), release)
    with _lib.use_debug_library() as raw_debug:
        assert _lib.checked() is not release and getattr(_lib.checked(), _lib.debug_setters()[0]).argtypes == [ctypes.c_int]
        refused(raw_debug, _lib.checked())
    assert _lib.checked() is release and _lib.lib() is not raw_debug


def test_ops_calls_through_the_checked_handle_only():
    with open(os.path.join(ROOT, "video_watermarking_forgery_detection_amd", "ops.py")) as f:
        src = f.read()
    assert "_lib.check(" not in src and "_lib.lib()" not in src and "_lib.checked()" in src


def test_every_direct_call_passes_the_header_arity():
    """ctypes refuses too few arguments but passes surplus ones through: each call of a wm_* attribute with positional arguments in the
    package, tests/ and tools/ passes exactly as many as include/wm_hip.h declares (a wm_debug_* setter: one)"""
    import ast
    from video_watermarking_forgery_detection_amd import _lib
    arity = {n: len(a) for n, (_, a) in _lib.signatures().items()}
    arity.update((n, 1) for n in _lib.debug_setters())
    bad, seen = [], 0
    for top in ("video_watermarking_forgery_detection_amd", "tests", "tools"):
        for dp, _, fs in os.walk(os.path.join(ROOT, top)):
            for f in fs:
                if not f.endswith(".py"):
                    continue
                path = os.path.join(dp, f)
                with open(path) as fh:
                    tree = ast.parse(fh.read(), path)
                for node in ast.walk(tree):
                    if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("wm_")
                            and not node.keywords and not any(isinstance(a, ast.Starred) for a in node.args)):
                        seen += 1
                        if arity.get(node.func.attr) != len(node.args):
                            bad.append(f"{os.path.relpath(path, ROOT)}:{node.lineno} {node.func.attr}: {len(node.args)} arguments, "
                                       f"header: {arity.get(node.func.attr)}")
    assert seen >= 150
    assert not bad, bad


def test_no_cpu_fallback():
    from video_watermarking_forgery_detection_amd.hidden_models import Encoder, Hidden
    from video_watermarking_forgery_detection_amd.noise_layers import Jpeg, Identity
    from video_watermarking_forgery_detection_amd.options import HiDDenConfiguration
    cfg = HiDDenConfiguration(H=16, W=16)
    with pytest.raises(RuntimeError, match="HIP path only"):
        Encoder(cfg)(torch.zeros(1, 3, 16, 16), torch.zeros(1, 30))
    with pytest.raises(RuntimeError, match="HIP path only"):
        Jpeg(50)(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="HIP path only"):
        Hidden(cfg, torch.device("cpu"), Identity(), None)


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "video_watermarking_forgery_detection_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f


def test_jpeg_layer_names_and_scale():
    from video_watermarking_forgery_detection_amd.noise_layers import Jpeg, JpegSS, JpegMask, Combined, Identity
    assert Jpeg(50).name == "Jpeg50" and JpegSS(70).name == "JpegSS70" and JpegMask(90).name == "JpegMask90"
    assert Jpeg(50).scale_factor == 1.0 and abs(Jpeg(90).scale_factor - 0.2) < 1e-12 and Jpeg(10).scale_factor == 5.0
    c = Combined([JpegMask(80), Jpeg(80), Identity()])
    assert c.name == "NotChosenYet"
    c._pick(1)
    assert c.name == "Jpeg80"
    c._pick(7)
    assert c.name in ("JpegMask80", "Jpeg80", "Identity")


def test_host_step_logic_without_a_gpu():
    """host-side pieces of the step that need no kernel: sweep alternation along a chain of layers, deferred BatchNorm counter
    bumps (one multi-tensor add per step, nesting), the asynchronous gradient bucket on a single rank."""
    import torch
    from video_watermarking_forgery_detection_amd import engine
    from video_watermarking_forgery_detection_amd.distributed import GradSync
    # a chain of fresh tensors alternates the sweep direction; a tensor that is not fresh is walked forwards
    assert engine._opposite(None) is False and engine._opposite(False) is True and engine._opposite(True) is False
    d, seq = None, []
    for _ in range(5):
        d = engine._opposite(d)
        seq.append(d)
    assert seq == [False, True, False, True, False]

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.bn1, self.bn2 = torch.nn.BatchNorm2d(4), torch.nn.BatchNorm2d(4)
    net = Net()
    nbt = torch.stack([net.bn1.num_batches_tracked, net.bn2.num_batches_tracked])
    net.bn1._buffers["num_batches_tracked"], net.bn2._buffers["num_batches_tracked"] = nbt[0], nbt[1]
    object.__setattr__(net, "_nbt", nbt)
    engine.bump_bn_counters(net)
    assert nbt.tolist() == [1, 1]
    with engine.defer_bn_counters():
        engine.bump_bn_counters(net)
        with engine.defer_bn_counters():       # nested: the outer block flushes
            engine.bump_bn_counters(net)
        engine.bump_bn_counters(net)
        assert nbt.tolist() == [1, 1]           # nothing applied yet
    assert nbt.tolist() == [4, 4] and int(net.bn2.num_batches_tracked) == 4
    # world size 1: start / finish are no-ops, the buffer is untouched
    gs = GradSync()
    g = torch.arange(6.0)
    h = gs.start(g)
    gs.finish(h)
    assert h is None and torch.equal(gs(g), torch.arange(6.0))


def test_flat_adam_state_interchanges_with_torch_optim_adam():
    """training-state files (base_model.py:129-150 of the reference hold torch.optim.Adam state_dicts): FlatAdam emits and accepts
    that layout -- per-parameter {step, exp_avg, exp_avg_sq} in parameters() order, one param group -- and still reads round 1's flat one"""
    from video_watermarking_forgery_detection_amd.hidden_models import Decoder, Discriminator
    from video_watermarking_forgery_detection_amd.optim import FlatAdam
    from video_watermarking_forgery_detection_amd.options import HiDDenConfiguration
    cfg = HiDDenConfiguration(H=16, W=16)
    torch.manual_seed(0)
    nets = [Discriminator(cfg), Decoder(cfg)]
    for n in nets:
        n.flatten_parameters_()
    params = [p for n in nets for p in n.parameters()]
    topt = torch.optim.Adam(params, lr=2e-3, betas=(0.8, 0.99), weight_decay=0.01)
    for _ in range(3):
        for p in params:
            p.grad = torch.randn_like(p)
        topt.step()
    sd = topt.state_dict()
    flat = FlatAdam(nets)
    flat.load_state_dict(sd)
    assert flat.step_count == 3 and flat.param_groups[0]["lr"] == 2e-3 and tuple(flat.param_groups[0]["betas"]) == (0.8, 0.99)
    assert flat.param_groups[0]["weight_decay"] == 0.01
    off = 0
    for i, p in enumerate(nets[0].parameters()):
        n = p.numel()
        assert torch.equal(flat._m[0][off:off + n].view_as(p), sd["state"][i]["exp_avg"])
        assert torch.equal(flat._v[0][off:off + n].view_as(p), sd["state"][i]["exp_avg_sq"])
        off += n
    out = flat.state_dict()
    fresh = torch.optim.Adam(params, lr=1.0)
    fresh.load_state_dict(out)                      # torch accepts what we write
    back = fresh.state_dict()
    assert back["param_groups"][0]["lr"] == 2e-3 and len(back["state"]) == len(params)
    for i in range(len(params)):
        assert torch.equal(back["state"][i]["exp_avg"], sd["state"][i]["exp_avg"])
        assert torch.equal(back["state"][i]["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
        assert float(back["state"][i]["step"]) == 3.0
    # a state with a different parameter list is refused, not silently truncated
    with pytest.raises(ValueError):
        FlatAdam(nets[:1]).load_state_dict(sd)
    # round 1's flat layout is still readable
    legacy = {"step": 5, "param_groups": [{"lr": 1e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0}],
              "exp_avg": [t.clone() for t in flat._m], "exp_avg_sq": [t.clone() for t in flat._v]}
    f2 = FlatAdam(nets)
    f2.load_state_dict(legacy)
    assert f2.step_count == 5 and f2.param_groups[0]["lr"] == 1e-4 and torch.equal(f2._m[1], flat._m[1])


@pytest.mark.parametrize("variant", ["amsgrad", "maximize"])
def test_flat_adam_refuses_torch_state_of_an_adam_variant_it_does_not_run(variant):
    """a torch.optim.Adam state_dict with amsgrad=True (which carries max_exp_avg_sq) or maximize=True is refused: continuing it as plain
    Adam would silently change the optimiser"""
    from video_watermarking_forgery_detection_amd.hidden_models import Discriminator
    from video_watermarking_forgery_detection_amd.optim import FlatAdam
    from video_watermarking_forgery_detection_amd.options import HiDDenConfiguration
    torch.manual_seed(1)
    net = Discriminator(HiDDenConfiguration(H=16, W=16))
    net.flatten_parameters_()
    params = list(net.parameters())
    topt = torch.optim.Adam(params, lr=1e-3, **{variant: True})
    for p in params:
        p.grad = torch.randn_like(p)
    topt.step()
    sd = topt.state_dict()
    flat = FlatAdam([net])
    with pytest.raises(ValueError, match=variant):
        flat.load_state_dict(sd)
    assert flat.step_count == 0 and flat.param_groups[0]["lr"] == 1e-3
    sd["param_groups"][0][variant] = False      # the same state as plain Adam loads
    flat.load_state_dict(sd)
    assert flat.step_count == 1


def test_median_selection_networks_of_the_attack_kernel():
    """csrc/attacks.hip selects the median of 9 / 25 taps with min/max exchange networks (Devillard's opt_med9 / opt_med25 orders):
    replay the exchange lists parsed from the kernel source on random vectors (with ties) against numpy's median"""
    import numpy as np
    src = open(os.path.join(ROOT, "video_watermarking_forgery_detection_amd", "csrc", "attacks.hip")).read()
    rng = np.random.RandomState(0)
    for n, out in ((9, 4), (25, 12)):
        body = src[src.index(f"median_select<{n}>(float (&v)[{n}])"):]
        body = body[:body.index("return")]
        ces = [(int(a), int(b)) for a, b in re.findall(r"WM_CE\((\d+), (\d+)\)", body)]
        assert len(ces) == (19 if n == 9 else 99)
        for trial in range(4000):
            v = rng.randint(0, 6 if trial % 2 else 1000, size=n).astype(np.float64)   # every other trial is full of ties
            w = v.copy()
            for a, b in ces:
                lo, hi = min(w[a], w[b]), max(w[a], w[b])
                w[a], w[b] = lo, hi
            assert w[out] == np.sort(v)[n // 2], (n, trial)
