"""ctypes loader for libwm_hip.so (the C ABI declared in include/wm_hip.h).

There is NO fallback: if the library is missing or a call fails, a RuntimeError
is raised.  Nothing under oracle/ is ever imported from here.

Two builds of the same sources live in lib/: libwm_hip.so (release: no knobs, no environment variables, no state between
calls) is what every product path loads; libwm_hip_dbg.so (-DWM_DEBUG: the wm_debug_* A/B switches) is loaded only on
request, by tools/ and by the tests that compare a fused kernel with its unfused form (use_debug_library()).

Every handle _load() returns is typed from include/wm_hip.h: each declared function carries the argtypes and restype of its
prototype, so callers pass plain Python ints, floats, None and ctypes arrays, and a call with too few arguments raises.

Each build has two kinds of handle on the same shared object.  The raw ones (lib(), debug_lib(), what use_debug_library() yields) hand every
return code back: tools/ and the tests that assert a refusal code call them, with check() where they want the exception.  The checked ones
(checked(), what ops.py calls through) carry an errcheck on every status function -- status_functions(): returns int and takes a pointer -- that
raises RuntimeError with the function's own name and wm_last_error_string(); queries (int from scalars only) answer through either kind.
"""
import contextlib
import ctypes
import functools
import os
import re

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libwm_hip.so")
# tools/ only (same-box A/B of two BUILDS, tools/ab_libs.sh): WM_LIB_VARIANT=<name> loads tools/micro/ab/libwm_hip_<name>.so in place of the
# release file -- the release file is never overwritten, so an interrupted A/B cannot leave a variant installed.  loaded_path() says which
_VARIANT = os.environ.get("WM_LIB_VARIANT")
if _VARIANT:
    LIB_PATH = os.path.join(os.path.dirname(_PKG), "tools", "micro", "ab", f"libwm_hip_{_VARIANT}.so")
DEBUG_LIB_PATH = os.path.join(_PKG, "lib", "libwm_hip_dbg.so")
_lib = None
_release = None
_debug = None
_twins = {}         # raw handle -> its checked twin


# the header's C types -> ctypes.  Closed: a type not listed here is a load error, never an untyped argument
_ARG = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_RET = dict(_ARG, **{"const char*": ctypes.c_char_p})
# `ret name(params);` from the start of a line, the parameter list possibly over several lines
_DECL = re.compile(r"^[ \t]*([^;{}()#\n]*?)\s*\b(wm_\w+)\s*\(([^()]*)\)\s*;", re.M)


def _argtype(param, fn):
    m = re.fullmatch(r"(.*?[\s*])\s*\w+", param.strip(), flags=re.S)
    if m is None:
        raise RuntimeError(f"wm_hip.h: {fn}: unnamed or unparsed parameter {param.strip()!r}")
    if "*" in m.group(1):
        return ctypes.c_void_p       # device and host pointers alike: takes None, an int, a ctypes array or byref(struct)
    t = " ".join(w for w in m.group(1).split() if w != "const")
    if t not in _ARG:
        raise RuntimeError(f"wm_hip.h: {fn}: parameter type {t!r} has no ctypes mapping")
    return _ARG[t]


def parse_header(text):
    """{name: (restype, [argtypes])} of every wm_* function declared in `text` (a C header)"""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    sigs = {}
    for ret, name, params in _DECL.findall(src):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RET:
            raise RuntimeError(f"wm_hip.h: {name}: return type {ret!r} has no ctypes mapping")
        sigs[name] = (_RET[ret], [] if params.strip() == "void" else [_argtype(p, name) for p in params.split(",")])
    missed = set(re.findall(r"\b(wm_\w+)\s*\(", src)) - set(sigs)
    if missed:
        raise RuntimeError(f"wm_hip.h: declarations not parsed: {sorted(missed)}")
    return sigs


@functools.lru_cache(maxsize=None)
def signatures():
    """parse_header of include/wm_hip.h"""
    from .build import HEADER      # (imported here: `python -m ...build` must not find this module already loaded)
    with open(HEADER) as f:
        return parse_header(f.read())


@functools.lru_cache(maxsize=None)
def debug_setters():
    """names of the wm_debug_* switches (WM_KNOB in csrc/): void setter(int), exported by the -DWM_DEBUG build only"""
    from .build import CSRC
    names = set()
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".cpp")):
            with open(os.path.join(CSRC, f)) as fh:
                names.update(re.findall(r"^\s*WM_KNOB\(\s*\w+\s*,\s*(wm_debug_\w+)", fh.read(), flags=re.M))
    return sorted(names)


@functools.lru_cache(maxsize=None)
def status_functions():
    """names of the functions whose int is a status (0 or WM_E_*): those that return int and take a pointer.  An int function of scalars
    only is a query and its int the answer (include/wm_hip.h, Conventions)"""
    return frozenset(n for n, (restype, argtypes) in signatures().items() if restype is ctypes.c_int and ctypes.c_void_p in argtypes)


def _load(path, debug=False, checked=False):
    """a handle on `path` whose functions carry the header's argtypes and restype (debug=True: and the wm_debug_* setters').  checked=True:
    a CDLL of its own (so function objects of its own) whose status functions raise on a non-zero return instead of handing it back"""
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build it with `python -m video_watermarking_forgery_detection_amd.build` "
            "(there is no CPU / PyTorch fallback for the HIP path)")
    h = ctypes.CDLL(path)
    sigs = dict(signatures())
    if debug:
        sigs.update((n, (None, [ctypes.c_int])) for n in debug_setters())
    for name, (restype, argtypes) in sigs.items():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = restype, argtypes
    if checked:
        last_error = h.wm_last_error_string

        def raise_on_error(rc, fn, args):
            if rc == 0:
                return rc
            raise RuntimeError(f"{fn.__name__} failed (rc={rc}): {last_error().decode(errors='replace')}")
        for name in status_functions():
            getattr(h, name).errcheck = raise_on_error
    return h


def lib():
    """the raw handle on the library every op goes through: the release build unless a use_debug_library() block is open"""
    global _lib, _release
    if _lib is None:
        if _release is None:
            _release = _load(LIB_PATH)
        _lib = _release
    return _lib


def checked():
    """the checked twin of lib(), created once per raw handle: what ops.py calls through"""
    raw = lib()
    twin = _twins.get(raw)
    if twin is None:
        twin = _twins[raw] = _load(raw._name, debug=raw is _debug, checked=True)
    return twin


def loaded_path():
    """path of the library lib() loads (bench.py reports its hash next to the kernel sources' hash)"""
    return LIB_PATH


def debug_lib():
    global _debug
    if _debug is None:
        _debug = _load(DEBUG_LIB_PATH, debug=True)
    return _debug


@contextlib.contextmanager
def use_debug_library():
    """inside the block every op runs on the -DWM_DEBUG build, whose wm_debug_* switches the caller may flip; yields its raw handle"""
    global _lib
    prev = lib()
    _lib = debug_lib()
    try:
        yield _lib
    finally:
        _lib = prev


def check(rc, name):
    if rc != 0:
        msg = lib().wm_last_error_string().decode(errors="replace")
        raise RuntimeError(f"{name} failed (rc={rc}): {msg}")
