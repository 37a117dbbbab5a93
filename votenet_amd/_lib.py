"""ctypes binding of libvotenet_hip.so (the C ABI declared in include/votenet_hip.h).

torch is used for device memory and streams only: every call passes raw device pointers,
sizes and the current HIP stream across the C ABI.  No fallback path exists -- if the library
is missing or a call fails, an exception is raised.
"""
import ctypes
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "lib", "libvotenet_hip.so")
_MON_PATH = os.path.join(_HERE, "lib", "libvotenet_monitors.so")  # the training summaries (include/votenet_monitors.h): a library of its own
_GUARD_PATH = os.path.join(_HERE, "lib", "libvotenet_guard.so")  # the guarded optimizer step (include/votenet_step_guard.h): likewise
_FEAT_PATH = os.path.join(_HERE, "lib", "libvotenet_features.so")  # the input step with point features (include/votenet_point_features.h): likewise
_lib = None
_mon = None
_guard = None
_feat = None
_DETECT_PATH = os.path.join(_HERE, "lib", "libvotenet_detect.so")  # per-class detections (include/votenet_detections.h): likewise
_detect = None
_BOXPTS_PATH = os.path.join(_HERE, "lib", "libvotenet_boxpts.so")  # points inside predicted boxes (include/votenet_box_points.h): likewise
_boxpts = None
_AABB_PATH = os.path.join(_HERE, "lib", "libvotenet_aabb.so")  # axis-aligned NMS overlaps (include/votenet_aabb_nms.h): likewise
_aabb = None


class VotenetError(RuntimeError):
    """A HIP runtime / launch / workspace error reported by libvotenet_hip.so."""


class InvalidArgumentError(ValueError):
    """Mirror of tf.errors.InvalidArgumentError raised by the reference's OP_REQUIRES checks."""


def lib_path():
    return _LIB_PATH


def build(force=False):
    """Compile libvotenet_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:  # a clean build: the library AND every cached object file (build.sh recompiles what is missing)
        import glob
        mon = os.path.join(os.path.dirname(_LIB_PATH), os.path.basename(_MON_PATH))
        guard = os.path.join(os.path.dirname(_LIB_PATH), os.path.basename(_GUARD_PATH))
        feat = os.path.join(os.path.dirname(_LIB_PATH), os.path.basename(_FEAT_PATH))
        detect = os.path.join(os.path.dirname(_LIB_PATH), os.path.basename(_DETECT_PATH))
        boxpts = os.path.join(os.path.dirname(_LIB_PATH), os.path.basename(_BOXPTS_PATH))
        aabb = os.path.join(os.path.dirname(_LIB_PATH), os.path.basename(_AABB_PATH))
        for f in [_LIB_PATH, mon, guard, feat, detect, boxpts, aabb] + [o for d in ("obj", os.path.join("monitors", "obj"), os.path.join("guard", "obj"), os.path.join("features", "obj"),
                                                                               os.path.join("detect", "obj"), os.path.join("boxpts", "obj"), os.path.join("aabb", "obj"))
                                            for o in glob.glob(os.path.join(_HERE, "csrc", d, "*.o"))]:
            if os.path.exists(f):
                os.remove(f)
    out = subprocess.run(["bash", os.path.join(_HERE, "csrc", "build.sh")], capture_output=True, text=True)
    if out.returncode != 0:
        raise VotenetError("libvotenet_hip.so build failed:\n" + out.stdout + out.stderr)
    return _LIB_PATH


# The C subset of include/votenet_hip.h and votenet_hip_debug.h -> ctypes.  The headers are the one statement of the ABI (every .hip
# file is compiled against them); nothing below restates a prototype.
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double, "unsigned": ctypes.c_uint,
            "unsigned long long": ctypes.c_ulonglong, "size_t": ctypes.c_size_t}
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char", "unsigned short", "long long"}  # all cross the ABI as void*


def _declarator(text, where):
    """'const float *gamma' -> ('float', 1, 'gamma'): type, pointer depth, name"""
    words = text.replace("*", " * ").split()
    if not words or not words[-1].isidentifier():
        raise ValueError("%s: cannot read the declaration '%s'" % (where, " ".join(text.split())))
    return " ".join(w for w in words[:-1] if w != "const" and w != "*"), words.count("*"), words[-1]


def _ctype(base, stars, structs, where, ret=False):
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 0 and ret and base == "void":
        return None
    if stars == 1 and base in structs:
        return ctypes.POINTER(structs[base])
    if stars == 1 and ret and base == "char":
        return ctypes.c_char_p
    if stars == 1 and base in _POINTEES:
        return ctypes.c_void_p  # device pointers, host arrays and the stream alike: callers pass plain ints
    raise ValueError("%s: no ctypes type for the C type '%s'" % (where, base + " *" * stars))


def parse_header(text, structs):
    """{function: (restype, argtypes)} of every declaration in a header's text; every `typedef struct {...} votenet_x;` becomes a
    ctypes.Structure in structs[votenet_x].  A declaration this cannot type raises ValueError with its name."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", "", text, flags=re.S)  # extern "C" { ... }
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

    def struct(m):
        name, fields = m.group(2), []
        for line in filter(str.strip, m.group(1).split(";")):  # 'const float *gamma, *beta': the first declarator's type holds for all
            decls = [_declarator(d, name) for d in line.split(",")]
            fields += [(n, _ctype(decls[0][0], stars, structs, name + "." + n)) for _, stars, n in decls]
        structs[name] = type("".join(w.capitalize() for w in name.split("_")[1:]), (ctypes.Structure,),
                             {"_fields_": fields, "__doc__": "struct %s of the C ABI." % name})
        return ""
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    funcs = {}
    for stmt in text.split(";"):
        if not stmt.strip():
            continue
        m = re.fullmatch(r"(.*?)\((.*)\)\s*", stmt, flags=re.S)
        if not m:
            raise ValueError("not a function declaration: '%s'" % " ".join(stmt.split()))
        base, stars, name = _declarator(m.group(1), "function")
        params = [] if m.group(2).strip() == "void" else m.group(2).split(",")
        funcs[name] = (_ctype(base, stars, structs, name, ret=True),
                       [_ctype(*_declarator(p, name)[:2], structs, name) for p in params])
    return funcs


_STRUCTS = ("BnRaw", "CoefTail", "MlpInput", "RowSegment", "CopySegment")  # votenet_bn_raw, ... of votenet_hip.h
_abi_read = None


def _abi():
    """({function: (restype, argtypes)} of votenet_hip.h, the same of votenet_hip_debug.h); the headers are read once, found relative
    to the package as csrc/common.h finds them, and their structs become this module's BnRaw ... CopySegment."""
    global _abi_read
    if _abi_read is None:
        structs, protos = {}, []
        for h in ("votenet_hip.h", "votenet_hip_debug.h"):
            with open(os.path.join(_HERE, os.pardir, "include", h)) as f:
                protos.append(parse_header(f.read(), structs))
        globals().update({cls.__name__: cls for cls in structs.values()})
        _abi_read = tuple(protos)
    return _abi_read


def __getattr__(name):  # the structs, for a caller that builds one before anything has loaded the library
    if name in _STRUCTS:
        _abi()
        return globals()[name]
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


class _Library(ctypes.CDLL):
    """Every function gets its header's prototype when it is first looked up.  The library's measurement / tuning switches
    (include/votenet_hip_debug.h) are inert until the host opts in.  This host opts in the first time something (a test, a profile tool,
    mlp.debug_switch) looks one up; code that never touches a switch never does."""

    def __getattr__(self, name):  # only reached for names not bound yet (CDLL caches what it has resolved)
        fn = super().__getattr__(name)
        for protos in _abi():
            if name in protos:  # (anything else is one of the reference's eight C++ launcher names: the caller types those)
                fn.restype, fn.argtypes = protos[name]
        if "debug" in name and name not in ("votenet_debug_enable", "votenet_debug_enabled", "votenet_debug_fps_split_timeouts"):
            self.votenet_debug_enable(1)
        return fn


def lib():
    """Load the library once; raise loudly if it has not been built or lacks a function votenet_hip.h declares."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise VotenetError(
                "libvotenet_hip.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)" % _LIB_PATH)
        L = _Library(_LIB_PATH)
        for name in _abi()[0]:  # (not the debug header's: looking a switch up opts in)
            getattr(L, name)
        _lib = L
    return _lib


def monitors_lib():
    """libvotenet_monitors.so, loaded when a summary is first asked for; every function of include/votenet_monitors.h gets its header's
    prototype (parse_header, as for the main library).  No fallback: a missing library is an error."""
    global _mon
    if _mon is None:
        if not os.path.exists(_MON_PATH):
            raise VotenetError("libvotenet_monitors.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)" % _MON_PATH)
        with open(os.path.join(_HERE, os.pardir, "include", "votenet_monitors.h")) as f:
            protos = parse_header(f.read(), {})
        M = ctypes.CDLL(_MON_PATH)
        for name, (restype, argtypes) in protos.items():
            fn = getattr(M, name)
            fn.restype, fn.argtypes = restype, argtypes
        _mon = M
    return _mon


def guard_lib():
    """libvotenet_guard.so, loaded when a step guard is first asked for; every function of include/votenet_step_guard.h gets its
    header's prototype (parse_header, as for the main library).  No fallback: a missing library is an error."""
    global _guard
    if _guard is None:
        if not os.path.exists(_GUARD_PATH):
            raise VotenetError("libvotenet_guard.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)" % _GUARD_PATH)
        with open(os.path.join(_HERE, os.pardir, "include", "votenet_step_guard.h")) as f:
            protos = parse_header(f.read(), {})
        G = ctypes.CDLL(_GUARD_PATH)
        for name, (restype, argtypes) in protos.items():
            fn = getattr(G, name)
            fn.restype, fn.argtypes = restype, argtypes
        _guard = G
    return _guard


def features_lib():
    """libvotenet_features.so, loaded when point features are first asked for; every function of include/votenet_point_features.h gets
    its header's prototype (parse_header, as for the main library).  No fallback: a missing library is an error."""
    global _feat
    if _feat is None:
        if not os.path.exists(_FEAT_PATH):
            raise VotenetError("libvotenet_features.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)" % _FEAT_PATH)
        with open(os.path.join(_HERE, os.pardir, "include", "votenet_point_features.h")) as f:
            protos = parse_header(f.read(), {})
        F = ctypes.CDLL(_FEAT_PATH)
        for name, (restype, argtypes) in protos.items():
            fn = getattr(F, name)
            fn.restype, fn.argtypes = restype, argtypes
        _feat = F
    return _feat


def detect_lib():
    """libvotenet_detect.so, loaded when per-class detections are first asked for; every function of include/votenet_detections.h gets
    its header's prototype (parse_header, as for the main library).  No fallback: a missing library is an error."""
    global _detect
    if _detect is None:
        if not os.path.exists(_DETECT_PATH):
            raise VotenetError("libvotenet_detect.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)" % _DETECT_PATH)
        with open(os.path.join(_HERE, os.pardir, "include", "votenet_detections.h")) as f:
            protos = parse_header(f.read(), {})
        D = ctypes.CDLL(_DETECT_PATH)
        for name, (restype, argtypes) in protos.items():
            fn = getattr(D, name)
            fn.restype, fn.argtypes = restype, argtypes
        _detect = D
    return _detect


def boxpts_lib():
    """libvotenet_boxpts.so, loaded when the points inside predicted boxes are first asked for; every function of
    include/votenet_box_points.h gets its header's prototype (parse_header, as for the main library).  No fallback: a missing library
    is an error."""
    global _boxpts
    if _boxpts is None:
        if not os.path.exists(_BOXPTS_PATH):
            raise VotenetError("libvotenet_boxpts.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)" % _BOXPTS_PATH)
        with open(os.path.join(_HERE, os.pardir, "include", "votenet_box_points.h")) as f:
            protos = parse_header(f.read(), {})
        B = ctypes.CDLL(_BOXPTS_PATH)
        for name, (restype, argtypes) in protos.items():
            fn = getattr(B, name)
            fn.restype, fn.argtypes = restype, argtypes
        _boxpts = B
    return _boxpts


def aabb_lib():
    """libvotenet_aabb.so, loaded when an axis-aligned NMS overlap is first asked for; every function of include/votenet_aabb_nms.h
    gets its header's prototype (parse_header, as for the main library).  No fallback: a missing library is an error."""
    global _aabb
    if _aabb is None:
        if not os.path.exists(_AABB_PATH):
            raise VotenetError("libvotenet_aabb.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)" % _AABB_PATH)
        with open(os.path.join(_HERE, os.pardir, "include", "votenet_aabb_nms.h")) as f:
            protos = parse_header(f.read(), {})
        A = ctypes.CDLL(_AABB_PATH)
        for name, (restype, argtypes) in protos.items():
            fn = getattr(A, name)
            fn.restype, fn.argtypes = restype, argtypes
        _aabb = A
    return _aabb


def check_aabb(rc):
    """check() for a status libvotenet_aabb.so returned (it keeps its own error text)."""
    if rc == 0:
        return
    msg = aabb_lib().votenet_aabb_last_error().decode()
    if rc == 1:
        raise InvalidArgumentError(msg)
    raise VotenetError("libvotenet_aabb error %d: %s" % (rc, msg))


def check_boxpts(rc):
    """check() for a status libvotenet_boxpts.so returned (it keeps its own error text)."""
    if rc == 0:
        return
    msg = boxpts_lib().votenet_box_points_last_error().decode()
    if rc == 1:
        raise InvalidArgumentError(msg)
    raise VotenetError("libvotenet_boxpts error %d: %s" % (rc, msg))


def check_detect(rc):
    """check() for a status libvotenet_detect.so returned (it keeps its own error text)."""
    if rc == 0:
        return
    msg = detect_lib().votenet_detections_last_error().decode()
    if rc == 1:
        raise InvalidArgumentError(msg)
    raise VotenetError("libvotenet_detect error %d: %s" % (rc, msg))


def check_features(rc):
    """check() for a status libvotenet_features.so returned (it keeps its own error text)."""
    if rc == 0:
        return
    msg = features_lib().votenet_point_features_last_error().decode()
    if rc == 1:
        raise InvalidArgumentError(msg)
    raise VotenetError("libvotenet_features error %d: %s" % (rc, msg))


def check_guard(rc):
    """check() for a status libvotenet_guard.so returned (it keeps its own error text)."""
    if rc == 0:
        return
    msg = guard_lib().votenet_step_guard_last_error().decode()
    if rc == 1:
        raise InvalidArgumentError(msg)
    raise VotenetError("libvotenet_guard error %d: %s" % (rc, msg))


def check_monitors(rc):
    """check() for a status libvotenet_monitors.so returned (it keeps its own error text)."""
    if rc == 0:
        return
    msg = monitors_lib().votenet_monitors_last_error().decode()
    if rc == 1:
        raise InvalidArgumentError(msg)
    raise VotenetError("libvotenet_monitors error %d: %s" % (rc, msg))


def check(rc):
    if rc == 0:
        return
    msg = lib().votenet_last_error().decode()
    if rc == 1:
        raise InvalidArgumentError(msg)
    raise VotenetError("libvotenet_hip error %d: %s" % (rc, msg))


# The host side of a train step is ~250 launches: the Python objects behind torch.cuda.current_stream() / torch.cuda.device(...)
# were a quarter of its enqueue time (cProfile, tools/probe/host_profile.py).  The raw-handle calls below are what those wrappers
# end up calling.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def stream_ptr():
    """The current HIP stream of the current device as a void* for the C ABI."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())  # (a plain int: ctypes converts it)
    return torch.cuda.current_stream().cuda_stream


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NOGUARD = _NoGuard()


def device_guard(device):
    """`with device_guard(t.device):` the launches inside run on t's device.  One process per GPU is the rule here, so the device
    almost always IS the current one: then this is a shared no-op object instead of a torch.cuda.device context."""
    idx = device.index
    if _cur_device is not None and (idx is None or idx == _cur_device()):
        return _NOGUARD
    return torch.cuda.device(device)


def ptr(t):
    """The device address of a tensor for a void* argument (a plain int: ctypes converts it; no c_void_p object per argument)."""
    return t.data_ptr() if t is not None else None


def dev_f32(t, name, rank=None, last=None):
    """Validate a float32 device tensor the way the TF wrappers validate shapes; return contiguous."""
    if not isinstance(t, torch.Tensor):
        raise InvalidArgumentError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise VotenetError("%s must live on the GPU (no CPU fallback in votenet_amd)" % name)
    if t.dtype != torch.float32:
        raise InvalidArgumentError("%s must be float32" % name)
    if rank is not None and t.dim() != rank:
        raise InvalidArgumentError("%s expects rank %d, got shape %s" % (name, rank, tuple(t.shape)))
    if last is not None and t.shape[-1] != last:
        raise InvalidArgumentError("%s expects last dimension %d, got shape %s" % (name, last, tuple(t.shape)))
    return t.contiguous()


def dev_i32(t, name, rank=None):
    if not isinstance(t, torch.Tensor):
        raise InvalidArgumentError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise VotenetError("%s must live on the GPU (no CPU fallback in votenet_amd)" % name)
    if t.dtype != torch.int32:
        raise InvalidArgumentError("%s must be int32" % name)
    if rank is not None and t.dim() != rank:
        raise InvalidArgumentError("%s expects rank %d, got shape %s" % (name, rank, tuple(t.shape)))
    return t.contiguous()
