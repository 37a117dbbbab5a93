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
_lib = None
# The side libraries: each feature that must stay out of the drop-in library's export list is libvotenet_<name>.so beside it, built
# from csrc/<name>/ (csrc/build.sh has the same rows), with its own header and its own error text.  name -> header under include/.
SIDE_LIBS = {
    "monitors": "votenet_monitors.h",        # the training summaries
    "guard": "votenet_step_guard.h",         # the guarded optimizer step
    "features": "votenet_point_features.h",  # the input step with point features
    "detect": "votenet_detections.h",        # class-wise 3D NMS, per-class detections and their matching
    "boxpts": "votenet_box_points.h",        # points inside predicted boxes, the empty-box gate
    "aabb": "votenet_aabb_nms.h",            # the axis-aligned overlaps of the paper's NMS
    "depth": "votenet_depth_scan.h",         # the raw scan from the depth image
    "votesup": "votenet_vote_supervision.h",  # the paper's vote supervision, one launch behind the loss
    "propsup": "votenet_proposal_supervision.h",  # the paper's objectness and centre supervision, one launch behind the loss
    "votesamp": "votenet_vote_sampling.h",   # the proposal module's clusters sampled on the votes, one launch
    "instbox": "votenet_instance_boxes.h",   # ground-truth boxes from instance-labelled points
    "instvote": "votenet_instance_votes.h",  # vote supervision from instance labels, one launch behind the loss
    "unitvote": "votenet_unit_votes.h",      # unit-length vote features as in the authors' VoteNet, in place of the voting glue launches
}
_side = {}  # name -> (the loaded library, its *_last_error function)


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
        objs = [o for d in ["obj"] + [os.path.join(name, "obj") for name in SIDE_LIBS] for o in glob.glob(os.path.join(_HERE, "csrc", d, "*.o"))]
        for f in [_LIB_PATH] + [side_path(name) for name in SIDE_LIBS] + objs:
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


def side_path(name):
    """Where libvotenet_<name>.so of SIDE_LIBS lies: beside the main library."""
    return os.path.join(os.path.dirname(_LIB_PATH), "libvotenet_%s.so" % name)


def side_loaded(name):
    return name in _side


def side_lib(name):
    """libvotenet_<name>.so, loaded when something of it is first asked for; every function of its header gets the header's prototype
    (parse_header, as for the main library).  No fallback: a missing library is an error."""
    if name not in _side:
        path = side_path(name)
        if not os.path.exists(path):
            raise VotenetError("libvotenet_%s.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)" % (name, path))
        with open(os.path.join(_HERE, os.pardir, "include", SIDE_LIBS[name])) as f:
            protos = parse_header(f.read(), {})
        S = ctypes.CDLL(path)
        for fname, (restype, argtypes) in protos.items():
            fn = getattr(S, fname)
            fn.restype, fn.argtypes = restype, argtypes
        last_error, = [getattr(S, fname) for fname in protos if fname.endswith("_last_error")]  # each library keeps its own text
        _side[name] = (S, last_error)
    return _side[name][0]


def check(rc, side=None):
    """Raise what a status means, with the text of the library that returned it: the main library's, or side library `side`'s."""
    if rc == 0:
        return
    if side is None:
        msg, who = lib().votenet_last_error().decode(), "hip"
    else:
        side_lib(side)
        msg, who = _side[side][1]().decode(), side
    if rc == 1:
        raise InvalidArgumentError(msg)
    raise VotenetError("libvotenet_%s error %d: %s" % (who, rc, msg))


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


def pitched_rows(t):
    """Whether t is 3-D rows with unit column stride at one uniform pitch: what a kernel that takes a row pitch reads in place."""
    return t.dim() == 3 and t.stride(2) == 1 and t.stride(1) >= t.shape[2] and t.stride(0) == t.shape[1] * t.stride(1)


def dev_f32_rows(t, name):
    """A 3-D float32 device tensor for a kernel that takes a row pitch: t itself where pitched_rows(t), else dev_f32's errors or copy."""
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and pitched_rows(t):
        return t
    return dev_f32(t, name, 3)


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
