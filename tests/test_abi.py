"""CPU: the C-ABI library loads, exports every symbol include/votenet_hip.h declares (and the
reference's own launcher names), and validates arguments like the reference's OP_REQUIRES checks.
No compute is launched here (no GPU)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(headers=("votenet_hip.h", "votenet_hip_debug.h")):
    syms = set()
    for h in headers:
        text = open(os.path.join(ROOT, "include", h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        syms |= set(re.findall(r"\b(votenet_[a-z0-9_]+)\s*\(", text))
    return sorted(syms)


LAUNCHERS = ["farthestpointsamplingLauncher(int, int, int, float const*, float*, int*)",
             "gatherpointLauncher(int, int, int, float const*, int const*, float*)",
             "scatteraddpointLauncher(int, int, int, float const*, int const*, float*)",
             "queryBallPointLauncher(int, int, int, float, int, float const*, float const*, int*, int*)",
             "groupPointLauncher(int, int, int, int, int, float const*, int const*, float*)",
             "groupPointGradLauncher(int, int, int, int, int, float const*, int const*, float*)",
             "probsampleLauncher(int, int, int, float const*, float const*, float*, int*)",
             "selectionSortLauncher(int, int, int, int, float const*, int*, float*)"]


def test_export_list_is_exactly_the_two_headers_plus_the_eight_launchers(hiplib):
    """The drop-in library exports the C ABI it declares and the reference's launcher names -- no kernel stubs, no votenet:: internals,
    no global variables (csrc/exports.map, -fvisibility=hidden)."""
    from votenet_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = set()
    for line in out.splitlines():
        parts = line.split(None, 2)
        assert parts[1] in "Tt", "a non-function export: " + line   # no data symbols (the old g_* switches)
        exported.add(parts[2])
    assert exported == set(declared_symbols()) | set(LAUNCHERS), sorted(exported ^ (set(declared_symbols()) | set(LAUNCHERS)))
    assert not [s for s in exported if "votenet::" in s]
    # the switches are all in the debug header, none in the drop-in one
    assert not [s for s in declared_symbols(("votenet_hip.h",)) if "debug" in s]


def test_debug_switches_are_inert_until_the_host_opts_in():
    """include/votenet_hip_debug.h: a consumer that never calls votenet_debug_enable(1) gets launches that depend on their arguments only.
    Own process (the suite's shared handle has long opted in)."""
    import sys
    from votenet_amd import _lib
    code = (
        "import ctypes, os, sys\n"
        "os.environ.pop('VOTENET_DEBUG', None)\n"
        "L = ctypes.CDLL(sys.argv[1])\n"
        "L.votenet_last_error.restype = ctypes.c_char_p\n"
        "assert L.votenet_debug_enabled() == 0\n"
        "L.votenet_debug_fast_bf3(0)\n"
        "assert b'debug switches are disabled' in L.votenet_last_error(), L.votenet_last_error()\n"
        "assert L.votenet_debug_enabled() == 0\n"
        "L.votenet_debug_enable(1)\n"
        "assert L.votenet_debug_enabled() == 1\n"
        "L.votenet_debug_enable(0)\n"
        "assert L.votenet_debug_enabled() == 0\n"
        "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code, _lib.lib_path()], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    env = dict(os.environ, VOTENET_DEBUG="1")
    code2 = ("import ctypes, sys\nL = ctypes.CDLL(sys.argv[1])\nL.votenet_debug_fast_bf3(1)\nassert L.votenet_debug_enabled() == 1\nprint('ok')\n")
    r = subprocess.run([sys.executable, "-c", code2, _lib.lib_path()], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_python_host_opts_in_on_first_switch_lookup(hiplib):
    from votenet_amd import _lib
    L = _lib.lib()
    L.votenet_debug_gram_workgroups  # a lookup is enough
    assert L.votenet_debug_enabled() == 1


def test_header_declares_the_path():
    syms = declared_symbols()
    for must in ["votenet_farthest_point_sample", "votenet_gather_point", "votenet_gather_point_grad",
                 "votenet_query_ball_point", "votenet_group_point", "votenet_group_point_grad", "votenet_three_nn",
                 "votenet_three_interpolate", "votenet_three_interpolate_grad", "votenet_nms3d", "votenet_mlp_linear"]:
        assert must in syms


def test_library_exports_every_declared_symbol(hiplib):
    for name in declared_symbols():
        assert hasattr(hiplib, name), "libvotenet_hip.so does not export %s" % name


def test_library_exports_reference_launcher_names(hiplib):
    """tf_sampling.cpp:65,94,125,150 and tf_grouping.cpp:66,108,142,173 declare these eight (C++ linkage)."""
    from votenet_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", _lib.lib_path()], capture_output=True, text=True).stdout
    for sig in LAUNCHERS:
        assert sig in out, sig
    assert out.count("Launcher(") == 8


def test_reference_wrappers_link_with_no_undefined_symbol(linklib):
    """The drop-in link line of INTEGRATION.md 1 with -Wl,-z,defs (the conftest fixture asserts the link) and a dlopen RTLD_NOW."""
    for name in ("link_prob_sample", "link_fps", "link_gather", "link_scatter_add", "link_query_ball", "link_selection_sort",
                 "link_group", "link_group_grad"):
        assert hasattr(linklib, name)


def test_link_fails_when_a_launcher_is_missing(hiplib, tmp_path):
    """The link test has teeth: a ninth, unexported launcher name makes the same link line fail."""
    from votenet_amd import _lib
    libdir = os.path.dirname(_lib.lib_path())
    src = tmp_path / "missing.cpp"
    src.write_text("void notALauncher(int b);\nextern \"C\" void f(int b) { notALauncher(b); }\n")
    r = subprocess.run(["g++", "-shared", "-fPIC", "-Wl,-z,defs", str(src), "-o", str(tmp_path / "m.so"), "-L" + libdir, "-lvotenet_hip"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "notALauncher" in r.stderr


def test_version_and_error_text(hiplib):
    assert b"gfx950" in hiplib.votenet_version()
    rc = hiplib.votenet_farthest_point_sample(1, 10, 0, None, None, None, None)
    assert rc == 1  # VOTENET_E_INVALID_ARGUMENT
    assert b"positive npoint" in hiplib.votenet_last_error()  # tf_sampling.cpp:99


def test_argument_validation_mirrors_op_requires(hiplib):
    f = ctypes.c_float
    assert hiplib.votenet_query_ball_point(1, 8, 4, f(0.0), 4, None, None, None, None, None) == 1
    assert b"positive radius" in hiplib.votenet_last_error()  # tf_grouping.cpp:71
    assert hiplib.votenet_query_ball_point(1, 8, 4, f(0.1), 0, None, None, None, None, None) == 1
    assert b"positive nsample" in hiplib.votenet_last_error()  # tf_grouping.cpp:74
    assert hiplib.votenet_nms3d(1, 4, None, None, None, f(1.5), None, ctypes.c_void_p(8), None, 0, None) == 1
    assert b"iou_threshold must be in [0, 1]" in hiplib.votenet_last_error()  # tf_nms3d.cpp:300
    # empty problems are accepted without touching the device
    assert hiplib.votenet_gather_point(0, 8, 4, None, None, None, None) == 0
    assert hiplib.votenet_group_point(2, 8, 3, 0, 4, None, None, None, None) == 0
    assert hiplib.votenet_three_nn(0, 0, 0, None, None, None, None, None) == 0


def test_ball_threshold_table(hiplib):
    """T(r) = smallest fp32 with sqrtf(T) >= r; differs from r*r for most radii."""
    table = {0.2: 0.03999999910593033, 0.4: 0.1599999964237213, 0.8: 0.6399999856948853, 1.2: 1.440000057220459,
             0.3: 0.09000000357627869, 0.1: 0.009999999776482582}
    for r, t in table.items():
        got = hiplib.votenet_ball_threshold(ctypes.c_float(np.float32(r)))
        assert np.float32(got) == np.float32(t), (r, got, t)
        r32 = np.float32(r)
        assert np.sqrt(np.float32(got), dtype=np.float32) >= r32
        assert np.sqrt(np.nextafter(np.float32(got), np.float32(0)), dtype=np.float32) < r32


def test_workspace_queries(hiplib):
    assert hiplib.votenet_fps_temp_floats(8, 2048) == 0                         # register-resident, brute force
    work = 16 * 4096 + 6 * 16 + 8                                               # per-workgroup cell histograms + partial bounds
    # the spatial index: Morton permutation + bucket boxes + sorted float4 points + work (also what the indexed ball query reads)
    assert hiplib.votenet_fps_temp_floats(8, 20480) == 8 * (20480 + 6 * 320 + 256 * 320 + work) + 4
    # 24 576 < n <= 98 304: behind the index, the exchange words of the scene-over-several-workgroups kernel ([b][2][12][5] x 8 bytes + alignment)
    assert hiplib.votenet_fps_temp_floats(4, 80000) == 4 * (80000 + 6 * 1250 + 256 * 1250 + work) + 4 + 4 * 2 * 12 * 5 * 2 + 4
    assert hiplib.votenet_fps_temp_floats(1, 140000) == hiplib.votenet_spatial_index_floats(1, 140000)
    assert hiplib.votenet_spatial_index_floats(8, 20480) == hiplib.votenet_fps_temp_floats(8, 20480)
    assert hiplib.votenet_fps_temp_floats(4, 300000) == 4 * 300000              # unpruned streaming fallback
    assert hiplib.votenet_fps_temp_floats(64, 300000) == 32 * 300000            # tf_sampling.cpp:115: 32 rows whatever the batch
    assert hiplib.votenet_nms3d_workspace_bytes(8, 256) >= 8 * 256 * 256 * 4


def test_no_cpu_fallback_in_python_ops(hiplib):
    import torch
    from votenet_amd import VotenetError, tf_grouping, tf_interpolate, tf_sampling
    x = torch.zeros(1, 16, 3)
    with pytest.raises(VotenetError):
        tf_sampling.farthest_point_sample(4, x)
    with pytest.raises(VotenetError):
        tf_grouping.query_ball_point(0.1, 4, x, x)
    with pytest.raises(VotenetError):
        tf_interpolate.three_nn(x, x)


def test_build_force_is_a_clean_build(monkeypatch, tmp_path):
    """build(force=True) removes the library AND every cached object file before build.sh runs (round-3 verdict: it used to relink
    the cached csrc/obj/*.o).  The compile itself is stubbed out: the files live in a scratch copy of the package layout."""
    from votenet_amd import _lib
    here = tmp_path / "votenet_amd"
    (here / "csrc" / "obj").mkdir(parents=True)
    (here / "csrc" / "guard" / "obj").mkdir(parents=True)  # a side library's files go with the main library's
    (here / "lib").mkdir()
    objs = [here / "csrc" / "obj" / n for n in ("fps.o", "mlp_fast.o")] + [here / "csrc" / "guard" / "obj" / "step_guard.o"]
    for f in objs + [here / "lib" / "libvotenet_hip.so", here / "lib" / "libvotenet_guard.so"]:
        f.write_bytes(b"stale")
    seen = {}

    def fake_run(cmd, **kw):
        seen["left"] = sorted(p.name for p in (here / "csrc" / "obj").iterdir()) + sorted(p.name for p in (here / "lib").iterdir())
        seen["guard"] = sorted(p.name for p in (here / "csrc" / "guard" / "obj").iterdir()) + sorted(p.name for p in (here / "lib").glob("*guard*"))
        return subprocess.CompletedProcess(cmd, 0, "", "")
    monkeypatch.setattr(_lib, "_HERE", str(here))
    monkeypatch.setattr(_lib, "_LIB_PATH", str(here / "lib" / "libvotenet_hip.so"))
    monkeypatch.setattr(_lib.subprocess, "run", fake_run)
    _lib.build(force=False)
    assert seen["left"] == ["fps.o", "mlp_fast.o", "libvotenet_guard.so", "libvotenet_hip.so"]   # an incremental build keeps its cache
    assert seen["guard"] == ["step_guard.o", "libvotenet_guard.so"]
    _lib.build(force=True)
    assert seen["left"] == [] and seen["guard"] == []


def test_library_has_no_packed_f32_op_reading_the_high_register_of_src1(hiplib):
    """v_pk_{fma,mul,add}_f32 with op_sel[1] = 1 returns wrong low halves beside another kernel's MFMA wavefronts on MI355X
    (tools/probe/src/pk_opsel_hazard.hip, profiles/r05_pk_opsel_hazard.txt): the form must not be in the shipped code object."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_isa_hazards", os.path.join(ROOT, "tools", "check_isa_hazards.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from votenet_amd import _lib
    found = mod.hazards(_lib.lib_path())
    assert not found, "%d hazardous instructions, e.g. %s in %s" % (len(found), found[0][1], found[0][0])
    # ... and the check sees the form when it is there
    assert mod.BAD.search("v_pk_fma_f32 v[18:19], v[56:57], v[52:53], v[18:19] op_sel:[0,1,0]")
    assert not mod.BAD.search("v_pk_fma_f32 v[18:19], v[52:53], v[56:57], v[18:19] op_sel:[1,0,0]")
    assert not mod.BAD.search("v_pk_fma_f32 v[18:19], v[36:37], v[52:53], v[18:19] op_sel_hi:[1,0,1]")


# ---- the Python prototypes are read from the two headers (votenet_amd/_lib.py: parse_header) ----

def _declared_arity(headers):
    """{function: number of parameters}, counted in the header text itself (not by the reader under test)."""
    out = {}
    for h in headers:
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        for name, params in re.findall(r"\b(votenet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
            out[name] = 0 if params.strip() == "void" else params.count(",") + 1
    return out


def test_every_declared_function_has_its_prototype(hiplib):
    arity = _declared_arity(("votenet_hip.h",))
    assert sorted(arity) == declared_symbols(("votenet_hip.h",)) and len(arity) == 131
    for name, n in arity.items():
        fn = hiplib.__dict__[name]  # bound when the library was loaded, not by this lookup
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
    debug = _declared_arity(("votenet_hip_debug.h",))
    assert sorted(debug) == sorted(set(declared_symbols()) - set(arity)) and len(debug) == 30
    for name, n in debug.items():
        fn = getattr(hiplib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, name
        assert fn.restype is (ctypes.c_int if name == "votenet_debug_enabled" else
                              ctypes.c_uint if name == "votenet_debug_fps_split_timeouts" else None), name


def test_spot_prototypes(hiplib):
    """Hand-read from the headers; together they cover the whole type mapping."""
    from votenet_amd import _lib
    I, L, F, V, Z = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
    want = {
        "votenet_farthest_point_sample": (I, [I, I, I, V, V, V, V]),
        "votenet_query_ball_point": (I, [I, I, I, F, I, V, V, V, V, V]),
        "votenet_nms3d": (I, [I, I, V, V, V, F, V, V, V, Z, V]),
        "votenet_select_boxes": (I, [I, I, V, I, I, V, V, ctypes.c_ulonglong, L, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, V, Z, V]),
        "votenet_mlp_linear": (I, [ctypes.POINTER(_lib.MlpInput), L, I, I, V, V, V, V, V]),
        "votenet_bn_relu": (I, [L, I, V, V, V, ctypes.POINTER(_lib.BnRaw), I, V, V]),
        "votenet_copy_segments": (I, [I, ctypes.POINTER(_lib.CopySegment), V]),
        "votenet_eval_match": (I, [I, I, I, I, V, V, I, V, V, V, V, V, I, V, L, ctypes.c_uint, V, I, V, V, V, V]),
        "votenet_clip_adam": (I, [I, V, V, V, V, V, V, F, F, F, F, I, F, F, V]),
        "votenet_mlp_split_k_floats": (L, [L, I, I]),
        "votenet_fps_temp_floats": (Z, [I, I]),
        "votenet_last_error": (ctypes.c_char_p, []),
        "votenet_half_piece_rows": (I, []),
        "votenet_ball_threshold": (F, [F]),
        "votenet_debug_fps_split_timeouts": (ctypes.c_uint, []),
        "votenet_debug_fast_bf3": (None, [I]),
        "votenet_debug_split_k": (None, [I, I, I, I]),
    }
    for name, (restype, argtypes) in want.items():
        fn = getattr(hiplib, name)
        assert fn.restype is restype, name
        assert len(fn.argtypes) == len(argtypes) and all(a is b for a, b in zip(fn.argtypes, argtypes)), (name, fn.argtypes)
    assert _lib.MlpInput._fields_[4] == ("in_bn", ctypes.POINTER(_lib.BnRaw))
    assert _lib.CoefTail._fields_[:2] == [("ticket", V), ("rows", L)] and _lib.BnRaw._fields_[4] == ("eps", F)


STRUCT_FIELDS = {  # hand-read from include/votenet_hip.h: Python class, C struct, fields in order
    "BnRaw": ("votenet_bn_raw", "stats gamma beta rows eps out"),
    "CoefTail": ("votenet_coef_tail", "ticket rows gamma coef dgamma dbeta"),
    "MlpInput": ("votenet_mlp_input", "x in_scale in_shift in_relu in_bn xyz new_xyz feat idx b n m nsample c"),
    "RowSegment": ("votenet_row_segment", "dst dst_pitch dst_off width a a_pitch a_off b b_pitch b_off"),
    "CopySegment": ("votenet_copy_segment", "dst src bytes"),
}


def test_struct_layout_is_the_compilers(tmp_path):
    """sizeof and every offsetof as g++ lays the header's structs out == what ctypes lays out for the classes read from the header."""
    from votenet_amd import _lib
    lines = ["#include <cstdio>", "#include <cstddef>", '#include "votenet_hip.h"', "int main() {"]
    for cname, fields in STRUCT_FIELDS.values():
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f in fields.split()]
    src = tmp_path / "layout.cpp"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    r = subprocess.run(["g++", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout
    theirs = {tuple(l.split()[:2]): int(l.split()[2]) for l in out.splitlines()}
    ours = {}
    for pyname, (cname, fields) in STRUCT_FIELDS.items():
        cls = getattr(_lib, pyname)
        assert [f for f, _ in cls._fields_] == fields.split()
        ours[(cname, "sizeof")] = ctypes.sizeof(cls)
        ours.update({(cname, f): getattr(cls, f).offset for f in fields.split()})
    assert ours == theirs and len(ours) == 5 + 39


def test_header_reader_has_teeth():
    from votenet_amd._lib import parse_header
    for bad in ("int votenet_x(short a);", "short votenet_x(int a);", "int votenet_x(float **a);", "int votenet_x(int);",
                "int votenet_x(const votenet_nope *p);", "const char *votenet_y(void);\nint votenet_x(const char *s, wchar_t c);"):
        with pytest.raises(ValueError, match="votenet_x"):
            parse_header(bad, {})
    with pytest.raises(ValueError, match="votenet_s.a"):
        parse_header("typedef struct votenet_s { int n; short a; } votenet_s;", {})
    with pytest.raises(ValueError, match="votenet_x"):  # a definition, a macro call: anything that is not a declaration
        parse_header("int votenet_x(int a) { return a; }", {})
    structs = {}
    funcs = parse_header("""
        /* a comment with a declaration inside: int votenet_not(int a); */
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define VOTENET_SOMETHING 3 /* (void) */
        typedef struct votenet_pair {
            const float *gamma, *beta; /* c each */
            int b, n,
                m;
            unsigned *ticket;
        } votenet_pair;
        int votenet_many(int b, const votenet_pair *p /* may be NULL */,
                         unsigned long long seed, unsigned arrival0,
                         double *sums /* 2*c, pre-zeroed */, size_t bytes, void *stream);
        size_t votenet_bytes(void);
        void votenet_set(int on); // trailing
        #ifdef __cplusplus
        }
        #endif
        """, structs)
    I, V = ctypes.c_int, ctypes.c_void_p
    pair = structs["votenet_pair"]
    assert issubclass(pair, ctypes.Structure) and pair.__name__ == "Pair"
    assert pair._fields_ == [("gamma", V), ("beta", V), ("b", I), ("n", I), ("m", I), ("ticket", V)]
    assert funcs == {"votenet_many": (I, [I, ctypes.POINTER(pair), ctypes.c_ulonglong, ctypes.c_uint, V, ctypes.c_size_t, V]),
                     "votenet_bytes": (ctypes.c_size_t, []), "votenet_set": (None, [I])}


# ------------------------------------------------------------------ the side libraries (votenet_amd._lib.SIDE_LIBS), one rule for all
def _side_names():
    from votenet_amd import _lib
    return sorted(_lib.SIDE_LIBS)


@pytest.mark.parametrize("name", _side_names())
def test_side_library_loads_and_exports_exactly_its_header_with_its_prototypes(hiplib, name):
    """libvotenet_<name>.so loads, exports the functions its header declares and nothing else, each bound with the header's prototype."""
    from votenet_amd import _lib
    with open(os.path.join(ROOT, "include", _lib.SIDE_LIBS[name])) as f:
        protos = _lib.parse_header(f.read(), {})
    S = _lib.side_lib(name)
    assert _lib.side_loaded(name) and os.path.basename(_lib.side_path(name)) == "libvotenet_%s.so" % name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.side_path(name)], capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines()]
    assert all(r[1] == "T" for r in rows), rows
    assert sorted(r[2] for r in rows) == sorted(protos) == declared_symbols((_lib.SIDE_LIBS[name],))
    for fname, (restype, argtypes) in protos.items():
        fn = getattr(S, fname)
        assert (fn.restype, list(fn.argtypes or [])) == (restype, argtypes), fname
    last_error, = [fname for fname in protos if fname.endswith("_last_error")]
    assert getattr(S, last_error).restype is ctypes.c_char_p and getattr(S, last_error).argtypes == []


@pytest.mark.parametrize("name", _side_names())
def test_check_raises_with_the_side_library_s_name(hiplib, name):
    from votenet_amd import _lib
    with pytest.raises(_lib.InvalidArgumentError):
        _lib.check(1, side=name)
    with pytest.raises(_lib.VotenetError) as e:
        _lib.check(2, side=name)
    assert str(e.value).startswith("libvotenet_%s error 2" % name)
    _lib.check(0, side=name)


def test_error_texts_are_per_library(hiplib):
    """A failure in one library leaves the text of every other one alone: three libraries fail in turn (status 1, nothing launched), and
    each *_last_error() still returns its own text afterwards."""
    from votenet_amd import _lib
    A, D = _lib.side_lib("aabb"), _lib.side_lib("detect")
    buf = np.zeros(4096, np.float32)
    p = buf.ctypes.data
    assert A.votenet_class_nms_aabb(2, 513, 10, p, p, p, 0.25, 0.0, 1, 1, 0, 0, p, 2 * 513 * 10, p, p, 1 << 20, None) == 1
    assert D.votenet_class_nms3d(2, 513, 10, p, p, p, 0.25, 0.0, 1, 1, p, 2 * 513 * 10, p, p, 1 << 20, None) == 1
    assert hiplib.votenet_farthest_point_sample(1, 10, 0, None, None, None, None) == 1
    aabb, detect, main = A.votenet_aabb_last_error(), D.votenet_detections_last_error(), hiplib.votenet_last_error()
    assert b"class_nms_aabb" in aabb and b"at most 512 boxes per scene, got n = 513" in aabb
    assert b"class_nms3d" in detect and b"at most 512 boxes per scene, got n = 513" in detect and detect != aabb
    assert b"positive npoint" in main and b"512 boxes" not in main
    with pytest.raises(_lib.InvalidArgumentError, match="class_nms_aabb"):
        _lib.check(1, side="aabb")
    with pytest.raises(_lib.InvalidArgumentError, match="class_nms3d"):
        _lib.check(1, side="detect")
    with pytest.raises(_lib.InvalidArgumentError, match="positive npoint"):
        _lib.check(1)
