"""CPU: the training summaries' ABI (votenet_accuracies, votenet_tensor_stats), the float64 restatement the GPU tests compare against
(monitors_ref) on hand-made cases, the host side of Monitors.read() on numpy stand-ins, and the histogram's bucket rule."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import monitors_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"votenet_accuracies": 21, "votenet_tensor_stats": 8, "votenet_monitors_last_error": 0}  # name -> parameters, counted by hand in the header


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {name: (0 if params.strip() == "void" else params.count(",") + 1)
            for name, params in re.findall(r"\b(votenet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


@pytest.fixture(scope="module")
def monlib(hiplib):
    """libvotenet_monitors.so, built by the same build as the main library."""
    from votenet_amd import _lib
    return _lib.side_lib("monitors")


def test_header_declares_the_new_entries_and_the_library_exports_them_and_nothing_else(monlib):
    """include/votenet_monitors.h declares the entries, libvotenet_monitors.so exports exactly them (functions only), and the drop-in
    library exports what its own two headers declare -- nothing new came with the summaries."""
    from votenet_amd import _lib
    assert _declared("votenet_monitors.h") == NEW
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.side_path("monitors")], capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines()]
    assert all(r[1] in "Tt" for r in rows), rows
    assert {r[2] for r in rows} == set(NEW)
    main, debug = _declared("votenet_hip.h"), _declared("votenet_hip_debug.h")
    assert not (set(NEW) & (set(main) | set(debug)))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[2] for line in out.splitlines() if line.split()[2].startswith("votenet_")}
    assert exported == set(main) | set(debug), sorted(exported ^ (set(main) | set(debug)))
    for name, arity in NEW.items():
        fn = getattr(monlib, name)  # bound from the header when the library was loaded
        assert len(fn.argtypes) == arity, name
        assert fn.restype is (ctypes.c_char_p if name == "votenet_monitors_last_error" else ctypes.c_int), name
    V, I, F, Lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
    assert monlib.votenet_accuracies.argtypes == [I, I, I, I, I, I, V, V, Lg, V, V, F, F, V, V, I, I, V, V, V, V]
    assert monlib.votenet_tensor_stats.argtypes == [I, V, V, F, F, V, V, V]


def test_existing_loss_entries_keep_their_signatures(hiplib):
    """The summaries are additions: the loss entries are declared as before (27 / 28 parameters, twelve losses)."""
    main = _declared("votenet_hip.h")
    assert main["votenet_loss"] == 27 and main["votenet_loss_pitched"] == 28 and main["votenet_clip_adam"] == 15
    from votenet_amd import loss as VL
    assert len(VL.NAMES) == 12 and VL.NAMES[10:] == ("n_pos", "n_neg") and not [n for n in VL.NAMES if "accuracy" in n]


def test_a_missing_monitors_library_is_an_error(monkeypatch, tmp_path):
    from votenet_amd import _lib
    monkeypatch.delitem(_lib._side, "monitors", raising=False)
    monkeypatch.setattr(_lib, "_LIB_PATH", str(tmp_path / "libvotenet_hip.so"))  # the side libraries lie beside the main one
    with pytest.raises(_lib.VotenetError, match="no CPU fallback"):
        _lib.side_lib("monitors")


def test_argument_validation_without_a_device(monlib):
    hiplib = monlib
    f = ctypes.c_float
    p = ctypes.c_void_p(16)
    assert hiplib.votenet_accuracies(0, 4, 2, 12, 10, 10, p, p, 79, p, p, f(0.3), f(0.6), None, None, 0, 0, p, p, p, None) == 1
    assert b"b, n_prop, n_box > 0" in hiplib.votenet_monitors_last_error()
    assert hiplib.votenet_accuracies(1, 4, 257, 12, 10, 10, p, p, 79, p, p, f(0.3), f(0.6), None, None, 0, 0, p, p, p, None) == 1
    assert b"at most 256 boxes" in hiplib.votenet_monitors_last_error()
    assert hiplib.votenet_accuracies(1, 4, 2, 12, 10, 10, p, p, 78, p, p, f(0.3), f(0.6), None, None, 0, 0, p, p, p, None) == 1
    assert b"pitch" in hiplib.votenet_monitors_last_error()
    assert hiplib.votenet_accuracies(1, 4, 2, 12, 10, 10, p, p, 79, p, p, f(0.3), f(0.6), None, p, 100, 100, p, p, p, None) == 1
    assert b"ring_row" in hiplib.votenet_monitors_last_error()
    assert hiplib.votenet_accuracies(1, 4, 2, 12, 10, 10, p, p, 79, p, p, f(0.3), f(0.6), None, None, 0, 0, p, p, None, None) == 1
    assert b"null buffer" in hiplib.votenet_monitors_last_error()
    assert hiplib.votenet_tensor_stats(0, p, p, f(1.0), f(0.0), p, p, None) == 1
    assert hiplib.votenet_tensor_stats(3, p, ctypes.c_void_p(20), f(1.0), f(0.0), p, p, None) == 1
    assert b"16-byte aligned" in hiplib.votenet_monitors_last_error()


def test_constants_agree_with_the_header():
    from votenet_amd import loss as VL
    from votenet_amd import monitors as MON
    text = open(os.path.join(ROOT, "include", "votenet_monitors.h")).read()
    macro = lambda n: int(re.search(r"#define %s (\d+)" % n, text).group(1))
    assert macro("VOTENET_MONITOR_RING_COLS") == VL.RING_COLS == len(MON.RING_NAMES)
    assert macro("VOTENET_TENSOR_HIST_BINS") == MON.HIST_BINS == R.HIST_BINS
    assert macro("VOTENET_TENSOR_STATS_FLOATS") == MON.STATS_FLOATS and macro("VOTENET_TENSOR_STATS_INTS") == MON.STATS_INTS == 1 + MON.HIST_BINS
    assert macro("VOTENET_ACCURACIES_WORKSPACE_INTS") == 8


# ---- monitors_ref on hand-made cases ------------------------------------------------------------------------------------------

def test_in_top_1_is_tensorflows_in_top_k():
    assert R.in_top_1([0.5, 0.5], 1) and R.in_top_1([0.5, 0.5], 0)            # a tie counts as correct
    assert R.in_top_1([0.0, 1.0], 1) and not R.in_top_1([0.0, 1.0], 0)
    assert not R.in_top_1([0.0, np.nan], 1) and R.in_top_1([np.nan, 0.0], 1)   # a NaN target is wrong, a NaN rival does not win
    assert not R.in_top_1([np.inf, 0.0], 0) and not R.in_top_1([-np.inf, -np.inf], 0)  # the target's score must be finite
    assert not R.in_top_1([1.0, 2.0], 2) and not R.in_top_1([1.0, 2.0], -1)    # a label outside the classes is never correct


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_reference_on_hand_made_cases(name):
    prop, out, gt, want = R.HAND_CASES[name]()
    got = R.accuracies(prop, out, gt)
    for k, v in want.items():
        assert got[k] == v or (isinstance(v, float) and math.isnan(v) and math.isnan(got[k])), (k, got[k], v)
    if name == "no_positive":
        assert math.isnan(got["sem_accuracy"]) and math.isfinite(got["obj_accuracy"]) and got["n_pos"] == 0
    if name == "tie":
        assert got["obj_accuracy"] == 7 / 8  # both tied rows correct; all-correct would be 8 / 8
    if name == "nan_target":
        assert got["n_obj_correct"] == 6 and got["n_sem_correct"] == 1


# ---- the host side of read() --------------------------------------------------------------------------------------------------

def _ring(window, steps, rows):
    """What the device ring holds after `steps` steps that wrote rows[0], rows[1], ...: row i at i % window."""
    ring = np.zeros((window, 5), np.float32)
    for i in range(steps):
        ring[i % window] = rows[i]
    return ring


def test_summarize_ring_not_full_wrapped_and_nan():
    from votenet_amd import monitors as MON
    rows = np.arange(35, dtype=np.float32).reshape(7, 5) / 8
    assert MON.summarize_ring(_ring(4, 0, rows), 0) == (None, None)
    last, mean = MON.summarize_ring(_ring(4, 3, rows), 3)          # not yet full: the mean of three rows, not of four
    assert list(last.values()) == rows[2].tolist() and list(last) == list(MON.RING_NAMES)
    assert list(mean.values()) == rows[:3].astype(np.float64).mean(0).tolist()
    last, mean = MON.summarize_ring(_ring(4, 7, rows), 7)          # wrapped: the last four rows, the newest at (7 - 1) % 4
    assert list(last.values()) == rows[6].tolist()
    assert list(mean.values()) == rows[3:7].astype(np.float64).mean(0).tolist()
    rows[5, 1] = np.nan                                             # a step without positives: its column's average is NaN, the others not
    last, mean = MON.summarize_ring(_ring(4, 7, rows), 7)
    assert math.isnan(mean["sem_accuracy"]) and mean["obj_accuracy"] == float(rows[3:7, 0].astype(np.float64).mean())
    assert not math.isnan(last["sem_accuracy"])
    last, mean = MON.summarize_ring(_ring(4, 10, np.concatenate([rows, rows[:3] + 9])), 10)  # rows 6..9: the NaN row has left the window
    assert not math.isnan(mean["sem_accuracy"])


def test_tensor_table_from_the_launch_outputs():
    from votenet_amd import monitors as MON
    stats = np.array([[6.0, 14.0, 1.0, 3.0, 1.0], [0.0, 0.0, np.inf, -np.inf, np.nan]], np.float32)
    hist = np.zeros((2, 131), np.int32)
    hist[0, 1 + 41] = 1
    hist[0, 1 + 42] = 2
    hist[1, 0], hist[1, 1 + 129] = 2, 2
    t = MON.tensor_table(["a/W", "b/W"], [3, 2], stats, hist)
    assert t["a/W"]["mean"] == 2.0 and t["a/W"]["rms"] == math.sqrt(14 / 3) and t["a/W"]["nonfinite"] == 0 and t["a/W"]["hist"].sum() == 3
    assert t["b/W"]["nonfinite"] == 2 and math.isnan(t["b/W"]["mean"]) and math.isnan(t["b/W"]["rms"]) and math.isnan(t["b/W"]["clip_factor"])


# ---- the histogram's bucket rule ----------------------------------------------------------------------------------------------

BINS_BY_HAND = [(0.0, 0), (-0.0, 0), (1e-40, 0), (-1e-40, 0),       # zeros and subnormals
                (2.0 ** -41, 1), (-2.0 ** -41, 65),                    # below the range: clamped to e = -40
                (2.0 ** -40, 1), (-2.0 ** -40, 65),
                (1.0, 41), (-1.0, 105), (1.5, 41), (2.0, 42), (0.5, 40),
                (2.0 ** 24 - 1, 64), (-(2.0 ** 24 - 1), 128),          # e = 23
                (2.0 ** 24, 64), (-2.0 ** 24, 128),                    # above the range: clamped to e = 23
                (np.inf, 129), (-np.inf, 129), (np.nan, 129)]


def test_histogram_bucket_rule():
    from votenet_amd import monitors as MON
    vals = np.array([v for v, _ in BINS_BY_HAND], np.float32)
    assert MON.hist_bin(vals).tolist() == [b for _, b in BINS_BY_HAND]
    assert [R.hist_bin(v) for v in vals] == [b for _, b in BINS_BY_HAND]
    assert MON.hist_bin_label(0) == "0" and MON.hist_bin_label(41) == "+2^0" and MON.hist_bin_label(105) == "-2^0"
    assert MON.hist_bin_label(1) == "+2^-40" and MON.hist_bin_label(128) == "-2^23" and MON.hist_bin_label(129) == "nonfinite"
    rng = np.random.default_rng(0)   # the two restatements agree on random bit patterns too
    bits = rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert MON.hist_bin(bits).tolist() == [R.hist_bin(v) for v in bits]


def test_reference_tensor_stats_on_a_small_bucket():
    x = np.array([1.0, -2.0, 0.0, np.inf, 3.0, np.nan, 1e-40], np.float32)
    rows = R.tensor_stats(x, [(0, 3), (3, 4), (4, 7)], clip=0.5)
    assert rows[0]["sum"] == -1.0 and rows[0]["sumsq"] == 5.0 and rows[0]["min"] == -2.0 and rows[0]["max"] == 1.0 and rows[0]["nonfinite"] == 0
    assert rows[0]["clip_factor"] == 0.5 / max(math.sqrt(5.0) / 3, 0.5)
    assert rows[1]["nonfinite"] == 1 and rows[1]["min"] == np.inf and rows[1]["max"] == -np.inf and rows[1]["hist"][129] == 1
    assert rows[2]["nonfinite"] == 1 and rows[2]["hist"][0] == 1 and rows[2]["max"] == 3.0 and rows[2]["min"] == np.float32(1e-40)


def test_enable_monitors_is_off_by_default():
    from votenet_amd import model as VM
    assert VM.VoteNetHotPath.monitors is None and VM.VoteNetHotPath.last_accuracies is None
    assert callable(VM.VoteNetHotPath.enable_monitors) and callable(VM.VoteNetHotPath.disable_monitors)
