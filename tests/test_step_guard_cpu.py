"""CPU: the step guard's ABI (include/votenet_step_guard.h, libvotenet_guard.so), the numpy restatement of its verdict and counter rules
on the case table the GPU tests run (tests/step_guard_cases.py), and the argument errors of the Python layer.  Nothing is launched."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_guard_cases as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"votenet_clip_adam_guarded": 19, "votenet_step_guard_state_ints": 0, "votenet_step_guard_last_error": 0}  # counted by hand in the header


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {name: (0 if params.strip() == "void" else params.count(",") + 1)
            for name, params in re.findall(r"\b(votenet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


@pytest.fixture(scope="module")
def guardlib(hiplib):
    """libvotenet_guard.so, built by the same build as the main library."""
    from votenet_amd import _lib
    return _lib.side_lib("guard")


def test_header_declares_the_entries_and_the_library_exports_exactly_them(guardlib):
    """A library of its own: the drop-in library still exports what its two headers declare, votenet_clip_adam included and unchanged."""
    from votenet_amd import _lib
    assert _declared("votenet_step_guard.h") == NEW
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.side_path("guard")], capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines()]
    assert all(r[1] in "Tt" for r in rows), rows
    assert {r[2] for r in rows} == set(NEW)
    main, debug = _declared("votenet_hip.h"), _declared("votenet_hip_debug.h")
    assert not (set(NEW) & (set(main) | set(debug))) and main["votenet_clip_adam"] == 15
    V, I, F, Lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
    fn = guardlib.votenet_clip_adam_guarded
    # votenet_clip_adam's arguments, then ema, ema_snapshot, n_ema, guard_state ahead of the stream
    assert fn.restype is I and fn.argtypes == [I, V, V, V, V, V, V, F, F, F, F, I, F, F, V, V, Lg, V, V]
    assert fn.argtypes[:14] == _lib.lib().votenet_clip_adam.argtypes[:14]
    assert guardlib.votenet_step_guard_last_error.restype is ctypes.c_char_p


def test_constants_agree_with_the_header(guardlib):
    from votenet_amd import mlp as M
    from votenet_amd import step_guard as SG
    text = open(os.path.join(ROOT, "include", "votenet_step_guard.h")).read()
    macro = lambda n: int(re.search(r"#define %s (\d+)" % n, text).group(1))
    assert guardlib.votenet_step_guard_state_ints() == macro("VOTENET_STEP_GUARD_STATE_INTS") == 8
    order = ["VERDICT", "SEEN", "SKIPPED", "CONSECUTIVE", "LAST_SKIP", "EMA_RESTORES"]
    assert [macro("VOTENET_STEP_GUARD_" + n) for n in order] == list(range(6))
    assert SG.COUNTERS == ("seen", "skipped", "consecutive", "last_skip_step", "ema_restores")
    assert C.SLICES == M.SUMSQ_SLICES


def test_argument_validation_without_a_device(guardlib):
    f, p = ctypes.c_float, ctypes.c_void_p(16)
    q = ctypes.c_void_p(32)
    call = lambda nt=1, step=1, ema=None, snap=None, n=0, state=p, buf=p: guardlib.votenet_clip_adam_guarded(
        nt, p, p, buf, p, p, p, f(1e-3), f(0.9), f(0.999), f(1e-8), step, f(1.0), f(0.5), ema, snap, n, state, None)
    assert call(nt=0) == 1 and b"ntensors > 0" in guardlib.votenet_step_guard_last_error()
    assert call(step=0) == 1
    assert call(buf=None) == 1 and b"null buffer" in guardlib.votenet_step_guard_last_error()
    assert call(state=None) == 1 and b"guard_state" in guardlib.votenet_step_guard_last_error()
    assert call(ema=p, snap=None, n=4) == 1 and b"n_ema = 4" in guardlib.votenet_step_guard_last_error()
    assert call(ema=None, snap=None, n=-1) == 1
    assert call(ema=q, snap=q, n=4) == 1 and b"buffer of its own" in guardlib.votenet_step_guard_last_error()


# ---- the verdict and the counters, restated -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def clean():
    return C.bucket(0)


def test_the_bucket_is_what_the_cases_need(clean):
    b, seg = clean
    assert [e - a for a, e in seg] == list(C.LENS) == [1, 257, 32769, 140000]
    assert any(a % 4 for a, _ in seg)  # segments off the 16-byte grid
    for _, scale in C.STEPS_SCALES:    # one tensor above the clip and one below, under both gradient scales
        norms = C.average_norms(b["g"], seg, scale)
        assert norms[0] > C.CLIP and norms[2] > C.CLIP and norms[1] < C.CLIP and norms[3] < C.CLIP, norms
    assert np.isnan(b["g"][:seg[0][0]]).all() and np.isnan(b["g"][seg[-1][1]:]).all()  # NaN padding outside every segment
    a, e = seg[3]
    for k in "pmv":
        assert np.signbit(b[k][a]) and b[k][a] == 0 and 0 < abs(b[k][e - 1]) < 1.2e-38  # a -0.0 and a denormal
    # the positions sit where the table says: which loop of seg_sumsq_kernel reads them
    unrolled = lambda n: (n // C.SWEEP) * C.SWEEP if n % C.SWEEP else n  # elements [0, unrolled) go through the unrolled loop ...
    # (... for these lengths: no thread starts another unrolled iteration, which reads three quarter sweeps ahead, in a shorter remainder)
    assert all(n % C.SWEEP <= 3 * (C.SWEEP // 4) for n in C.LENS[2:])
    assert C.POSITIONS["one_past_a_sweep"][1] == unrolled(C.LENS[2]) and C.POSITIONS["tail_region"][1] >= unrolled(C.LENS[3])
    t, off = C.POSITIONS["unrolled_third_accumulator"]
    assert off < unrolled(C.LENS[t]) and (off % C.SWEEP) // (C.SLICES * C.BLOCK) == 2
    assert C.POSITIONS["last_of_tensor3"][1] == C.LENS[3] - 1 and C.POSITIONS["first_of_tensor0"] == (0, 0)


def test_a_clean_and_an_all_zero_gradient_are_good(clean):
    b, seg = clean
    assert not C.verdict(b["g"], seg)                      # the NaN padding takes no part
    assert not C.verdict(np.zeros_like(b["g"]), seg)


@pytest.mark.parametrize("position,value", C.BAD_CASES)
def test_every_poisoned_case_is_bad_in_exactly_one_partial(clean, position, value):
    b, seg = clean
    g = C.poisoned(b["g"], seg, position, value)
    assert np.isfinite(np.float32(C.VALUES[value])) == (value == "overflow_3e19")
    ps = C.partial_sums(g, seg)
    t, off = C.POSITIONS[position]
    bad = np.argwhere(~np.isfinite(ps)).tolist()
    assert bad == [[t, (off // C.BLOCK) % C.SLICES]] and C.verdict(g, seg)


def test_counter_rules():
    from votenet_amd import step_guard as SG
    s = [0] * 6
    s, r = SG.apply_rules(s, False, False, 1)
    assert s == [0, 1, 0, 0, 0, 0] and not r
    s, r = SG.apply_rules(s, True, False, 2)
    assert s == [1, 2, 1, 1, 2, 1] and r                   # a bad gradient restores the averages too
    s, r = SG.apply_rules(s, True, True, 3)
    assert s == [1, 3, 2, 2, 3, 2] and r
    s, r = SG.apply_rules(s, False, True, 4)
    assert s == [0, 4, 2, 0, 3, 3] and r                   # a good step with poisoned averages: applied, averages restored
    s, r = SG.apply_rules(s, True, False, 5, have_ema=False)
    assert s == [1, 5, 3, 1, 5, 3] and not r               # no averages: nothing to restore, nothing counted
    s, r = SG.apply_rules(s, False, False, 6)
    assert s == [0, 6, 3, 0, 5, 3] and not r


# ---- the Python layer -----------------------------------------------------------------------------------------------------------

def test_the_guard_is_off_by_default_and_needs_an_optimizer(hiplib):
    from votenet_amd import InvalidArgumentError
    from votenet_amd import model as VM
    from votenet_amd import step_guard as SG
    assert VM.VoteNetHotPath.step_guard is None
    assert callable(VM.VoteNetHotPath.enable_step_guard) and callable(VM.VoteNetHotPath.disable_step_guard)
    with pytest.raises(InvalidArgumentError, match="init_optimizer"):
        SG.StepGuard(types.SimpleNamespace())              # no _seg: the optimizer has no state yet
    net = VM.VoteNetHotPath(torch.device("cpu"), seed=0, npoints=(64, 32, 16, 8))
    with pytest.raises(InvalidArgumentError, match="init_optimizer"):
        net.enable_step_guard()
    assert net.step_guard is None
    net.init_optimizer(1e-3)
    g = net.enable_step_guard()
    assert net.step_guard is g and g.state.dtype == torch.int32 and g.state.numel() == 8 and not g.state.any()
    assert g.snapshot is not net._ema_flat and torch.equal(g.snapshot, net._ema_flat)
    assert g.read() == dict(seen=0, skipped=0, consecutive=0, last_skip_step=0, ema_restores=0, last_step_skipped=False)
    net._ema_flat.add_(1.0)
    assert not torch.equal(g.snapshot, net._ema_flat)
    g.refresh_snapshot()
    assert torch.equal(g.snapshot, net._ema_flat)
    net.disable_step_guard()
    assert net.step_guard is None


def test_a_restore_refreshes_the_snapshot(hiplib):
    """checkpoint.load_state_dict rewrites _ema_flat in place: the guard's snapshot follows, or a bad step after a resume would bring
    back the averages from before it."""
    from votenet_amd import model as VM
    a = VM.VoteNetHotPath(torch.device("cpu"), seed=0, npoints=(64, 32, 16, 8))
    b = VM.VoteNetHotPath(torch.device("cpu"), seed=1, npoints=(64, 32, 16, 8))
    for n in (a, b):
        n.init_optimizer(1e-3)
    for t in b._ema_state().values():
        t[2:].add_(0.25)
    g = a.enable_step_guard()
    before = g.snapshot.clone()
    a.load_state_dict(b.state_dict())
    assert torch.equal(a._ema_flat, b._ema_flat) and torch.equal(g.snapshot, a._ema_flat) and not torch.equal(g.snapshot, before)


def test_wrong_state_size_and_mismatched_averages_are_argument_errors(guardlib):
    from votenet_amd import InvalidArgumentError, VotenetError
    from votenet_amd import mlp as M
    seg = torch.tensor([0, 4], dtype=torch.int64)
    x = torch.zeros(4)
    sumsq = torch.zeros(M.SUMSQ_SLICES)
    ok = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(InvalidArgumentError, match="guard_state must be 8"):
        M.clip_adam_guarded(seg, sumsq, x, x, x, x, 1e-3, 1, torch.zeros(6, dtype=torch.int32))
    with pytest.raises(InvalidArgumentError, match="guard_state must be 8"):
        M.clip_adam_guarded(seg, sumsq, x, x, x, x, 1e-3, 1, torch.zeros(8, dtype=torch.int64))
    with pytest.raises(InvalidArgumentError, match="scratch holds"):
        M.clip_adam_guarded(seg, sumsq[:8], x, x, x, x, 1e-3, 1, ok)
    with pytest.raises(InvalidArgumentError, match="go together"):
        M.clip_adam_guarded(seg, sumsq, x, x, x, x, 1e-3, 1, ok, ema=torch.zeros(4))
    with pytest.raises(InvalidArgumentError, match="one size"):
        M.clip_adam_guarded(seg, sumsq, x, x, x, x, 1e-3, 1, ok, ema=torch.zeros(4), ema_snapshot=torch.zeros(5))
    with pytest.raises(VotenetError, match="no CPU fallback"):   # host tensors never reach the launcher
        M.clip_adam_guarded(seg, sumsq, x, x, x, x, 1e-3, 1, ok)


def test_a_missing_guard_library_is_an_error(monkeypatch, tmp_path):
    from votenet_amd import _lib
    monkeypatch.delitem(_lib._side, "guard", raising=False)
    monkeypatch.setattr(_lib, "_LIB_PATH", str(tmp_path / "libvotenet_hip.so"))  # the side libraries lie beside the main one
    with pytest.raises(_lib.VotenetError, match="no CPU fallback"):
        _lib.side_lib("guard")
