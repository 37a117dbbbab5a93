"""CPU: pointnet2.WgradLane -- the weight-gradient side stream's one owner -- driven with recording stand-ins for
torch.cuda.current_stream / set_stream / Event: what is recorded, awaited and made current, in which order, and what the scopes put back.
(That the kernels it launches compute the same step is what the GPU tests of the train step pin.)"""
import pytest
import torch

from votenet_amd import pointnet2 as P


class _Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_event(self, ev):
        self.log.append(("wait", self.name, ev.n))


class _Tensor(torch.Tensor):
    log = None

    def record_stream(self, stream):
        self.log.append(("record_stream", self.tag, stream.name))


class _Cuda:
    """The stand-ins and the sequence they record."""

    def __init__(self, monkeypatch):
        cuda = self
        self.log = []
        self.main = self.current = _Stream("main", self.log)
        self.events = 0

        class Event:
            def __init__(self):
                self.n = cuda.events
                cuda.events += 1

            def record(self, stream):
                cuda.log.append(("record", self.n, stream.name))

        def set_stream(s):
            cuda.current = s
            cuda.log.append(("set", s.name))
        monkeypatch.setattr(torch.cuda, "current_stream", lambda: cuda.current)
        monkeypatch.setattr(torch.cuda, "set_stream", set_stream)
        monkeypatch.setattr(torch.cuda, "Event", Event)

    def stream(self, name):
        return _Stream(name, self.log)

    def tensor(self, tag):
        t = torch.zeros(1).as_subclass(_Tensor)
        t.tag, t.log = tag, self.log
        return t

    def thunk(self, tag):
        def f():
            self.log.append(("thunk", tag, self.current.name))
        return f


@pytest.fixture
def cuda(monkeypatch):
    monkeypatch.setattr(P, "WGRAD_BATCH", False)
    return _Cuda(monkeypatch)


def _state(lane):
    return (lane.stream, lane._fine, lane._keep, lane._defer)


def test_the_module_level_names_are_the_process_lane():
    assert isinstance(P.WGRAD, P.WgradLane) and _state(P.WGRAD) == (None, False, None, None)
    assert not P.WGRAD._deferred and not P.WGRAD._pending
    assert P.on_wgrad_stream == P.WGRAD.run and P.wgrad_flush == P.WGRAD.flush and P.wgrad_join == P.WGRAD.join


def test_without_a_stream_run_calls_the_thunk_at_once(cuda):
    lane = P.WgradLane()
    lane.run(cuda.thunk("a"), cuda.tensor("x"))
    assert cuda.log == [("thunk", "a", "main")] and cuda.events == 0
    with lane.on(None):
        lane.run(cuda.thunk("b"))
        lane.flush()
        lane.join()
    assert cuda.log == [("thunk", "a", "main"), ("thunk", "b", "main")] and cuda.events == 0


def test_a_hand_over_records_on_main_waits_on_the_lane_and_runs_the_thunk_there(cuda):
    lane, side = P.WgradLane(), cuda.stream("side")
    with lane.on(side):
        lane.run(cuda.thunk("a"), cuda.tensor("x"), None, 3, cuda.tensor("y"))  # (only tensors are tracked)
    assert cuda.log == [("record", 0, "main"), ("wait", "side", 0), ("record_stream", "x", "side"), ("record_stream", "y", "side"),
                        ("set", "side"), ("thunk", "a", "side"), ("set", "main")]
    assert cuda.current is cuda.main and lane._pending


def test_main_is_current_again_when_the_thunk_raises(cuda):
    lane, side = P.WgradLane(), cuda.stream("side")

    def boom():
        assert cuda.current is side
        raise RuntimeError("launch failed")
    with pytest.raises(RuntimeError, match="launch failed"):
        with lane.on(side):
            lane.run(boom)
    assert cuda.current is cuda.main and cuda.log[-2:] == [("set", "side"), ("set", "main")]


def test_pooled_events_are_reused_round_robin_and_fresh_while_capturing(cuda):
    lane, side = P.WgradLane(), cuda.stream("side")
    with lane.on(side):
        for _ in range(64 + 3):
            lane.run(lambda: None)
        assert cuda.events == 64
        recorded = [e[1] for e in cuda.log if e[0] == "record"]
        assert recorded[:64] == list(range(64)) and len(set(recorded[64:])) == 3 and set(recorded[64:]) < set(range(64))
        with lane.capturing([]):
            lane.run(lambda: None)
            lane.run(lambda: None)
        assert cuda.events == 66 and [e[1] for e in cuda.log if e[0] == "record"][-2:] == [64, 65]


def test_inside_a_capture_scope_tensors_and_thunks_land_in_the_keep_list(cuda):
    lane, side, keep = P.WgradLane(), cuda.stream("side"), []
    x, f = cuda.tensor("x"), cuda.thunk("a")
    with lane.on(side), lane.capturing(keep):
        lane.run(f, x)
    assert len(keep) == 2 and keep[0] is x and keep[1] == [f]
    assert cuda.log == [("record", 0, "main"), ("wait", "side", 0), ("set", "side"), ("thunk", "a", "side"), ("set", "main")]
    assert _state(lane) == (None, False, None, None)


def test_batch_mode_defers_until_flush_and_hands_all_thunks_over_in_order(cuda, monkeypatch):
    monkeypatch.setattr(P, "WGRAD_BATCH", True)
    lane, side = P.WgradLane(), cuda.stream("side")
    with lane.on(side):
        lane.run(cuda.thunk("a"), cuda.tensor("x"))
        lane.run(cuda.thunk("b"), cuda.tensor("y"))
        lane.run(cuda.thunk("c"))
        assert cuda.log == [] and not lane._pending
        lane.flush()
        assert cuda.log == [("record", 0, "main"), ("wait", "side", 0), ("record_stream", "x", "side"), ("record_stream", "y", "side"),
                            ("set", "side"), ("thunk", "a", "side"), ("thunk", "b", "side"), ("thunk", "c", "side"), ("set", "main")]
        lane.flush()  # nothing left
        assert len(cuda.log) == 9
        del cuda.log[:]
        with lane.fine():
            lane.run(cuda.thunk("d"))
            assert cuda.log == [("record", 1, "main"), ("wait", "side", 1), ("set", "side"), ("thunk", "d", "side"), ("set", "main")]
            lane.run(cuda.thunk("e"))
            assert len(cuda.log) == 10 and cuda.log[8] == ("thunk", "e", "side")
        lane.run(cuda.thunk("f"))  # the fine scope is over: deferred again
        assert len(cuda.log) == 10 and len(lane._deferred) == 1
        lane.flush()
    # deferred thunks flushed without a stream run inline
    with lane.on(side):
        lane.run(cuda.thunk("g"))
    del cuda.log[:]
    lane.flush()
    assert cuda.log == [("thunk", "g", "main")]


def test_join_flushes_first_waits_only_for_something_handed_over_and_clears(cuda, monkeypatch):
    lane, side = P.WgradLane(), cuda.stream("side")
    with lane.on(side):
        lane.join()
        assert cuda.log == [] and cuda.events == 0  # nothing handed over: no wait
        monkeypatch.setattr(P, "WGRAD_BATCH", True)
        lane.run(cuda.thunk("a"))
        lane.join()
        assert cuda.log == [("record", 0, "main"), ("wait", "side", 0), ("set", "side"), ("thunk", "a", "side"), ("set", "main"),
                            ("record", 1, "side"), ("wait", "main", 1)]
        assert not lane._pending and not lane._deferred
        lane.join()
        assert len(cuda.log) == 7  # nothing since the last join
    lane2 = P.WgradLane()
    with lane2.on(side), lane2.fine():
        lane2.run(cuda.thunk("b"))
    del cuda.log[:]
    lane2.join()  # no stream in force: nothing to wait on, the flag stays for the scope that has one
    assert cuda.log == [] and lane2._pending
    with lane2.on(side):
        lane2.join()
    assert [e[0] for e in cuda.log] == ["record", "wait"] and not lane2._pending


def test_a_capture_scope_with_a_defer_list_records_the_launch_and_runs_nothing(cuda):
    lane, side, keep, defer = P.WgradLane(), cuda.stream("side"), [], []
    x, f = cuda.tensor("x"), cuda.thunk("a")
    for stream in (side, None):
        with lane.on(stream), lane.capturing(keep, defer):
            lane.run(f, x, None)
    assert cuda.log == [] and cuda.events == 0 and keep == [] and not lane._pending and not lane._deferred
    assert len(defer) == 2 and all(g is f and len(ts) == 1 and ts[0] is x for g, ts in defer)


def test_hand_over_of_ready_thunks_tracks_no_tensors(cuda):
    lane, side = P.WgradLane(), cuda.stream("side")
    with lane.on(side):
        lane.hand_over([cuda.thunk("a"), cuda.thunk("b")])
    assert cuda.log == [("record", 0, "main"), ("wait", "side", 0), ("set", "side"), ("thunk", "a", "side"), ("thunk", "b", "side"),
                        ("set", "main")]
    assert lane._pending


def test_scopes_restore_what_they_found(cuda):
    lane, s1, s2, keep, defer = P.WgradLane(), cuda.stream("s1"), cuda.stream("s2"), [], []
    with lane.on(s1):
        with lane.on(s2):
            assert lane.stream is s2
        assert lane.stream is s1  # not None
        with lane.on(None):
            assert lane.stream is None
            lane.run(cuda.thunk("inline"))
        assert lane.stream is s1 and cuda.log == [("thunk", "inline", "main")]
        with lane.fine():
            with lane.fine():
                assert lane._fine
            assert lane._fine
        assert not lane._fine
        with lane.capturing(keep, defer):
            with lane.capturing([], None):
                assert lane._keep == [] and lane._keep is not keep and lane._defer is None
            assert lane._keep is keep and lane._defer is defer and lane.stream is s1
        assert _state(lane) == (s1, False, None, None)
    assert _state(lane) == (None, False, None, None)


def test_scopes_restore_what_they_found_on_exceptional_exit(cuda, monkeypatch):
    monkeypatch.setattr(P, "WGRAD_BATCH", True)
    lane, s1, s2, keep = P.WgradLane(), cuda.stream("s1"), cuda.stream("s2"), []
    with lane.on(s1):
        lane.run(cuda.thunk("a"))
        with lane.fine():
            lane.run(cuda.thunk("b"))
        assert len(lane._deferred) == 1 and lane._pending
        for inner in (s2, None):
            with pytest.raises(KeyError):
                with lane.on(inner), lane.fine(), lane.capturing(keep, []):
                    raise KeyError("inner")
            # the outer scope is still in force, with its deferred thunk and its pending flag: only the OUTERMOST scope drops them
            assert _state(lane) == (s1, False, None, None) and len(lane._deferred) == 1 and lane._pending
    assert _state(lane) == (None, False, None, None) and len(lane._deferred) == 1 and lane._pending  # a normal exit keeps both


def test_an_exception_escaping_the_outermost_scope_leaves_no_deferred_thunk_and_no_pending_flag(cuda, monkeypatch):
    monkeypatch.setattr(P, "WGRAD_BATCH", True)
    lane, side = P.WgradLane(), cuda.stream("side")
    with pytest.raises(ValueError):
        with lane.on(side):
            with lane.fine():
                lane.run(cuda.thunk("a"))  # handed over: pending
            with lane.on(None):
                lane.run(cuda.thunk("b"))
                lane.run(cuda.thunk("c"))  # (no stream: inline)
            lane.run(cuda.thunk("d"))      # deferred
            assert lane._pending and len(lane._deferred) == 1
            raise ValueError("the pass failed")
    assert _state(lane) == (None, False, None, None) and lane._deferred == [] and not lane._pending
    del cuda.log[:]
    with lane.on(side):  # the next pass starts clean: no stale thunk is launched, no wait on a stream nobody used
        lane.flush()
        lane.join()
    assert cuda.log == []
