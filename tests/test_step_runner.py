"""What both trainers share around a step (everyvoice_amd/train/step.py) and the scoped operator switches (ops.mode), on the CPU:
the bookkeeping only -- a fake stands in for the HIP graph capture."""

import pytest
import torch

from everyvoice_amd.train import ops, step


def _switches():
    return ops.CONV_BACKEND["operands"], ops.SIDE_WGRAD["on"], ops.SEED_BASE[0], ops.LN_DEFER["on"]


def test_mode_restores_on_exit_and_when_the_body_raises():
    before = _switches()
    base = torch.zeros(1)
    with ops.mode(operands="bf16", side_wgrad=True, seed_base=base, ln_defer=True):
        assert _switches() == ("bf16", True, base, True)
    assert _switches() == before
    with pytest.raises(KeyError):
        with ops.mode(operands="bf16", side_wgrad=True, seed_base=base, ln_defer=True):
            raise KeyError("from the body")
    assert _switches() == before


def test_mode_nests():
    before = _switches()
    with ops.mode(operands="bf16", side_wgrad=True):
        with ops.mode(operands="f32"):
            assert _switches()[:2] == ("f32", True)
            with ops.exact_f32():
                assert _switches()[:2] == ("f32", False)
            assert _switches()[:2] == ("f32", True)
        assert _switches()[:2] == ("bf16", True)
    assert _switches() == before


def test_mode_leaves_unspecified_switches_alone():
    before = _switches()
    try:
        with ops.mode(operands="bf16"):
            assert _switches() == ("bf16",) + before[1:]
            ops.LN_DEFER["on"] = not before[3]  # not this scope's: neither set on the way in nor put back on the way out
        assert _switches() == (before[0], before[1], before[2], not before[3])
        with ops.mode(seed_base=None):  # None is a value of the seed base, not "not given"
            assert ops.SEED_BASE[0] is None
    finally:
        ops.LN_DEFER["on"] = before[3]


def _queued_side_state():
    st = object.__new__(ops._SideState)  # (its constructor makes a HIP stream)
    st.pending, st.keep, st.queue, st.keep_next = object(), [torch.zeros(1)], [lambda: None], [torch.zeros(1)]
    return st


def test_step_scope_restores_and_empties_the_side_queue_when_the_body_raises(monkeypatch):
    st = _queued_side_state()
    monkeypatch.setattr(ops, "_SIDE", {0: st})
    before = _switches()
    base = torch.zeros(1)
    with pytest.raises(KeyError):
        with step.step_scope(torch.device("cpu"), operands="bf16", side_wgrad=True, seed_base=base, ln_defer=True):
            assert _switches() == ("bf16", True, base, True)
            assert st.queue == [] and st.pending is None  # what an aborted step before this one left is gone on the way in
            st.queue.append(lambda: None)
            st.keep.append(torch.zeros(1))
            st.pending = object()
            raise KeyError("from the step")
    assert _switches() == before
    assert st.queue == [] and st.keep == [] and st.keep_next == [] and st.pending is None


def test_step_scope_checks_that_a_clean_step_drained_its_weight_gradients(monkeypatch):
    st = _queued_side_state()
    monkeypatch.setattr(ops, "_SIDE", {0: st})
    before = _switches()
    with pytest.raises(RuntimeError, match="never issued"):
        with step.step_scope(torch.device("cpu"), operands="bf16", side_wgrad=False):
            st.queue.append(lambda: None)  # a backward chain that ended without its wgrad_join
    assert _switches() == before


class _Trainer(step.CapturedStep):
    """Counts what the policy asks of a trainer; `capture` is the stand-in for HipCapture."""

    def __init__(self, bound=None, fail=None):
        self.GRAPH_CACHE = bound
        self.device, self._stream = torch.device("cpu"), None
        self._graph_init()
        self.counter, self.captures, self.failure_hooks, self.log, self.fail = 0, 0, 0, [], fail

    def _host_counters(self):
        return self.counter

    def _set_host_counters(self, state):
        self.counter = state

    def _count_replay(self, entry):
        self.counter += 1

    def _capture_failed(self):
        self.failure_hooks += 1

    def capture(self, device, stream):
        assert device is self.device and stream is self._stream

        def stretch(fn):
            self.captures += 1
            if self.fail is not None:
                raise RuntimeError(self.fail)
            fn()
            return _Graph(self.log, len(self.log_names) - 1)

        self.log_names = []
        return stretch

    def record(self, cap):
        self.counter += 7  # the recorded step's code bumps the host counters although nothing runs
        cap(lambda: self.log_names.append("a"), lambda: self.log.append("after 0"))
        cap(lambda: self.log_names.append("b"))
        cap(lambda: self.log_names.append("c"), lambda: self.log.append("after 2"))
        return dict(inputs="static")

    def entry(self, key):
        return self._graph_entry(key, self.record, capture=self.capture)


class _Graph:
    def __init__(self, log, i):
        self.log, self.i = log, i

    def replay(self):
        self.log.append(f"graph {self.i}")


def test_capture_policy_warms_up_then_captures_once():
    tr = _Trainer()
    for _ in range(tr.GRAPH_WARMUP_STEPS):
        assert tr.entry("k") == "eager" and tr.captures == 0
    e = tr.entry("k")
    assert e != "eager" and tr.captures == 3 and tr.counter == 0  # captured; the counters are back where they were
    assert len(e["graphs"]) == len(e["after"]) == 3 and e["inputs"] == "static"
    assert tr.entry("k") is e and tr.captures == 3
    assert tr._graph_failed is None and list(tr._graphs) == ["k"]


def test_capture_policy_keep_eager_never_captures():
    tr = _Trainer()
    for _ in range(tr.GRAPH_WARMUP_STEPS + 3):
        assert tr._graph_entry("k", tr.record, keep_eager=True, capture=tr.capture) == "eager"
    assert tr.captures == 0


def test_failed_capture_latches_and_restores():
    tr = _Trainer(fail="the runtime said no")
    tr.counter = 5
    for _ in range(tr.GRAPH_WARMUP_STEPS + 1):
        assert tr.entry("k") == "eager"
    assert tr._graph_failed == "RuntimeError: the runtime said no"
    assert tr.counter == 5 and tr.failure_hooks == 1 and tr.captures == 1 and not tr._graphs
    tr.fail = None
    for key in ("k", "k", "k", "other", "other", "other"):
        assert tr.entry(key) == "eager"
    assert tr.captures == 1 and tr.failure_hooks == 1  # never again


def _capture_key(tr, key):
    for _ in range(tr.GRAPH_WARMUP_STEPS):
        assert tr.entry(key) == "eager"
    assert tr.entry(key) != "eager"


def test_bounded_cache_evicts_the_least_recently_used_key():
    tr = _Trainer(bound=2)
    _capture_key(tr, "a")
    _capture_key(tr, "b")
    assert tr.entry("a") != "eager"  # looked up: "b" is now the least recently used
    _capture_key(tr, "c")
    assert set(tr._graphs) == {"a", "c"}


def test_unbounded_cache_keeps_every_key():
    tr = _Trainer(bound=None)
    keys = [f"k{i}" for i in range(40)]
    for key in keys:
        _capture_key(tr, key)
    assert list(tr._graphs) == keys


def test_replay_calls_each_exchange_behind_its_graph_and_skips_none():
    tr = _Trainer()
    _capture_key(tr, "k")
    e = tr.entry("k")
    assert e["after"][1] is None
    tr.log.clear()
    tr._replay(e)
    assert tr.log == ["graph 0", "after 0", "graph 1", "graph 2", "after 2"]
    assert tr.counter == 1  # the host counters follow the replayed step
