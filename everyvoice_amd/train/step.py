"""What both trainers do around and inside a step: its environment (``step_scope``), the trainer's own stream joined to the caller's
(``on_own_stream``), a chain beside the main one (``SideBranch``), the captured-step policy (``CapturedStep``) and the data-parallel
gradient exchange (``BucketReducer``)."""

import torch

from . import ops
from .autograd import Tape, Var


class step_scope(ops.mode):
    """``with step_scope(device, operands=..., side_wgrad=...):`` one training step's environment: the operator switches (``ops.mode``),
    and nothing an aborted step left collected reaches this one.  A body that raises: the step's device is drained and what it collected
    dropped (``ops.side_reset``) before the switches go back; a clean one: every backward chain must have joined its weight gradients."""

    def __init__(self, device, *, operands, side_wgrad, seed_base=ops.UNSET, ln_defer=None):
        super().__init__(operands, side_wgrad, seed_base, ln_defer)
        self.device = device

    def __enter__(self):
        super().__enter__()
        ops.side_reset()
        return self

    def __exit__(self, exc_type, *exc):
        try:
            if exc_type is not None:
                ops.side_reset(abort=True, device=self.device)
        finally:
            super().__exit__(exc_type, *exc)
        if exc_type is None:
            ops.side_check_drained()
        return False


def on_own_stream(stream, device, fn, *args):
    """``fn(*args)`` on `stream`, behind what the caller's stream holds; the caller's stream then waits for it -> (result, caller's stream)."""
    caller = torch.cuda.current_stream(device)
    stream.wait_stream(caller)
    with torch.cuda.stream(stream):
        out = fn(*args)
    caller.wait_stream(stream)
    return out, caller


def _held_tensors(fns, depth: int = 4) -> list:
    """Every tensor the closures `fns` (tape operators) can reach through their cells: Vars, dicts, lists, nested closures."""
    out, seen = [], set()

    def visit(o, d):
        if id(o) in seen or d < 0:
            return
        seen.add(id(o))
        if torch.is_tensor(o):
            out.append(o)
        elif isinstance(o, Var):
            visit(o.data, d)
            visit(o.grad, d)
        elif isinstance(o, dict):
            for v in o.values():
                visit(v, d - 1)
        elif isinstance(o, (list, tuple)):
            for v in o:
                visit(v, d - 1)
        elif callable(o) and getattr(o, "__closure__", None):
            for c in o.__closure__:
                try:
                    visit(c.cell_contents, d - 1)
                except ValueError:  # (an empty cell)
                    pass

    for f in fns:
        visit(f, depth)
    return out


class SideBranch:
    """A chain that runs beside the main chain and is joined later: a stream (given, or a new one of `device`), ONE fork and ONE done
    event re-recorded on every use (a wait takes the record that precedes it in host order), a tape of its own and the tensors it keeps
    alive until the join.  Not `enabled`: every operation runs inline on the current stream and the joins do nothing -- the same
    operators in the same order, so both forms leave the same bits.  ``begin()`` opens a step's use, ``close()`` ends it.

    What holds for every such chain, and is written down here only:
    - What the branch's operators hold must outlive their KERNELS, not just their launches.  An operator that drops a tensor once it
      has launched (``packed.clear()``, a Var going out of scope) hands the block back to the pool of the stream that allocated it, and
      that stream's next allocation may write it while the branch still reads it: ``backward`` keeps ``_held_tensors`` of its tape
      until ``close``.
    - A tensor allocated under the branch and used (and released) under the main stream is handed over with ``record_stream``; that
      applies outside graph capture only (a capture's pool is private to the graph): ``hand_over``.
    - The branch IS a side chain: its backward runs under ``ops.mode(side_wgrad=False)``, its weight gradients stay on its stream.
    - A captured stretch must not end with a fork open: every ``fork`` / ``backward`` that records done is followed by a ``join`` (an
      operator of the main tape, the ``join`` of a ``Tape.cut``) or by ``close`` inside the same stretch.  A join waits ONCE and
      forgets the event: a later stretch must not wait on an event that belongs to an earlier one."""

    def __init__(self, device, stream=None, enabled: bool = True):
        self.device, self.stream = device, stream
        if enabled:
            self.stream = stream if stream is not None else torch.cuda.Stream(device)
            self._fork, self._done = torch.cuda.Event(), torch.cuda.Event()
        self.begin(enabled)

    def begin(self, enabled: bool = True):
        """A new use (a step): an empty tape, nothing kept, nothing pending.  A branch constructed enabled may sit a step out."""
        self.enabled = bool(enabled) and self.stream is not None
        self.tape, self.kept, self._pending = Tape(), [], None
        return self

    def fork(self, fn, *args, done: bool = True):
        """``fn(*args)`` on the branch, behind everything queued so far on the current stream -> its result.  ``done=False``: no done
        event (the branch's next use follows on the same stream: the predictors' backward behind their forward)."""
        if not self.enabled:
            return fn(*args)
        self._fork.record(torch.cuda.current_stream(self.device))
        self.stream.wait_event(self._fork)
        with torch.cuda.stream(self.stream):
            out = fn(*args)
            if done:
                self._done.record(self.stream)
        if done:
            self._pending = self._done
        return out

    def _tape_backward(self):
        with ops.mode(side_wgrad=False):
            self.kept += _held_tensors(self.tape._ops)
            self.tape.backward()

    def backward(self):
        """The backward of the branch's tape, forked here (an empty tape: nothing, so a second call is harmless)."""
        if not self.tape._ops:
            return
        if not self.enabled:
            return self.tape.backward()
        self.fork(self._tape_backward)

    def hand_over(self, *tensors):
        """`tensors` were allocated under the branch; the current stream uses and releases them."""
        if self.enabled and not torch.cuda.is_current_stream_capturing():
            cur = torch.cuda.current_stream(self.device)
            for t in tensors:
                t.record_stream(cur)

    def join(self):
        """The current stream waits for what the branch has recorded as done -- once."""
        if self._pending is not None:
            torch.cuda.current_stream(self.device).wait_event(self._pending)
            self._pending = None

    def close(self):
        """Join if nothing needed the branch's results so far, then let go of what was kept."""
        self.join()
        self.kept = []


class HipCapture:
    """The stretches of one captured step: each call records what `fn` launches on `stream` (and the streams forked from it) into a
    graph of its own, all of them in one memory pool."""

    def __init__(self, device, stream):
        torch.cuda.synchronize(device)
        self.stream, self.pool = stream, torch.cuda.graph_pool_handle()

    def __call__(self, fn):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self.pool, stream=self.stream, capture_error_mode="thread_local"):
            fn()
        return g


EAGER = "eager"


class CapturedStep:
    """Base of the trainers: a step of a fixed shape (the trainer's key) runs eagerly the first GRAPH_WARMUP_STEPS times it is seen
    (workspaces grow, kernel attributes are set), is captured the next time -- as one graph, or as several stretches with an exchange
    behind each (RCCL calls are not captured) -- and replayed from then on.  Any failure while capturing falls back to eager execution
    for good (``_graph_failed`` holds the reason).  The trainer has ``device`` and ``_stream`` and says what its host-side counters are
    (the step's code bumps them, but capturing executes nothing): ``_host_counters() -> state``, ``_set_host_counters(state)`` and
    ``_count_replay(entry)``, which advances them by the step a replay has run on the device."""

    GRAPH_WARMUP_STEPS = 2
    GRAPH_CACHE = None      # captured keys kept (least recently used out first); None: all
    GRAPH_WARM_KEYS = None  # the table of keys still warming up is cleared beyond this many; None: never

    def _graph_init(self):
        self._graphs, self._graph_warm, self._graph_failed = {}, {}, None

    def _capture_failed(self):
        """Host-side state of an aborted capture that the eager step must not find (beyond the counters)."""

    def _graph_entry(self, key, record, keep_eager=False, capture=HipCapture):
        """The captured step for `key`, or EAGER: not seen often enough yet, `keep_eager`, or capturing failed (now or before).
        ``record(cap) -> dict``: issues the step as ``cap(fn, then=None)`` calls, one per stretch (`then`: the exchange behind it),
        and returns what the trainer keeps with the entry (static inputs, outputs)."""
        if self._graph_failed is not None:
            return EAGER
        entry = self._graphs.get(key)
        if entry is not None:
            self._graphs[key] = self._graphs.pop(key)  # most recently used last
            return entry
        n = self._graph_warm.get(key, 0)
        if n < self.GRAPH_WARMUP_STEPS or keep_eager:
            self._graph_warm[key] = n + 1
            if self.GRAPH_WARM_KEYS is not None and len(self._graph_warm) > self.GRAPH_WARM_KEYS:
                self._graph_warm.clear()
            return EAGER
        counters = self._host_counters()
        graphs, after = [], []
        try:
            stretch = capture(self.device, self._stream)
            entry = dict(graphs=graphs, after=after, **record(lambda fn, then=None: (graphs.append(stretch(fn)), after.append(then))))
        except Exception as e:  # noqa: BLE001 -- whatever the runtime objected to: the eager path is always available
            self._graph_failed = f"{type(e).__name__}: {e}"
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            ops.side_reset()  # the aborted capture's collected weight-gradient launches and events must not reach the eager step
            self._capture_failed()
            return EAGER
        finally:
            self._set_host_counters(counters)  # (also after a capture that went well: replay bumps them again)
        self._graphs[key] = entry
        while self.GRAPH_CACHE is not None and len(self._graphs) > self.GRAPH_CACHE:
            self._graphs.pop(next(iter(self._graphs)))
        return entry

    def _replay(self, entry):
        for g, then in zip(entry["graphs"], entry["after"]):
            g.replay()
            if then is not None:
                then()  # the gradient exchange behind this stretch: RCCL calls sit between the captured stretches
        self._count_replay(entry)  # the host-side counters follow the device-side ones the graphs increment


# ---- data-parallel gradient exchange -----------------------------------------------------------------------------------------------
def scale_(t: torch.Tensor, sc: float):
    """t *= sc on the device (the 1 / world of a gradient mean)."""
    return ops.elementwise(ops.EW_SCALE, t, out=t, p0=sc)


def allreduce_mean_(flat_grad: torch.Tensor, process_group, scale_fn=scale_) -> torch.Tensor:
    """flat_grad <- mean over ranks (sum all-reduce, then ``scale_fn(flat_grad, 1 / world)``)."""
    import torch.distributed as dist

    dist.all_reduce(flat_grad, op=dist.ReduceOp.SUM, group=process_group)
    scale_fn(flat_grad, 1.0 / dist.get_world_size(process_group))
    return flat_grad


class BucketReducer:
    """Data-parallel gradient exchange overlapped with backward: the flat gradient buffer of one optimiser is
    reduced in contiguous buckets, each launched -- asynchronously, on a side stream when the buffer lives on a GPU -- the
    moment backward has finished the last layer that writes into it; ``finish()`` waits for all of them and applies the
    1/world scaling.  Backward visits the layers in reverse declaration order, so finished gradients form a growing suffix
    of the buffer: ``launch(lo, hi)`` is called with adjacent, descending ranges.  RCCL over xGMI under backend "nccl"."""

    def __init__(self, flat_grad: torch.Tensor, process_group, scale_fn=scale_):
        self.flat, self.pg, self.scale_fn = flat_grad, process_group, scale_fn
        self.works = []
        self.stream = torch.cuda.Stream(flat_grad.device) if flat_grad.is_cuda else None
        self.timing = None  # a list: every launch appends (start, end) events on the side stream (bench.py: all-reduce ms per step)

    def launch(self, lo: int, hi: int) -> None:
        import torch.distributed as dist

        if hi <= lo:
            return
        chunk = self.flat[lo:hi]
        if self.stream is not None:
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(self.flat.device))  # gradients of this bucket are final from here on
            with torch.cuda.stream(self.stream):
                self.stream.wait_event(ready)
                if self.timing is not None:
                    e0 = torch.cuda.Event(enable_timing=True)
                    e0.record(self.stream)
                # RCCL: enqueued behind `ready` on the side stream, runs while the launching stream goes on with backward
                work = dist.all_reduce(chunk, op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
                if self.timing is not None:  # (measurement runs only: order the side stream behind the collective, then stamp)
                    work.wait()
                    e1 = torch.cuda.Event(enable_timing=True)
                    e1.record(self.stream)
                    self.timing.append((e0, e1))
                else:
                    self.works.append(work)
        else:
            self.works.append(dist.all_reduce(chunk, op=dist.ReduceOp.SUM, group=self.pg, async_op=True))

    def finish(self) -> None:
        import torch.distributed as dist

        for w in self.works:
            w.wait()
        self.works.clear()
        if self.stream is not None:
            torch.cuda.current_stream(self.flat.device).wait_stream(self.stream)
        self.scale_fn(self.flat, 1.0 / dist.get_world_size(self.pg))

    def comm_ms(self, reset: bool = True) -> float:
        """Summed device time of the recorded all-reduces (synchronises)."""
        if not self.timing:
            return 0.0
        self.timing[-1][1].synchronize()
        ms = sum(a.elapsed_time(b) for a, b in self.timing)
        if reset:
            self.timing.clear()
        return ms
