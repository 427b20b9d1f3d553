"""Host side of the GAN step (everyvoice_amd/train/hifigan.py) without a GPU: the routing table of the generator step's discriminator
pass, the library calls and collectives of whole steps on ``device="cpu"`` (tools/gan_step_digest.py on the recorder of
tools/ops_call_trace.py: no library is loaded) and the lifetime of the step object's tensors."""

import gc
import importlib.util
import weakref
from collections import Counter
from pathlib import Path

import pytest

from everyvoice_amd.train.hifigan import _DiscFacts, g_step_routing, routing_pyramids

_spec = importlib.util.spec_from_file_location("gan_step_digest", Path(__file__).resolve().parent.parent / "tools" / "gan_step_digest.py")
digest = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(digest)


def _facts(n_periods, scales):
    """scales: one bool per scale discriminator, True = spectral norm; stream slots as the trainer's constructor counts them."""
    flags = [False] * n_periods + list(scales)
    out, slot = [], 0
    for i, sn in enumerate(flags):
        out.append(_DiscFacts(sn, max(0, i - n_periods), slot))
        slot += 2 if sn else 1
    return out


DEFAULT = _facts(5, [True, False, False])  # 5 period discriminators, 3 scales, the first spectral-norm


def _rows(chains):
    return [(c.disc, c.role, c.kind, c.level) for c in chains]


def _host_order(chains):
    return [c.branch for c in sorted(chains, key=lambda c: c.order)]


def test_default_model_facts():
    assert [f.slot for f in DEFAULT] == [0, 1, 2, 3, 4, 5, 7, 8]  # the spectral-norm scale: slots 5 and 6
    assert [f.scale for f in DEFAULT] == [0, 0, 0, 0, 0, 0, 1, 2]
    assert [f.reads_waveform for f in DEFAULT] == [True] * 6 + [False] * 2


def test_two_call_routing_of_the_default_model():
    chains = g_step_routing(DEFAULT, pair_mode=False)
    assert [c.branch for c in chains] == list(range(17))
    levels = [0, 0, 0, 0, 0, 0, 1, 2]
    assert _rows(chains[:8]) == [(i, "g_fake", "fake", levels[i]) for i in range(8)]
    assert _rows(chains[8:16]) == [(i, "g_real", "real", levels[i]) for i in range(8)]
    assert _rows(chains[16:]) == [(None, "recon", None, 0)]
    # the spectral-norm scale (discriminator 5) hands out its real call first
    assert _host_order(chains) == [8 + 5] + [j for j in range(17) if j != 13]
    assert routing_pyramids(chains) == ["real", "fake"]


def test_pair_routing_of_the_default_model():
    chains = g_step_routing(DEFAULT, pair_mode=True)
    assert [c.branch for c in chains] == list(range(10))
    levels = [0, 0, 0, 0, 0, 0, 1, 2]
    assert _rows(chains[:8]) == [(i, "g_fake", "fake", 0) if i == 5 else (i, "g_both", "pair", levels[i]) for i in range(8)]
    assert _rows(chains[8:]) == [(5, "g_real", "real", 0), (None, "recon", None, 0)]
    assert _host_order(chains) == [8, 0, 1, 2, 3, 4, 5, 6, 7, 9]
    assert routing_pyramids(chains) == ["pair"]  # real and generated waveforms are read unpooled only


def test_routing_without_pooled_scales():
    facts = _facts(2, [True])
    two = g_step_routing(facts, pair_mode=False)
    assert _rows(two) == [(0, "g_fake", "fake", 0), (1, "g_fake", "fake", 0), (2, "g_fake", "fake", 0),
                          (0, "g_real", "real", 0), (1, "g_real", "real", 0), (2, "g_real", "real", 0), (None, "recon", None, 0)]
    assert _host_order(two) == [5, 0, 1, 2, 3, 4, 6]
    assert routing_pyramids(two) == []  # nothing behind a pooling: no pyramid level is ever read
    pair = g_step_routing(facts, pair_mode=True)
    assert _rows(pair) == [(0, "g_both", "pair", 0), (1, "g_both", "pair", 0), (2, "g_fake", "fake", 0), (2, "g_real", "real", 0), (None, "recon", None, 0)]
    assert _host_order(pair) == [3, 0, 1, 2, 4]
    assert routing_pyramids(pair) == ["pair"]


def test_routing_with_a_spectral_norm_scale_behind_the_pooling():
    facts = _facts(2, [False, True, False])  # (not in the upstream model)
    pair = g_step_routing(facts, pair_mode=True)
    assert _rows(pair) == [(0, "g_both", "pair", 0), (1, "g_both", "pair", 0), (2, "g_both", "pair", 0), (3, "g_fake", "fake", 1), (4, "g_both", "pair", 2),
                           (3, "g_real", "real", 1), (None, "recon", None, 0)]
    assert _host_order(pair) == [5, 0, 1, 2, 3, 4, 6]
    assert routing_pyramids(pair) == ["pair", "real", "fake"]  # its two calls read pooled real and pooled generated waveforms
    two = g_step_routing(facts, pair_mode=False)
    assert [c.role for c in two] == ["g_fake"] * 5 + ["g_real"] * 5 + ["recon"]
    assert _host_order(two) == [5 + 3] + [j for j in range(11) if j != 8]
    assert routing_pyramids(two) == ["real", "fake"]


def _recorder():
    import sys

    sys.path.insert(0, str(Path(digest.__file__).resolve().parent))
    import ops_call_trace

    return ops_call_trace


def _is_collective(call):
    return call[0] in ("d.launch", "d.finish", "g.launch", "g.finish")


@pytest.mark.parametrize("warm", [False, True], ids=["gan_step", "warmup_step"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_data_parallel_and_single_process_steps_issue_the_same_library_calls(precision, warm):
    settings = dict(precision=precision, generator_warmup_steps=1 if warm else 0)
    (single,) = digest.trace_config(settings, steps=1)
    (dp,) = digest.trace_config(dict(settings, process_group=True), steps=1)
    assert not [c for c in single if _is_collective(c)]
    collectives = [c for c in dp if _is_collective(c)]
    library = [c for c in dp if not _is_collective(c)]
    key = lambda c: repr(c)  # noqa: E731
    assert Counter(map(key, library)) == Counter(map(key, single))
    if warm:  # no discriminator step: nothing for the bucket schedule to reorder
        assert library == single
    # the collectives: the discriminators' two bucket groups, the padding in front, then the generator's buffer from the top down
    from everyvoice_amd.train.hifigan import HiFiGANTrainer

    oct = _recorder()
    with oct.recording():
        oct.REC.begin([], {})
        tr = HiFiGANTrainer(device="cpu", seed=5, **settings)
    ds = tr.discriminators()
    d_want = []
    if not warm:
        d_want = [["d.launch", list(tr._bucket_range(tr.d_params, [layer for i in idxs for layer in ds[i].layers()]))] for idxs in tr.d_bucket_groups()]
        d_want += [["d.launch", [0, min(tr.d_params.offset_of(n) for n in tr.d_params.names())]], ["d.finish", []]]
    assert collectives[: len(d_want)] == d_want
    g = collectives[len(d_want):]
    assert g[-1] == ["g.finish", []] and all(c[0] == "g.launch" for c in g[:-1]) and len(g) > 2
    ranges = [tuple(c[1]) for c in g[:-1]]
    assert ranges[0][1] == tr.g_params.grad.numel() and ranges[-1][0] == 0
    assert all(lo < hi for lo, hi in ranges) and all(a[0] == b[1] for a, b in zip(ranges, ranges[1:]))  # they tile [0, numel)


@pytest.mark.parametrize("data_parallel", [False, True], ids=["single", "data_parallel"])
def test_the_step_objects_tensors_are_released(data_parallel):
    """After ``training_step`` returns, or raises inside a phase, the trainer holds no reference to the step's tensors."""
    from everyvoice_amd.train.hifigan import HiFiGANTrainer

    oct = _recorder()
    mel, y = digest._batch("cpu")
    with oct.recording():
        oct.REC.begin([], {})
        tr = HiFiGANTrainer(device="cpu", seed=5, process_group=True if data_parallel else None)
        if data_parallel:
            tr._dp_reducers = (digest._RecordingReducer("d", oct.REC), digest._RecordingReducer("g", oct.REC))
        seen = []
        update = tr._phase_g_update

        def watching(step, fail=False):
            seen.append((weakref.ref(step.y_hat.data), weakref.ref(step.g_tape), step))
            if fail:
                raise RuntimeError("raised inside a phase")
            update(step)

        tr._phase_g_update = watching
        tr.training_step(mel, y, sync=False)
        tr._phase_g_update = lambda step: watching(step, fail=True)
        with pytest.raises(RuntimeError, match="raised inside a phase"):
            tr.training_step(mel, y, sync=False)
    gc.collect()
    assert len(seen) == 2
    for y_hat_data, g_tape, step in seen:
        assert step.y is None and step.y_hat is None and step.g_tape is None and step.d_ins is None and step.g_segments is None
        assert y_hat_data() is None and g_tape() is None
