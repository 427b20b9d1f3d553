"""Prosody steering of FastSpeech2 on the device (csrc/fs2_prosody.hip, fs2.py, pipeline.py):

  1. the two generalised kernels against the ones they generalise, bit for bit, and ``evmi_fs2_variance_apply_f32`` alone against torch
     in fp32 (every value is one multiplication or one addition: ``torch.equal``);
  2. the fit kernel against its restatement (``tests/fs2_prosody_ref.fit_ref``), exactly on the lattice where double sums are exact,
     by its invariants on random fp32 weights;
  3. the whole model on ``FastSpeech2ConfigRef.small()`` against ``tests/fs2_prosody_ref.forward_prosody_ref``: durations and lengths
     equal, everything else within 2e-4 of the oracle's scale.  The restatement asserts that no predicted value sits within 1e-3 of a
     bin edge or a rounding boundary; the model seeds below are the first ones at which that holds (found on the CPU);
  4. the default path issues none of the new entry points;
  5. teacher forcing of the variances and ``target_seconds`` through the synthesis helpers."""

import math

import pytest
import torch

from everyvoice_amd import _lib
from tests.fs2_prosody_ref import fit_ref, fit_shares_ref, forward_prosody_ref, symbol_of_frame
from tests.test_gpu_fs2 import _close
from tests.test_gpu_fs2_levels import FRAME, PHONE, _inference_pair, inference_ref

pytestmark = pytest.mark.gpu


def call(fn, *args):
    """fn(...) with tensors passed as their pointers (None as NULL); the tensors stay referenced until the launch has been issued."""
    return fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else 0 if a is None else a for a in args])


def stream(dev):
    return _lib.current_stream_ptr(dev)


def i32(values, dev):
    return torch.tensor(list(values), dtype=torch.int32, device=dev)


def lib():
    return _lib.load()


SHAPES = [(1, 1, 2), (3, 37, 24), (2, 300, 256)]  # (B, n, D); 2 x 300 columns cross a 256-thread block, 256 channels eight channel slices
INF = torch.tensor(float("inf"))


def _lens_for(B, n):
    return [n, max(1, n // 2), max(1, n - 1)][:B]


def _apply(dev, x, pred, bins, table, lens, forced=None, control=None, cum=None, scalar=1.0):
    """evmi_fs2_variance_apply_f32 on copies -> (x, used) on the host."""
    D, B, n = x.shape
    n_bins = table.shape[0]
    L = cum.shape[1] if cum is not None else n
    xd, used = x.to(dev), torch.full((B, n), -1234.5, device=dev)
    hold = [t if t is None else t.to(dev) for t in (pred, forced, control, cum)]
    rc = call(lib().evmi_fs2_variance_apply_f32, xd, hold[0], hold[1], 0 if forced is None else forced.shape[1], hold[2],
              None if hold[3] is None else hold[3].to(torch.int32), i32(lens, dev), bins.to(dev), table.to(dev), used, n_bins, B, L, n, D, scalar,
              stream(dev))
    assert rc == _lib.EVMI_OK, lib().evmi_last_error()
    return xd.cpu(), used.cpu()


# =====================================================================================================================
# 1. the generalised kernels
# =====================================================================================================================
@pytest.mark.parametrize("scalar", [1.0, 1.3])
@pytest.mark.parametrize("B,n,D", SHAPES)
def test_variance_apply_is_bucket_embed_add_without_steering(cuda_device, B, n, D, scalar):
    dev, n_bins = cuda_device, 16
    g = torch.Generator().manual_seed(B * 1000 + n)
    lens = _lens_for(B, n)
    pad = torch.arange(n)[None] >= torch.tensor(lens)[:, None]
    pred = (torch.randn(B, n, generator=g) * 2.0).masked_fill(pad, 0.0)  # (a predictor's output: zero at the padded columns)
    x, table, bins = torch.randn(D, B, n, generator=g), torch.randn(n_bins, D, generator=g), torch.linspace(-3.0, 3.0, n_bins - 1)
    want = x.to(dev)
    assert call(lib().evmi_fs2_bucket_embed_add_f32, want, pred.to(dev), bins.to(dev), table.to(dev), n_bins, B, n, D, scalar, stream(dev)) == _lib.EVMI_OK
    got, used = _apply(dev, x, pred, bins, table, lens, scalar=scalar)
    assert torch.equal(got, want.cpu())
    assert torch.equal(used, pred * torch.tensor(scalar, dtype=torch.float32))


@pytest.mark.parametrize("scalar", [1.0, 1.3])
@pytest.mark.parametrize("B,L,_D", SHAPES)
def test_durations_ctl_is_durations_without_a_control(cuda_device, B, L, _D, scalar):
    dev = cuda_device
    g = torch.Generator().manual_seed(B * 1000 + L)
    log_d = torch.rand(B, L, generator=g) * 4.0 - 1.0
    lens = i32(_lens_for(B, L), dev)
    want, got = (torch.full((B, L), -7, dtype=torch.int32, device=dev) for _ in range(2))
    assert call(lib().evmi_fs2_durations_i32, log_d.to(dev), lens, want, B, L, scalar, stream(dev)) == _lib.EVMI_OK
    assert call(lib().evmi_fs2_durations_ctl_i32, log_d.to(dev), lens, None, got, None, B, L, scalar, stream(dev)) == _lib.EVMI_OK
    assert torch.equal(got, want) and int(want.max()) > 0


def test_durations_ctl_with_a_control_and_weights(cuda_device):
    """dur = (int)max(0, (rint(e) * scalar) * control), weights = max(0, (e * scalar) * control) with e = expf(log_d) - 1 as the device
    computes it: e is read back through a control of 1 (weights = e * 1 * 1), so every other number is one or two fp32 products."""
    dev, B, L = cuda_device, 3, 37
    g = torch.Generator().manual_seed(1)
    log_d = torch.rand(B, L, generator=g) * 4.0 - 1.0
    control = torch.tensor([0.0, 0.5, 1.0, 2.0, 1.3, -1.0])[torch.randint(0, 6, (B, L), generator=g)]
    lens = [37, 18, 36]
    pad = torch.arange(L)[None] >= torch.tensor(lens)[:, None]

    def run(ctl, scalar):
        dur, w = torch.full((B, L), -7, dtype=torch.int32, device=dev), torch.full((B, L), -7.0, device=dev)
        assert call(lib().evmi_fs2_durations_ctl_i32, log_d.to(dev), i32(lens, dev), ctl, dur, w, B, L, scalar, stream(dev)) == _lib.EVMI_OK
        return dur.cpu(), w.cpu()

    _, e = run(None, 1.0)  # max(0, e * 1): the device's e wherever it is positive
    live = (e > 0) & ~pad
    raw = torch.exp(log_d.double()) - 1.0
    assert int(live.sum()) > 40 and bool(((raw - e).abs() <= 4e-6 * raw.abs().clamp_min(1.0))[live].all())  # (expf within a few ulp)
    s = torch.tensor(1.3, dtype=torch.float32)
    dur, w = run(control.to(dev), 1.3)
    assert torch.equal(w[live], ((e * s) * control).clamp_min(0.0)[live]) and not w[pad].any()
    assert torch.equal(dur[live], ((torch.round(e) * s) * control).clamp_min(0.0).to(torch.int32)[live]) and not dur[pad].any()


def _edge_values(bins):
    return torch.cat([bins, torch.nextafter(bins, INF), torch.nextafter(bins, -INF), torch.tensor([-2.5, -1e30, 3.5, 1e30, 0.0])])


def _apply_ref(x, pred, bins, table, lens, forced=None, control=None, cum=None, scalar=1.0):
    D, B, n = x.shape
    pad = torch.arange(n)[None] >= torch.tensor(lens)[:, None]
    if forced is not None:
        v = forced[:, :n]
    else:
        v = pred * torch.tensor(scalar, dtype=torch.float32)
        if control is not None:
            sym = torch.arange(n)[None].expand(B, n) if cum is None else torch.searchsorted(cum, torch.arange(n)[None].expand(B, n).contiguous(), right=True).clamp_max(cum.shape[1] - 1)
            v = v * torch.gather(control, 1, sym)
    v = torch.where(pad, torch.zeros(()), v)
    return x + table[torch.bucketize(v, bins)].permute(2, 0, 1), v


@pytest.mark.parametrize("n_bins", [2, 9, 256])
def test_variance_apply_on_the_symbol_axis(cuda_device, n_bins):
    """Values on every bin edge, its two fp32 neighbours, below the first and above the last edge; a control per column; forced values
    whose padded columns hold NaN (not read); rows of forced values longer than n."""
    dev, D = cuda_device, 5
    bins = torch.linspace(-2.0, 3.0, n_bins - 1)
    vals = _edge_values(bins)
    g = torch.Generator().manual_seed(n_bins)
    B, n = 2, len(vals)
    pred = torch.stack([vals, vals.flip(0)])
    control = torch.stack([torch.ones(n), torch.tensor([0.5, 2.0, 1.3])[torch.randint(0, 3, (n,), generator=g)]])
    lens = [n, n - 3]
    x, table = torch.randn(D, B, n, generator=g), torch.randn(n_bins, D, generator=g)
    for scalar, ctl in ((1.0, control), (1.3, control), (1.3, None)):
        got, used = _apply(dev, x, pred, bins, table, lens, control=ctl, scalar=scalar)
        want, v = _apply_ref(x, pred, bins, table, lens, control=ctl, scalar=scalar)
        assert torch.equal(used, v) and torch.equal(got, want)
        if scalar == 1.0:  # (row 0: every value as it is)
            assert set(torch.bucketize(v, bins).tolist()[0]) == set(range(n_bins)), "every bucket is hit"
    forced = torch.full((B, n + 2), float("nan"))
    forced[0, :n], forced[1, : n - 3] = vals, vals.flip(0)[: n - 3]
    for p in (pred, None):  # (a forced variance's predictor is not run: no prediction is needed)
        got, used = _apply(dev, x, p, bins, table, lens, forced=forced)
        want, v = _apply_ref(x, p, bins, table, lens, forced=forced)
        assert torch.equal(used, v) and torch.equal(got, want) and not torch.isnan(got).any()


def test_variance_apply_on_the_frame_axis(cuda_device):
    """A control per symbol followed through the prefix sums: symbols of no frames (the first one, two in a row, the last one), an
    item shorter than T, an item whose only symbol owns every frame; 300 frames: two blocks."""
    dev, D, n_bins, L = cuda_device, 40, 12, 9
    durs = torch.tensor([[0, 50, 0, 0, 100, 1, 99, 50, 0], [300, 0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 7, 30, 0, 60, 0, 0, 0]])
    cum, lens = torch.cumsum(durs, 1), durs.sum(1).tolist()
    B, T = 3, 300
    g = torch.Generator().manual_seed(4)
    control = torch.rand(B, L, generator=g) + 0.5
    control[durs == 0] = float("nan")  # (a symbol of no frames owns no column: its control is never read)
    pred = torch.randn(B, T, generator=g)
    bins = torch.linspace(-2.0, 2.0, n_bins - 1)
    x, table = torch.randn(D, B, T, generator=g), torch.randn(n_bins, D, generator=g)
    sym = symbol_of_frame(durs, T)
    assert sym[0, 0] == 1 and sym[0, 49] == 1 and sym[0, 50] == 4 and sym[0, 150] == 5 and sym[0, 299] == 7 and sym[2, 6] == 2 and sym[2, 7] == 3
    got, used = _apply(dev, x, pred, bins, table, lens, control=control, cum=cum, scalar=1.3)
    want, v = _apply_ref(x, pred, bins, table, lens, control=control, cum=cum, scalar=1.3)
    assert not torch.isnan(v).any() and torch.equal(used, v) and torch.equal(got, want)
    assert not used[2, 97:].any()


# =====================================================================================================================
# 2. the fit
# =====================================================================================================================
def _fit(dev, weights, lens, targets, dur):
    B, L = weights.shape
    d = dur.to(dev, torch.int32)
    assert call(lib().evmi_fs2_fit_durations_i32, weights.to(dev), i32(lens, dev), i32(targets, dev), d, B, L, stream(dev)) == _lib.EVMI_OK
    return d.cpu()


def _lattice(shape, g):
    return torch.randint(0, 512, shape, generator=g).float() / 8.0  # multiples of 1/8 below 64: every double sum and product is exact


def _check_exact(dev, weights, lens, targets):
    B, L = weights.shape
    sentinel = torch.full((B, L), -5, dtype=torch.int32)
    got = _fit(dev, weights, lens, targets, sentinel)
    for b in range(B):
        n = lens[b]
        if targets[b] <= 0:
            assert torch.equal(got[b], sentinel[b])  # no target: the row is not touched, padding included
            continue
        assert got[b, :n].tolist() == fit_ref(weights[b, :n].tolist(), targets[b]), b
        assert int(got[b].sum()) == targets[b] and not got[b, n:].any()


def test_fit_against_the_restatement_on_the_lattice(cuda_device):
    g = torch.Generator().manual_seed(2)
    lens, targets = [70, 64, 65, 1, 33], [500, 0, 7, 64, 1]
    w = _lattice((5, 70), g)
    w[2, :5] = 0.0
    _check_exact(cuda_device, w, lens, targets)
    _check_exact(cuda_device, torch.full((5, 70), 1.375), lens, targets)   # all equal: every remainder ties, the lower indices win
    _check_exact(cuda_device, torch.zeros(5, 70), lens, targets)            # no weight anywhere: all equal
    _check_exact(cuda_device, torch.zeros(5, 70), [5] * 5, [3, 5, 6, 0, 1])  # ([1, 1, 1, 0, 0] of the fixed cases among them)


def test_fit_of_an_item_without_symbols(cuda_device):
    """The header's rule: no symbol to give a frame to -- with a target the row becomes all zero; its neighbour is fitted as usual."""
    w = torch.full((2, 6), 0.5)
    got = _fit(cuda_device, w, [0, 6], [9, 9], torch.full((2, 6), -5, dtype=torch.int32))
    assert got.tolist() == [[0] * 6, [2, 2, 2, 1, 1, 1]]


@pytest.mark.parametrize("L", [1000, _lib.EVMI_FS2_FIT_MAX_SYMBOLS])
def test_fit_of_a_long_item(cuda_device, L):
    g = torch.Generator().manual_seed(L)
    _check_exact(cuda_device, _lattice((1, L), g), [L], [3 * L + 17])
    _check_exact(cuda_device, _lattice((2, L), g), [L - 1, 257], [L // 2, 100000])


def test_fit_invariants_on_random_weights(cuda_device):
    g = torch.Generator().manual_seed(6)
    B, L = 16, 300
    w = torch.rand(B, L, generator=g) * torch.tensor([1e-3, 1.0, 50.0, 1e4])[torch.randint(0, 4, (B, 1), generator=g)]
    w[torch.rand(B, L, generator=g) < 0.1] = 0.0
    lens = torch.randint(1, L + 1, (B,), generator=g).tolist()
    lens[0], lens[1] = L, 257
    targets = torch.randint(1, 3000, (B,), generator=g).tolist()
    got = _fit(cuda_device, w, lens, targets, torch.full((B, L), -5, dtype=torch.int32))
    for b in range(B):
        n = lens[b]
        wb = w[b, :n].double()
        x = wb * targets[b] / wb.sum()
        assert int(got[b].sum()) == targets[b] and not got[b, n:].any()
        d = got[b, :n].double()
        assert bool((d >= torch.floor(x - 1e-6)).all() and (d <= torch.floor(x + 1e-6) + 1).all()), b


# =====================================================================================================================
# 3. the whole model
# =====================================================================================================================
B, L = 3, 14
LENS = torch.tensor([14, 9, 11])
# model seeds: the first from 1 upwards at which the restatement's guards hold for the case (found on the CPU; `python -m
# tests.test_gpu_fs2_prosody` prints them)
SEEDS = {"phone_controls": 1, "duration_control": 1, "forced_phone": 1, "frame_controls": 11, "frame_forced": 1, "target": 1}


def _ids(ref_cfg):
    g = torch.Generator().manual_seed(9)
    return torch.randint(1, ref_cfg.n_symbols, (B, L), generator=g).masked_fill(torch.arange(L)[None] >= LENS[:, None], 0)


def _controls(seed, lo=0.6, hi=1.5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, L, generator=g) * (hi - lo) + lo


def case_kwargs(name, ref_cfg, ref):
    """The steering of each whole-model case, on the host."""
    ids = _ids(ref_cfg)
    if name == "phone_controls":
        return dict(pitch_control=_controls(1), energy_control=_controls(2))
    if name == "duration_control":
        g = torch.Generator().manual_seed(3)
        ctl = torch.tensor([0.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (B, L), generator=g)]
        ctl[:, 0], ctl[:, 1] = 2.0, 0.0
        return dict(duration_control=ctl, pitch_control=0.9)
    if name == "forced_phone":
        g = torch.Generator().manual_seed(4)
        return dict(pitch=torch.randn(B, L, generator=g) * 1.5, energy=torch.randn(B, L, generator=g) * 1.5)
    if name == "frame_controls":
        return dict(pitch_control=_controls(5), energy_control=_controls(6), duration_control=_controls(7, 0.8, 1.6))
    if name == "frame_forced":
        T = int(forward_prosody_ref(ref, ids, LENS, guard=False)[5].max())
        g = torch.Generator().manual_seed(8)
        return dict(pitch=torch.randn(B, T + 2, generator=g) * 1.5, energy=torch.randn(B, T, generator=g) * 1.5)
    raise KeyError(name)


def case_levels(name):
    return (FRAME, FRAME) if name.startswith("frame") else (PHONE, PHONE)


def _run_case(name, cuda_device):
    ref_cfg, ref, model = _inference_pair(case_levels(name), cuda_device, SEEDS[name], duration_bias=1.2)
    ids = _ids(ref_cfg)
    kw = case_kwargs(name, ref_cfg, ref)
    want = forward_prosody_ref(ref, ids, LENS, guard=True, **kw)
    got = [t.cpu() for t in model(ids, LENS, **kw)]
    assert torch.equal(got[2], want[2]) and torch.equal(got[5], want[5]) and int(want[5].min()) > 0
    for i in (3, 4, 0, 1):
        assert got[i].shape == want[i].shape, i
        _close(got[i], want[i])
    return ids, kw, got, want


def test_model_with_per_symbol_pitch_and_energy_controls(cuda_device):
    _run_case("phone_controls", cuda_device)


def test_model_with_a_per_symbol_duration_control(cuda_device):
    _, kw, got, _ = _run_case("duration_control", cuda_device)
    ctl = kw["duration_control"]
    assert (ctl == 0.0).any() and (ctl == 2.0).any()
    assert not got[2][ctl == 0.0].any() and int(got[2][:, 0].min()) >= 2


def test_model_with_forced_phone_level_values(cuda_device):
    _, kw, got, _ = _run_case("forced_phone", cuda_device)
    pad = torch.arange(L)[None] >= LENS[:, None]
    assert torch.equal(got[3], kw["pitch"].masked_fill(pad, 0.0)) and torch.equal(got[4], kw["energy"].masked_fill(pad, 0.0))


def test_model_at_frame_level_with_per_symbol_controls(cuda_device):
    _, _, got, want = _run_case("frame_controls", cuda_device)
    assert got[3].shape == (B, int(want[5].max()))


def test_model_at_frame_level_with_forced_values(cuda_device):
    _, kw, got, want = _run_case("frame_forced", cuda_device)
    T = int(want[5].max())
    fpad = torch.arange(T)[None] >= want[5][:, None]
    assert torch.equal(got[3], kw["pitch"][:, :T].masked_fill(fpad, 0.0)) and torch.equal(got[4], kw["energy"].masked_fill(fpad, 0.0))


def test_forced_frame_level_values_shorter_than_the_mel_are_refused(cuda_device):
    ref_cfg, ref, model = _inference_pair((FRAME, PHONE), cuda_device, SEEDS["frame_forced"], duration_bias=1.2)
    ids = _ids(ref_cfg)
    T = int(model(ids, LENS)[5].max())
    with pytest.raises(ValueError, match="shorter"):
        model(ids, LENS, pitch=torch.zeros(B, T - 1))
    assert model(ids, LENS, pitch=torch.zeros(B, T))[0].shape[1] == T


@pytest.mark.parametrize("levels", [(PHONE, PHONE), (FRAME, FRAME)])
def test_a_number_a_row_and_a_full_tensor_are_the_same_control(cuda_device, levels):
    ref_cfg, _, model = _inference_pair(levels, cuda_device, 3, duration_bias=1.2)
    ids = _ids(ref_cfg)
    number = model(ids, LENS, pitch_control=1.3)
    full = model(ids, LENS, pitch_control=torch.full((B, L), 1.3))
    for a, b in zip(number, full):
        assert torch.equal(a, b)
    row = torch.tensor([0.7, 1.0, 1.9])
    for name in ("pitch_control", "energy_control", "duration_control"):
        per_item = model(ids, LENS, **{name: row})
        per_symbol = model(ids, LENS, **{name: row[:, None].expand(B, L).contiguous()})
        for a, b in zip(per_item, per_symbol):
            assert torch.equal(a, b), name
        assert not torch.equal(per_item[1], model(ids, LENS)[1]), name


TARGETS = torch.tensor([40, 0, 9])


def _target_control():
    return _controls(11, 0.5, 2.0)


def test_model_with_target_frames(cuda_device):
    ref_cfg, ref, model = _inference_pair((PHONE, PHONE), cuda_device, SEEDS["target"], duration_bias=1.2)
    ids = _ids(ref_cfg)
    targets, ctl = TARGETS, _target_control()
    plain = model(ids, LENS, duration_control=ctl)
    got = [t.cpu() for t in model(ids, LENS, duration_control=ctl, target_frames=targets)]
    assert got[5].tolist() == [40, int(plain[5][1]), 9] and torch.equal(got[2][1], plain[2][1].cpu())  # no target: the predicted length
    assert got[2].sum(1).tolist() == got[5].tolist() and int(got[2].min()) >= 0
    # within one frame of the oracle's float64 share x_l (the restatement asserts that no share sits within 1e-3 of a whole number)
    x = fit_shares_ref(ref, ids, LENS, _target_control(), targets, guard=True)
    for b in (0, 2):
        n = int(LENS[b])
        assert bool(((got[2][b, :n].double() - x[b, :n]).abs() < 1.0).all()), (b, got[2][b], x[b])
        assert not got[2][b, n:].any()
    want = forward_prosody_ref(ref, ids, LENS, durations=got[2], guard=True)  # the oracle on the durations the device returned
    assert torch.equal(want[5], got[5])
    for i in (3, 4, 0, 1):
        _close(got[i], want[i])


# =====================================================================================================================
# 4. the default path
# =====================================================================================================================
NEW = ("evmi_fs2_variance_apply_f32", "evmi_fs2_durations_ctl_i32", "evmi_fs2_fit_durations_i32")
OLD = ("evmi_fs2_bucket_embed_add_f32", "evmi_fs2_durations_i32")


def _spy(monkeypatch):
    seen, L_ = [], lib()
    for name in NEW + OLD:
        fn = getattr(L_, name)
        monkeypatch.setattr(L_, name, lambda *a, _fn=fn, _name=name: (seen.append(_name), _fn(*a))[1])
    return seen


@pytest.mark.parametrize("levels", [(PHONE, PHONE), (FRAME, PHONE)])
def test_the_default_path_issues_none_of_the_new_entry_points(cuda_device, monkeypatch, levels):
    ref_cfg, _, model = _inference_pair(levels, cuda_device, 3, duration_bias=1.2)
    ids = _ids(ref_cfg)
    seen = _spy(monkeypatch)
    model(ids, LENS)
    model(ids, LENS, duration_control=1.2, pitch_control=0.8, energy_control=1.1)
    model(ids, LENS, durations=torch.full((B, L), 2))
    assert sorted(set(seen)) == sorted(OLD) and seen.count(OLD[0]) == 6 and seen.count(OLD[1]) == 2
    del seen[:]
    model(ids, LENS, pitch_control=torch.ones(B, L), target_frames=torch.tensor([30, 0, 9]))  # (and the spy sees the new ones)
    assert seen.count(NEW[0]) == 1 and seen.count(OLD[0]) == 1 and seen.count(NEW[1]) == 1 and seen.count(NEW[2]) == 1 and OLD[1] not in seen


# =====================================================================================================================
# 5. the synthesis helpers
# =====================================================================================================================
def _aligner_model(dev):
    from tests.test_gpu_align_infer import _model

    return _model(dev, width=128)


def _preprocessed(tmp_path):
    g = torch.Generator().manual_seed(3)
    rows = []
    for i, (n_sym, n_frm) in enumerate([(12, 70), (7, 33)]):
        base = f"utt{i}"
        rows.append({"basename": base, "ids": torch.randint(1, 80, (n_sym,), generator=g).tolist(), "speaker": "default", "language": "default"})
        # (pitch: one value more than the spectrogram has frames, energy: one fewer -- pyworld's frame count, the dataset's tolerance)
        for kind, fn, t in (("spec", "spec-22050-mel-librosa.pt", torch.randn(80, n_frm, generator=g)),
                            ("pitch", "pitch.pt", torch.randn(n_frm + 1, generator=g)), ("energy", "energy.pt", torch.randn(n_frm - 1, generator=g))):
            path = tmp_path / kind / f"{base}--default--default--{fn}"
            path.parent.mkdir(parents=True, exist_ok=True)
            torch.save(t, path)
    return rows


def test_teacher_forcing_of_the_variances(tmp_path, cuda_device):
    from everyvoice_amd.pipeline import generate_teacher_forced_specs, synthesize_helper
    from everyvoice_amd.train import ops

    dev = cuda_device
    model = _aligner_model(dev)
    assert model.has_aligner and model.levels["pitch"] == model.levels["energy"] == "phone"
    rows = _preprocessed(tmp_path)
    load = lambda kind, base, fn: torch.load(tmp_path / kind / f"{base}--default--default--{fn}", weights_only=True)  # noqa: E731
    *_, forced, _ = synthesize_helper(model, [], None, None, 1.0, 0, ["spec"], filelist_data=rows, output_dir=tmp_path / "forced",
                                      teacher_forcing_directory=tmp_path, teacher_force_variances=True)
    plain = generate_teacher_forced_specs(model, rows, tmp_path)
    # the direct call: the aligner's durations, the frame-level files (held to the item's frames) averaged over them
    lens = torch.tensor([len(r["ids"]) for r in rows])
    ids = torch.zeros(2, int(lens.max()), dtype=torch.long)
    mels = [load("spec", r["basename"], "spec-22050-mel-librosa.pt").t() for r in rows]
    for j, r in enumerate(rows):
        ids[j, : lens[j]] = torch.tensor(r["ids"])
    frames = torch.tensor([m.shape[0] for m in mels])
    durs = model.align(ids, lens, torch.nn.utils.rnn.pad_sequence(mels, batch_first=True), frames)
    dur32 = durs.to(dev, torch.int32).contiguous()
    pad = (torch.arange(ids.shape[1])[None] >= lens[:, None]).to(dev)
    values = {}
    for key in ("pitch", "energy"):
        t = torch.zeros(2, int(frames.max()))
        for j, r in enumerate(rows):
            v = load(key, r["basename"], f"{key}.pt")
            v = v[: frames[j]] if v.shape[0] > frames[j] else torch.cat([v, v[-1:]])
            t[j, : frames[j]] = v
        values[key] = ops.phone_average(t.to(dev), torch.cumsum(dur32, 1, dtype=torch.int32).contiguous(), dur32, pad)
    direct = model(ids, lens, durations=durs, **values)
    for j, (f, p) in enumerate(zip(forced, plain)):
        spec = torch.load(f["spec"], weights_only=True)
        assert f["frames"] == int(frames[j]) and torch.equal(spec, direct[1][j, : frames[j]].t().cpu())
        assert not torch.equal(spec, torch.load(p["spec"], weights_only=True))  # without the flag: the predictors' own values
    again = generate_teacher_forced_specs(model, rows, tmp_path, teacher_force_variances=True)
    assert torch.equal(torch.load(again[0]["spec"], weights_only=True), direct[1][0, : frames[0]].t().cpu())
    missing = tmp_path / "pitch" / "utt1--default--default--pitch.pt"
    missing.unlink()
    with pytest.raises(FileNotFoundError, match="utt1--default--default--pitch.pt"):
        generate_teacher_forced_specs(model, rows, tmp_path, teacher_force_variances=True)
    with pytest.raises(ValueError, match="teacher_forcing_directory"):
        synthesize_helper(model, [], None, None, 1.0, 0, ["spec"], filelist_data=rows, output_dir=tmp_path / "x", teacher_force_variances=True)
    # a per-frame file may run past the item's frames by the dataset's slack (10 frames of the durations and pyworld's one), no further
    energy = tmp_path / "energy" / "utt0--default--default--energy.pt"
    torch.save(torch.cat([load("energy", "utt0", "energy.pt"), torch.zeros(12)]), energy)  # 69 + 12 = 70 + 11
    generate_teacher_forced_specs(model, rows[:1], tmp_path, teacher_force_variances=True)
    torch.save(torch.zeros(70 + 12), energy)
    with pytest.raises(ValueError, match="utt0--default--default--energy.pt"):
        generate_teacher_forced_specs(model, rows[:1], tmp_path, teacher_force_variances=True)
    torch.save(torch.zeros(70 - 2), energy)
    with pytest.raises(ValueError, match="wants 70"):
        generate_teacher_forced_specs(model, rows[:1], tmp_path, teacher_force_variances=True)


def test_target_seconds_gives_a_wav_of_exactly_that_many_frames(tmp_path, cuda_device):
    import wave

    from everyvoice_amd.config import HiFiGANConfig
    from everyvoice_amd.pipeline import synthesize_from_text, synthesize_helper
    from everyvoice_amd.vocoder import HiFiGANGenerator

    model = _aligner_model(cuda_device)
    model.duration_predictor.b_lin.fill_(1.0)
    voc = HiFiGANGenerator(HiFiGANConfig(), precision="bf16").to(cuda_device).eval()
    ids, lens = torch.tensor([[3, 4, 5, 6, 7, 8], [9, 10, 11, 0, 0, 0]]), torch.tensor([6, 3])
    seconds, sr, hop = [0.31, 0.12], 22050, 256
    recs = synthesize_from_text(ids, lens, model, voc, tmp_path, ["a", "b"], target_seconds=seconds)
    for rec, s in zip(recs, seconds):
        frames = round(s * sr / hop)
        assert rec["frames"] == frames == int(rec["durations"].sum()) and torch.load(rec["spec"]).shape == (80, frames)
        with wave.open(str(rec["wav"])) as w:
            assert w.getnframes() == frames * hop and w.getframerate() == sr
    # a row's own target and per-symbol controls through synthesize_helper; the row without one keeps its predicted length
    rows = [{"basename": "a", "ids": [3, 4, 5, 6, 7, 8], "target_seconds": 0.31, "duration_control": [2.0, 1.0, 1.0, 0.0, 1.0, 1.0], "pitch_control": [1.2] * 6},
            {"basename": "b", "ids": [9, 10, 11]}]
    *_, preds, _ = synthesize_helper(model, [], None, None, None, 0, ["spec"], filelist_data=rows, output_dir=tmp_path / "rows")
    ctl = torch.tensor([[2.0, 1.0, 1.0, 0.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])
    pc = torch.tensor([[1.2] * 6, [1.0] * 6])
    direct = model(ids, lens, duration_control=ctl, pitch_control=pc, target_frames=torch.tensor([round(0.31 * sr / hop), 0]))
    assert preds[0]["frames"] == round(0.31 * sr / hop) and int(preds[0]["durations"][3]) == 0
    for j, p in enumerate(preds):
        assert torch.equal(torch.load(p["spec"], weights_only=True), direct[1][j, : int(direct[5][j])].t().cpu())
    assert preds[1]["frames"] == int(model(ids, lens)[5][1])  # (no target: the predicted length)
    # the call's own target serves a row without one, and a row whose entry is None, as the call's controls do
    fallback = [dict(rows[0], target_seconds=None), dict(rows[1]), dict(rows[1], basename="c", target_seconds=0.31)]
    *_, preds, _ = synthesize_helper(model, [], None, None, None, 0, ["spec"], filelist_data=fallback, output_dir=tmp_path / "call", target_seconds=0.2)
    assert [p["frames"] for p in preds] == [round(0.2 * sr / hop)] * 2 + [round(0.31 * sr / hop)]
    with pytest.raises(ValueError, match="6 symbols"):
        synthesize_helper(model, [], None, None, None, 0, ["spec"], filelist_data=[dict(rows[0], duration_control=[1.0] * 5)], output_dir=tmp_path / "bad")


if __name__ == "__main__":  # the seed search (CPU only): the first model seed at which each case's guards hold
    for case in SEEDS:
        for seed in range(1, 200):
            cfg_, ref_ = inference_ref(case_levels(case), seed, 1.2)
            try:
                if case == "target":
                    forward_prosody_ref(ref_, _ids(cfg_), LENS, guard=True)
                    fit_shares_ref(ref_, _ids(cfg_), LENS, _target_control(), TARGETS, guard=True)
                else:
                    forward_prosody_ref(ref_, _ids(cfg_), LENS, guard=True, **case_kwargs(case, cfg_, ref_))
            except AssertionError:
                continue
            print(case, seed)
            break
