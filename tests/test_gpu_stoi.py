"""STOI on the GPU: ``evmi_stoi_f32`` against the float64 restatement of tests/stoi_ref.py, on a ragged batch in
NaN padding, in a captured graph; ``pipeline.stoi`` through the resampler; ``evaluate_vocoder`` on a preprocessed folder.

THE BOUND is calibrated, not chosen: the restatement runs in float32 on the CPU on every input used here (rounded to float32, as the
kernel gets it), its largest deviation from the float64 restatement of the signal as defined is taken -- 3.6e-6 on ``stoi`` and 1.0e-5
on a single segment's value when this file was written (the figures are printed by
``test_inputs_keep_their_distance_and_calibrate_the_bound``; 1.9e-6 on the closed-form signal) -- and the kernel is allowed four times
that, 1.4e-5 and 4.2e-5: the factor covers another summation order in the 256-term transform and in the reductions over 30 and 15 J
values.  The largest figures come from the closed-form signal: its reference is three tones, so most of its bands hold only the window's
leakage, orders of magnitude below the frame's peak, and any float32 transform leaves its rounding floor there (on an MI355X the
kernel's largest deviations were 1.09e-5 and 2.05e-5, on a truncation of that signal; 6e-8 and 1.7e-7 on the noise-like pairs).  F, K, J and ``frame_of`` are
compared exactly: every input against the bound keeps each frame's energy at least 0.1 dB from the 40 dB threshold in the
restatement (asserted on the CPU; 0.2055 dB on the closed-form signal), so a float32 rounding cannot move a frame across it."""

from functools import lru_cache

import numpy as np
import pytest
import torch

import stoi_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
RATE = 22050  # of the resampled inputs


def i32(values, dev):
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device=dev)


def signal_22k(n, f0=180.0):
    """A modulated harmonic tone over a noise floor (no band is left empty) at 22050 Hz, with a silent stretch: float32 [n]."""
    t = np.arange(n, dtype=np.float64) / RATE
    x = sum(np.sin(2 * np.pi * f0 * h * t) / h for h in (1, 2, 3, 5, 8, 13)) + 0.3 * np.random.default_rng(n + 1).standard_normal(n)
    x *= 0.5 + 0.45 * np.sin(2 * np.pi * 2.0 * t)
    x[n // 3 : n // 3 + 4000] = 0.0
    return (0.2 * x).astype(np.float32)


def pair_22k(n):
    x = signal_22k(n)
    rng = np.random.default_rng(n)
    return x, (x + 0.05 * rng.standard_normal(n)).astype(np.float32)


RESAMPLED = (30000, 21000)  # samples at 22050 Hz of the two items of the resampling test
CASE_NAMES = ["closed-form-g0.0", "closed-form-g0.1", "closed-form-g0.5", "closed-form-g2.0", "noise", "one-segment", "no-segment", "n256", "n257", "n385",
              "zero-reference", "unequal-lengths", "unequal-lengths-the-other-way", "resampled-30000", "resampled-21000"]


@lru_cache(maxsize=None)
def cases():
    """name -> (ref, deg) at 10 kHz as defined, in float64 (the kernel and the float32 restatement get them rounded to float32).  Every one
    is run against THE BOUND."""
    from oracle.preprocess_ref import resample_ref

    out = {f"closed-form-g{g}": R.closed_form(g) for g in (0.0, 0.1, 0.5, 2.0)}
    out["noise"] = R.noise_pair(3, 9000, gap=(3000, 4500))
    out["one-segment"] = R.noise_pair(5, 4224)  # every frame kept: K = F = 31
    out["no-segment"] = R.noise_pair(5, 4096)   # K = F = 30
    for n in (256, 257, 385):                   # F = 0, 1, 2
        out[f"n{n}"] = R.noise_pair(7, n)
    out["zero-reference"] = (np.zeros(6000), R.closed_form(0.5)[1][:6000])
    x, y = R.closed_form(0.5)
    out["unequal-lengths"] = (x, y[:15000])
    out["unequal-lengths-the-other-way"] = (x[:12345], y)
    for n in RESAMPLED:
        out[f"resampled-{n}"] = tuple(resample_ref(torch.from_numpy(v), RATE, 10000).numpy() for v in pair_22k(n))
    return {name: (np.asarray(a, np.float64), np.asarray(b, np.float64)) for name, (a, b) in out.items()}


@lru_cache(maxsize=None)
def expectations():
    """name -> (float64 restatement of the signal, float32 restatement of the signal rounded to float32); computed once, never changed."""
    return {name: (R.stoi(a, b, np.float64), R.stoi(a.astype(np.float32), b.astype(np.float32), np.float32)) for name, (a, b) in cases().items()}


@lru_cache(maxsize=None)
def bounds():
    """(on stoi, on a segment's value): four times the float32 restatement's largest deviation from float64 over every input."""
    err_stoi, err_segment = 0.0, 0.0
    for w64, w32 in expectations().values():
        assert (w32["F"], w32["K"], w32["J"]) == (w64["F"], w64["K"], w64["J"]) and np.array_equal(w32["frame_of"], w64["frame_of"])
        if w64["J"]:
            err_stoi = max(err_stoi, abs(w32["stoi"] - w64["stoi"]))
            err_segment = max(err_segment, float(np.abs(w32["segment"].astype(np.float64) - w64["segment"]).max()))
    return 4.0 * err_stoi, 4.0 * err_segment


def fused(ref, deg, dev):
    """One item alone -> (stoi, (F, K, J), segment [J_cap], frame_of [F_cap]) numpy."""
    from everyvoice_amd.train import ops

    ref, deg = np.asarray(ref, np.float32), np.asarray(deg, np.float32)
    a = torch.from_numpy(np.ascontiguousarray(ref))[None].to(dev) if len(ref) else torch.zeros(1, 1, device=dev)
    b = torch.from_numpy(np.ascontiguousarray(deg))[None].to(dev) if len(deg) else torch.zeros(1, 1, device=dev)
    value, counts, segment, frame_of = ops.stoi(a, i32([len(ref)], dev), b, i32([len(deg)], dev))
    return float(value[0]), tuple(counts[0].tolist()), segment[0].cpu().numpy(), frame_of[0].cpu().numpy()


def test_inputs_keep_their_distance_and_calibrate_the_bound():
    """(On the CPU.)  The condition on the inputs and the two figures of THE BOUND."""
    assert list(cases()) == CASE_NAMES
    for name, (w64, w32) in expectations().items():
        assert w64["margin"] >= 0.1 and w32["margin"] >= 0.09, (name, w64["margin"], w32["margin"])
    assert abs(expectations()["closed-form-g0.5"][0]["margin"] - 0.2055) < 1e-3
    assert expectations()["one-segment"][0]["K"] == 31 and expectations()["one-segment"][0]["J"] == 1
    assert expectations()["no-segment"][0]["K"] == 30 and [expectations()[f"n{n}"][0]["F"] for n in (256, 257, 385)] == [0, 1, 2]
    b_stoi, b_segment = bounds()
    print(f"float32 restatement against float64: stoi {b_stoi / 4:.2e}, segment {b_segment / 4:.2e}; the kernel is allowed {b_stoi:.2e} and {b_segment:.2e}")
    assert 0 < b_stoi < 1e-4 and 0 < b_segment < 1e-3  # far below any difference that matters: a wrong band or frame moves the third digit


@pytest.mark.parametrize("name", CASE_NAMES)
def test_values_against_the_restatement(name, cuda_device):
    ref, deg = cases()[name]
    w64, _ = expectations()[name]
    b_stoi, b_segment = bounds()
    value, counts, segment, frame_of = fused(ref, deg, cuda_device)
    assert counts == (w64["F"], w64["K"], w64["J"]), (counts, w64["F"], w64["K"], w64["J"])
    K, J = w64["K"], w64["J"]
    assert np.array_equal(frame_of[:K], w64["frame_of"]) and (frame_of[K:] == -1).all() and not segment[J:].any()
    if J == 0:
        assert np.isnan(value)
        return
    print(f"{name}: stoi {value:.7f} float64 {w64['stoi']:.7f} kernel err {abs(value - w64['stoi']):.2e} (allowed {b_stoi:.2e}), "
          f"segment err {np.abs(segment[:J] - w64['segment']).max():.2e} (allowed {b_segment:.2e})")
    assert abs(value - w64["stoi"]) <= b_stoi
    assert np.abs(segment[:J].astype(np.float64) - w64["segment"]).max() <= b_segment
    if name == "zero-reference":
        assert value == 0.0 and not segment.any() and K == w64["F"]


# ---- ragged batches -----------------------------------------------------------------------------------------------------------------
def _ragged(S_ref, S_deg):
    """Five items in NaN padding -> (ref [5, S_ref], deg [5, S_deg], the lengths given, the items as (ref, deg) alone)."""
    c = cases()
    full = [np.asarray(v, np.float32) for v in R.closed_form(0.1, n=max(S_ref, S_deg))]
    items = [(c["noise"][0][:0], c["noise"][1][:5000]),              # no reference samples
             c["noise"],                                              # 9000 / 9000
             c["unequal-lengths"],                                    # 20000 / 15000
             (c["one-segment"][0], c["noise"][1][:4300]),             # 4224 / 4300: one segment
             (full[0][:S_ref], full[1][:S_deg])]                      # lengths above the rows: clamped
    ref, deg = torch.full((5, S_ref), NAN), torch.full((5, S_deg), NAN)
    for i, (a, b) in enumerate(items):
        ref[i, : len(a)], deg[i, : len(b)] = torch.from_numpy(a.astype(np.float32)), torch.from_numpy(b.astype(np.float32))
    lens = ([len(a) for a, _ in items[:4]] + [S_ref + 500], [len(b) for _, b in items[:4]] + [2 ** 31 - 1])
    return ref, deg, lens, items


def _guarded(shapes, dtypes, dev, guard=64):
    """Outputs filled with NaN / -7 inside one buffer each, with sentinels in front and behind."""
    bufs, views = [], []
    for shape, dtype in zip(shapes, dtypes):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * guard,), 12345.0 if dtype == torch.float32 else 12345, dtype=dtype, device=dev)
        buf[guard : guard + n] = NAN if dtype == torch.float32 else -7
        bufs.append(buf)
        views.append(buf[guard : guard + n].view(shape))
    return bufs, tuple(views)


def _same_as_alone(got, alone):
    """Row ``got`` = (stoi, counts, segment row, frame_of row) tensors against ``fused``'s tuple, every output, under torch.equal."""
    value, counts, segment, frame_of = got
    v1, c1, s1, f1 = alone
    F, K, J = c1
    assert tuple(counts.tolist()) == c1
    assert torch.equal(torch.nan_to_num(value, nan=-1.0), torch.nan_to_num(torch.tensor(v1, dtype=torch.float32), nan=-1.0))
    assert torch.equal(segment[:J], torch.from_numpy(s1[:J])) and not segment[J:].any() and not s1[J:].any()
    assert torch.equal(frame_of[:K], torch.from_numpy(f1[:K])) and (frame_of[K:] == -1).all() and (f1[K:] == -1).all()


@pytest.mark.parametrize("S_ref,S_deg", [(20000, 20480), (23001, 21003)])
def test_ragged_batch_in_nan_padding_equals_the_items_alone(S_ref, S_deg, cuda_device):
    from everyvoice_amd.train import ops

    dev = cuda_device
    ref, deg, lens, items = _ragged(S_ref, S_deg)
    alone = [fused(a, b, dev) for a, b in items]
    assert np.isnan(alone[0][0]) and alone[0][1] == (0, 0, 0) and alone[3][1][2] == 1 and alone[4][1][0] == R.stoi(*items[4])["F"]
    _, f_cap, j_cap = ops.stoi_plan(min(S_ref, S_deg))
    bufs, out = _guarded([(5,), (5, 3), (5, j_cap), (5, f_cap)], [torch.float32, torch.int32, torch.float32, torch.int32], dev)
    ops.stoi(ref.to(dev), i32(lens[0], dev), deg.to(dev), i32(lens[1], dev), out=out)
    for buf in bufs:
        assert (buf[:64] == 12345).all() and (buf[-64:] == 12345).all()
    value, counts, segment, frame_of = (t.cpu() for t in out)
    for i in range(5):
        _same_as_alone((value[i], counts[i], segment[i], frame_of[i]), alone[i])


def test_a_row_above_the_limit_is_refused_before_any_launch(cuda_device):
    from everyvoice_amd import _lib
    from everyvoice_amd.train import ops

    max_n = ops.stoi_plan(1)[0]
    rows = torch.empty(1, max_n + 1, device=cuda_device)  # never read
    small = torch.zeros(1, 8, dtype=torch.float32, device=cuda_device)
    lib = _lib.load()
    rc = lib.evmi_stoi_f32(rows.data_ptr(), rows.data_ptr(), small.data_ptr(), small.data_ptr(), small.data_ptr(), small.data_ptr(), small.data_ptr(),
                           small.data_ptr(), 1, max_n + 1, max_n + 1, None)
    assert rc == _lib.EVMI_ERR_UNSUPPORTED and str(max_n) in lib.evmi_last_error().decode()
    assert not small.any()
    with pytest.raises(RuntimeError, match=str(max_n)):
        ops.stoi(rows, i32([5000], cuda_device), rows, i32([5000], cuda_device))
    # at the limit itself the call runs: 11 s and more of a periodic signal
    x = torch.from_numpy(np.asarray(R.closed_form(0.5, n=20000)[0], np.float32)).repeat(max_n // 20000 + 1)[None, :max_n].contiguous().to(cuda_device)
    value, counts, _, frame_of = ops.stoi(x, i32([max_n], cuda_device), x, i32([max_n], cuda_device))
    F = (max_n - 256) // 128
    # a signal against itself: every rho is the 30-term inner product of one unit vector with itself: 1 within the roundings of 30
    # products and two norms of 30 terms, each 6e-8: below 4e-6
    assert counts[0, 0] == F and 31 <= counts[0, 1] < F and counts[0, 2] == counts[0, 1] - 30 and abs(float(value[0]) - 1.0) < 4e-6
    assert int(frame_of[0, int(counts[0, 1]) - 1]) <= F - 1


def test_captured_call_follows_the_lengths_in_device_memory(cuda_device):
    from everyvoice_amd.train import ops

    dev = cuda_device
    S_ref, S_deg = 20000, 20480
    ref, deg, first, _ = _ragged(S_ref, S_deg)
    ref, deg = torch.nan_to_num(ref).to(dev), torch.nan_to_num(deg).to(dev)
    second = ([9000, 0, 4224, 20000, 300], [8000, 77, 9999, 4096, 20480])
    eager = [[t.cpu() for t in ops.stoi(ref, i32(x, dev), deg, i32(y, dev))] for x, y in (first, second)]
    lr, ld = i32(first[0], dev), i32(first[1], dev)
    _, f_cap, j_cap = ops.stoi_plan(S_ref)
    out = (torch.full((5,), NAN, device=dev), torch.zeros(5, 3, dtype=torch.int32, device=dev), torch.full((5, j_cap), NAN, device=dev),
           torch.zeros(5, f_cap, dtype=torch.int32, device=dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.stoi(ref, lr, deg, ld, out=out)
    for which in (0, 1, 0):
        lr.copy_(i32((first, second)[which][0], dev))
        ld.copy_(i32((first, second)[which][1], dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        for got, want in zip(out, eager[which]):
            assert torch.equal(torch.nan_to_num(got.cpu().float(), nan=-1.0), torch.nan_to_num(want.float(), nan=-1.0)), which
    assert not torch.equal(eager[0][1], eager[1][1]) and eager[1][1][1].tolist() == [0, 0, 0]


# ---- pipeline.stoi -----------------------------------------------------------------------------------------------------------------
def test_pipeline_stoi_resamples_each_item_as_alone(cuda_device):
    from everyvoice_amd.pipeline import Stoi, stoi

    dev = cuda_device
    pairs = [pair_22k(n) for n in RESAMPLED]
    S = max(RESAMPLED) + 777
    ref, deg = torch.full((2, S), NAN), torch.full((2, 1, S), NAN)
    for i, (a, b) in enumerate(pairs):
        ref[i, : len(a)], deg[i, 0, : len(b)] = torch.from_numpy(a), torch.from_numpy(b)
    got = stoi(ref.to(dev), torch.tensor(RESAMPLED), deg.to(dev), torch.tensor(RESAMPLED), RATE)
    assert isinstance(got, Stoi) and got.stoi.device.type == "cuda" and got.stoi.dtype == torch.float32 and got.frames.dtype == torch.int32
    b_stoi, b_segment = bounds()
    for i, (a, b) in enumerate(pairs):
        alone = stoi(torch.from_numpy(a)[None].to(dev), [len(a)], torch.from_numpy(b)[None].to(dev), [len(b)], RATE)
        F, K, J = int(alone.frames[0]), int(alone.active[0]), int(alone.segments[0])
        assert (int(got.frames[i]), int(got.active[i]), int(got.segments[i])) == (F, K, J) and torch.equal(got.stoi[i], alone.stoi[0])
        assert torch.equal(got.segment_stoi[i, :J], alone.segment_stoi[0, :J]) and not got.segment_stoi[i, J:].any()
        assert torch.equal(got.frame_of[i, :K], alone.frame_of[0, :K]) and (got.frame_of[i, K:] == -1).all()
        w64, _ = expectations()[f"resampled-{len(a)}"]  # the restatement on oracle.preprocess_ref.resample_ref of the same input
        assert (F, K, J) == (w64["F"], w64["K"], w64["J"]) and J > 0 and np.array_equal(alone.frame_of[0, :K].cpu().numpy(), w64["frame_of"])
        print(f"resampled {len(a)}: stoi {float(alone.stoi[0]):.7f} float64 {w64['stoi']:.7f} err {abs(float(alone.stoi[0]) - w64['stoi']):.2e}")
        assert abs(float(alone.stoi[0]) - w64["stoi"]) <= b_stoi
        assert np.abs(alone.segment_stoi[0, :J].cpu().numpy().astype(np.float64) - w64["segment"]).max() <= b_segment
    # at 10 kHz nothing is resampled: the kernel's own values
    a, b = (v.astype(np.float32) for v in cases()["noise"])
    direct = fused(a, b, dev)
    at_10k = stoi(torch.from_numpy(a)[None].to(dev), [len(a)], torch.from_numpy(b)[None, None].to(dev), [len(b)], 10000)
    assert float(at_10k.stoi[0]) == direct[0] and (int(at_10k.frames[0]), int(at_10k.active[0]), int(at_10k.segments[0])) == direct[1]


# ---- a preprocessed folder ---------------------------------------------------------------------------------------------------------
def _vocoder(dev):
    from everyvoice_amd.config import HiFiGANConfig
    from everyvoice_amd.vocoder import HiFiGANGenerator

    torch.manual_seed(5)
    return HiFiGANGenerator(HiFiGANConfig(model=dict(upsample_initial_channel=128)), precision="f32").to(dev)


FOLDER = [(70, 100), (131, -57), (26, 0)]  # (mel frames, recorded samples beyond frames x 256); the last is 0.3 s


def _preprocessed(tmp_path):
    from everyvoice_amd.pipeline import save_wav

    g = torch.Generator().manual_seed(3)
    rows = []
    for i, (n_frm, extra) in enumerate(FOLDER):
        base = f"utt{i}"
        rows.append({"basename": base, "speaker": "default", "language": "default"})
        path = tmp_path / "spec" / f"{base}--default--default--spec-22050-mel-librosa.pt"
        path.parent.mkdir(parents=True, exist_ok=True)
        torch.save(torch.randn(80, n_frm, generator=g) - 4.0, path)
        save_wav(torch.from_numpy(signal_22k(n_frm * 256 + extra, 120.0 + 40.0 * i)), tmp_path / "audio" / f"{base}--default--default--audio-22050.wav", 22050)
    return rows


def _same(x, y):
    return x == y or (isinstance(x, float) and isinstance(y, float) and np.isnan(x) and np.isnan(y))


def test_evaluate_vocoder_on_a_folder_of_three(tmp_path, cuda_device):
    from everyvoice_amd.config import AudioConfig
    from everyvoice_amd.dataset import generic_psv_filelist_reader
    from everyvoice_amd.pipeline import VOCODER_EVALUATION_FIELDS, evaluate_vocoder, extract_pitch, f0_agreement, load_wav, stoi
    from everyvoice_amd.spectral import get_spectral_transform, vocoder_output_transform

    dev = cuda_device
    vocoder = _vocoder(dev)
    rows = _preprocessed(tmp_path)
    records = evaluate_vocoder(vocoder, rows, tmp_path, batch_size=3, out_path=tmp_path / "check" / "vocoder.psv")
    one_by_one = evaluate_vocoder(vocoder, rows, tmp_path, batch_size=1)
    assert [r["basename"] for r in records] == ["utt0", "utt1", "utt2"]
    t = vocoder_output_transform(AudioConfig())
    log_mel = get_spectral_transform(t["spec_type"], t["n_fft"], t["win_length"], t["hop_length"], t["filter_sample_rate"], t["n_mels"], t["f_min"], t["f_max"])
    for r, other, (n_frm, extra) in zip(records, one_by_one, FOLDER):
        assert set(r) <= set(VOCODER_EVALUATION_FIELDS) and set(r) == set(other) and all(_same(r[f], other[f]) for f in r), (r, other)
        # against the vocoder's own output of that utterance alone
        spec = torch.load(tmp_path / "spec" / f"{r['basename']}--default--default--spec-22050-mel-librosa.pt", weights_only=True)
        wav = vocoder(spec[None].to(dev))[:, 0]
        recorded = load_wav(tmp_path / "audio" / f"{r['basename']}--default--default--audio-22050.wav")[0][:1].to(dev)
        n = min(wav.shape[1], recorded.shape[1])
        assert n == n_frm * 256 + min(extra, 0) and (r["frames"], r["samples"], r["seconds"]) == (n_frm, n, n / 22050)
        a, b = wav[:, :n].contiguous(), recorded[:, :n].contiguous()
        assert r["mel_error"] == float((log_mel(a, log=True) - log_mel(b, log=True)).abs().mean()) > 0
        direct = stoi(b, [n], a, [n], 22050)
        F, K, J = int(direct.frames[0]), int(direct.active[0]), int(direct.segments[0])
        assert _same(r["stoi"], float(direct.stoi[0])) and r["stoi_active"] == K / F and r["stoi_segments"] == J
        if n_frm == 26:  # 0.3 s: frames, but no segment
            assert 0 < F < 31 and J == 0 and np.isnan(r["stoi"]) and np.isnan(r["stoi_worst"]) and np.isnan(r["stoi_worst_at"]) and "no STOI segment" in r["note"]
        else:
            seg = direct.segment_stoi[0, :J].cpu()
            worst = int(torch.argmin(seg))
            assert J > 0 and "note" not in r and -1.0 <= r["stoi"] <= 1.0
            assert r["stoi_worst"] == float(seg[worst]) <= r["stoi"] and r["stoi_worst_at"] == int(direct.frame_of[0, worst]) * 128 / 10000
            assert 0.0 <= r["stoi_worst_at"] < r["seconds"]
        f0_syn, f0_ref = (extract_pitch(x, None, 256, 22050, interpolate=False)[0].cpu().numpy() for x in (a, b))
        want = f0_agreement(f0_syn, f0_ref, np.arange(len(f0_ref)))
        assert all(_same(x, y) for x, y in zip(want, (r["f0_rmse_cents"], r["vuv_error"], r["voiced_pairs"])))
        assert n_frm == 26 or (f0_ref > 0).sum() > len(f0_ref) // 4  # (the longer recordings are voiced)
    lines = (tmp_path / "check" / "vocoder.psv").read_text().splitlines()
    assert len(lines) == 4 and lines[0].split("|") == [f for f in VOCODER_EVALUATION_FIELDS]
    written = generic_psv_filelist_reader(tmp_path / "check" / "vocoder.psv")
    assert len(written) == 3
    for w, r in zip(written, records):
        assert w["basename"] == r["basename"] and int(w["samples"]) == r["samples"] and _same(float(w["stoi"]), r["stoi"])
        assert float(w["mel_error"]) == r["mel_error"] and int(w["stoi_segments"]) == r["stoi_segments"]
