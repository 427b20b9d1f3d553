"""Mel-cepstral distortion along the warping path on the GPU: ``evmi_dtw_cepstral_f32`` alone on the lattice
cases of tests/dtw_ref.py (bit for bit: tests/test_dtw_host.py asserts that their arithmetic is exact in float32), on the real-valued
cases within THE BOUND 4 x max(err32, 1e-6 x max(1, |value|)), on a ragged batch in NaN padding, on zero and out-of-range lengths and
in a captured graph; ``mel_cepstral_distortion`` of a mel with itself; ``evaluate_synthesis`` on a preprocessed folder."""

import numpy as np
import pytest
import torch

import dtw_ref as D

pytestmark = pytest.mark.gpu

NAN = float("nan")


def i32(values, dev):
    return torch.tensor([int(v) for v in values], dtype=torch.int32, device=dev)


def fused(a, b, basis, scale, dev):
    """One item alone -> (dist, steps, lo, hi, col) numpy."""
    from everyvoice_amd.train import ops

    ta, tb = torch.from_numpy(a)[None].contiguous().to(dev), torch.from_numpy(b)[None].contiguous().to(dev)
    out = ops.dtw_cepstral(ta, i32([a.shape[0]], dev), tb, i32([b.shape[0]], dev), torch.from_numpy(basis).to(dev), float(scale))
    return tuple(t.cpu().numpy()[0] for t in out)


def _chunk():
    from everyvoice_amd.train import ops

    return ops.dtw_plan(13, 64)[1]


def pytest_generate_tests(metafunc):
    if "lattice_key" in metafunc.fixturenames:
        keys = D.lattice_keys(_chunk())
        metafunc.parametrize("lattice_key", keys, ids=["-".join(str(v) for v in k) for k in keys])


def test_lattice_cases_bit_for_bit(lattice_key, cuda_device):
    r, want = D.lattice_case(*lattice_key), D.lattice_expectation(lattice_key)
    dist, steps, lo, hi, col = fused(r["a"], r["b"], r["basis"], r["scale"], cuda_device)
    assert steps == want["steps"], (steps, want["steps"])
    assert np.array_equal(lo, want["lo"]) and np.array_equal(hi, want["hi"])
    assert dist.tobytes() == np.float32(want["dist"]).tobytes(), (dist, want["dist"])
    assert col.tobytes() == want["col"].astype(np.float32).tobytes()


@pytest.mark.parametrize("Ta,Tb", D.REAL_SHAPES)
def test_real_valued_cases_within_the_bound(Ta, Tb, cuda_device):
    r = D.real_case(Ta, Tb)
    w64, w32 = D.real_expectation(Ta, Tb)
    dist, steps, lo, hi, col = fused(r["a"], r["b"], r["basis"], r["scale"], cuda_device)
    err32 = abs(float(w32["dist"]) - float(w64["dist"]))
    print(f"({Ta}, {Tb}): dist {dist:.6f} float64 {w64['dist']:.6f} err32 {err32:.2e} kernel err {abs(dist - w64['dist']):.2e}")
    assert abs(float(dist) - float(w64["dist"])) <= D.bound(err32, float(w64["dist"]))
    assert D.is_path(lo, hi, Ta) and steps == len(D.path_cells(lo, hi))
    # the kernel's own path: optimal in float64 up to the same bound (path equality with float64 is not demanded)
    optimum = float(w64["D"][-1, -1])
    err_total = abs(float(w32["D"][-1, -1]) - optimum)
    assert D.path_cost64(r["a"], r["b"], r["basis"], lo, hi) - optimum <= D.bound(err_total, optimum)
    # col: the mean float64 cost of the kernel's own path cells of each column, scaled
    c64 = w64["c"]
    want_col = np.array([float(r["scale"]) * c64[lo[j] : hi[j] + 1, j].mean() for j in range(Tb)])
    col32 = np.array([np.float32(r["scale"]) * w32["c"][lo[j] : hi[j] + 1, j].sum(dtype=np.float32) / np.float32(hi[j] - lo[j] + 1) for j in range(Tb)])
    assert (np.abs(col - want_col) <= D.bound(np.abs(col32 - want_col), want_col)).all()


RAGGED = D.RAGGED  # (Na, Nb) of the five items, K 13, M 80


def _ragged(dev, Ta, Tb):
    cases = [D.lattice_case(*key) for key in D.ragged_keys()]
    a, b = torch.full((len(RAGGED), Ta, 80), NAN), torch.full((len(RAGGED), Tb, 80), NAN)
    for i, r in enumerate(cases):
        a[i, : r["a"].shape[0]] = torch.from_numpy(r["a"])
        b[i, : r["b"].shape[0]] = torch.from_numpy(r["b"])
    return cases, a.to(dev), b.to(dev), torch.from_numpy(cases[0]["basis"]).to(dev)


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


def _alone(cases, dev):
    return [fused(r["a"], r["b"], r["basis"], r["scale"], dev) for r in cases]


@pytest.mark.parametrize("Ta,Tb", [(257, 300), (400, 513)])
def test_ragged_batch_in_nan_padding_equals_the_items_alone(Ta, Tb, cuda_device):
    from everyvoice_amd.train import ops

    dev = cuda_device
    cases, a, b, basis = _ragged(dev, Ta, Tb)
    alone = _alone(cases, dev)
    B = len(RAGGED)
    la, lb = i32([na for na, _ in RAGGED], dev), i32([nb for _, nb in RAGGED], dev)
    for _ in range(2):
        bufs, out = _guarded([(B,), (B,), (B, Tb), (B, Tb), (B, Tb)], [torch.float32, torch.int32, torch.int32, torch.int32, torch.float32], dev)
        ops.dtw_cepstral(a, la, b, lb, basis, D.LATTICE_SCALE, out=out)
        dist, steps, lo, hi, col = (t.cpu().numpy() for t in out)
        for buf in bufs:
            assert (buf[:64] == 12345).all() and (buf[-64:] == 12345).all()
        for i, (na, nb) in enumerate(RAGGED):
            d1, s1, lo1, hi1, col1 = alone[i]
            assert dist[i].tobytes() == d1.tobytes() and steps[i] == s1
            assert np.array_equal(lo[i, :nb], lo1) and np.array_equal(hi[i, :nb], hi1) and col[i, :nb].tobytes() == col1.tobytes()
            assert (lo[i, nb:] == -1).all() and (hi[i, nb:] == -1).all() and not col[i, nb:].any()
            want = D.lattice_expectation(D.ragged_keys()[i])
            assert steps[i] == want["steps"] and np.array_equal(lo[i, :nb], want["lo"]) and dist[i].tobytes() == np.float32(want["dist"]).tobytes()


def test_zero_and_out_of_range_lengths(cuda_device):
    from everyvoice_amd.train import ops

    dev = cuda_device
    Ta, Tb = 257, 300
    cases, a, b, basis = _ragged(dev, Ta, Tb)
    a, b = torch.nan_to_num(a), torch.nan_to_num(b)  # (beyond an item's frames: zeros, so that a clamped length reads numbers)
    alone = _alone(cases, dev)
    #            item 0 as it is | no a frames | beyond Ta and Tb: clamped | negative | item 4 as it is
    la, lb = [64, 0, 9999, 5, 128], [65, 5, 2 ** 31 - 1, -3, 127]
    _, out = _guarded([(5,), (5,), (5, Tb), (5, Tb), (5, Tb)], [torch.float32, torch.int32, torch.int32, torch.int32, torch.float32], dev)
    ops.dtw_cepstral(a, i32(la, dev), b, i32(lb, dev), basis, D.LATTICE_SCALE, out=out)
    dist, steps, lo, hi, col = (t.cpu().numpy() for t in out)
    for i in (1, 3):
        assert np.isnan(dist[i]) and steps[i] == 0 and (lo[i] == -1).all() and (hi[i] == -1).all() and not col[i].any()
    for i in (0, 4):
        nb = RAGGED[i][1]
        assert dist[i].tobytes() == alone[i][0].tobytes() and steps[i] == alone[i][1] and np.array_equal(lo[i, :nb], alone[i][2])
        assert np.array_equal(hi[i, :nb], alone[i][3]) and col[i, :nb].tobytes() == alone[i][4].tobytes() and (lo[i, nb:] == -1).all()
    full = fused(a[2].cpu().numpy(), b[2].cpu().numpy(), cases[0]["basis"], D.LATTICE_SCALE, dev)  # clamped to the whole padded item
    assert dist[2].tobytes() == full[0].tobytes() and steps[2] == full[1] and np.array_equal(lo[2], full[2]) and np.array_equal(hi[2], full[3])
    assert D.is_path(lo[2], hi[2], Ta)


def test_captured_call_follows_the_lengths_in_device_memory(cuda_device):
    from everyvoice_amd.train import ops

    dev = cuda_device
    Ta, Tb = 257, 300
    _, a, b, basis = _ragged(dev, Ta, Tb)
    a, b = torch.nan_to_num(a), torch.nan_to_num(b)
    B = len(RAGGED)
    first = ([na for na, _ in RAGGED], [nb for _, nb in RAGGED])
    second = ([30, 0, 100, 5, 257], [33, 4, 64, 1, 300])
    eager = [[t.cpu() for t in ops.dtw_cepstral(a, i32(x, dev), b, i32(y, dev), basis, D.LATTICE_SCALE)] for x, y in (first, second)]
    la, lb = i32(first[0], dev), i32(first[1], dev)
    ws = torch.empty(ops.dtw_ws_bytes(B, Ta, Tb), dtype=torch.uint8, device=dev)
    out = (torch.full((B,), NAN, device=dev), torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, Tb, dtype=torch.int32, device=dev),
           torch.zeros(B, Tb, dtype=torch.int32, device=dev), torch.full((B, Tb), NAN, device=dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.dtw_cepstral(a, la, b, lb, basis, D.LATTICE_SCALE, out=out, ws=ws)
    for which in (0, 1, 0):
        la.copy_(i32((first, second)[which][0], dev))
        lb.copy_(i32((first, second)[which][1], dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        for got, want in zip(out, eager[which]):
            assert torch.equal(torch.nan_to_num(got.cpu().float(), nan=-1.0), torch.nan_to_num(want.float(), nan=-1.0)), which
    assert not torch.equal(eager[0][1], eager[1][1]) and int(eager[1][1][1]) == 0


def test_a_mel_against_itself_and_against_itself_doubled(cuda_device):
    from everyvoice_amd.pipeline import mel_cepstral_distortion

    g = torch.Generator().manual_seed(2)
    lens = torch.tensor([131, 97, 1])
    mel = torch.randn(3, 131, 80, generator=g) * 2.0 - 5.0
    got = mel_cepstral_distortion(mel.to(cuda_device), lens, mel.to(cuda_device), lens)
    assert got.mcd.device.type == "cuda" and got.mcd.dtype == torch.float32 and got.steps.dtype == torch.int32
    for i, T in enumerate(lens.tolist()):
        assert float(got.mcd[i]) == 0.0 and int(got.steps[i]) == T and not got.frame_mcd[i].any()
        assert torch.equal(got.lo[i, :T].cpu(), torch.arange(T, dtype=torch.int32)) and torch.equal(got.hi[i, :T].cpu(), torch.arange(T, dtype=torch.int32))
        assert (got.lo[i, T:] == -1).all() and (got.hi[i, T:] == -1).all()
    doubled = torch.repeat_interleave(mel, 2, dim=1)
    got = mel_cepstral_distortion(doubled.to(cuda_device), 2 * lens, mel.to(cuda_device), lens)
    for i, T in enumerate(lens.tolist()):
        assert float(got.mcd[i]) == 0.0 and int(got.steps[i]) == 2 * T
        assert torch.equal(got.lo[i, :T].cpu(), 2 * torch.arange(T, dtype=torch.int32)) and torch.equal(got.hi[i, :T].cpu(), 2 * torch.arange(T, dtype=torch.int32) + 1)
    # against another mel: positive, symmetric in its scale (dB), and the per-frame values average the path's costs
    other = mel + 0.3 * torch.randn(mel.shape, generator=g)
    got = mel_cepstral_distortion(other.to(cuda_device), lens, mel.to(cuda_device), lens)
    assert (got.mcd > 0).all() and torch.isfinite(got.mcd).all()


# =====================================================================================================================
# a preprocessed folder
# =====================================================================================================================
def _model(dev, seed=11):
    from dataclasses import replace

    from everyvoice_amd.fs2 import FastSpeech2, FastSpeech2ModelConfig

    return FastSpeech2(replace(FastSpeech2ModelConfig(), mask_padding=True), device=dev).init_random(seed, aligner=True)


def _vocoder(dev):
    from everyvoice_amd.config import HiFiGANConfig
    from everyvoice_amd.vocoder import HiFiGANGenerator

    torch.manual_seed(5)
    return HiFiGANGenerator(HiFiGANConfig(model=dict(upsample_initial_channel=128)), precision="f32").to(dev)


def _preprocessed(tmp_path, with_audio):
    from everyvoice_amd.pipeline import save_wav

    g = torch.Generator().manual_seed(3)
    rows = []
    for i, (n_sym, n_frm) in enumerate([(12, 70), (20, 131), (7, 33)]):
        base = f"utt{i}"
        rows.append({"basename": base, "ids": torch.randint(1, 80, (n_sym,), generator=g).tolist(), "speaker": "default", "language": "default"})
        path = tmp_path / "spec" / f"{base}--default--default--spec-22050-mel-librosa.pt"
        path.parent.mkdir(parents=True, exist_ok=True)
        torch.save(torch.randn(80, n_frm, generator=g) - 4.0, path)
        if with_audio:  # a voiced recording: a gliding harmonic tone, a silent stretch in the middle
            t = torch.arange(n_frm * 256) / 22050.0
            f = 120.0 + 40.0 * i + 30.0 * t
            x = sum(torch.sin(2 * np.pi * h * torch.cumsum(f, 0) / 22050.0) / h for h in (1, 2, 3)) * 0.25
            x[len(x) // 3 : len(x) // 2] = 0.0
            save_wav(x, tmp_path / "audio" / f"{base}--default--default--audio-22050.wav", 22050)
    return rows


SCALARS = ("basename", "speaker", "language", "symbols", "frames_ref", "frames_syn", "length_ratio", "mcd_dtw", "mcd_dtw_sl", "path_steps", "off_diagonal",
           "worst_symbol", "worst_symbol_mcd", "f0_rmse_cents", "vuv_error", "voiced_pairs")


def _same(x, y):
    return x == y or (isinstance(x, float) and isinstance(y, float) and np.isnan(x) and np.isnan(y))


@pytest.mark.parametrize("with_vocoder", [False, True], ids=["mel", "vocoded"])
def test_evaluate_synthesis_on_a_folder_of_three(tmp_path, cuda_device, with_vocoder):
    from everyvoice_amd.dataset import generic_psv_filelist_reader
    from everyvoice_amd.pipeline import SYNTHESIS_EVALUATION_FIELDS, evaluate_synthesis, extract_pitch, f0_agreement, load_wav, mel_cepstral_distortion

    dev = cuda_device
    model = _model(dev)
    vocoder = _vocoder(dev) if with_vocoder else None
    rows = _preprocessed(tmp_path, with_vocoder)
    records = evaluate_synthesis(model, rows, tmp_path, batch_size=2, vocoder=vocoder, out_path=tmp_path / "check" / "synthesis.psv")
    assert [r["basename"] for r in records] == ["utt0", "utt1", "utt2"]
    for r, row in zip(records, rows):
        alone = evaluate_synthesis(model, [row], tmp_path, vocoder=vocoder)[0]
        assert set(r) == set(SCALARS) | {"lo", "hi"} and "note" not in r
        assert all(_same(r[f], alone[f]) for f in SCALARS), (r, alone)
        assert torch.equal(r["lo"], alone["lo"]) and torch.equal(r["hi"], alone["hi"])
        n, f_ref, f_syn = len(row["ids"]), r["frames_ref"], r["frames_syn"]
        spec = torch.load(tmp_path / "spec" / f"{r['basename']}--default--default--spec-22050-mel-librosa.pt", weights_only=True).transpose(0, 1)
        assert r["symbols"] == n and f_ref == spec.shape[0] and f_syn >= 1 and r["length_ratio"] == f_syn / f_ref
        # against the model and the kernel called directly
        _, post, _, _, _, mel_lens = model(torch.tensor([row["ids"]]), torch.tensor([n]))
        assert int(mel_lens[0]) == f_syn
        direct = mel_cepstral_distortion(post[:, :f_syn].contiguous(), mel_lens, spec[None].to(dev), torch.tensor([f_ref]))
        assert r["mcd_dtw"] == float(direct.mcd[0]) > 0 and r["path_steps"] == int(direct.steps[0])
        assert torch.equal(r["lo"], direct.lo[0].cpu()) and torch.equal(r["hi"], direct.hi[0].cpu()) and r["lo"].dtype == torch.int32
        assert r["mcd_dtw_sl"] == r["mcd_dtw"] * max(f_ref, f_syn) / min(f_ref, f_syn)
        lo, hi = r["lo"].numpy(), r["hi"].numpy()
        assert D.is_path(lo, hi, f_syn) and r["path_steps"] == len(D.path_cells(lo, hi))
        diagonal = sum(1 for (i0, j0), (i1, j1) in zip(D.path_cells(lo, hi)[:-1], D.path_cells(lo, hi)[1:]) if i1 == i0 + 1 and j1 == j0 + 1)
        assert r["off_diagonal"] == (1.0 - diagonal / (r["path_steps"] - 1) if r["path_steps"] > 1 else 0.0)
        # the worst symbol: the aligner's durations of the recording (no duration/ file here), the mean per-frame distortion of each symbol
        durations = model.align(torch.tensor([row["ids"]]), torch.tensor([n]), spec[None], torch.tensor([f_ref]))[0].cpu()
        frame = direct.frame_mcd[0].cpu()
        ends = torch.cumsum(durations, 0)
        means = [float(frame[int(e - d) : int(e)].mean()) if d > 0 else -1.0 for d, e in zip(durations, ends)]
        assert r["worst_symbol"] == int(np.argmax(means)) and r["worst_symbol_mcd"] == max(means)
        if not with_vocoder:
            assert r["f0_rmse_cents"] is None and r["vuv_error"] is None and r["voiced_pairs"] is None
        else:  # restated on the host from extract_pitch's outputs and the returned hi
            wav = vocoder(post[:, :f_syn].transpose(1, 2).contiguous(), lens=mel_lens.to(dev))
            recorded = load_wav(tmp_path / "audio" / f"{r['basename']}--default--default--audio-22050.wav")[0][:1].to(dev)
            f0_syn = extract_pitch(wav[0, :1, : f_syn * 256], None, 256, 22050, interpolate=False)[0].cpu().numpy().astype(np.float64)
            f0_ref = extract_pitch(recorded, None, 256, 22050, interpolate=False)[0].cpu().numpy().astype(np.float64)
            assert (f0_ref[:f_ref] > 0).sum() > f_ref // 4  # (the recording is voiced)
            cents, differ, pairs = [], 0, 0
            for j in range(f_ref):
                s, t = f0_syn[hi[j]], f0_ref[j]
                differ += (s > 0) != (t > 0)
                if s > 0 and t > 0:
                    cents.append(1200.0 * np.log2(s / t))
                    pairs += 1
            assert r["voiced_pairs"] == pairs and r["vuv_error"] == differ / f_ref
            want = float(np.sqrt(np.mean(np.square(cents)))) if cents else NAN
            assert _same(r["f0_rmse_cents"], want) or abs(r["f0_rmse_cents"] - want) <= 1e-9 * want
            assert all(_same(x, y) for x, y in zip(f0_agreement(f0_syn, f0_ref, hi), (r["f0_rmse_cents"], r["vuv_error"], r["voiced_pairs"])))
    written = generic_psv_filelist_reader(tmp_path / "check" / "synthesis.psv")
    assert all(set(w) <= set(SYNTHESIS_EVALUATION_FIELDS) and "lo" not in w for w in written) and len(written) == 3
    for w, r in zip(written, records):
        assert w["basename"] == r["basename"] and int(w["frames_syn"]) == r["frames_syn"] and float(w["mcd_dtw"]) == r["mcd_dtw"]
        assert int(w["path_steps"]) == r["path_steps"] and int(w["worst_symbol"]) == r["worst_symbol"]


def test_evaluate_synthesis_notes_an_utterance_beyond_the_limits(tmp_path, cuda_device):
    from everyvoice_amd.pipeline import evaluate_synthesis

    model = _model(cuda_device)
    rows = _preprocessed(tmp_path, False)
    long_path = tmp_path / "spec" / "utt1--default--default--spec-22050-mel-librosa.pt"
    torch.save(torch.randn(80, 1025) - 4.0, long_path)
    records = evaluate_synthesis(model, rows, tmp_path, batch_size=3)
    assert "1024 recorded frames" in records[1]["note"] and np.isnan(records[1]["mcd_dtw"]) and np.isnan(records[1]["mcd_dtw_sl"])
    assert records[1]["lo"] is None and records[1]["path_steps"] == 0 and records[1]["frames_ref"] == 1025
    for i in (0, 2):
        alone = evaluate_synthesis(model, [rows[i]], tmp_path)[0]
        assert "note" not in records[i] and records[i]["mcd_dtw"] == alone["mcd_dtw"] > 0 and torch.equal(records[i]["hi"], alone["hi"])
