"""The fused mel front end at any AudioConfig (short windows, any hop, the output-rate side of preprocessing) against the CPU
oracle (oracle/mel_ref.py: torch.stft, which takes win).

Tolerances are those of tests/test_gpu_mel.py: |log-mel diff| <= 2e-3; magnitude rtol 1e-3 with atol 2e-4 (n_fft <= 1024) or
4e-4 (n_fft 2048); energy rtol 2e-4.  Where two runs of the kernel are compared (support loop against full loop, an item of a ragged
batch against the same utterance alone) the arithmetic is the same fmaf chain and the comparison is torch.equal."""

import wave

import numpy as np
import pytest
import torch

from everyvoice_amd import _lib, pipeline
from everyvoice_amd.config import AudioConfig
from oracle import mel_ref

pytestmark = pytest.mark.gpu

LOGMEL_ATOL = 2e-3

# (sr, n_fft, win, hop, n_mels, f_max)
CONFIGS = [
    (16000, 1024, 800, 200, 80, 8000),      # the usual 16 kHz setting
    (24000, 2048, 1200, 300, 100, 12000),   # the usual 24 kHz setting; chunked bins
    (22050, 1024, 1024, 275, 80, 8000),     # odd hop (12.5 ms at 22.05 kHz): no skew
    (16000, 512, 400, 160, 80, 8000),       # short window
    (22050, 64, 50, 13, 16, 8000),          # odd left = 7: k0 rounds down to 6
    (22050, 64, 32, 48, 16, 8000),          # hop > win
    (22050, 64, 64, 64, 16, 8000),          # hop == n_fft
    (22050, 64, 64, 1, 16, 8000),           # hop 1
    (22050, 1024, 1024, 256, 80, 8000),     # today's path through the new entry point
]
_ID = lambda c: "-".join(str(v) for v in c)  # noqa: E731


def _signal(B, S, seed):
    return 0.3 * torch.tanh(torch.randn(B, S, generator=torch.Generator().manual_seed(seed)))


def _transform(cfg):
    from everyvoice_amd.spectral import MelSpectrogram

    sr, n_fft, win, hop, n_mels, f_max = cfg
    return MelSpectrogram(n_fft, win, hop, sr, n_mels, 0, f_max)


def _shapes(cfg):
    _, n_fft, _, hop, _, _ = cfg
    if hop == 1:
        return [(2, 40), (1, 33), (3, 65)]
    return [(2, 33 * hop + 7), (1, n_fft // 2 + 1), (3, 65 * hop)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_against_the_oracle(cuda_device, cfg):
    sr, n_fft, win, hop, n_mels, f_max = cfg
    tr = _transform(cfg)
    for B, S in _shapes(cfg):
        audio = _signal(B, S, S)
        got_log, got_energy, got_mag = tr(audio.to(cuda_device), log=True, return_energy=True, return_magnitude=True)
        lin = tr(audio.to(cuda_device), log=False).cpu()
        want_log = mel_ref.mel_spectrogram_ref(audio, sr, n_fft, win, hop, n_mels, 0, f_max)
        want_mag = mel_ref.magnitude_spectrogram_ref(audio, n_fft, win, hop)
        assert got_log.shape == want_log.shape == (B, n_mels, 1 + S // hop)
        err = float((got_log.cpu() - want_log).abs().max())
        print(f"{_ID(cfg)} [{B}, {S}]: max |log-mel diff| {err:.3e}, max |mag diff| {float((got_mag.cpu() - want_mag).abs().max()):.3e}")
        assert err <= LOGMEL_ATOL
        torch.testing.assert_close(got_mag.cpu(), want_mag, rtol=1e-3, atol=4e-4 if n_fft == 2048 else 2e-4)
        # the linear mel (log=False), held to the log-mel bound as tests/test_gpu_mel.py holds it
        assert lin.shape == want_log.shape and float(lin.min()) >= 0.0
        torch.testing.assert_close(torch.log(torch.clamp(lin, min=1e-5)), want_log, rtol=0, atol=LOGMEL_ATOL)
        np.testing.assert_allclose(got_energy.cpu().numpy(), np.linalg.norm(want_log.numpy(), axis=1), rtol=2e-4)


def _launch(tr, x, declared_win, lens=None):
    """evmi_mel_spectrogram_win_f32 with tr's constants, declaring ``declared_win`` as the window length -> (mel, magnitude)."""
    B, S = x.shape
    frames = 1 + S // tr.hop
    basis, melb = tr._consts(x.device)
    mel = torch.empty(B, tr.n_mels, frames, device=x.device)
    mag = torch.empty(B, tr.n_fft // 2 + 1, frames, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().evmi_mel_spectrogram_win_f32(x.data_ptr(), _lib.ptr(lens), basis.data_ptr(), melb.data_ptr(), mel.data_ptr(), 0,
                                                            mag.data_ptr(), B, S, tr.n_fft, declared_win, tr.hop, tr.nb_pad, tr.n_mels, 1,
                                                            _lib.current_stream_ptr(x.device)), "evmi_mel_spectrogram_win_f32")
    return mel.cpu(), mag.cpu()


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c[2] < c[1]], ids=_ID)
def test_support_loop_equals_full_loop(cuda_device, cfg):
    """The same basis (built for win) walked over the window's support and over all n_fft rows: a dropped product is a * 0 added
    to a finite accumulator, so not one bit may differ."""
    _, n_fft, win, hop, _, _ = cfg
    tr = _transform(cfg)
    assert (tr.plan["k0"], tr.plan["k1"]) != (0, n_fft)
    for B, S in _shapes(cfg):
        x = _signal(B, S, S + 1).to(cuda_device)
        mel_s, mag_s = _launch(tr, x, win)
        mel_f, mag_f = _launch(tr, x, n_fft)
        assert torch.equal(mel_s, mel_f) and torch.equal(mag_s, mag_f), (B, S)
        assert torch.isfinite(mel_s).all()


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_ragged_items_equal_the_utterance_alone(cuda_device, cfg):
    _, n_fft, _, hop, n_mels, _ = cfg
    tr = _transform(cfg)
    lens = [65 * hop, 40 * hop + 3, n_fft // 2 + 1]
    batch = torch.zeros(3, max(lens))
    for b, n in enumerate(lens):
        batch[b, :n] = _signal(1, n, 100 + b)[0]
    mel, energy, mag = tr(batch.to(cuda_device), log=True, return_energy=True, return_magnitude=True, lens=torch.tensor(lens, dtype=torch.int32))
    assert mel.shape == (3, n_mels, 1 + max(lens) // hop)
    for b, n in enumerate(lens):
        f = 1 + n // hop
        m1, e1, g1 = tr(batch[b, :n].to(cuda_device), log=True, return_energy=True, return_magnitude=True)
        assert torch.equal(mel[b, :, :f], m1) and torch.equal(energy[b, :f], e1) and torch.equal(mag[b, :, :f], g1), (b, n)


# ---- the preprocessor at such a configuration, and its output-rate side ----------------------------------------------------------------
def _write_wav(path, x, sr=22050):
    pcm = np.clip(np.round(np.asarray(x) * 32767), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


@pytest.fixture(scope="module")
def wav_items(tmp_path_factory):
    """Three synthetic PCM-16 wavs at 22050 Hz, 0.6 - 1.0 s."""
    d = tmp_path_factory.mktemp("wavs")
    gen = torch.Generator().manual_seed(21)
    items = []
    for i, n in enumerate((13230, 17000, 22050)):
        _write_wav(d / f"u{i}.wav", 0.3 * torch.tanh(torch.randn(n, generator=gen)).numpy())
        items.append(dict(basename=f"u{i}", speaker="default", language="default", wav=d / f"u{i}.wav"))
    return items


def _load(save_dir, kind, base, fn):
    path = save_dir / kind / f"{base}--default--default--{fn}"
    return pipeline.load_wav(path)[0][0] if fn.endswith(".wav") else torch.load(path, weights_only=True)


def test_preprocessor_at_16k_win800_hop200(tmp_path, cuda_device, wav_items):
    cfg = AudioConfig(input_sampling_rate=16000, output_sampling_rate=16000, n_fft=1024, fft_window_size=800, fft_hop_size=200)
    pre = pipeline.GpuPreprocessor(cfg, device=cuda_device)
    kept = pre.process(wav_items, tmp_path)
    assert len(kept) == 3 and pre.counters["processed_files"] == 3
    for k in kept:
        assert k["frames"] == k["samples"] // 200 and k["samples"] % 200 == 0
        wav = _load(tmp_path, "audio", k["basename"], "audio-16000.wav")
        assert wav.numel() == k["samples"]
        spec = _load(tmp_path, "spec", k["basename"], "spec-16000-mel-librosa.pt")
        want = mel_ref.mel_spectrogram_ref(wav, 16000, 1024, 800, 200, 80, 0, 8000, truncate=True)
        assert spec.shape == want.shape == (80, k["frames"])
        assert float((spec - want).abs().max()) <= 3e-3  # (the saved wav is PCM-16 quantised: the bound of tests/test_pipeline.py)
        for kind in ("energy", "pitch"):
            v = _load(tmp_path, kind, k["basename"], f"{kind}.pt")
            assert v.shape == (k["frames"],) and torch.isfinite(v).all(), kind


def test_process_audio_batch_truncates_to_the_given_hop(cuda_device, wav_items):
    wavs = [pipeline.load_wav(it["wav"])[0] for it in wav_items]
    cfg = AudioConfig()
    _, lens, kept, _ = pipeline.process_audio_batch(wavs, 22050, cfg, cuda_device, True, 22050)
    assert kept == [0, 1, 2] and lens == [n // 256 * 256 for n in (13230, 17000, 22050)]
    x, lens, kept, _ = pipeline.process_audio_batch(wavs, 22050, cfg, cuda_device, True, 44100, hop_size=512)
    assert kept == [0, 1, 2] and lens == [2 * n // 512 * 512 for n in (13230, 17000, 22050)] and x.shape[1] >= max(lens)


def test_output_rate_side_of_preprocessing(tmp_path, cuda_device, wav_items):
    """output_sampling_rate = 2 x input_sampling_rate: audio-44100.wav / spec-44100-... next to an unchanged input side.  The spec is held
    to 3e-3 of the oracle's log-mel of the SAVED wav.  The preprocessor takes that spec of the audio as PCM-16 rounds it (as the
    reference, which reads the file back): on these wavs the oracle's own log-mel of the audio before and after the rounding differs by
    3.7e-3, 4.0e-3 and 2.9e-3 in the top mel row, whose band holds only the resampling filter's residue -- a spec of the unrounded
    audio measured 3.72e-3 here."""
    from everyvoice_amd.config import HiFiGANConfig
    from everyvoice_amd.dataset import SpecDataset

    cfg = AudioConfig(input_sampling_rate=22050, output_sampling_rate=44100)
    pre = pipeline.GpuPreprocessor(cfg, device=cuda_device)
    kept = pre.process(wav_items, tmp_path / "up")
    plain = pipeline.GpuPreprocessor(AudioConfig(), device=cuda_device)
    kept_plain = plain.process(wav_items, tmp_path / "plain")
    assert len(kept) == 3 and kept == kept_plain and pre.counters == plain.counters  # (the second pass leaves the counters alone)
    for k in kept:
        out_wav = _load(tmp_path / "up", "audio", k["basename"], "audio-44100.wav")
        assert out_wav.numel() % 512 == 0 and out_wav.numel() == 2 * k["samples"]  # (2 L // 512 == L // 256: the same utterance, twice the rate)
        spec = _load(tmp_path / "up", "spec", k["basename"], "spec-44100-mel-librosa.pt")
        want = mel_ref.mel_spectrogram_ref(out_wav, sr=22050, n_fft=2048, win=2048, hop=512, truncate=True)
        assert spec.shape == want.shape == (80, out_wav.numel() // 512)
        assert float((spec - want).abs().max()) <= 3e-3
        # the input side is what it is without an output rate
        for kind, fn in (("audio", "audio-22050.wav"), ("spec", "spec-22050-mel-librosa.pt"), ("energy", "energy.pt"), ("pitch", "pitch.pt")):
            assert torch.equal(_load(tmp_path / "up", kind, k["basename"], fn), _load(tmp_path / "plain", kind, k["basename"], fn)), kind
    voc = HiFiGANConfig()
    voc.preprocessing.audio = cfg
    voc.preprocessing.save_dir = tmp_path / "up"
    spec_in, y, name, spec_out = SpecDataset(kept, voc)[0]
    assert name == "u0" and y.numel() == spec_out.shape[1] * 512 and spec_in.shape == (80, kept[0]["frames"])


def test_style_reference_mel_at_16k(cuda_device):
    cfg = AudioConfig(input_sampling_rate=16000, output_sampling_rate=16000, n_fft=1024, fft_window_size=800, fft_hop_size=200)
    wave16 = _signal(1, 16000, 5)[0]
    mel = pipeline.style_reference_mel(wave16, cfg, device=cuda_device)
    want = mel_ref.mel_spectrogram_ref(wave16, 16000, 1024, 800, 200, 80, 0, 8000, truncate=True)
    assert mel.shape == (1, 80, 80) == (1, want.shape[1], 80)
    assert float((mel[0].cpu().t() - want).abs().max()) <= LOGMEL_ATOL
