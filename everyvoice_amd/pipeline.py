"""Data formats on either side of the hot path: the audio gating + on-disk layout of
the reference's preprocessor for the features computed on the GPU (spec, energy, audio), phone-level averaging,
and the synthesis writers (PCM-16 wav, ``[n_mels, T]`` spec) with the reference's file naming.

Mirrors (paths relative to the reference):
  process_audio            everyvoice/preprocessor/preprocessor.py:131-218  (channel / length gates, the -36 LUFS "audio_empty"
                           gate, the default SoX effect "channels 1" (mix-down), resampling, peak normalise to 0.95, truncate
                           to a multiple of the hop).  Loudness, resampling and normalisation run on the device
                           (csrc/preprocess_ops.hip; torchaudio's algorithms restated, parity unpinned: torchaudio is not in
                           the image).  A dataset's SoX effect chain (``sox_effects``: channels 1, norm, reverse, silence) runs
                           on the device after the mix-down, before resampling (sox.py, csrc/sox_effects.hip); any other effect
                           is refused with a ValueError before a file is read
  preprocess / .config-lock  preprocessor.py:974-1082 (what the lock records, when a run refuses to continue)
  compute_stats / normalize_stats  preprocessor.py:378-490 (dataset statistics of energy / pitch -> Stats, files rewritten normalised)
  create_path naming       everyvoice/preprocessor/preprocessor.py:502-508, 529-533, 633-639
                           ``<save_dir>/<kind>/<basename>--<speaker>--<language>--<kind-file>``
  average_data_by_durations  everyvoice/preprocessor/preprocessor.py:287-300 (host loop, as in the reference)
  save_wav / save_tensor   everyvoice/preprocessor/helpers.py:23-44  (PCM_S 16-bit)
  prediction file names    everyvoice/base_cli/prediction_writing_callback.py:35-41
File IO and per-utterance scalars stay on the host (they are IO-bound plumbing); every per-sample transform
(STFT, mel, log, energy, vocoding) runs in libevmi_hip.
"""

from __future__ import annotations

import json
import math
import wave
from glob import glob
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch

from .config import AudioConfig
from .sox import DEFAULT_CHAIN, Effect, apply_sox_effects, parse_sox_effects
from .spectral import MelSpectrogram, get_spectral_transform

SEP = "--"


def load_wav(path) -> tuple[torch.Tensor, int, float]:
    """PCM wav -> (float32 [channels, samples] in [-1, 1), sampling rate, seconds), like torchaudio.load."""
    with wave.open(str(path), "rb") as w:
        sr, ch, width, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
        raw = w.readframes(n)
    if width == 2:
        data = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 4:
        data = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    elif width == 1:
        data = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    else:
        raise ValueError(f"{path}: unsupported sample width {width}")
    audio = torch.from_numpy(data.reshape(-1, ch).T.copy()) if n else torch.zeros(ch, 0)
    return audio, sr, (n / sr if sr else 0.0)


def save_wav(audio: torch.Tensor, path, sr: int, bits_per_sample: int = 16) -> None:
    """float [-1, 1] [S] or [1, S] -> PCM_S wav (creates the directory), as preprocessor/helpers.py:31-44."""
    if bits_per_sample != 16:
        raise NotImplementedError("only 16-bit PCM (AudioConfig.target_bit_depth default)")
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    x = audio.detach().to("cpu", torch.float32).reshape(-1).numpy()
    pcm = np.clip(np.round(x * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.tobytes())


def pcm16_round_trip(audio: torch.Tensor) -> torch.Tensor:
    """Host float audio as save_wav writes it and load_wav reads it back: rounded to 16-bit PCM (file-format plumbing)."""
    return torch.round(audio.to(torch.float32) * 32768.0).clamp_(-32768.0, 32767.0) / 32768.0


def save_tensor(tensor: torch.Tensor, path) -> None:
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    torch.save(tensor.detach().cpu(), path)


def feature_path(save_dir, kind: str, basename: str, speaker: str, language: str, fn: str) -> Path:
    return Path(save_dir) / kind / SEP.join([basename, speaker, language, fn])


def sinc_resample_kernel(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """The polyphase windowed-sinc filter bank of torchaudio.functional.resample (defaults: sinc_interp_hann): ``new`` filters of
    ``2 * width + orig`` taps applied at stride ``orig`` -> (kernel [new, 1, taps] float32, width, orig, new), rates reduced
    by their gcd.  Built in float64 on the host, as torchaudio does; the convolution itself runs on the device."""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    taps = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = (np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + taps) * base
    t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(t) / t)
    return torch.from_numpy((sinc * window * (base / orig)).astype(np.float32))[:, None, :].contiguous(), width, orig, new


_RESAMPLE_KERNELS: dict = {}


def resample(audio: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    """[B, S] (device) -> [B, ceil(new * S / orig)]: torchaudio.functional.resample as ONE strided convolution on the device
    (evmi_conv1d_f32: exact fp32 fmaf chains) with the filter bank above (preprocessor.py:196-198)."""
    from . import _lib

    if orig_freq == new_freq:
        return audio
    if not audio.is_cuda:
        raise RuntimeError("everyvoice_amd.pipeline.resample computes on the GPU only (no CPU fallback)")
    key = (int(orig_freq), int(new_freq), audio.device)
    if key not in _RESAMPLE_KERNELS:
        k, width, orig, new = sinc_resample_kernel(orig_freq, new_freq)
        _RESAMPLE_KERNELS[key] = (k.to(audio.device), width, orig, new)
    kernel, width, orig, new = _RESAMPLE_KERNELS[key]
    x = audio.to(torch.float32)
    B, S = x.shape
    xp = torch.nn.functional.pad(x, (width, width + orig)).contiguous()  # (memory plumbing: the zero margin of the filter)
    taps = kernel.shape[-1]
    frames = (xp.shape[1] - taps) // orig + 1
    y = torch.empty(B, new, frames, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().evmi_conv1d_f32(xp.data_ptr(), kernel.data_ptr(), 0, 0, y.data_ptr(), B, 1, xp.shape[1], new, taps, orig, 0, 1, 1,
                                           1.0, 1.0, 0, _lib.current_stream_ptr(x.device)), "evmi_conv1d_f32")
    return y.transpose(1, 2).reshape(B, -1)[:, : math.ceil(new * S / orig)].contiguous()


def loudness(audio: torch.Tensor, lens: torch.Tensor, sample_rate: int) -> torch.Tensor:
    """Integrated loudness (LKFS) of a zero-padded batch [items, channels, t_max] with lengths [items] -> [items] on the device
    (torchaudio.transforms.Loudness restated: K-weighting, 400 ms blocks, absolute / relative gates)."""
    from . import _lib

    if not audio.is_cuda:
        raise RuntimeError("everyvoice_amd.pipeline.loudness computes on the GPU only (no CPU fallback)")
    x = audio.to(torch.float32).contiguous()
    items, channels, t_max = x.shape
    lib = _lib.load()
    lens32 = lens.to(x.device, torch.int32).contiguous()
    y2 = torch.empty_like(x)
    z = torch.empty(max(1, lib.evmi_loudness_scratch_elems(items, channels, t_max, sample_rate)), device=x.device, dtype=torch.float32)
    out = torch.empty(items, device=x.device, dtype=torch.float32)
    _lib.check(lib.evmi_loudness_lkfs_f32(x.data_ptr(), lens32.data_ptr(), y2.data_ptr(), z.data_ptr(), out.data_ptr(), items, channels, t_max,
                                          int(sample_rate), _lib.current_stream_ptr(x.device)), "evmi_loudness_lkfs_f32")
    return out


def world_frames(n_samples: int, hop: int, sample_rate: int) -> int:
    """pyworld's frame count for n_samples: GetSamplesForDIO with frame_period = hop / fs * 1000, in the same double arithmetic."""
    frame_period = hop / sample_rate * 1000.0
    return int(1000.0 * n_samples / sample_rate / frame_period) + 1


def extract_pitch(audio: torch.Tensor, lens: torch.Tensor | None, hop: int, sample_rate: int, f0_floor: float = 71.0, f0_ceil: float = 800.0,
                  voicing_threshold: float = 0.8, interpolate: bool = True, estimator: str = "world", speed: int = 4) -> torch.Tensor:
    """Frame-level pitch (Hz) of a zero-padded batch [items, t_max] on the device: ``Preprocessor.extract_pitch``
    (preprocessor.py:244-285) -- ``pyworld.dio(x.f64, fs, frame_period = hop / fs * 1000, speed = 4)`` -> ``pyworld.stonemask`` -> unvoiced
    frames -> NaN -> linear interpolation across them, an utterance without any voiced frame -> zeros.

    ``estimator="world"`` (default, round 5): WORLD's DIO + StoneMask themselves, in float64 on the device (csrc/pitch_world.hip;
    oracle/pitch_world_ref.py restates the algorithm and reproduces the reference's pyworld fixture to 1e-13 Hz).  Output
    [items, world_frames(t_max)]: pyworld's frame count ((int)(1000 n / fs / frame_period) + 1, which is n // hop + 1 or one fewer when
    the double division lands below the integer); item i is valid up to world_frames(lens[i]), zero behind.
    ``estimator="acf"``: the normalised-autocorrelation tracker of rounds 2-4 (its own estimator: values differ from the reference's;
    output [items, t_max // hop + 1]; ``voicing_threshold`` applies to it only)."""
    from . import _lib

    if not audio.is_cuda:
        raise RuntimeError("everyvoice_amd.pipeline.extract_pitch computes on the GPU only (no CPU fallback)")
    if estimator not in ("world", "acf"):
        raise ValueError("extract_pitch: estimator 'world' (DIO + StoneMask, the reference's) or 'acf'")
    x = audio.to(torch.float32).reshape(-1, audio.shape[-1]).contiguous()
    items, t_max = x.shape
    lens32 = (torch.full((items,), t_max) if lens is None else lens).to(x.device, torch.int32).contiguous()
    lib = _lib.load()
    if estimator == "world":
        frames = world_frames(t_max, hop, sample_rate)
        f0 = torch.empty(items, frames, device=x.device, dtype=torch.float32)
        n_ws = lib.evmi_pitch_world_ws_elems(items, t_max, int(sample_rate), hop, int(speed), float(f0_floor), float(f0_ceil), 2.0)
        if n_ws <= 0:
            raise RuntimeError("extract_pitch: evmi_pitch_world_ws_elems rejected the shape")
        ws = torch.empty(n_ws, device=x.device, dtype=torch.float64)
        _lib.check(lib.evmi_pitch_world_f64(x.data_ptr(), lens32.data_ptr(), f0.data_ptr(), ws.data_ptr(), n_ws, items, t_max, int(sample_rate), hop, int(speed),
                                            float(f0_floor), float(f0_ceil), 2.0, 0.1, _lib.current_stream_ptr(x.device)), "evmi_pitch_world_f64")
        n_valid = [world_frames(int(n), hop, sample_rate) for n in lens32.cpu().tolist()]
    else:
        f0 = torch.empty(items, t_max // hop + 1, device=x.device, dtype=torch.float32)
        _lib.check(lib.evmi_pitch_acf_f32(x.data_ptr(), lens32.data_ptr(), f0.data_ptr(), items, t_max, hop, int(sample_rate), float(f0_floor),
                                          float(f0_ceil), float(voicing_threshold), _lib.current_stream_ptr(x.device)), "evmi_pitch_acf_f32")
        n_valid = [int(n) // hop + 1 for n in lens32.cpu().tolist()]
    if not interpolate:
        return f0
    out = f0.cpu().numpy().astype(np.float64)  # (per-utterance 1-D interpolation over a few hundred frames: host plumbing, as in the reference)
    for i in range(items):
        n = min(n_valid[i], out.shape[1])
        row = out[i, :n]
        voiced = row > 0
        if voiced.any():
            row[~voiced] = np.interp(np.nonzero(~voiced)[0], np.nonzero(voiced)[0], row[voiced])
        out[i, n:] = 0.0
    return torch.from_numpy(out.astype(np.float32)).to(x.device)


LOUDNESS_GATE_LKFS = -36.0  # preprocessor.py:180: "a conservative threshold"


def gate_audio(wav_path, cfg: AudioConfig):
    """The host-side gates of process_audio (file IO and counts): -> (audio [channels, S], sr) or (None, reason)."""
    audio, sr, seconds = load_wav(wav_path)
    if audio.shape[0] > 2:
        return None, "multichannel_files"
    if seconds > cfg.max_audio_length:
        return None, "audio_too_long"
    if seconds < cfg.min_audio_length:
        return None, "audio_too_short"
    return audio, sr


def _effects(sox_effects) -> list[Effect]:
    """A chain as written in a config (``list[list[str]]``, None) or already parsed -> effect records (ValueError if not reproduced)."""
    if sox_effects and all(isinstance(e, Effect) for e in sox_effects):
        return list(sox_effects)
    return parse_sox_effects(sox_effects)


def process_audio_batch(wavs: list[torch.Tensor], sr: int, cfg: AudioConfig, device, normalize: bool = True, resample_rate: int | None = None,
                        sox_effects=None, hop_size: int | None = None):
    """The device part of process_audio for a batch of gated utterances at one source rate: loudness gate -> mix-down -> the SoX
    effect chain ``sox_effects`` (sox.py; None, [] and the default ``[["channels", "1"]]`` are the mix-down alone) -> resample
    -> peak normalise -> truncate to a multiple of the hop (``hop_size``, default ``cfg.fft_hop_size``: process_audio(..., hop_size=),
    preprocessor.py:131).  wavs: [channels_i, S_i] host tensors.  An utterance the chain leaves shorter than one hop is skipped and
    counted under "audio_empty".
    -> (audio [n, t_max] on the device, lens [n] python ints (multiples of the hop), kept indices, {reason: count})."""
    from . import _lib

    effects = _effects(sox_effects)
    counters: dict[str, int] = {}
    n = len(wavs)
    if n == 0:
        return None, [], [], counters
    target_sr = resample_rate or sr
    kept_idx = []
    keep_mask = torch.ones(n, dtype=torch.bool)
    # loudness is measured on the file as loaded (all its channels, original rate), before any effect
    for ch in sorted({w.shape[0] for w in wavs}):
        idx = [i for i, w in enumerate(wavs) if w.shape[0] == ch]
        t_max = max(wavs[i].shape[1] for i in idx)
        batch = torch.zeros(len(idx), ch, t_max)
        for j, i in enumerate(idx):
            batch[j, :, : wavs[i].shape[1]] = wavs[i]
        lk = loudness(batch.to(device), torch.tensor([wavs[i].shape[1] for i in idx]), sr).cpu()
        for j, i in enumerate(idx):
            if torch.isnan(lk[j]) or float(lk[j]) < LOUDNESS_GATE_LKFS:
                keep_mask[i] = False
                counters["audio_empty"] = counters.get("audio_empty", 0) + 1
    kept_idx = [i for i in range(n) if keep_mask[i]]
    if not kept_idx:
        return None, [], [], counters
    t_max = max(wavs[i].shape[1] for i in kept_idx)
    mono = torch.zeros(len(kept_idx), t_max)
    for j, i in enumerate(kept_idx):
        mono[j, : wavs[i].shape[1]] = wavs[i].mean(0)  # SoX "channels 1" (the reference's default effect): the channels' mean
    x = mono.to(device)
    lens = [wavs[i].shape[1] for i in kept_idx]
    if effects:  # at the file's own rate, before resampling (preprocessor.py:187-198); lengths are read back once, here
        x, lens_dev = apply_sox_effects(x, torch.tensor(lens, dtype=torch.int32), sr, effects)
        lens = lens_dev.cpu().tolist()
        x = x[:, : max(1, max(lens))].contiguous()
    if target_sr != sr:
        x = resample(x, sr, target_sr)
        g = math.gcd(sr, target_sr)
        lens = [math.ceil((target_sr // g) * L / (sr // g)) for L in lens]
    if normalize:
        y = torch.empty_like(x)
        lens_t = torch.tensor(lens, dtype=torch.int32, device=x.device)
        _lib.check(_lib.load().evmi_peak_normalize_f32(x.data_ptr(), y.data_ptr(), lens_t.data_ptr(), x.shape[0], x.shape[1], 0.95,
                                                       _lib.current_stream_ptr(x.device)), "evmi_peak_normalize_f32")
        x = y
    hop = int(hop_size or cfg.fft_hop_size)
    lens = [L // hop * hop for L in lens]
    if effects and min(lens) == 0:  # trimmed to less than one hop (the reference fails there: torch.max of an empty tensor)
        rows = [j for j, L in enumerate(lens) if L > 0]
        counters["audio_empty"] = counters.get("audio_empty", 0) + len(lens) - len(rows)
        if not rows:
            return None, [], [], counters
        x = x[torch.tensor(rows, device=x.device)].contiguous()
        lens, kept_idx = [lens[j] for j in rows], [kept_idx[j] for j in rows]
    return x, lens, kept_idx, counters


def process_audio(wav_path, cfg: AudioConfig, normalize: bool = True, device="cuda:0", resample_rate: int | None = None, sox_effects=None):
    """(audio [S'] on the host, sr) with S' a multiple of the hop, or (None, reason) when the file is skipped
    (everyvoice/preprocessor/preprocessor.py:131-218).  ``sox_effects``: the dataset's SoX chain (see process_audio_batch),
    parsed before the file is read."""
    effects = _effects(sox_effects)
    audio, info = gate_audio(wav_path, cfg)
    if audio is None:
        return None, info
    x, lens, kept, counters = process_audio_batch([audio], info, cfg, torch.device(device), normalize, resample_rate or cfg.input_sampling_rate,
                                                  effects)
    if not kept:
        return None, next(iter(counters))
    return x[0, : lens[0]].cpu(), resample_rate or cfg.input_sampling_rate


def average_data_by_durations(data: torch.Tensor, durations) -> torch.Tensor:
    """Per-phone mean of ``data`` over ``d_i`` consecutive frames, 1e-7 where d_i == 0."""
    out, pos = [], 0
    for d in torch.as_tensor(durations).tolist():
        d = int(d)
        out.append(float(data[pos : pos + d].mean()) if d > 0 else 1e-7)
        pos += d
    return torch.tensor(out, dtype=torch.float32)


class ConfigLockMismatch(RuntimeError):
    """The preprocessed directory was written with another configuration (or an interrupted run): refuse to mix outputs."""


class GpuPreprocessor:
    """spec + energy (+ normalised audio) of a list of wavs, in the reference's on-disk layout, several utterances per launch."""

    def __init__(self, cfg: AudioConfig | None = None, device="cuda:0", batch_items: int = 32, pitch: bool = True):
        self.cfg = cfg or AudioConfig()
        self.device = torch.device(device)
        self.batch_items = batch_items
        self.pitch = pitch  # also write pitch/<...>--pitch.pt (FastSpeech2's pitch targets: WORLD's DIO + StoneMask on the device, see extract_pitch)
        in_sr, out_sr = self.cfg.input_sampling_rate, self.cfg.output_sampling_rate
        if out_sr <= 0 or in_sr <= 0 or out_sr % in_sr:  # (the reference floors the ratio silently; nothing downstream can use such a pair)
            raise ValueError(f"preprocessing.audio: output_sampling_rate {out_sr} must be a positive integer multiple of input_sampling_rate {in_sr}")
        self.rate_change = out_sr // in_sr
        self.transform = MelSpectrogram(self.cfg.n_fft, self.cfg.fft_window_size, self.cfg.fft_hop_size,
                                        self.cfg.input_sampling_rate, self.cfg.n_mels, self.cfg.f_min, self.cfg.f_max)
        # spec_type "mel" / "linear" (heavy.py:59-68, 101-107): the generic transforms, one utterance at a time (the ragged one-launch
        # front end above is the default type's); "raw" is complex and has no log / energy -- the reference's process_spec fails on it too
        self.generic = None
        if self.cfg.spec_type != "mel-librosa":
            if self.cfg.spec_type not in ("mel", "linear"):
                raise ValueError(f"preprocessing.audio.spec_type {self.cfg.spec_type!r}: a real-valued spectrogram type is needed")
            self.generic = get_spectral_transform(self.cfg.spec_type, self.cfg.n_fft, self.cfg.fft_window_size, self.cfg.fft_hop_size,
                                                  self.cfg.input_sampling_rate, self.cfg.n_mels, self.cfg.f_min, self.cfg.f_max)
        # the output side of a vocoder that upsamples (preprocessor.py:112-121): the same transform at n_fft c / win c / hop c.  The
        # reference hands it the INPUT sampling rate (so its mel filters sit at 1 / c of the output-rate audio's frequencies); reproduced.
        self.output_transform = None
        if self.rate_change > 1:
            c = self.rate_change
            self.output_transform = get_spectral_transform(self.cfg.spec_type, self.cfg.n_fft * c, self.cfg.fft_window_size * c,
                                                           self.cfg.fft_hop_size * c, self.cfg.input_sampling_rate, self.cfg.n_mels,
                                                           self.cfg.f_min, self.cfg.f_max)
        self.counters: dict[str, int] = {}
        self._interp = None
        self._source_data: dict = {}  # label -> the source_data entry of the current process() call (the .config-lock records it)

    def features(self, audio: torch.Tensor):
        """audio [S] (host or device) -> (log-mel [n_mels, S // hop], energy [S // hop]) on the device."""
        x = audio.to(self.device)
        n = x.shape[-1] // self.cfg.fft_hop_size
        if self.generic is not None:  # extract_spectral_features + extract_energy (preprocessor.py:220-233, 302-309) on any real spec
            spec = torch.log(torch.clamp(self.generic(x), min=1e-5))[..., :n].contiguous()
            return spec, torch.linalg.norm(spec, dim=-2)
        mel, energy = self.transform(x, log=True, return_energy=True)
        return mel[..., :n].contiguous(), energy[..., :n].contiguous()

    # -- .config-lock (preprocessor.py:974-1082) ----------------------------------------------------------------------
    def get_config_lock(self, in_progress: bool = True) -> dict:
        return {"info": "This file has the configuration that was used to preprocess files. Do not edit.",
                "status": "in progress" if in_progress else "completed",
                "preprocessing.audio": self.cfg.model_dump(mode="json"), "preprocessing.source_data": dict(self._source_data), "text": {}}

    def set_source(self, source: dict | None) -> list[Effect]:
        """Make ``source`` (a ``preprocessing.source_data`` entry: ``label``, ``sox_effects`` (default ``[["channels", "1"]]``), ...)
        the dataset of the next run and return its parsed chain; None: no dataset entry, the mix-down alone."""
        if source is None:
            self._source_data = {}
            return []
        if "label" not in source:
            raise ValueError("a source_data entry needs a 'label'")
        entry = {k: v for k, v in source.items() if k not in ("data_dir", "filelist")}  # as preprocessor.py:985-988 records it
        entry.setdefault("sox_effects", DEFAULT_CHAIN)
        effects = parse_sox_effects(entry["sox_effects"])
        self._source_data = {str(source["label"]): json.loads(json.dumps(entry, default=str))}
        return effects

    def save_config_lock(self, save_dir, in_progress: bool, merge: bool = True):
        """Write the lock; with ``merge`` the entries of the other labels an earlier run recorded there are kept."""
        save_dir = Path(save_dir)
        save_dir.mkdir(parents=True, exist_ok=True)
        lock = save_dir / ".config-lock"
        data = self.get_config_lock(in_progress)
        if lock.exists():
            if merge:
                try:
                    saved = json.loads(lock.read_text(encoding="utf8")).get("preprocessing.source_data") or {}
                except (json.JSONDecodeError, AttributeError):
                    saved = {}
                data["preprocessing.source_data"] = {**saved, **data["preprocessing.source_data"]}
            lock.chmod(0o666)
        with open(lock, "w", encoding="utf8") as f:
            json.dump(data, f, indent=2, ensure_ascii=False)
            f.write("\n")
        lock.chmod(0o444)  # read-only: discourages edits

    def config_lock_has_conflicts(self, save_dir) -> bool:
        lock = Path(save_dir) / ".config-lock"
        try:
            saved = json.loads(lock.read_text(encoding="utf8"))
        except FileNotFoundError:
            return False
        except json.JSONDecodeError:
            return True
        if saved.get("status") != "completed":  # an interrupted run's partial results cannot be trusted
            return True
        current = self.get_config_lock()
        if saved.get("preprocessing.audio") != current["preprocessing.audio"] or saved.get("text") != {}:
            return True
        locked = saved.get("preprocessing.source_data") or {}  # entries of a label in both must be equal (preprocessor.py:1072-1081)
        return any(locked[k] != v for k, v in current["preprocessing.source_data"].items() if k in locked)

    def process(self, items: list[dict], save_dir, overwrite: bool = False, source: dict | None = None) -> list[dict]:
        """items: dicts with ``basename``, ``speaker``, ``language``, ``wav``.  Returns the items that were kept.  Utterances are
        gated on the host (file IO), then run through the device pipeline in ragged batches of ``batch_items``: loudness gate,
        mix-down, the dataset's SoX effect chain, resampling to input_sampling_rate, peak normalisation, STFT -> mel -> log + energy
        in ONE launch per batch.  ``source``: the ``preprocessing.source_data`` entry the items belong to (``label``,
        ``sox_effects``, ...; preprocessor.py:591): its chain is applied and the lock records it under its label.  The chain is
        parsed (and refused with a ValueError) before anything is read or written."""
        effects = self.set_source(source)
        if self.config_lock_has_conflicts(save_dir) and not overwrite:
            raise ConfigLockMismatch(f"{save_dir}/.config-lock records another audio configuration, another configuration of the same "
                                     "source_data label or an interrupted run; preprocess into a new directory or pass overwrite=True")
        self.save_config_lock(save_dir, in_progress=True, merge=not overwrite)
        kept = []
        sr_tag, spec_fn = self.cfg.input_sampling_rate, f"spec-{self.cfg.input_sampling_rate}-{self.cfg.spec_type}.pt"
        hop = self.cfg.fft_hop_size
        pending: dict[int, list] = {}  # source sampling rate -> [(item, audio)]

        def flush(sr):
            group = pending.pop(sr, [])
            if not group:
                return
            x, lens, kept_idx, counters = process_audio_batch([a for _, a in group], sr, self.cfg, self.device, True, sr_tag, effects)
            for k, v in counters.items():
                self.counters[k] = self.counters.get(k, 0) + v
            if not kept_idx:
                return
            t_max = max(lens)
            x = x[:, :t_max].contiguous()
            if self.generic is None:
                mel, energy = self.transform(x, log=True, return_energy=True, lens=torch.tensor(lens, dtype=torch.int32))
            else:
                per_item = [self.features(x[j, : lens[j]]) for j in range(len(lens))]
                mel = torch.nn.utils.rnn.pad_sequence([m.t() for m, _ in per_item], batch_first=True).transpose(1, 2)
                energy = torch.nn.utils.rnn.pad_sequence([e for _, e in per_item], batch_first=True)
            pitch_host = extract_pitch(x, torch.tensor(lens), hop, sr_tag).cpu() if self.pitch else None
            x_host, mel_host, energy_host = x.cpu(), mel.cpu(), energy.cpu()
            for j, i in enumerate(kept_idx):
                it = group[i][0]
                ids = (it["basename"], it.get("speaker", "default"), it.get("language", "default"))
                n, frames = lens[j], lens[j] // hop
                save_wav(x_host[j, :n], feature_path(save_dir, "audio", *ids, f"audio-{sr_tag}.wav"), sr_tag, self.cfg.target_bit_depth)
                save_tensor(mel_host[j, :, :frames].clone(), feature_path(save_dir, "spec", *ids, spec_fn))
                save_tensor(energy_host[j, :frames].clone(), feature_path(save_dir, "energy", *ids, "energy.pt"))
                self.process_attn_prior(it, frames, save_dir, overwrite)  # (the reference's stage order: ... spec, attn, energy, pitch)
                if pitch_host is not None:
                    save_tensor(pitch_host[j, :frames].clone(), feature_path(save_dir, "pitch", *ids, "pitch.pt"))
                self.counters["processed_files"] = self.counters.get("processed_files", 0) + 1
                kept.append(dict(it, frames=frames, samples=n))
            if self.rate_change > 1:
                self._process_output_rate([group[i] for i in kept_idx], sr, effects, save_dir)

        for it in items:
            audio, info = gate_audio(it["wav"], self.cfg)
            if audio is None:
                self.counters[info] = self.counters.get(info, 0) + 1
                continue
            pending.setdefault(info, []).append((it, audio))
            if len(pending[info]) >= self.batch_items:
                flush(info)
        for sr in list(pending):
            flush(sr)
        self.save_config_lock(save_dir, in_progress=False)
        return kept

    def _process_output_rate(self, group: list, sr: int, effects, save_dir) -> None:
        """The output-rate side of the kept items of one batch (preprocessor.py:562-581, 898-915): the same chain from the file's rate
        straight to output_sampling_rate, truncated to a multiple of hop c -> ``audio-{output_sr}.wav``, and its log-mel through the
        output transform -> ``spec-{output_sr}-{spec_type}.pt``.  Counters are not touched (the reference's update_counters=False).
        The reference saves this audio to the INPUT path (its process_spec then reads the output path): a slip, not reproduced."""
        out_sr, hop = self.cfg.output_sampling_rate, self.cfg.fft_hop_size * self.rate_change
        x, lens, kept_idx, _ = process_audio_batch([a for _, a in group], sr, self.cfg, self.device, True, out_sr, effects, hop_size=hop)
        if not kept_idx:
            return
        # The spec is taken of the audio as the file holds it, PCM-16 rounding included: the reference's process_spec reads the saved file
        # back (preprocessor.py:898-915).  It matters here as it does not on the input side: the band above the input rate's Nyquist
        # frequency holds only the resampling filter's residue, and the mel rows that cover it move by 4e-3 under that rounding.
        x_host = pcm16_round_trip(x[:, : max(lens)].cpu())
        x = x_host.to(self.device)
        if self.generic is None:
            mel = self.output_transform(x, log=True, lens=torch.tensor(lens, dtype=torch.int32))
        else:
            mel = torch.nn.utils.rnn.pad_sequence([torch.log(torch.clamp(self.output_transform(x[j, : lens[j]]), min=1e-5)).t()
                                                   for j in range(len(lens))], batch_first=True).transpose(1, 2)
        mel_host = mel.cpu()
        for j, i in enumerate(kept_idx):
            it = group[i][0]
            ids = (it["basename"], it.get("speaker", "default"), it.get("language", "default"))
            save_wav(x_host[j, : lens[j]], feature_path(save_dir, "audio", *ids, f"audio-{out_sr}.wav"), out_sr, self.cfg.target_bit_depth)
            save_tensor(mel_host[j, :, : lens[j] // hop].clone(), feature_path(save_dir, "spec", *ids, f"spec-{out_sr}-{self.cfg.spec_type}.pt"))

    def process_attn_prior(self, item: dict, frames: int, save_dir, overwrite: bool = False) -> list[Path]:
        """The ``attn`` stage (preprocessor.py:672-740): one beta-binomial prior [frames, tokens] (float64, computed on the device
        by evmi_attention_prior_f64) per text representation the item carries -- ``attn/<...>--characters-attn-prior.pt`` for
        ``character_tokens``, ``...--phones-attn-prior.pt`` for ``phone_tokens`` ("/"-joined token strings, as the reference's text
        stage writes them into the filelist; a list of tokens is accepted too).  Existing files are kept unless ``overwrite``."""
        from .heavy import BetaBinomialInterpolator

        written = []
        ids = (item["basename"], item.get("speaker", "default"), item.get("language", "default"))
        for key, name in (("character_tokens", "characters"), ("phone_tokens", "phones")):
            toks = item.get(key)
            if not toks:  # None in datasets of the other representation, "" in multi-source datasets
                continue
            n_tok = len(toks.split("/")) if isinstance(toks, str) else len(toks)
            path = feature_path(save_dir, "attn", *ids, f"{name}-attn-prior.pt")
            if path.exists() and not overwrite:
                continue
            if self._interp is None:
                self._interp = BetaBinomialInterpolator(device=self.device)
            prior = self._interp(frames, n_tok)
            assert tuple(prior.shape) == (frames, n_tok)
            save_tensor(prior, path)
            written.append(path)
            if len(self._interp._cache) > 256:
                self._interp._cache.clear()
        return written

    @staticmethod
    def write_filelist(items: list[dict], path, fields=("basename", "speaker", "language", "characters", "character_tokens", "phone_tokens")) -> Path:
        """The processed filelist (``<save_dir>/<name>.psv``, preprocessor.py:1113-1180: text lives in the filelist, not on disk):
        pipe-separated with a header line, the columns the items actually carry."""
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        cols = [f for f in fields if any(it.get(f) not in (None, "") for it in items)] or ["basename"]
        with open(path, "w", encoding="utf8", newline="") as f:
            f.write("|".join(cols) + "\n")
            for it in items:
                vals = [it.get(c, "") for c in cols]
                vals = ["/".join(v) if isinstance(v, (list, tuple)) else ("" if v is None else str(v)) for v in vals]
                f.write("|".join(v.replace("\\", "\\\\").replace("|", "\\|") for v in vals) + "\n")
        return path

    # -- dataset statistics (preprocessor.py:378-490) -------------------------------------------------------------------
    def compute_stats(self, save_dir, energy: bool = True, pitch: bool = True):
        """(energy Scaler, pitch Scaler) over every saved ``energy/*energy*`` / ``pitch/*pitch*`` tensor (None where disabled)."""
        out = []
        for kind, on in (("energy", energy), ("pitch", pitch)):
            sc = None
            if on:
                sc = Scaler()
                for path in sorted(glob(str(Path(save_dir) / f"{kind}/**/*{kind}*"), recursive=True)):
                    sc.append(torch.load(path, weights_only=True).to(self.device))
            out.append(sc)
        return tuple(out)

    def normalize_stats(self, save_dir, energy_scaler, pitch_scaler) -> dict:
        """Standardise every saved energy / pitch tensor with the dataset statistics and return them as the ``stats`` dict that
        becomes FastSpeech2's ``Stats(pitch=StatsInfo(...), energy=StatsInfo(...))`` (tests/model_stubs.py:50-57)."""
        stats = {}
        for kind, sc in (("energy", energy_scaler), ("pitch", pitch_scaler)):
            if not sc or not len(sc):
                continue
            st = sc.calculate_stats()
            for path in sorted(glob(str(Path(save_dir) / f"{kind}/**/*{kind}*"), recursive=True)):
                save_tensor(sc.normalize(torch.load(path, weights_only=True).to(self.device)), path)
            stats[kind] = st
        return stats


def synthesize_from_spec(spec: torch.Tensor, vocoder, out_dir, basename: str, speaker: str = "default",
                         language: str = "default", sr: int = 22050) -> Path:
    """``everyvoice synthesize from-spec``: a saved ``[n_mels, T]`` (or ``[B, n_mels, T]``) log-mel -> wav file named
    like the reference's prediction writers (``<basename>--<speaker>--<language>--pred.wav``)."""
    dev = next(vocoder.parameters()).device
    mel = spec.to(dev, torch.float32)
    if mel.dim() == 2:
        mel = mel.unsqueeze(0)
    wav = vocoder(mel)
    path = Path(out_dir) / SEP.join([basename, speaker, language, "pred.wav"])
    save_wav(wav[0, 0], path, sr)
    return path


class Scaler:
    """Dataset-level statistics of a per-utterance feature (pitch, energy) and its standardisation -- the behaviour of the
    reference's ``Scaler`` (``everyvoice/preprocessor/helpers.py:47-106``): values are collected with ``append``; ``calculate_stats``
    takes min / max / unbiased std over the non-NaN entries and ``nanmean`` over all of them, and reports the extrema after
    ``(x - mean) / std``; the collected list is read-only from outside.  Tensors may live on any device."""

    _FIELDS = ("min", "max", "std", "mean", "norm_min", "norm_max")

    def __init__(self):
        self.clear_data()

    def clear_data(self):
        self._chunks: list[torch.Tensor] = []
        self._all: torch.Tensor | None = None
        for f in self._FIELDS:
            setattr(self, f, None)

    def append(self, value: torch.Tensor):
        self._chunks.append(value)
        self._all = None

    @property
    def data(self):
        return self._chunks

    @data.setter
    def data(self, value):
        raise ValueError(f"Scaler.data is read-only (got {value!r}): use Scaler.append(...) or Scaler.clear_data()")

    def __len__(self):
        return len(self._chunks)

    def normalize(self, x):
        return (x - self.mean) / self.std

    def denormalize(self, x):
        return x * self.std + self.mean

    def calculate_stats(self):
        if not self._chunks:
            return None
        if self._all is None:
            self._all = torch.cat(self._chunks)
        finite = self._all[~torch.isnan(self._all)]
        self.min, self.max, self.std = finite.min(), finite.max(), finite.std()
        self.mean = torch.nanmean(self._all)
        self.norm_min, self.norm_max = self.normalize(self.min), self.normalize(self.max)
        return {"sample_size": len(self), **{f: float(getattr(self, f)) for f in self._FIELDS}}


def _has_style_tokens(model) -> bool:
    cfg = getattr(model, "config", None)
    cfg = getattr(cfg, "model", cfg)  # (a FastSpeech2Config holds the model's configuration under .model)
    return bool(getattr(cfg, "use_global_style_token_module", False))


def _style_audio_config(model, audio_config=None, vocoder_config=None) -> AudioConfig:
    """The front end the model's training mels were made with: the caller's ``audio_config``, else the model's own (``model.audio_config``,
    or ``model.config.preprocessing.audio`` of a module that carries its whole FastSpeech2Config), else the vocoder configuration's -- the
    two are trained on the same features -- else the defaults."""
    if audio_config is not None:
        return audio_config
    own = getattr(model, "audio_config", None) or getattr(getattr(getattr(model, "config", None), "preprocessing", None), "audio", None)
    if own is not None:
        return own
    return vocoder_config.preprocessing.audio if vocoder_config is not None else AudioConfig()


def style_reference_mel(style_reference, cfg: AudioConfig | None = None, device="cuda:0", sampling_rate: int | None = None) -> torch.Tensor:
    """The style reference of a Global Style Token model -> its mel [1, T, n_mels] on the device, through the front end the training mels
    were made with (``cfg``: the model's ``preprocessing.audio``): load -> mono -> resample to ``input_sampling_rate`` -> log-mel.
    ``style_reference``: the path of a wav file (what the reference's demo passes, ``demo/app.py:410-431``) or a 1-D float waveform at
    ``sampling_rate`` (default: ``cfg.input_sampling_rate``)."""
    cfg = cfg or AudioConfig()
    if torch.is_tensor(style_reference) or isinstance(style_reference, np.ndarray):
        audio = torch.as_tensor(style_reference, dtype=torch.float32)
        if audio.dim() != 1:
            raise ValueError(f"style_reference: a 1-D waveform or the path of a wav file, got a tensor of shape {tuple(audio.shape)}")
        sr = int(sampling_rate or cfg.input_sampling_rate)
    else:
        audio, sr, _ = load_wav(style_reference)
        audio = audio.mean(0)  # mono, as the default `channels 1` of preprocessing mixes down
    x = audio.to(device)[None]
    if sr != cfg.input_sampling_rate:
        x = resample(x, sr, cfg.input_sampling_rate)
    mel, _ = GpuPreprocessor(cfg, device=device, pitch=False).features(x[0])
    if mel.shape[-1] < 1:
        raise ValueError(f"style_reference: {audio.numel()} samples at {sr} Hz give no mel frame (hop {cfg.fft_hop_size})")
    return mel.transpose(0, 1)[None].contiguous()


def style_reference_batch(references, cfg: AudioConfig | None = None, device="cuda:0", sampling_rate: int | None = None):
    """One style reference per item (each a wav path or a 1-D waveform, as ``style_reference_mel`` takes them) ->
    (mel [n, Tmax, n_mels] zero padded, lens int32 [n]) on the device: what ``FastSpeech2.__call__`` takes as ``style_mel`` /
    ``style_lens``, so that every item's style embedding is that of its own reference alone."""
    if isinstance(references, (str, Path)) or torch.is_tensor(references) or isinstance(references, np.ndarray) or not len(references):
        raise ValueError("style_reference_batch: a non-empty list of references (wav paths or 1-D waveforms), one per item")
    mels = [style_reference_mel(r, cfg, device, sampling_rate)[0] for r in references]
    lens = torch.tensor([m.shape[0] for m in mels], dtype=torch.int32)
    mel = torch.zeros(len(mels), int(lens.max()), mels[0].shape[1], device=mels[0].device, dtype=torch.float32)
    for i, m in enumerate(mels):
        mel[i, : m.shape[0]] = m
    return mel, lens.to(mel.device)


def target_frames_of(seconds, sampling_rate: int, hop: int) -> torch.Tensor:
    """Lengths in seconds (one per item; None or 0 = no target) -> ``target_frames`` as ``FastSpeech2.__call__`` takes them:
    ``round(seconds * sampling_rate / hop)`` frames of the model's front end (``input_sampling_rate`` / ``fft_hop_size``)."""
    return torch.tensor([int(round(float(s or 0.0) * sampling_rate / hop)) for s in seconds], dtype=torch.int64)


def _padded_controls(rows: list[dict], lens: torch.Tensor, defaults: dict) -> dict:
    """The ``duration_control`` / ``pitch_control`` / ``energy_control`` of a batch of rows: where no row carries one, the call's own
    value (``defaults``); where one does, a tensor [B, L] -- a row's per-symbol list (one value per symbol, ``ValueError`` otherwise) or
    number, the call's value for the rows without one, 1 at the padding."""
    out = {}
    for key, default in defaults.items():
        if not any(r.get(key) is not None for r in rows):
            out[key] = default
            continue
        if isinstance(default, torch.Tensor):
            raise ValueError(f"{key}: given as a tensor for the call and in a row of filelist_data; use one of the two")
        t = torch.ones(len(rows), int(lens.max()), dtype=torch.float32)
        for j, r in enumerate(rows):
            v, n = r.get(key), int(lens[j])
            if v is None or isinstance(v, (int, float)):
                t[j, :n] = float(default if v is None else v)
                continue
            v = torch.as_tensor(v, dtype=torch.float32).flatten()
            if v.shape[0] != n:
                raise ValueError(f"{r.get('basename')!r}: {key} has {v.shape[0]} values for {n} symbols")
            t[j, :n] = v
        out[key] = t
    return out


FORCED_FRAMES_SLACK = 11  # values a per-frame pitch / energy file may hold beyond the item's frames (fs2_dataset.py: 10 of the durations + 1)


def _forced_variances(model, directory, chunk: list[dict], spk: list, lang: list, durs: torch.Tensor, lens: torch.Tensor) -> dict:
    """``pitch=`` / ``energy=`` of a teacher-forced batch from the ``pitch/`` and ``energy/`` files next to its spectrograms: what the trainer
    embedded for these utterances.  Whether a file holds one value per symbol or per frame is the dataset's rule (``FastSpeech2Dataset``),
    never the tensor's length: per symbol iff ``learn_alignment`` is off and the predictor's level is "phone".  A per-frame file is held
    to the item's frames under the durations in use (``durs``) with the dataset's tolerances: one value short repeats the last and one
    value more is cut (pyworld's frame count against the STFT's), and up to ``FORCED_FRAMES_SLACK`` = 11 values more are cut -- that one,
    plus the 10 frames by which the dataset lets given durations sum to fewer frames than the spectrogram has; anything else is a
    ``ValueError``.  For a phone-level predictor the per-frame values are averaged over the durations in use
    (``ops.phone_average``, the trainer's function)."""
    from .fs2 import variance_settings
    from .train import ops

    cfg = getattr(model.config, "model", model.config)
    levels = variance_settings(cfg)["level"]
    L, frames = durs.shape[1], durs.clamp_min(0).sum(1)
    out = {}
    for key in ("pitch", "energy"):
        file_phone = (not bool(cfg.learn_alignment)) and levels[key] == "phone"
        rows = []
        for j, r in enumerate(chunk):
            p = feature_path(directory, key, r["basename"], spk[j], lang[j], f"{key}.pt")
            if not p.exists():
                raise FileNotFoundError(f"teacher forcing {r['basename']!r}: no {key} file {p}")
            v = torch.load(p, weights_only=True).to(torch.float32).flatten()
            want = int(lens[j]) if file_phone else int(frames[j])
            if not file_phone and v.shape[0] > 0 and -1 <= v.shape[0] - want <= FORCED_FRAMES_SLACK:
                v = v[:want] if v.shape[0] >= want else torch.cat([v, v[-1:]])
            if v.shape[0] != want:
                raise ValueError(f"teacher forcing {r['basename']!r}: {p} has {v.shape[0]} values, the configuration "
                                 f"({'phone' if file_phone else 'frame'} level) wants {want}")
            rows.append(v)
        width = L if file_phone else max(1, int(frames.max()))
        t = torch.zeros(len(chunk), width, dtype=torch.float32)
        for j, v in enumerate(rows):
            t[j, : v.shape[0]] = v
        if not file_phone and levels[key] == "phone":
            dev = model.device
            dur32 = durs.clamp_min(0).to(dev, torch.int32).contiguous()
            pad = torch.arange(L, device=dev)[None, :] >= lens.to(dev)[:, None]
            t = ops.phone_average(t.to(dev).contiguous(), torch.cumsum(dur32, 1, dtype=torch.int32).contiguous(), dur32, pad)
        out[key] = t
    return out


def synthesize_from_text(ids: torch.Tensor, lens: torch.Tensor, fs2, vocoder, out_dir, basenames: list[str], speaker: str = "default",
                         language: str = "default", output_types=("wav", "spec"), sr: int = 22050, hop: int = 256,
                         duration_control: float = 1.0, global_step: int | None = None, style_reference=None,
                         audio_config: AudioConfig | None = None, style_reference_sampling_rate: int | None = None,
                         mask_vocoder_padding: bool = False, pitch_control=1.0, energy_control=1.0, target_seconds=None) -> list[dict]:
    """The device part of ``everyvoice synthesize from-text`` (``fs2.cli.synthesize.synthesize_helper``,
    ``everyvoice/demo/app.py:84-106``): token ids -> FastSpeech2 (postnet mel) -> HiFiGAN -> files named as the reference's
    prediction writers name them (``everyvoice/base_cli/prediction_writing_callback.py:35-41``):
    ``<out_dir>/wav/<basename>--<speaker>--<language>--pred.wav`` and ``<out_dir>/synthesized_spec/...--spec-pred....pt``
    holding ``[n_mels, T]``.  Text normalisation / g2p (CPU string work) stays with the caller: ``ids`` are symbol ids, 0 pads.
    ``style_reference`` (a wav path, or a 1-D waveform at ``style_reference_sampling_rate``; ``audio_config``: the model's
    ``preprocessing.audio``, default as in ``synthesize_helper``): a model with the Global Style Token module needs it, any other refuses it.
    A list of references gives every item its own (``style_reference_batch``: padded together, passed with their lengths).
    ``mask_vocoder_padding``: the vocoder gets the mel lengths (``vocoder(mel, lens=mel_lens)``), so every item's waveform is the one
    it gets alone, whatever else is in the batch, and the padding frames are not computed.  Off: the batch runs as a rectangle.
    ``duration_control`` / ``pitch_control`` / ``energy_control``: a number, or a tensor per symbol [B, L] or per item [B], as
    ``FastSpeech2.__call__`` takes them.  ``target_seconds`` (a number for every item, or one per item; None or 0 = no target): the item is
    synthesised in exactly ``round(seconds * sr / hop)`` frames, i.e. that many times ``hop`` samples."""
    kw = {}
    if target_seconds is not None:
        per_item = target_seconds if isinstance(target_seconds, (list, tuple, torch.Tensor)) else [target_seconds] * ids.shape[0]
        kw["target_frames"] = target_frames_of(per_item, sr, hop)
    if style_reference is not None:
        if not _has_style_tokens(fs2):
            raise ValueError("style_reference given, but this model has no Global Style Token module (model.use_global_style_token_module)")
        cfg = _style_audio_config(fs2, audio_config)
        if isinstance(style_reference, (list, tuple)):  # one reference per item, each embedded alone at its own length
            if len(style_reference) != ids.shape[0]:
                raise ValueError(f"style_reference: a list needs one reference per item ({ids.shape[0]}), got {len(style_reference)}")
            kw["style_mel"], kw["style_lens"] = style_reference_batch(style_reference, cfg, fs2.device, style_reference_sampling_rate)
        else:
            kw["style_mel"] = style_reference_mel(style_reference, cfg, fs2.device, style_reference_sampling_rate)
    for key, control in (("pitch_control", pitch_control), ("energy_control", energy_control)):
        if isinstance(control, torch.Tensor) or control != 1.0:  # (a call that steers nothing stays the call it was)
            kw[key] = control
    mel, post, durations, _, _, mel_lens = fs2(ids, lens, duration_control=duration_control, **kw)
    wav = None
    if "wav" in output_types:
        vmel = post.transpose(1, 2).contiguous()
        wav = vocoder(vmel, lens=mel_lens) if mask_vocoder_padding else vocoder(vmel)
    results = []
    for i, base in enumerate(basenames):
        T = int(mel_lens[i])
        rec = {"basename": base, "frames": T, "durations": durations[i, : int(lens[i])].cpu()}
        if "spec" in output_types:
            p = Path(out_dir) / "synthesized_spec" / SEP.join([base, speaker, language, f"spec-pred-{sr}-mel-librosa.pt"])
            save_tensor(post[i, :T].transpose(0, 1).contiguous(), p)
            rec["spec"] = p
        if wav is not None:
            p = Path(out_dir) / "wav" / SEP.join([base, speaker, language, "pred.wav"])
            save_wav(wav[i, 0, : T * hop], p, sr)
            rec["wav"] = p
        results.append(rec)
    return results


class PredictionWriter:
    """A prediction writer of the reference's synthesis (``base_cli/prediction_writing_callback.py:14-41``): one per output format;
    ``get_filename(basename, speaker, language)`` = ``<save_dir>/<basename>--<speaker>--<language>[--ckpt=<step>]--<file_extension>``,
    ``last_file_written`` is what the demo hands back (``demo/app.py:107-108``)."""

    def __init__(self, save_dir: Path, file_extension: str, global_step: int = 0, include_global_step_in_filename: bool = False):
        self.file_extension = file_extension
        self.global_step = f"ckpt={global_step}"
        self.save_dir = Path(save_dir)
        self.sep = SEP
        self.include_global_step_in_filename = include_global_step_in_filename
        self.save_dir.mkdir(parents=True, exist_ok=True)
        self.last_file_written = None

    def get_filename(self, basename: str, speaker: str, language: str) -> str:
        parts = [basename, speaker, language, self.file_extension]
        if self.include_global_step_in_filename:
            parts.insert(-1, self.global_step)
        path = self.save_dir / self.sep.join(parts)
        path.parent.mkdir(parents=True, exist_ok=True)
        return str(path)


def synthesize_helper(model, texts: list, language: str | None, speaker: str | None, duration_control: float | None, global_step: int, output_type,
                      text_representation=None, accelerator: str = "auto", devices: str = "1", device=None, batch_size: int = 16, num_workers: int = 0,
                      filelist=None, filelist_data=None, output_dir: Path = Path("synthesis_output"), teacher_forcing_directory: Path | None = None,
                      vocoder_model=None, vocoder_config=None, vocoder_global_step: int | None = None, style_reference=None, return_scores: bool = False,
                      text_to_ids=None, audio_config: AudioConfig | None = None, style_reference_sampling_rate: int | None = None,
                      mask_vocoder_padding: bool = False, write_durations: bool = False, pitch_control=1.0, energy_control=1.0, target_seconds=None,
                      teacher_force_variances: bool = False, alignment_scores: bool = False):
    """``fs2.cli.synthesize.synthesize_helper`` (call site ``everyvoice/demo/app.py:84-106``, same keyword names) for the path this
    library accelerates: texts -> symbol ids -> FastSpeech2 -> (vocoder) -> files through per-format writers.
    Returns ``(config, device, predictions, callbacks)`` with ``callbacks`` keyed by output format ("wav", "spec").

    ``texts`` are strings mapped to ids by ``text_to_ids`` (the reference's TextProcessor: CPU string work, out of scope) or already
    lists / tensors of symbol ids; ``filelist_data`` rows (dicts with basename / ids / speaker / language) replace ``texts``.
    ``teacher_forcing_directory``: synthesise every utterance with its ground-truth durations -- how the spectrograms for vocoder
    matching are produced (docs/guides/finetune.md:18-43): the written spectrogram has the frame count of the real one.  The durations
    are read from ``duration/<basename>--<speaker>--<language>--duration.pt`` there where that file exists (a model trained with
    ``learn_alignment: false`` on supplied durations).  Where it does not and the model carries its aligner (``model.has_aligner``: trained
    with the default ``learn_alignment: true``, whose durations never reach the disk) they come from ``model.align`` over the utterance's
    ``spec/<basename>--<speaker>--<language>--spec-<input_sr>-<spec_type>.pt`` ([n_mels, T]); otherwise ``FileNotFoundError`` names both
    files.  ``write_durations``: also save what the aligner found as the ``duration/`` file.
    ``style_reference``: the path of a wav file (the demo's ``gr.Audio(type="filepath")``) or a 1-D float waveform (at
    ``style_reference_sampling_rate``, default the front end's input rate), for a model with the Global Style Token module: it goes through
    the front end the training mels were made with (``audio_config``; default: the model's own ``audio_config`` /
    ``config.preprocessing.audio``, else the vocoder configuration's, else the defaults) and ONE style embedding serves every text of the call.  A model without the module refuses it; a model with the module refuses a call without it.
    ``mask_vocoder_padding``: the vocoder gets each batch's mel lengths (``vocoder_model(mel, lens=mel_lens)``): an utterance's audio no
    longer depends on ``batch_size`` or on its neighbours, and the padding frames are not computed.  A keyword, not a configuration
    field (the vocoder's model configuration mirrors the reference's schema).  Off (the default): the batch runs as a rectangle.
    Steering: ``pitch_control`` / ``energy_control`` beside ``duration_control``, numbers for the whole call; a
    ``filelist_data`` row may carry its own under the same names -- a number, or a list with one value per symbol -- which are padded
    into the batch's [B, L] tensors.  ``target_seconds`` (for the call, or a row's own): the utterance is synthesised in exactly
    ``round(seconds * input_sampling_rate / fft_hop_size)`` frames of the audio configuration the file names come from.
    ``teacher_force_variances`` (needs ``teacher_forcing_directory``): every utterance's ``pitch/...--pitch.pt`` and ``energy/...--energy.pt``
    are read and forced as well, so that the spectrogram is made under what the trainer embedded (``_forced_variances``: the dataset's
    rule for phone- or frame-level files; a missing file is a ``FileNotFoundError`` naming it).  Off: the predictors' own values.
    ``alignment_scores`` (needs ``teacher_forcing_directory``): every prediction record gets the key
    ``alignment_scores`` -- for an utterance the model aligned itself ``{"attn_ctc", "attn_path"}`` (numbers) and ``"symbol"`` (float32
    [symbols]: the mean log soft attention of each symbol over its frames), from ``model.align(return_scores=True)``; ``None`` for one
    whose durations were read from a ``duration/`` file.  (``return_scores`` is the reference's keyword and is not this.)"""
    if alignment_scores and teacher_forcing_directory is None:
        raise ValueError("alignment_scores needs a teacher_forcing_directory: the scores are those of the utterances the model aligns there")
    if teacher_force_variances and teacher_forcing_directory is None:
        raise ValueError("teacher_force_variances needs a teacher_forcing_directory: the pitch/ and energy/ files are read from it")
    if style_reference is not None and not _has_style_tokens(model):
        raise ValueError("style_reference given, but this model has no Global Style Token module (model.use_global_style_token_module)")
    formats = [getattr(f, "value", f) for f in (output_type if isinstance(output_type, (list, tuple)) else [output_type])]
    unsupported = [f for f in formats if f not in ("wav", "spec")]
    if unsupported:
        raise NotImplementedError(f"output formats {unsupported}: textgrid / readalong outputs belong to the reference's text front-end (out of scope)")
    dev = torch.device(device) if device is not None else model.device
    output_dir = Path(output_dir)
    sr = vocoder_config.preprocessing.audio.output_sampling_rate if vocoder_config is not None else 22050
    in_sr = vocoder_config.preprocessing.audio.input_sampling_rate if vocoder_config is not None else 22050
    hop_out = (vocoder_config.preprocessing.audio.fft_hop_size * (sr // in_sr)) if vocoder_config is not None else 256
    hop_in = vocoder_config.preprocessing.audio.fft_hop_size if vocoder_config is not None else 256  # (a frame of the model, in input samples)
    tf_audio = vocoder_config.preprocessing.audio if vocoder_config is not None else audio_config
    spec_fn = f"spec-{in_sr}-{getattr(tf_audio, 'spec_type', 'mel-librosa')}.pt"  # the ground-truth spectrogram teacher forcing aligns
    callbacks = {}
    if "wav" in formats:
        if vocoder_model is None:
            raise ValueError("output_type 'wav' needs a vocoder_model")
        callbacks["wav"] = PredictionWriter(output_dir / "wav", "pred.wav", vocoder_global_step or 0, include_global_step_in_filename=False)
    if "spec" in formats:
        callbacks["spec"] = PredictionWriter(output_dir / "synthesized_spec", f"spec-pred-{in_sr}-mel-librosa.pt", global_step)
    rows = []
    if filelist_data is not None:
        rows = [dict(r) for r in filelist_data]
    else:
        for i, t in enumerate(texts):
            ids = text_to_ids(t) if isinstance(t, str) else t
            if isinstance(t, str) and text_to_ids is None:
                raise ValueError("synthesize_helper: pass text_to_ids (text -> symbol ids) or symbol ids; text processing is host-side string work")
            rows.append({"basename": f"utt-{i:04d}" if not isinstance(t, str) else "".join(c if c.isalnum() else "-" for c in t)[:20] or f"utt-{i:04d}",
                         "ids": ids, "speaker": speaker, "language": language})
    predictions = []
    style_mel = None
    if style_reference is not None:
        style_mel = style_reference_mel(style_reference, _style_audio_config(model, audio_config, vocoder_config), dev, style_reference_sampling_rate)
    for lo in range(0, len(rows), batch_size):
        chunk = rows[lo : lo + batch_size]
        lens = torch.tensor([len(r["ids"]) for r in chunk])
        ids = torch.zeros(len(chunk), int(lens.max()), dtype=torch.long)
        for j, r in enumerate(chunk):
            ids[j, : lens[j]] = torch.as_tensor(r["ids"], dtype=torch.long)
        kw = {}
        spk = [r.get("speaker") or speaker or "default" for r in chunk]
        lang = [r.get("language") or language or "default" for r in chunk]
        if getattr(model, "speaker2id", None) and getattr(model.config, "multispeaker", False):
            kw["speakers"] = torch.tensor([model.speaker2id[s] for s in spk])
        if getattr(model, "lang2id", None) and getattr(model.config, "multilingual", False):
            kw["languages"] = torch.tensor([model.lang2id[x] for x in lang])
        scored = {}  # row of the chunk -> the alignment scores of an utterance the model aligned itself
        if teacher_forcing_directory is not None:
            durs = torch.zeros_like(ids)
            found = [feature_path(teacher_forcing_directory, "duration", r["basename"], spk[j], lang[j], "duration.pt") for j, r in enumerate(chunk)]
            for j in range(len(chunk)):
                if found[j].exists():
                    durs[j, : lens[j]] = torch.load(found[j], weights_only=True)[: lens[j]].long()
            missing = [j for j in range(len(chunk)) if not found[j].exists()]
            if missing:  # no duration file: the model's own aligner over the utterance's ground-truth spectrogram
                specs = [feature_path(teacher_forcing_directory, "spec", chunk[j]["basename"], spk[j], lang[j], spec_fn) for j in missing]
                for j, p in zip(missing, specs):
                    if not getattr(model, "has_aligner", False) or not p.exists():
                        raise FileNotFoundError(f"teacher forcing {chunk[j]['basename']!r}: no duration file {found[j]} and "
                                                + (f"no spectrogram {p} to align" if getattr(model, "has_aligner", False)
                                                   else f"the model has no aligner to find the durations from {p}"))
                mels = [torch.load(p, weights_only=True).to(torch.float32).transpose(0, 1) for p in specs]  # [T, n_mels] each
                mel = torch.nn.utils.rnn.pad_sequence(mels, batch_first=True)
                sel = torch.tensor(missing)
                akw = {key: kw[key][sel] for key in ("speakers", "languages") if key in kw}
                if alignment_scores:
                    akw["return_scores"] = True
                aligned = model.align(ids[sel], lens[sel], mel, torch.tensor([m.shape[0] for m in mels]), **akw)
                if alignment_scores:
                    aligned, sc = aligned
                    ctc, on_path, symbol = sc.ctc.cpu(), sc.path.cpu(), sc.symbol.cpu()
                    for row, j in enumerate(missing):
                        scored[j] = {"attn_ctc": float(ctc[row]), "attn_path": float(on_path[row]), "symbol": symbol[row, : lens[j]].clone()}
                aligned = aligned.cpu()
                for row, j in enumerate(missing):
                    durs[j, : lens[j]] = aligned[row, : lens[j]]
                    if write_durations:
                        save_tensor(aligned[row, : lens[j]].clone(), found[j])
            kw["durations"] = durs
            if teacher_force_variances:
                kw.update(_forced_variances(model, teacher_forcing_directory, chunk, spk, lang, durs, lens))
        if style_mel is not None:
            kw["style_mel"] = style_mel
        controls = _padded_controls(chunk, lens, {"duration_control": 1.0 if duration_control is None else duration_control,
                                                  "pitch_control": pitch_control, "energy_control": energy_control})
        for key in ("pitch_control", "energy_control"):
            if isinstance(controls[key], torch.Tensor) or controls[key] != 1.0:  # (a call that steers nothing stays the call it was)
                kw[key] = controls[key]
        if target_seconds is not None or any(r.get("target_seconds") is not None for r in chunk):
            kw["target_frames"] = target_frames_of([target_seconds if r.get("target_seconds") is None else r["target_seconds"] for r in chunk], in_sr, hop_in)
        _, post, durations, _, _, mel_lens = model(ids, lens, duration_control=controls["duration_control"], **kw)
        wav = None
        if "wav" in formats:
            vmel = post.transpose(1, 2).contiguous()
            wav = vocoder_model(vmel, lens=mel_lens) if mask_vocoder_padding else vocoder_model(vmel)
        for j, r in enumerate(chunk):
            T = int(mel_lens[j])
            rec = {"basename": r["basename"], "speaker": spk[j], "language": lang[j], "frames": T, "durations": durations[j, : int(lens[j])].cpu()}
            if alignment_scores:
                rec["alignment_scores"] = scored.get(j)
            if "spec" in formats:
                path = callbacks["spec"].get_filename(r["basename"], spk[j], lang[j])
                save_tensor(post[j, :T].transpose(0, 1).contiguous(), path)
                callbacks["spec"].last_file_written = rec["spec"] = path
            if wav is not None:
                path = callbacks["wav"].get_filename(r["basename"], spk[j], lang[j])
                save_wav(wav[j, 0, : T * hop_out], path, sr)
                callbacks["wav"].last_file_written = rec["wav"] = path
            predictions.append(rec)
    return model.config, dev, predictions, callbacks


def generate_teacher_forced_specs(model, filelist_data: list[dict], preprocessed_dir, global_step: int = 0, batch_size: int = 16,
                                  write_durations: bool = False, teacher_force_variances: bool = False, alignment_scores: bool = False):
    """Vocoder matching, step 1 (docs/guides/finetune.md:18-43: ``everyvoice synthesize from-text ... -O spec
    --teacher-forcing-directory <preprocessed>``): the feature-prediction network's spectrogram of every training utterance under its
    ground-truth durations, written next to the real features as ``synthesized_spec/...--spec-pred-<sr>-mel-librosa.pt`` -- what
    ``training.finetune: true`` then feeds the vocoder (dataset.SpecDataset).  The durations: the ``duration/`` files, or the model's
    aligner over ``spec/`` (``synthesize_helper``); ``write_durations`` keeps what the aligner found as ``duration/`` files.
    ``teacher_force_variances``: the ``pitch/`` and ``energy/`` files are forced too, as the trainer embedded them (``synthesize_helper``).
    ``alignment_scores``: each record carries the aligner's scores of the utterance, ``None`` where a ``duration/`` file was read
    (``synthesize_helper``)."""
    _, _, preds, callbacks = synthesize_helper(model, [], None, None, 1.0, global_step, ["spec"], filelist_data=filelist_data,
                                               output_dir=Path(preprocessed_dir), teacher_forcing_directory=Path(preprocessed_dir), batch_size=batch_size,
                                               write_durations=write_durations, teacher_force_variances=teacher_force_variances,
                                               alignment_scores=alignment_scores)
    return preds


ALIGNMENT_SCORE_FIELDS = ("basename", "speaker", "language", "symbols", "frames", "seconds", "symbols_per_second", "attn_ctc", "attn_path",
                          "worst_symbol", "worst_symbol_score")


def score_alignments(model, filelist_data: list[dict], preprocessed_dir, batch_size: int = 16, audio_config: AudioConfig | None = None,
                     out_path=None) -> list[dict]:
    """The device half of the reference's ``everyvoice check data`` (``base_cli/check_group.py:15-50``): how well the model's own aligner
    explains every utterance of a preprocessed dataset, for finding the mis-transcribed and the clipped ones.
    Each row's ``spec/<basename>--<speaker>--<language>--spec-<input_sr>-<spec_type>.pt`` ([n_mels, T]; rate and type from
    ``audio_config``, default 22050 / mel-librosa) is read as teacher forcing reads it, the rows are aligned in ragged batches of
    ``batch_size`` by ``model.align(return_scores=True)``, and one record per row comes back in input order: ``basename``, ``speaker``,
    ``language``, ``symbols``, ``frames``, ``seconds`` (frames * fft_hop_size / input_sampling_rate), ``symbols_per_second``, ``attn_ctc``
    (the CTC forward-sum loss the trainer minimises, per symbol, of the utterance aligned ALONE over its own symbols: not the value a
    padded training batch produces, whose first log-softmax runs over the padded symbols too -- DESIGN.md section 34), ``attn_path`` (the binarisation loss on the aligner's own path),
    ``worst_symbol`` / ``worst_symbol_score`` (the index and the value of the lowest mean log soft attention over a symbol's frames) and
    ``durations`` (int64 [symbols]).  An utterance's record does not depend on ``batch_size`` or on its neighbours.
    ``out_path``: the records without the durations as a pipe-separated file with a header line.
    ``ValueError`` before any file is read: a model without an aligner.  ``FileNotFoundError``: a missing spectrogram, by name."""
    if not getattr(model, "has_aligner", False):
        raise ValueError("score_alignments: this model has no aligner (model.learn_alignment off, or the state dict held no `attention.*` tensors)")
    in_sr = audio_config.input_sampling_rate if audio_config is not None else 22050
    hop = audio_config.fft_hop_size if audio_config is not None else 256
    spec_fn = f"spec-{in_sr}-{getattr(audio_config, 'spec_type', 'mel-librosa')}.pt"
    rows = [dict(r) for r in filelist_data]
    records = []
    for lo in range(0, len(rows), batch_size):
        chunk = rows[lo : lo + batch_size]
        spk = [r.get("speaker") or "default" for r in chunk]
        lang = [r.get("language") or "default" for r in chunk]
        paths = [feature_path(preprocessed_dir, "spec", r["basename"], spk[j], lang[j], spec_fn) for j, r in enumerate(chunk)]
        for r, p in zip(chunk, paths):
            if not p.exists():
                raise FileNotFoundError(f"score_alignments {r['basename']!r}: no spectrogram {p} to align")
        lens = torch.tensor([len(r["ids"]) for r in chunk])
        ids = torch.zeros(len(chunk), int(lens.max()), dtype=torch.long)
        for j, r in enumerate(chunk):
            ids[j, : lens[j]] = torch.as_tensor(r["ids"], dtype=torch.long)
        mels = [torch.load(p, weights_only=True).to(torch.float32).transpose(0, 1) for p in paths]  # [T, n_mels] each
        durations, sc = model.align(ids, lens, torch.nn.utils.rnn.pad_sequence(mels, batch_first=True), torch.tensor([m.shape[0] for m in mels]),
                                    return_scores=True)
        durations, ctc, on_path, symbol = durations.cpu(), sc.ctc.cpu(), sc.path.cpu(), sc.symbol.cpu()
        for j, r in enumerate(chunk):
            n, frames = int(lens[j]), mels[j].shape[0]
            worst = int(torch.argmin(symbol[j, :n]))
            seconds = frames * hop / in_sr
            records.append({"basename": r["basename"], "speaker": spk[j], "language": lang[j], "symbols": n, "frames": frames, "seconds": seconds,
                            "symbols_per_second": n / seconds, "attn_ctc": float(ctc[j]), "attn_path": float(on_path[j]), "worst_symbol": worst,
                            "worst_symbol_score": float(symbol[j, worst]), "durations": durations[j, :n].clone()})
    if out_path is not None:
        GpuPreprocessor.write_filelist(records, out_path, fields=ALIGNMENT_SCORE_FIELDS)
    return records


# ---- synthesis against the recordings ------------------------------------------------------------------------
MCD_DB_SCALE = 10.0 * math.sqrt(2.0) / math.log(10.0)
MCD_MAX_CEPSTRA = 24  # evmi_dtw_cepstral_f32's limit on K


class MelCepstralDistortion(NamedTuple):
    """``mel_cepstral_distortion``'s results, on the device: mcd [B] (dB, the mean along the warping path), steps [B] int32 (the path's
    cells), lo / hi [B, Tb] int32 (first and last frame of ``mel_a`` the path pairs with frame j of ``mel_b``; -1 beyond the item),
    frame_mcd [B, Tb] (dB, the mean over the path's cells of that column; 0 beyond the item)."""

    mcd: torch.Tensor
    steps: torch.Tensor
    lo: torch.Tensor
    hi: torch.Tensor
    frame_mcd: torch.Tensor


def mel_cepstral_basis(n_mels: int, n_cepstra: int = 13) -> torch.Tensor:
    """Rows k = 1 .. n_cepstra of the orthonormal DCT-II over n_mels bins, sqrt(2 / M) cos(pi / M (m + 1/2) k), built in float64 and
    returned as float32 [n_cepstra, n_mels].  c0 (the frame's level) is left out."""
    if not 1 <= n_cepstra <= n_mels - 1:
        raise ValueError(f"mel_cepstral_basis: n_cepstra must be between 1 and n_mels - 1 = {n_mels - 1}, got {n_cepstra}")
    m = torch.arange(n_mels, dtype=torch.float64)
    k = torch.arange(1, n_cepstra + 1, dtype=torch.float64)
    return (math.sqrt(2.0 / n_mels) * torch.cos(math.pi / n_mels * (m[None, :] + 0.5) * k[:, None])).to(torch.float32)


def _check_n_cepstra(n_cepstra: int, n_mels: int, who: str) -> None:
    if not 1 <= n_cepstra <= MCD_MAX_CEPSTRA or n_cepstra > n_mels - 1:
        raise ValueError(f"{who}: n_cepstra must be between 1 and min({MCD_MAX_CEPSTRA}, n_mels - 1 = {n_mels - 1}), got {n_cepstra}")


def mel_cepstral_distortion(mel_a: torch.Tensor, lens_a: torch.Tensor, mel_b: torch.Tensor, lens_b: torch.Tensor,
                            n_cepstra: int = 13) -> MelCepstralDistortion:
    """Mel-cepstral distortion along the dynamic-time-warping path (MCD-DTW), in dB, of two batches of natural-log mels as the
    preprocessor stores them and ``FastSpeech2.__call__`` returns them: mel_a [B, Ta, n_mels], mel_b [B, Tb, n_mels] time-major with
    their frame counts; one launch (``evmi_dtw_cepstral_f32``), each item over its own lengths, Tb <= 1024.

    This is the distortion of the LOG-MEL CEPSTRUM (the DCT of the log-mel frame: MFCC 1 .. n_cepstra, c0 left out), scaled by
    10 sqrt(2) / ln 10 -- not of an mcep (mel-generalised cepstral) analysis of the waveform.  Absolute values compare only with
    tools that define it the same way."""
    from .train import ops

    if mel_a.dim() != 3 or mel_b.dim() != 3 or mel_a.shape[0] != mel_b.shape[0] or mel_a.shape[2] != mel_b.shape[2]:
        raise ValueError(f"mel_cepstral_distortion: expected [B, Ta, n_mels] and [B, Tb, n_mels], got {tuple(mel_a.shape)} and {tuple(mel_b.shape)}")
    _check_n_cepstra(n_cepstra, mel_a.shape[2], "mel_cepstral_distortion")
    if not mel_a.is_cuda:
        raise RuntimeError("everyvoice_amd.pipeline.mel_cepstral_distortion computes on the GPU only (no CPU fallback)")
    dev = mel_a.device
    a, b = mel_a.to(torch.float32).contiguous(), mel_b.to(dev, torch.float32).contiguous()
    basis = mel_cepstral_basis(a.shape[2], n_cepstra).to(dev)
    la, lb = torch.as_tensor(lens_a).to(dev, torch.int32).contiguous(), torch.as_tensor(lens_b).to(dev, torch.int32).contiguous()
    return MelCepstralDistortion(*ops.dtw_cepstral(a, la, b, lb, basis, MCD_DB_SCALE))


SYNTHESIS_EVALUATION_FIELDS = ("basename", "speaker", "language", "symbols", "frames_ref", "frames_syn", "length_ratio", "mcd_dtw", "mcd_dtw_sl",
                               "path_steps", "off_diagonal", "worst_symbol", "worst_symbol_mcd", "f0_rmse_cents", "vuv_error", "voiced_pairs", "note")


def f0_agreement(f0_syn, f0_ref, hi):
    """(f0_rmse_cents, vuv_error, voiced_pairs) of two uninterpolated F0 tracks (Hz, 0 = unvoiced; 1-D, on the host): recorded frame j
    is paired with synthesized frame hi[j].  RMSE in cents over the pairs that are both voiced (NaN without any); the share of recorded
    frames whose voicing differs."""
    f0_syn, f0_ref, hi = np.asarray(f0_syn, np.float64), np.asarray(f0_ref, np.float64), np.asarray(hi, np.int64)
    n = min(len(hi), len(f0_ref))
    ref, syn = f0_ref[:n], f0_syn[np.clip(hi[:n], 0, len(f0_syn) - 1)]
    both = (ref > 0) & (syn > 0)
    rmse = float(np.sqrt(np.mean((1200.0 * np.log2(syn[both] / ref[both])) ** 2))) if both.any() else float("nan")
    return rmse, float(np.mean((ref > 0) != (syn > 0))), int(both.sum())


def evaluate_synthesis(model, filelist_data: list[dict], preprocessed_dir, batch_size: int = 16, audio_config: AudioConfig | None = None,
                       vocoder=None, duration_control: float = 1.0, n_cepstra: int = 13, out_path=None) -> list[dict]:
    """How close the model's own, free-running synthesis is to the recording, per utterance of a preprocessed dataset (DESIGN.md section
    35): the free-running twin of ``score_alignments``.  Every row is synthesized from its symbols alone (speakers and languages
    resolved as ``synthesize_helper`` does; a model with the Global Style Token module gets the utterance's own recorded mel, with its
    length, as its style reference), its ``spec/`` file is read exactly as ``score_alignments`` reads it, and
    ``mel_cepstral_distortion(synthesized, recording)`` warps one onto the other.  One record per row, in input order:
    ``basename``, ``speaker``, ``language``, ``symbols``, ``frames_ref``, ``frames_syn``, ``length_ratio`` (syn / ref), ``mcd_dtw`` (dB; of
    the log-mel cepstrum, see ``mel_cepstral_distortion``), ``mcd_dtw_sl`` (mcd_dtw x max(frames) / min(frames): a wrong length costs),
    ``path_steps``, ``off_diagonal`` (1 - diagonal steps / (path_steps - 1); 0 for a one-cell path), ``worst_symbol`` /
    ``worst_symbol_mcd`` (the symbol with the highest mean per-frame distortion over its recorded frames; the recording's durations
    come from its ``duration/`` file, else from ``model.align`` where ``model.has_aligner``, else both are None; symbols without frames
    are skipped), ``lo`` / ``hi`` (int32 [frames_ref]: the synthesized frames the path pairs with each recorded frame).
    ``vocoder``: also ``f0_rmse_cents``, ``vuv_error``, ``voiced_pairs`` (``f0_agreement``) between ``extract_pitch(interpolate=False)`` of
    the vocoded synthesis and of the recording ``audio/...--audio-<output_sr>.wav``, both at the output rate with a hop of
    fft_hop_size x (output_sr // input_sr); recorded frame j is paired with synthesized frame hi[j].  Without a vocoder: None.
    An utterance beyond the kernel's limits (more than 1024 recorded frames, or more synthesized frames than ``ops.dtw_plan`` allows)
    gets NaN metrics and a ``note``, not an exception.
    A record does not depend on ``batch_size`` or on its neighbours whenever the model's mel does not: that needs the model's
    ``mask_padding``; the warping itself never depends on them.
    ``out_path``: the records without the tensors as a pipe-separated file with a header line.
    ``ValueError`` before any file is read: ``n_cepstra`` outside 1 .. 24 or above n_mels - 1.  ``FileNotFoundError``: a missing
    spectrogram or (with a vocoder) recording, by name."""
    from .train import ops

    n_mels = model.config.n_mels
    _check_n_cepstra(n_cepstra, n_mels, "evaluate_synthesis")
    in_sr = audio_config.input_sampling_rate if audio_config is not None else 22050
    out_sr = audio_config.output_sampling_rate if audio_config is not None else 22050
    hop = audio_config.fft_hop_size if audio_config is not None else 256
    hop_out = hop * (out_sr // in_sr)
    spec_fn = f"spec-{in_sr}-{getattr(audio_config, 'spec_type', 'mel-librosa')}.pt"
    nan = float("nan")
    rows = [dict(r) for r in filelist_data]
    records = []
    for start in range(0, len(rows), batch_size):
        chunk = rows[start : start + batch_size]
        spk = [r.get("speaker") or "default" for r in chunk]
        lang = [r.get("language") or "default" for r in chunk]
        paths = [feature_path(preprocessed_dir, "spec", r["basename"], spk[j], lang[j], spec_fn) for j, r in enumerate(chunk)]
        for r, p in zip(chunk, paths):
            if not p.exists():
                raise FileNotFoundError(f"evaluate_synthesis {r['basename']!r}: no spectrogram {p} to compare with")
        wavs = [feature_path(preprocessed_dir, "audio", r["basename"], spk[j], lang[j], f"audio-{out_sr}.wav") for j, r in enumerate(chunk)]
        if vocoder is not None:
            for r, p in zip(chunk, wavs):
                if not p.exists():
                    raise FileNotFoundError(f"evaluate_synthesis {r['basename']!r}: no recording {p} for the F0 comparison")
        lens = torch.tensor([len(r["ids"]) for r in chunk])
        ids = torch.zeros(len(chunk), int(lens.max()), dtype=torch.long)
        for j, r in enumerate(chunk):
            ids[j, : lens[j]] = torch.as_tensor(r["ids"], dtype=torch.long)
        mels = [torch.load(p, weights_only=True).to(torch.float32).transpose(0, 1) for p in paths]  # [T, n_mels] each
        ref = torch.nn.utils.rnn.pad_sequence(mels, batch_first=True)
        ref_lens = torch.tensor([m.shape[0] for m in mels])
        kw = {}
        if getattr(model, "speaker2id", None) and getattr(model.config, "multispeaker", False):
            kw["speakers"] = torch.tensor([model.speaker2id[s] for s in spk])
        if getattr(model, "lang2id", None) and getattr(model.config, "multilingual", False):
            kw["languages"] = torch.tensor([model.lang2id[x] for x in lang])
        if _has_style_tokens(model):
            kw["style_mel"], kw["style_lens"] = ref, ref_lens
        _, post, _, _, _, syn_lens = model(ids, lens, duration_control=duration_control, **kw)
        syn_lens = syn_lens.cpu()
        dev = post.device
        # the warping, over the rows inside the kernel's limits
        max_ta = ops.dtw_plan(n_cepstra, 1)[0]
        notes = [f"more than 1024 recorded frames ({int(ref_lens[j])}): not warped" if int(ref_lens[j]) > 1024 else
                 f"more than {max_ta} synthesized frames ({int(syn_lens[j])}): not warped" if int(syn_lens[j]) > max_ta else None for j in range(len(chunk))]
        ok = [j for j in range(len(chunk)) if notes[j] is None]
        warped = {}
        if ok:
            sel = torch.tensor(ok)
            a = post[sel.to(dev), : int(syn_lens[sel].max())].contiguous()
            b = ref[sel, : int(ref_lens[sel].max())].contiguous().to(dev)
            got = mel_cepstral_distortion(a, syn_lens[sel], b, ref_lens[sel], n_cepstra)
            mcd, steps, lo, hi, frame_mcd = (t.cpu() for t in got)
            warped = {j: (float(mcd[row]), int(steps[row]), lo[row, : int(ref_lens[j])].clone(), hi[row, : int(ref_lens[j])].clone(),
                          frame_mcd[row, : int(ref_lens[j])]) for row, j in enumerate(ok)}
        # the recording's durations: the duration/ file, else the model's aligner
        durs = {}
        found = [feature_path(preprocessed_dir, "duration", r["basename"], spk[j], lang[j], "duration.pt") for j, r in enumerate(chunk)]
        for j in range(len(chunk)):
            if found[j].exists():
                durs[j] = torch.load(found[j], weights_only=True)[: lens[j]].long()
        missing = [j for j in range(len(chunk)) if j not in durs]
        if missing and getattr(model, "has_aligner", False):
            sel = torch.tensor(missing)
            akw = {key: kw[key][sel] for key in ("speakers", "languages") if key in kw}
            aligned = model.align(ids[sel], lens[sel], ref[sel, : int(ref_lens[sel].max())].contiguous(), ref_lens[sel], **akw).cpu()
            for row, j in enumerate(missing):
                durs[j] = aligned[row, : lens[j]].long()
        f0 = {}
        if vocoder is not None:
            wav = vocoder(post.transpose(1, 2).contiguous(), lens=syn_lens.to(dev))
            for j in ok:
                recorded = load_wav(wavs[j])[0][:1].to(dev)
                pair = [extract_pitch(x, None, hop_out, out_sr, interpolate=False)[0].cpu().numpy()
                        for x in (wav[j, :1, : int(syn_lens[j]) * hop_out], recorded)]
                f0[j] = f0_agreement(pair[0], pair[1], warped[j][3].numpy())
        for j, r in enumerate(chunk):
            n, f_ref, f_syn = int(lens[j]), int(ref_lens[j]), int(syn_lens[j])
            rec = {"basename": r["basename"], "speaker": spk[j], "language": lang[j], "symbols": n, "frames_ref": f_ref, "frames_syn": f_syn,
                   "length_ratio": f_syn / f_ref, "mcd_dtw": nan, "mcd_dtw_sl": nan, "path_steps": 0, "off_diagonal": nan, "worst_symbol": None,
                   "worst_symbol_mcd": None, "f0_rmse_cents": None, "vuv_error": None, "voiced_pairs": None, "lo": None, "hi": None}
            if vocoder is not None:
                rec["f0_rmse_cents"], rec["vuv_error"], rec["voiced_pairs"] = f0.get(j, (nan, nan, 0))
            if notes[j] is not None:
                rec["note"] = notes[j]
            else:
                mcd_j, steps_j, lo_j, hi_j, frame_j = warped[j]
                diagonal = int((lo_j[1:] == hi_j[:-1] + 1).sum())
                rec.update({"mcd_dtw": mcd_j, "mcd_dtw_sl": mcd_j * max(f_ref, f_syn) / max(min(f_ref, f_syn), 1), "path_steps": steps_j,
                            "off_diagonal": 1.0 - diagonal / (steps_j - 1) if steps_j > 1 else 0.0, "lo": lo_j, "hi": hi_j})
                if j in durs:
                    ends = torch.cumsum(durs[j], 0).clamp(max=f_ref)
                    starts = torch.cat([torch.zeros(1, dtype=ends.dtype), ends[:-1]])
                    scores = [(float(frame_j[int(s) : int(e)].mean()), x) for x, (s, e) in enumerate(zip(starts, ends)) if e > s]
                    if scores:
                        rec["worst_symbol_mcd"], rec["worst_symbol"] = max(scores, key=lambda t: (t[0], -t[1]))
            records.append(rec)
    if out_path is not None:
        GpuPreprocessor.write_filelist(records, out_path, fields=SYNTHESIS_EVALUATION_FIELDS)
    return records


# ---- a vocoder against the recordings ------------------------------------------------------------------------
STOI_SAMPLE_RATE = 10000  # the rate the measure is defined at
STOI_HOP = 128            # samples between its frames at that rate


class Stoi(NamedTuple):
    """``stoi``'s results, on the device: stoi [B] (NaN without a segment), frames / active / segments [B] int32 (the frames of the
    common length, those within 40 dB of the recording's loudest, and the 384 ms segments scored), segment_stoi [B, J_cap] (the mean
    over the 15 bands of each segment; 0 beyond the item's), frame_of [B, F_cap] int32 (the original frame of each active frame: segment
    s starts at sample 128 frame_of[s] of the 10 kHz signal; -1 beyond the item's)."""

    stoi: torch.Tensor
    frames: torch.Tensor
    active: torch.Tensor
    segments: torch.Tensor
    segment_stoi: torch.Tensor
    frame_of: torch.Tensor


def third_octave_bands() -> list[tuple[int, int]]:
    """The 15 one-third-octave bands of STOI as (first bin, one past the last bin) of a 512-point transform at 10 kHz: centres
    150 x 2^(b/3) Hz, edges x 2^(-1/6) and x 2^(1/6), each snapped to the nearest of the 257 bins of linspace(0, 10000, 513); float64."""
    f = np.linspace(0.0, float(STOI_SAMPLE_RATE), 513)[:257]
    centres = 150.0 * 2.0 ** (np.arange(15, dtype=np.float64) / 3.0)
    lo, hi = centres * 2.0 ** (-1.0 / 6.0), centres * 2.0 ** (1.0 / 6.0)
    return [(int(np.argmin(np.abs(f - a))), int(np.argmin(np.abs(f - b)))) for a, b in zip(lo, hi)]


def _rows_at_10k(wav: torch.Tensor, lens: torch.Tensor, sample_rate: int):
    """[B, S] and lengths at ``sample_rate`` -> the same at 10 kHz: samples at or beyond an item's length zeroed, ``resample``, its length rule."""
    if sample_rate == STOI_SAMPLE_RATE:
        return wav.contiguous(), lens
    g = math.gcd(sample_rate, STOI_SAMPLE_RATE)
    orig, new = sample_rate // g, STOI_SAMPLE_RATE // g
    inside = torch.arange(wav.shape[1], device=wav.device)[None, :] < lens[:, None]
    return resample(torch.where(inside, wav, torch.zeros((), device=wav.device)), sample_rate, STOI_SAMPLE_RATE), (new * lens + orig - 1) // orig


def stoi(ref_wav: torch.Tensor, ref_lens, deg_wav: torch.Tensor, deg_lens, sample_rate: int) -> Stoi:
    """Short-time objective intelligibility (intrusive STOI: Taal, Hendriks, Heusdens, Jensen 2011, with the frame conventions of the
    widely used open implementation) of ``deg_wav`` (a synthesis) against ``ref_wav`` (its recording): [B, S] or [B, 1, S] on the GPU
    with their sample counts, one launch (``evmi_stoi_f32``), each item over its own min(length) samples, at most
    ``ops.stoi_plan``'s limit (11 s and more) in the shorter padded row.

    The measure is defined at 10 kHz.  At any other ``sample_rate`` both sides go through ``resample`` first (samples at or beyond an
    item's length zeroed, so an item's value does not depend on its batch; lengths by ``resample``'s own rule).  Absolute values
    therefore depend on this project's resampler in the fifth or sixth digit: they compare with the literature, not to the bit with a
    tool that resamples otherwise."""
    from .train import ops

    r = ref_wav[:, 0] if ref_wav.dim() == 3 and ref_wav.shape[1] == 1 else ref_wav
    d = deg_wav[:, 0] if deg_wav.dim() == 3 and deg_wav.shape[1] == 1 else deg_wav
    lr, ld = torch.as_tensor(ref_lens), torch.as_tensor(deg_lens)
    if r.dim() != 2 or d.dim() != 2 or r.shape[0] != d.shape[0] or tuple(lr.shape) != (r.shape[0],) or tuple(ld.shape) != (r.shape[0],):
        raise ValueError(f"stoi: expected [B, S] or [B, 1, S] waveforms with [B] lengths, got {tuple(ref_wav.shape)} / {tuple(lr.shape)} and "
                         f"{tuple(deg_wav.shape)} / {tuple(ld.shape)}")
    if int(sample_rate) != sample_rate or sample_rate <= 0:
        raise ValueError(f"stoi: sample_rate must be a positive integer, got {sample_rate!r}")
    if not r.is_cuda:
        raise RuntimeError("everyvoice_amd.pipeline.stoi computes on the GPU only (no CPU fallback)")
    dev = r.device
    r, d = r.to(torch.float32), d.to(dev, torch.float32)
    lr, ld = lr.to(dev, torch.int64).clamp(0, r.shape[1]), ld.to(dev, torch.int64).clamp(0, d.shape[1])
    r, lr = _rows_at_10k(r, lr, int(sample_rate))
    d, ld = _rows_at_10k(d, ld, int(sample_rate))
    value, counts, segment, frame_of = ops.stoi(r, lr.to(torch.int32).contiguous(), d, ld.to(torch.int32).contiguous())
    return Stoi(value, counts[:, 0], counts[:, 1], counts[:, 2], segment, frame_of)


VOCODER_EVALUATION_FIELDS = ("basename", "speaker", "language", "frames", "samples", "seconds", "mel_error", "stoi", "stoi_active", "stoi_segments",
                             "stoi_worst", "stoi_worst_at", "f0_rmse_cents", "vuv_error", "voiced_pairs", "note")


def _output_log_mel(cfg: AudioConfig):
    """The log-spectrogram ``validation/mel_spec_error`` is measured with: ``spectral.vocoder_output_transform`` of ``cfg``, [B, S] -> log."""
    from .spectral import vocoder_output_transform

    t = vocoder_output_transform(cfg)
    fn = get_spectral_transform(t["spec_type"], t["n_fft"], t["win_length"], t["hop_length"], t["filter_sample_rate"], t["n_mels"], t["f_min"], t["f_max"])
    if t["spec_type"] == "mel":  # the torchaudio mel comes out linear: log(clamp(., 1e-5)) as the preprocessor applies it
        from .train import ops

        return lambda x: ops.elementwise(ops.EW_LOG_CLAMP, fn(x).contiguous(), p0=1e-5)
    return lambda x: fn(x, log=True)


def evaluate_vocoder(vocoder, filelist_data: list[dict], preprocessed_dir, batch_size: int = 16, audio_config: AudioConfig | None = None,
                     out_path=None) -> list[dict]:
    """How close a vocoder's copy-synthesis is to the recording, per utterance of a preprocessed dataset: the
    copy-synthesis twin of ``evaluate_synthesis``.  Every row's ``spec/...--spec-<input_sr>-<spec_type>.pt`` is vocoded in ragged
    batches (``vocoder(mel, lens=)``) and compared with ``audio/...--audio-<output_sr>.wav`` on the first ``samples`` = min(synthesized,
    recorded) samples of both.  One record per row, in input order:
    ``basename``, ``speaker``, ``language``, ``frames`` (of the spectrogram), ``samples``, ``seconds`` (samples / output_sr),
    ``mel_error`` (the definition of ``validation/mel_spec_error``: the mean absolute difference of the log-spectrograms of both
    signals through ``spectral.vocoder_output_transform``, per item on its own samples),
    ``stoi`` (``stoi`` above, resampled to 10 kHz), ``stoi_active`` (active / all frames), ``stoi_segments``, ``stoi_worst`` /
    ``stoi_worst_at`` (the lowest segment value and the time in seconds, in the recording, where that segment starts:
    frame_of[s] x 128 / 10000),
    ``f0_rmse_cents``, ``vuv_error``, ``voiced_pairs`` (``f0_agreement`` of ``extract_pitch(interpolate=False)`` of both at the output
    rate and hop, paired frame by frame).
    An utterance beyond ``ops.stoi_plan``'s limit, or without a segment (fewer than 31 active frames: under about 0.4 s), gets NaN in
    the STOI fields and a ``note``, not an exception.  A record does not depend on ``batch_size`` or on its neighbours.
    ``out_path``: the records as a pipe-separated file with a header line.
    ``FileNotFoundError``: a missing spectrogram or recording, by name, before any device work on its batch."""
    from .train import ops

    cfg = audio_config if audio_config is not None else AudioConfig()
    in_sr, out_sr = cfg.input_sampling_rate, cfg.output_sampling_rate
    hop_out = cfg.fft_hop_size * (out_sr // in_sr)
    spec_fn = f"spec-{in_sr}-{cfg.spec_type}.pt"
    nan = float("nan")
    rows = [dict(r) for r in filelist_data]
    records = []
    log_mel, max_n = None, None
    for start in range(0, len(rows), batch_size):
        chunk = rows[start : start + batch_size]
        spk = [r.get("speaker") or "default" for r in chunk]
        lang = [r.get("language") or "default" for r in chunk]
        specs = [feature_path(preprocessed_dir, "spec", r["basename"], spk[j], lang[j], spec_fn) for j, r in enumerate(chunk)]
        wavs = [feature_path(preprocessed_dir, "audio", r["basename"], spk[j], lang[j], f"audio-{out_sr}.wav") for j, r in enumerate(chunk)]
        for r, p, q in zip(chunk, specs, wavs):
            if not p.exists():
                raise FileNotFoundError(f"evaluate_vocoder {r['basename']!r}: no spectrogram {p} to vocode")
            if not q.exists():
                raise FileNotFoundError(f"evaluate_vocoder {r['basename']!r}: no recording {q} to compare with")
        dev = next(vocoder.parameters()).device
        if log_mel is None:
            log_mel, max_n = _output_log_mel(cfg), ops.stoi_plan(1)[0]
        mels = [torch.load(p, weights_only=True).to(torch.float32) for p in specs]  # [n_mels, T] each
        frames = torch.tensor([m.shape[1] for m in mels])
        mel = torch.nn.utils.rnn.pad_sequence([m.transpose(0, 1) for m in mels], batch_first=True).transpose(1, 2).contiguous().to(dev)
        syn = vocoder(mel, lens=frames.to(dev))[:, 0]
        per_frame = syn.shape[1] // mel.shape[2]
        recorded = [load_wav(q)[0][0] for q in wavs]
        samples = [min(int(frames[j]) * per_frame, recorded[j].shape[0]) for j in range(len(chunk))]
        ref = torch.nn.utils.rnn.pad_sequence([x[:n] for x, n in zip(recorded, samples)], batch_first=True).to(dev)
        g = math.gcd(out_sr, STOI_SAMPLE_RATE)
        at_10k = [(STOI_SAMPLE_RATE // g * n + out_sr // g - 1) // (out_sr // g) for n in samples]
        notes = [f"more than {max_n} samples at 10 kHz ({at_10k[j]}): no STOI" if at_10k[j] > max_n else "no samples" if samples[j] == 0 else None
                 for j in range(len(chunk))]
        ok = [j for j in range(len(chunk)) if notes[j] is None]
        scored = {}
        if ok:
            sel, lens = torch.tensor(ok, device=dev), torch.tensor([samples[j] for j in ok])
            S = max(int(lens.max()), 1)
            got = stoi(ref[sel, :S], lens, syn[sel, :S], lens, out_sr)
            value, n_frames, active, segments, segment_stoi, frame_of = (t.cpu() for t in got)
            scored = {j: (float(value[row]), int(n_frames[row]), int(active[row]), int(segments[row]), segment_stoi[row], frame_of[row])
                      for row, j in enumerate(ok)}
        for j, r in enumerate(chunk):
            n = samples[j]
            rec = {"basename": r["basename"], "speaker": spk[j], "language": lang[j], "frames": int(frames[j]), "samples": n, "seconds": n / out_sr,
                   "mel_error": nan, "stoi": nan, "stoi_active": nan, "stoi_segments": 0, "stoi_worst": nan, "stoi_worst_at": nan,
                   "f0_rmse_cents": nan, "vuv_error": nan, "voiced_pairs": 0}
            if n > 0:
                a, b = syn[j : j + 1, :n].contiguous(), ref[j : j + 1, :n].contiguous()
                rec["mel_error"] = float((log_mel(a) - log_mel(b)).abs().mean())
                f0_syn, f0_ref = (extract_pitch(x, None, hop_out, out_sr, interpolate=False)[0].cpu().numpy() for x in (a, b))
                rec["f0_rmse_cents"], rec["vuv_error"], rec["voiced_pairs"] = f0_agreement(f0_syn, f0_ref, np.arange(len(f0_ref)))
            if j in scored:
                value, n_frames, active, segments, segment_stoi, frame_of = scored[j]
                rec.update({"stoi": value, "stoi_active": active / n_frames if n_frames else nan, "stoi_segments": segments})
                if segments > 0:
                    worst = int(torch.argmin(segment_stoi[:segments]))
                    rec.update({"stoi_worst": float(segment_stoi[worst]), "stoi_worst_at": int(frame_of[worst]) * STOI_HOP / STOI_SAMPLE_RATE})
                else:
                    notes[j] = f"fewer than 31 active frames ({active} of {n_frames}): no STOI segment"
            if notes[j] is not None:
                rec["note"] = notes[j]
            records.append(rec)
    if out_path is not None:
        GpuPreprocessor.write_filelist(records, out_path, fields=VOCODER_EVALUATION_FIELDS)
    return records
