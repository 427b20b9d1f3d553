"""The mel front end's host side for any AudioConfig: construction without a device, the planner's geometry
(evmi_mel_spectrogram_plan), the refusals of evmi_mel_spectrogram_win_f32 and how they surface from MelSpectrogram and
GpuPreprocessor.  No GPU is needed: the pointers handed over are host memory and are never dereferenced -- a refusal that came
after a HIP call would end in EVMI_ERR_HIP on a machine without a device."""

import ctypes as C

import numpy as np
import pytest
import torch

from everyvoice_amd import _lib, pipeline
from everyvoice_amd.config import AudioConfig
from everyvoice_amd.spectral import MelSpectrogram, get_spectral_transform, mel_frontend_plan, windowed_dft_basis

EVMI_ERR_INVALID_ARG = 1
EVMI_ERR_UNSUPPORTED = 4

# (sr, n_fft, win, hop, n_mels, f_max): the configurations tests/test_gpu_mel_configs.py runs on the device
CONFIGS = [
    (16000, 1024, 800, 200, 80, 8000),
    (24000, 2048, 1200, 300, 100, 12000),
    (22050, 1024, 1024, 275, 80, 8000),
    (16000, 512, 400, 160, 80, 8000),
    (22050, 64, 50, 13, 16, 8000),
    (22050, 64, 32, 48, 16, 8000),
    (22050, 64, 64, 64, 16, 8000),
    (22050, 64, 64, 1, 16, 8000),
    (22050, 1024, 1024, 256, 80, 8000),
]
_ID = lambda c: "-".join(str(v) for v in c)  # noqa: E731


@pytest.mark.parametrize("args", [(1024, 800, 200, 16000), (2048, 1200, 300, 24000, 100, 0, 12000), (1024, 1024, 275)], ids=str)
def test_constructs_without_a_device(args):
    tr = MelSpectrogram(*args)
    assert (tr.n_fft, tr.win, tr.hop) == args[:3]
    assert tr._dev == {}  # (nothing was uploaded: construction is host-only)
    assert tr._basis_host.shape == (args[0], 2 * tr.nb_pad)
    assert isinstance(get_spectral_transform("mel-librosa", 1024, 800, 200, 16000, 80, 0, 8000), MelSpectrogram)
    pre = pipeline.GpuPreprocessor(AudioConfig(input_sampling_rate=16000, output_sampling_rate=16000, n_fft=1024, fft_window_size=800,
                                               fft_hop_size=200), device="cpu")
    assert pre.transform.win == 800 and pre.output_transform is None


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_planner_geometry(cfg):
    _, n_fft, win, hop, n_mels, _ = cfg
    p = mel_frontend_plan(n_fft, win, hop, n_mels)
    k0, k1 = p["k0"], p["k1"]
    left = (n_fft - win) // 2
    assert k0 % 2 == 0 and k1 % 2 == 0 and 0 <= k0 < k1 <= n_fft
    rows = np.nonzero(np.abs(windowed_dft_basis(n_fft, win)[0]).max(axis=1))[0]
    assert k0 <= rows.min() and rows.max() < k1  # every non-zero basis row is walked
    assert k0 >= left - 1 and k1 <= left + win + 1  # ... and at most one zero row on either side
    assert p["frame_stride_words"] % 2 == 1 and p["frame_stride_words"] in (hop, hop + 1)
    assert 0 < p["lds_bytes"] <= 160 * 1024
    assert p["chunk_tiles"] >= 1
    if win == n_fft:
        assert (k0, k1) == (0, n_fft)


def test_planner_outputs_are_optional_and_chunks_at_2048():
    lib = _lib.load()
    assert lib.evmi_mel_spectrogram_plan(1024, 1024, 256, 80, None, None, None, None, None) == _lib.EVMI_OK
    n_tiles = (2048 // 2 + 1 + 15) // 16  # 16-bin tiles of 1025 bins
    assert mel_frontend_plan(2048, 2048, 512, 80)["chunk_tiles"] < n_tiles  # (the magnitude tile does not fit beside the audio)
    assert mel_frontend_plan(1024, 1024, 256, 80)["chunk_tiles"] == (1024 // 2 + 1 + 15) // 16


_BUF = torch.zeros(64)  # host memory standing in for every device pointer
P = _BUF.data_ptr()


def _win(audio=P, lens=0, basis=P, melb=P, mel=P, B=1, S=4096, n_fft=1024, win=1024, hop=256, nb_pad=528, n_mels=80):
    return (audio, lens, basis, melb, mel, 0, 0, B, S, n_fft, win, hop, nb_pad, n_mels, 1, None)


REFUSALS = {
    "win_length_0": (_win(win=0), EVMI_ERR_INVALID_ARG),
    "win_length_above_n_fft": (_win(win=1025), EVMI_ERR_INVALID_ARG),
    "hop_0": (_win(hop=0), EVMI_ERR_INVALID_ARG),
    "hop_above_n_fft": (_win(hop=1025), EVMI_ERR_INVALID_ARG),
    "odd_n_fft": (_win(n_fft=1023, win=1023, nb_pad=512), EVMI_ERR_UNSUPPORTED),
    "n_samples_is_half_n_fft": (_win(S=512), EVMI_ERR_INVALID_ARG),
    "n_mels_129": (_win(n_mels=129), EVMI_ERR_UNSUPPORTED),
    "tile_beyond_the_lds_budget": (_win(S=65536, n_fft=8192, win=8192, hop=2048, nb_pad=4112), EVMI_ERR_UNSUPPORTED),
    "null_audio": (_win(audio=0), EVMI_ERR_INVALID_ARG),
    "null_basis": (_win(basis=0), EVMI_ERR_INVALID_ARG),
    "null_mel_basis": (_win(melb=0), EVMI_ERR_INVALID_ARG),
    "null_output": (_win(mel=0), EVMI_ERR_INVALID_ARG),
}


@pytest.mark.parametrize("case", list(REFUSALS), ids=list(REFUSALS))
def test_refused_on_the_host_with_the_documented_code(case):
    args, code = REFUSALS[case]
    lib = _lib.load()
    rc = lib.evmi_mel_spectrogram_win_f32(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == code, f"returned {rc} ({msg!r}), wanted {code}"
    assert "mel_spectrogram_win" in msg, msg
    assert torch.count_nonzero(_BUF) == 0  # (nothing was written through the stand-in pointer)
    if not case.startswith(("null", "n_samples")):  # the planner gives the same refusal for the same sizes
        ints = [C.c_int() for _ in range(4)]
        rc = lib.evmi_mel_spectrogram_plan(args[9], args[10], args[11], args[13], *[C.byref(v) for v in ints], None)
        assert rc == code and "mel_spectrogram_plan" in (lib.evmi_last_error() or b"").decode()


def test_the_earlier_entry_points_forward_with_the_full_window():
    """evmi_mel_spectrogram_f32 / _ragged_f32 keep their signatures and their refusals, each under its own name."""
    lib = _lib.load()
    assert lib.evmi_mel_spectrogram_f32(P, P, P, P, 0, 0, 1, 512, 1024, 256, 528, 80, 1, None) == EVMI_ERR_INVALID_ARG
    assert b"mel_spectrogram:" in lib.evmi_last_error()
    assert lib.evmi_mel_spectrogram_ragged_f32(P, P, P, P, P, 0, 0, 1, 4096, 1024, 256, 528, 129, 1, None) == EVMI_ERR_UNSUPPORTED
    assert b"mel_spectrogram_ragged:" in lib.evmi_last_error()
    assert lib.evmi_mel_spectrogram_ragged_f32(P, 0, P, P, P, 0, 0, 1, 4096, 1024, 256, 528, 80, 1, None) == EVMI_ERR_INVALID_ARG
    assert lib.evmi_abi_version() == 2


@pytest.mark.parametrize("kwargs,field", [
    (dict(win_length=0), "fft_window_size"),
    (dict(win_length=1025), "fft_window_size"),
    (dict(hop_length=0), "fft_hop_size"),
    (dict(hop_length=1025), "fft_hop_size"),
    (dict(n_fft=1023, win_length=1023), "n_fft"),
    (dict(n_mels=129), "n_mels"),
    (dict(n_fft=8192, win_length=8192, hop_length=2048), "n_fft"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else v)
def test_constructor_names_the_audio_config_field(kwargs, field):
    with pytest.raises(ValueError, match=rf"AudioConfig\.{field}\b"):
        MelSpectrogram(**kwargs)


def test_preprocessor_refuses_a_non_integer_rate_ratio():
    with pytest.raises(ValueError, match="output_sampling_rate.*input_sampling_rate"):
        pipeline.GpuPreprocessor(AudioConfig(input_sampling_rate=22050, output_sampling_rate=48000), device="cpu")
    with pytest.raises(ValueError, match="output_sampling_rate.*input_sampling_rate"):
        pipeline.GpuPreprocessor(AudioConfig(input_sampling_rate=22050, output_sampling_rate=11025), device="cpu")
    with pytest.raises(ValueError, match=r"AudioConfig\.fft_window_size"):  # the transform's refusal surfaces at construction too
        pipeline.GpuPreprocessor(AudioConfig(fft_window_size=2048), device="cpu")
    pre = pipeline.GpuPreprocessor(AudioConfig(input_sampling_rate=22050, output_sampling_rate=44100), device="cpu")
    assert pre.rate_change == 2
    assert (pre.output_transform.n_fft, pre.output_transform.win, pre.output_transform.hop) == (2048, 2048, 512)
    # the reference hands the output transform the INPUT rate (preprocessor.py:112-121): its filterbank is the 22050 Hz one
    want = MelSpectrogram(2048, 2048, 512, 22050)._mel_host
    assert torch.equal(pre.output_transform._mel_host, want)
