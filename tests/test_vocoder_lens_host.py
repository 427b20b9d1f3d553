"""Host side of the ragged vocoder batch (no GPU): the refusals of ``vocoder.check_lens``, the error codes of
``evmi_generator_forward_lens`` that are decided before any device work, and the routing of ``mask_vocoder_padding`` in
``pipeline.synthesize_helper``."""

import ctypes as C

import pytest
import torch

from everyvoice_amd import _lib
from everyvoice_amd.config import HiFiGANConfig
from everyvoice_amd.vocoder import Generator, check_lens


def test_check_lens_refusals():
    ok = check_lens(torch.tensor([3, 7, 1]), 3, 7)
    assert ok.dtype == torch.int32 and ok.tolist() == [3, 7, 1]
    assert check_lens([2, 2], 2, 5).tolist() == [2, 2]
    with pytest.raises(ValueError, match="lens"):
        check_lens(torch.tensor([3, 7]), 3, 7)  # wrong shape
    with pytest.raises(ValueError, match="lens"):
        check_lens(torch.tensor([[3, 7, 1]]), 3, 7)
    with pytest.raises(ValueError, match="lens"):
        check_lens(torch.tensor([3.0, 7.0, 1.0]), 3, 7)  # float dtype
    with pytest.raises(ValueError, match="between 1 and T = 7"):
        check_lens(torch.tensor([3, 0, 1]), 3, 7)
    with pytest.raises(ValueError, match="between 1 and T = 7"):
        check_lens(torch.tensor([3, 8, 1]), 3, 7)
    with pytest.raises(ValueError, match="mel_lens"):
        check_lens(torch.tensor([3, 8, 1]), 3, 7, what="mel_lens")


def test_forward_lens_error_codes_before_any_device_work():
    lib = _lib.load()
    g = Generator(HiFiGANConfig())
    g._new_handle(0)  # host-only: the object is created, not finalized
    mel = torch.zeros(1, 80, 4)
    wav = torch.zeros(1, 1, 4 * 256)
    lens = torch.tensor([4], dtype=torch.int32)
    call = lambda lens_ptr, prec, mel_ptr=mel.data_ptr(), wav_ptr=wav.data_ptr(): lib.evmi_generator_forward_lens(  # noqa: E731
        g._handle, mel_ptr, lens_ptr, wav_ptr, 1, 4, prec, None)
    assert call(None, _lib.EVMI_PREC_BF16) == _lib.EVMI_ERR_INVALID_ARG  # null item_frames
    assert call(lens.data_ptr(), _lib.EVMI_PREC_BF16, mel_ptr=None) == _lib.EVMI_ERR_INVALID_ARG
    assert call(lens.data_ptr(), _lib.EVMI_PREC_BF16, wav_ptr=None) == _lib.EVMI_ERR_INVALID_ARG
    assert call(lens.data_ptr(), _lib.EVMI_PREC_F32) == _lib.EVMI_ERR_UNSUPPORTED
    assert b"BF16" in lib.evmi_last_error()
    assert call(lens.data_ptr(), _lib.EVMI_PREC_BF16) == _lib.EVMI_ERR_NOT_READY
    # the uniform entry point keeps its own answers
    assert lib.evmi_generator_forward(g._handle, mel.data_ptr(), wav.data_ptr(), 1, 4, _lib.EVMI_PREC_BF16, None) == _lib.EVMI_ERR_NOT_READY
    recs = (_lib.LaunchRecord * 4)()
    n = C.c_int(0)
    assert lib.evmi_generator_forward_lens_profiled(g._handle, mel.data_ptr(), None, wav.data_ptr(), 1, 4, _lib.EVMI_PREC_BF16, None,
                                                    recs, 4, C.byref(n)) == _lib.EVMI_ERR_INVALID_ARG


class _StubModel:
    """FastSpeech2's call signature on the host: two frames per token."""

    device = torch.device("cpu")
    config = None

    def __call__(self, ids, lens, duration_control=1.0, **kw):
        B, L = ids.shape
        mel_lens = 2 * lens
        post = torch.arange(B * 2 * L * 80, dtype=torch.float32).reshape(B, 2 * L, 80) / 1000.0
        return post, post, torch.full((B, L), 2), None, None, mel_lens


class _StubVocoder:
    def __init__(self):
        self.calls = []

    def __call__(self, mel, **kw):
        self.calls.append(kw)
        return torch.zeros(mel.shape[0], 1, mel.shape[2] * 256)


def test_synthesize_helper_passes_lens_exactly_when_asked(tmp_path):
    from everyvoice_amd.pipeline import synthesize_helper

    texts = [[3, 4, 5, 6], [7, 8]]

    def run(out, **kw):
        voc = _StubVocoder()
        _, _, preds, _ = synthesize_helper(_StubModel(), texts, None, None, 1.0, 0, ["wav"], output_dir=tmp_path / out, vocoder_model=voc, **kw)
        assert [p["frames"] for p in preds] == [8, 4]
        return voc.calls

    assert run("plain") == [{}]
    assert run("off", mask_vocoder_padding=False) == [{}]
    (on,) = run("on", mask_vocoder_padding=True)
    assert list(on) == ["lens"] and on["lens"].tolist() == [8, 4]
