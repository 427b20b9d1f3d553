"""Host side of the length-masked Global Style Token module: the per-layer lengths, the configuration field, the
``style_lens`` refusals, the batched style-reference front end and the argument refusals of the new entry points.  No GPU is needed."""

import json
import math
from dataclasses import asdict

import pytest
import torch

from everyvoice_amd import _lib
from everyvoice_amd.fs2 import FastSpeech2ModelConfig, check_style_lens
from everyvoice_amd.lightning import FastSpeech2Config, _dataclass_from_dict, parse_config_args

EVMI_ERR_INVALID_ARG = 1
_BUF = torch.zeros(64)  # host memory standing in for every device pointer: a refusal comes before anything is dereferenced
P = _BUF.data_ptr()


@pytest.mark.parametrize("n", [1, 2, 17, 566, 947])
def test_valid_rows_are_the_iterated_output_length(n):
    from everyvoice_amd.train import ops

    lens = torch.tensor([n, 1, max(1, n - 1)], dtype=torch.int32)
    got = ops.gst_valid_rows(lens, 6)
    assert len(got) == 6
    want = [int(v) for v in lens]
    for layer in got:
        want = [(v - 1) // 2 + 1 for v in want]
        assert layer.dtype == torch.int32 and layer.shape == lens.shape and layer.is_contiguous()
        assert layer.tolist() == want
    # ... and what the masked restatement of the tests uses
    from gst_masked_ref import valid_rows

    assert [v.tolist() for v in valid_rows(lens.long(), 6)] == [v.tolist() for v in got]
    assert torch.equal(lens, torch.tensor([n, 1, max(1, n - 1)], dtype=torch.int32))  # the argument is left alone


def test_mask_padding_field_defaults_to_false_and_round_trips():
    assert FastSpeech2ModelConfig().gst_mask_padding is False
    cfg = FastSpeech2Config(model={"use_global_style_token_module": True, "gst_mask_padding": True})
    assert cfg.model.gst_mask_padding is True
    cfg = FastSpeech2Config()
    assert cfg.model.gst_mask_padding is False
    cfg.update_config(parse_config_args(["model.gst_mask_padding=true"]))
    assert cfg.model.gst_mask_padding is True
    dumped = json.loads(json.dumps(cfg.model_checkpoint_dump()["model"]))
    assert dumped["gst_mask_padding"] is True
    again = _dataclass_from_dict(FastSpeech2ModelConfig, dumped)
    assert again.gst_mask_padding is True and (again.gst_num_heads, again.gst_num_tokens) == (8, 10)
    plain = asdict(FastSpeech2ModelConfig())
    assert plain["gst_mask_padding"] is False
    fields = list(plain)
    assert fields.index("gst_mask_padding") == fields.index("gst_num_heads") + 1
    # a checkpoint written before the field existed still loads: the default fills in
    plain.pop("gst_mask_padding")
    assert _dataclass_from_dict(FastSpeech2ModelConfig, json.loads(json.dumps(plain))).gst_mask_padding is False


def test_style_lens_refusals():
    shape = (3, 40, 80)
    assert check_style_lens(None, shape) is None and check_style_lens(None, None) is None
    ok = check_style_lens(torch.tensor([1, 40, 17]), shape)
    assert ok.tolist() == [1, 40, 17]
    assert check_style_lens([40, 40, 2], shape).tolist() == [40, 40, 2]  # a list is taken as well
    assert check_style_lens(torch.tensor([40], dtype=torch.int32), (1, 40, 80)).tolist() == [40]
    for bad in (torch.tensor([0, 40, 17]), torch.tensor([1, 41, 17]), torch.tensor([-3, 2, 2]),  # below 1, above Ts
                torch.tensor([40, 40]), torch.tensor([[40, 40, 40]]), torch.tensor(40),             # wrong shape
                torch.tensor([40.0, 3.0, 2.0]), torch.tensor([True, True, False])):                 # not integers
        with pytest.raises(ValueError, match="style_lens"):
            check_style_lens(bad, shape)
    with pytest.raises(ValueError, match="style_lens.*without `style_mel`"):
        check_style_lens(torch.tensor([3]), None)
    # one reference for the whole batch takes one length
    with pytest.raises(ValueError, match="style_lens"):
        check_style_lens(torch.tensor([40, 40, 40]), (1, 40, 80))


def test_model_refuses_style_lens_before_any_device_work():
    """``FastSpeech2.__call__`` runs the check first: without ``style_mel`` the refusal names ``style_lens`` (no GPU is touched: the
    model object is never built past its configuration)."""
    from everyvoice_amd.fs2 import FastSpeech2

    model = FastSpeech2.__new__(FastSpeech2)
    model._ready = True
    with pytest.raises(ValueError, match="style_lens"):
        model(torch.zeros(1, 3, dtype=torch.long), torch.tensor([3]), style_lens=torch.tensor([5]))
    with pytest.raises(ValueError, match="style_lens"):
        model(torch.zeros(1, 3, dtype=torch.long), torch.tensor([3]), style_mel=torch.zeros(1, 9, 80), style_lens=torch.tensor([10]))


def test_style_reference_batch_pads_and_reports_the_lengths(tmp_path):
    from everyvoice_amd import pipeline
    from everyvoice_amd.config import AudioConfig

    for bad in ([], "a.wav", tmp_path / "a.wav", torch.zeros(100)):
        with pytest.raises(ValueError, match="style_reference_batch"):
            pipeline.style_reference_batch(bad, AudioConfig(), "cpu")
    with pytest.raises(ValueError, match="1-D waveform"):
        pipeline.style_reference_batch([torch.zeros(2, 100)], AudioConfig(), "cpu")
    t = torch.arange(22050, dtype=torch.float32) / 22050.0
    long_ = 0.5 * torch.sin(2 * math.pi * 220.0 * t)
    short = 0.4 * torch.sin(2 * math.pi * 440.0 * t[:9000])
    try:
        alone = [pipeline.style_reference_mel(w, AudioConfig(), "cpu") for w in (long_, short)]
    except RuntimeError as e:  # the mel front end computes on the GPU only: the argument checks above are what runs without one
        assert "GPU only" in str(e), e  # (the padding itself is checked on the device: tests/test_gpu_gst_masked.py)
        return
    pipeline.save_wav(short, tmp_path / "short.wav", 22050)
    mel, lens = pipeline.style_reference_batch([long_, tmp_path / "short.wav"], AudioConfig(), "cpu")
    assert lens.dtype == torch.int32 and lens.tolist() == [alone[0].shape[1], alone[1].shape[1]] == [22050 // 256, 9000 // 256]
    assert mel.shape == (2, 22050 // 256, 80)
    assert torch.equal(mel[0], alone[0][0])
    n = int(lens[1])
    assert float((mel[1, :n] - alone[1][0]).abs().max()) < 1e-3  # (the wav file is 16-bit PCM)
    assert not mel[1, n:].any()


# (entry point, arguments): one refused call each; P is a valid non-null pointer, 0 is NULL
CASES = [
    ("evmi_gst_conv2d_fwd_rows_f32", (P, P, P, P, 0, 1, 32, 3, 17, 80, 0, None)),      # no lengths
    ("evmi_gst_conv2d_fwd_rows_f32", (0, P, P, P, P, 1, 32, 3, 17, 80, 0, None)),
    ("evmi_gst_conv2d_fwd_rows_f32", (P, 0, P, P, P, 1, 32, 3, 17, 80, 0, None)),
    ("evmi_gst_conv2d_fwd_rows_f32", (P, P, P, 0, P, 1, 32, 3, 17, 80, 0, None)),
    ("evmi_gst_conv2d_fwd_rows_f32", (P, P, P, P, P, 1, 32, 0, 17, 80, 0, None)),      # B < 1
    ("evmi_gst_conv2d_fwd_rows_f32", (P, P, P, P, P, 1, 32, 3, 0, 80, 0, None)),
    ("evmi_gst_conv2d_fwd_rows_f32", (P, P, P, P, P, 0, 32, 3, 17, 80, 0, None)),
    ("evmi_gst_conv2d_fwd_rows_f32", (P, P, P, P, P, 1, 32, 3, 17, 80, 2, None)),      # act: 0 or 3
    ("evmi_batchnorm_fwd_valid_cbt_f32", (P, P, P, P, P, P, P, P, 32, 72, 1e-5, 0.1, 3, 0, 3, 24, None)),   # no lengths
    ("evmi_batchnorm_fwd_valid_cbt_f32", (0, P, P, P, P, P, P, P, 32, 72, 1e-5, 0.1, 3, P, 3, 24, None)),
    ("evmi_batchnorm_fwd_valid_cbt_f32", (P, P, P, P, P, P, P, 0, 32, 72, 1e-5, 0.1, 3, P, 3, 24, None)),   # one running statistic only
    ("evmi_batchnorm_fwd_valid_cbt_f32", (P, P, P, P, P, P, 0, 0, 32, 72, 1e-5, -1.0, 3, P, 3, 24, None)),  # evaluation without them
    ("evmi_batchnorm_fwd_valid_cbt_f32", (P, P, P, P, P, P, P, P, 0, 72, 1e-5, 0.1, 3, P, 3, 24, None)),
    ("evmi_batchnorm_fwd_valid_cbt_f32", (P, P, P, P, P, P, P, P, 32, 72, 1e-5, 0.1, 3, P, 0, 24, None)),   # B < 1
    ("evmi_batchnorm_fwd_valid_cbt_f32", (P, P, P, P, P, P, P, P, 32, 72, 1e-5, 0.1, 3, P, 3, 0, None)),
    ("evmi_batchnorm_fwd_valid_cbt_f32", (P, P, P, P, P, P, P, P, 32, 71, 1e-5, 0.1, 3, P, 3, 24, None)),   # n_cols != B T
    ("evmi_batchnorm_fwd_valid_cbt_f32", (P, P, P, P, P, P, P, P, 32, 72, 1e-5, 0.1, 1, P, 3, 24, None)),   # act
    ("evmi_batchnorm_bwd_valid_cbt_f32", (P, P, P, P, P, P, P, P, P, 32, 72, 3, 0, 3, 24, None)),
    ("evmi_batchnorm_bwd_valid_cbt_f32", (P, P, P, P, P, 0, P, P, P, 32, 72, 3, P, 3, 24, None)),
    ("evmi_batchnorm_bwd_valid_cbt_f32", (P, P, P, P, P, P, P, P, P, 0, 72, 3, P, 3, 24, None)),
    ("evmi_batchnorm_bwd_valid_cbt_f32", (P, P, P, P, P, P, P, P, P, 32, 72, 3, P, 0, 24, None)),
    ("evmi_batchnorm_bwd_valid_cbt_f32", (P, P, P, P, P, P, P, P, P, 32, 70, 3, P, 3, 24, None)),
    ("evmi_batchnorm_bwd_valid_cbt_f32", (P, P, P, P, P, P, P, P, P, 32, 72, 5, P, 3, 24, None)),
    ("evmi_gst_gru_fwd_steps_f32", (P, P, P, P, P, P, P, 0, 3, 15, 32, None)),         # no step counts
    ("evmi_gst_gru_fwd_steps_f32", (0, P, P, P, P, P, P, P, 3, 15, 32, None)),
    ("evmi_gst_gru_fwd_steps_f32", (P, P, P, P, P, P, 0, P, 3, 15, 32, None)),
    ("evmi_gst_gru_fwd_steps_f32", (P, P, P, P, 0, P, P, P, 3, 15, 32, None)),         # the saved tensors go together
    ("evmi_gst_gru_fwd_steps_f32", (P, P, P, P, P, P, P, P, 0, 15, 32, None)),
    ("evmi_gst_gru_fwd_steps_f32", (P, P, P, P, P, P, P, P, 3, 0, 32, None)),
    ("evmi_gst_gru_bwd_steps_f32", (P, P, P, P, P, P, P, 0, 3, 15, 32, None)),
    ("evmi_gst_gru_bwd_steps_f32", (P, P, 0, P, P, P, P, P, 3, 15, 32, None)),
    ("evmi_gst_gru_bwd_steps_f32", (P, P, P, P, P, P, P, P, 0, 15, 32, None)),
    ("evmi_gst_gru_bwd_steps_f32", (P, P, P, P, P, P, P, P, 3, 0, 32, None)),
]


@pytest.mark.parametrize("name,args", CASES)
def test_new_entry_points_refuse_bad_arguments_on_the_host(name, args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == EVMI_ERR_INVALID_ARG, f"{name}{args}: returned {rc} ({msg!r})"
    stem = name[len("evmi_"):].rsplit("_f32", 1)[0].replace("_cbt", "")
    assert stem in msg, f"{name}: evmi_last_error() = {msg!r} does not name the function ({stem!r})"


def test_hidden_sizes_stay_32_64_128():
    lib = _lib.load()
    for name in ("evmi_gst_gru_fwd_steps_f32", "evmi_gst_gru_bwd_steps_f32"):
        rc = getattr(lib, name)(P, P, P, P, P, P, P, P, 3, 15, 48, None)
        assert rc not in (0, EVMI_ERR_INVALID_ARG) and b"hidden size 32, 64 or 128" in lib.evmi_last_error()
