"""Host side of ``model.mask_padding``: the configuration field, the masked restatement of the oracle that the GPU
tests rely on (validated here against the oracle run on each item alone) and the argument refusals of the two new entry points.  No GPU
is needed."""

import json
from dataclasses import asdict, fields

import pytest
import torch

from everyvoice_amd import _lib
from everyvoice_amd.fs2 import FastSpeech2, FastSpeech2ModelConfig, Stats
from everyvoice_amd.lightning import FastSpeech2Config, _dataclass_from_dict, parse_config_args
from fs2_masked_ref import item_differences, masked_padding, oracle_model, ragged_batch, solo
from oracle.fs2_ref import FastSpeech2ConfigRef

EVMI_ERR_INVALID_ARG = 1
_BUF = torch.zeros(64)  # host memory standing in for every device pointer: a refusal comes before anything is dereferenced
P = _BUF.data_ptr()


def test_mask_padding_field_defaults_to_false_and_round_trips():
    assert FastSpeech2ModelConfig().mask_padding is False
    cfg = FastSpeech2Config(model={"mask_padding": True})
    assert cfg.model.mask_padding is True and cfg.model.gst_mask_padding is False  # (the two switches are independent)
    cfg = FastSpeech2Config()
    assert cfg.model.mask_padding is False
    cfg.update_config(parse_config_args(["model.mask_padding=true"]))
    assert cfg.model.mask_padding is True
    dumped = json.loads(json.dumps(cfg.model_checkpoint_dump()["model"]))
    assert dumped["mask_padding"] is True
    again = _dataclass_from_dict(FastSpeech2ModelConfig, dumped)
    assert again.mask_padding is True and again.postnet_layers == 5
    plain = asdict(FastSpeech2ModelConfig())
    assert plain["mask_padding"] is False
    # appended behind the last field there was: every earlier field keeps its place
    names = [f.name for f in fields(FastSpeech2ModelConfig)]
    assert names[-1] == "mask_padding" and names[-2] == "gst_ref_enc_filters" and list(plain) == names
    # a checkpoint written before the field existed still loads: the default fills in
    plain.pop("mask_padding")
    assert _dataclass_from_dict(FastSpeech2ModelConfig, json.loads(json.dumps(plain))).mask_padding is False


def test_checkpoint_hyper_parameters_carry_the_field():
    """``hyper_parameters.config`` holds the field; a checkpoint without it means False (the model object is never built past its
    configuration here: no GPU is touched)."""
    model = FastSpeech2.__new__(FastSpeech2)
    model.config, model.stats, model.lang2id, model.speaker2id = FastSpeech2ModelConfig(mask_padding=True), Stats(), {}, {}
    ck = json.loads(json.dumps(model.to_checkpoint({})))
    assert ck["hyper_parameters"]["config"]["mask_padding"] is True
    c = ck["hyper_parameters"]["config"]
    rest = {k: v for k, v in c.items() if k not in ("encoder", "decoder", "variance_predictors")}  # what from_checkpoint passes on
    assert FastSpeech2ModelConfig(**rest).mask_padding is True
    rest.pop("mask_padding")
    assert FastSpeech2ModelConfig(**rest).mask_padding is False


# ---- the masked restatement against the oracle on each item alone ------------------------------------------------------------------
@pytest.mark.parametrize("name,lens", [("small", [12, 7, 5]), ("default", [40, 23])])
def test_masked_reference_on_a_batch_equals_the_oracle_on_each_item_alone(name, lens):
    """Eval mode.  fp32-rounding equality: both sides are the same torch-CPU arithmetic on the same values, only the shapes of the
    matrix products differ (1e-5 of each tensor's largest entry: 8 Conformer layers of fp32 re-association, two orders below the
    tolerances the GPU tests use).  The oracle itself, unmasked, is off by 1e-2 or more on the short items: the inputs are not vacuous.
    The padded output is zero."""
    ref_cfg = FastSpeech2ConfigRef.small() if name == "small" else FastSpeech2ConfigRef()
    ref = oracle_model(ref_cfg)
    ids, lens, durs = ragged_batch(ref_cfg.n_symbols, lens, seed=11)
    alone = []
    for b in range(len(lens)):
        i, n, kw = solo(ids, lens, b, durations=durs)
        alone.append(ref(i, n, **kw))
    plain = item_differences(ref(ids, lens, durations=durs), alone, lens)
    with masked_padding(ref):
        out = ref(ids, lens, durations=durs)
    masked = item_differences(out, alone, lens)
    print(name, "oracle batch vs solo:", plain, "masked reference vs solo:", masked)
    assert torch.equal(out[5], torch.cat([a[5] for a in alone]))
    for b in range(len(lens)):
        assert max(masked[b]) <= 1e-5, (b, masked[b])
        if b > 0:
            assert min(plain[b]) >= 1e-2, (b, plain[b])
    fpad = torch.arange(out[0].shape[1])[None, :] >= out[5][:, None]
    assert not out[0][fpad].any() and not out[1][fpad].any()
    # the hooks are gone: the oracle is itself again
    again = ref(ids, lens, durations=durs)
    assert all(torch.equal(a, b) for a, b in zip(again, ref(ids, lens, durations=durs))) and item_differences(again, alone, lens) == plain


def test_masked_reference_batchnorm_statistics_ignore_the_padding():
    """Training mode: a BatchNorm's batch statistics run over the valid columns only -- the running mean of the first postnet layer
    after one batch, recomputed by hand from that layer's convolution output over the frames below each item's length."""
    ref_cfg = FastSpeech2ConfigRef.small()
    ref_cfg.encoder.dropout = ref_cfg.decoder.dropout = 0.0
    ref_cfg.duration.dropout = ref_cfg.pitch.dropout = ref_cfg.energy.dropout = 0.0
    ref = oracle_model(ref_cfg).train()
    ids, lens, durs = ragged_batch(ref_cfg.n_symbols, [12, 7, 5], seed=11)
    conv, bn = ref.postnet.convolutions[0]
    old, seen = bn.running_mean.clone(), {}
    handle = conv.register_forward_hook(lambda m, a, out: seen.setdefault("y", out.detach()))
    with masked_padding(ref):
        ref(ids, lens, durations=durs)
    handle.remove()
    assert int(bn.num_batches_tracked) == 1
    y = seen["y"]  # [B, C, T]
    valid = (torch.arange(y.shape[2])[None] < durs.sum(1)[:, None])[:, None, :]
    mean = torch.where(valid, y, torch.zeros(())).sum((0, 2)) / float(durs.sum())
    assert float((bn.running_mean - (0.9 * old + 0.1 * mean)).abs().max()) <= 1e-6
    assert float((bn.running_mean - (0.9 * old + 0.1 * y.mean((0, 2)))).abs().max()) > 1e-4  # ... and not over all of them


# (entry point, arguments): one refused call each; P is a valid non-null pointer, 0 is NULL
CASES = [
    ("evmi_dwconv1d_cbt_lens_f32", (P, P, P, 0, P, 20, 6, 41, 3, 1, 0, None)),      # no lengths
    ("evmi_dwconv1d_cbt_lens_f32", (0, P, P, P, P, 20, 6, 41, 3, 1, 0, None)),
    ("evmi_dwconv1d_cbt_lens_f32", (P, 0, P, P, P, 20, 6, 41, 3, 1, 0, None)),
    ("evmi_dwconv1d_cbt_lens_f32", (P, P, P, P, 0, 20, 6, 41, 3, 1, 0, None)),
    ("evmi_dwconv1d_cbt_lens_f32", (P, P, P, P, P, 0, 6, 41, 3, 1, 0, None)),
    ("evmi_dwconv1d_cbt_lens_f32", (P, P, P, P, P, 20, 0, 41, 3, 1, 0, None)),
    ("evmi_dwconv1d_cbt_lens_f32", (P, P, P, P, P, 20, 6, -1, 3, 1, 0, None)),
    ("evmi_dwconv1d_cbt_lens_f32", (P, P, P, P, P, 20, 6, 41, 0, 1, 0, None)),
    ("evmi_dwconv1d_cbt_lens_f32", (P, P, P, P, P, 20, 6, 41, 3, 1, 3, None)),      # act: 0, 1 or 2
    ("evmi_dwconv1d_cbt_lens_f32", (P, P, P, P, P, 20, 6, 41, 3, 1, -1, None)),
    ("evmi_dwconv1d_bwd_cbt_lens_f32", (P, P, P, 0, P, P, P, P, 1024, 20, 6, 41, 3, 1, None)),  # no lengths
    ("evmi_dwconv1d_bwd_cbt_lens_f32", (0, P, P, P, P, P, P, P, 1024, 20, 6, 41, 3, 1, None)),
    ("evmi_dwconv1d_bwd_cbt_lens_f32", (P, 0, P, P, P, P, P, P, 1024, 20, 6, 41, 3, 1, None)),
    ("evmi_dwconv1d_bwd_cbt_lens_f32", (P, P, 0, P, P, P, P, P, 1024, 20, 6, 41, 3, 1, None)),
    ("evmi_dwconv1d_bwd_cbt_lens_f32", (P, P, P, P, P, P, P, P, 1024, 0, 6, 41, 3, 1, None)),
    ("evmi_dwconv1d_bwd_cbt_lens_f32", (P, P, P, P, P, P, P, P, 1024, 20, 0, 41, 3, 1, None)),
    ("evmi_dwconv1d_bwd_cbt_lens_f32", (P, P, P, P, P, P, P, P, 1024, 20, 6, 0, 3, 1, None)),
    ("evmi_dwconv1d_bwd_cbt_lens_f32", (P, P, P, P, P, P, P, P, 1024, 20, 6, 41, 0, 1, None)),
    ("evmi_dwconv1d_bwd_cbt_lens_f32", (P, P, P, P, P, P, P, P, 1024, 20, 6, 41, 33, 16, None)),  # more than 32 taps
    ("evmi_dwconv1d_bwd_cbt_lens_f32", (P, P, P, P, 0, P, P, 0, 1024, 20, 6, 41, 3, 1, None)),   # dw without its workspace
    ("evmi_dwconv1d_bwd_cbt_lens_f32", (P, P, P, P, 0, P, P, P, 479, 20, 6, 41, 3, 1, None)),    # ... or with too small a one (480 needed)
]


@pytest.mark.parametrize("name,args", CASES)
def test_new_entry_points_refuse_bad_arguments_on_the_host(name, args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == EVMI_ERR_INVALID_ARG, f"{name}{args}: returned {rc} ({msg!r})"
    stem = {"evmi_dwconv1d_cbt_lens_f32": "dwconv1d_cbt_lens", "evmi_dwconv1d_bwd_cbt_lens_f32": "dwconv_bwd_lens"}[name]
    assert stem in msg, f"{name}: evmi_last_error() = {msg!r} does not name the function ({stem!r})"


def test_workspace_query_is_the_existing_one():
    assert _lib.load().evmi_dwconv1d_bwd_cbt_f32_ws_elems(20, 6, 3) == 20 * 6 * 4
