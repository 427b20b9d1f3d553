"""variance_predictors.{pitch,energy}.level, variance_predictors.<name>.loss and mel_loss on the host: refusals where the configuration
is read, round trips through the dict, ``-c`` override and checkpoint forms, and the level-aware reference of the GPU tests
(tests/fs2_levels_ref.py) against the oracle's own phone-level / mse training forward."""

import enum

import pytest
import torch

from oracle.fs2_ref import FastSpeech2ConfigRef, FastSpeech2Ref, training_losses_ref


def _config(**variance):
    from everyvoice_amd.fs2 import FastSpeech2ModelConfig, VariancePredictorConfig, VariancePredictors

    return FastSpeech2ModelConfig(variance_predictors=VariancePredictors(**{k: VariancePredictorConfig(**v) for k, v in variance.items()}))


@pytest.mark.parametrize("where,field,value", [("pitch", "level", "word"), ("energy", "level", "frames"), ("duration", "level", None),
                                               ("duration", "loss", "l1"), ("pitch", "loss", "huber"), ("energy", "loss", ""), (None, "mel_loss", "l2")])
def test_values_outside_the_schema_are_refused_where_the_configuration_is_read(where, field, value):
    from everyvoice_amd.fs2 import FastSpeech2, variance_settings
    from everyvoice_amd.lightning import FastSpeech2Config
    from everyvoice_amd.train.fs2 import FastSpeech2Trainer

    def bad():
        cfg = _config()
        setattr(getattr(cfg.variance_predictors, where) if where else cfg, field, value)
        return cfg

    name = f"variance_predictors.{where}.{field}" if where else "mel_loss"
    with pytest.raises(ValueError, match=name):
        variance_settings(bad())
    # the constructors refuse it before anything else (on a machine without a GPU they end in a RuntimeError otherwise)
    with pytest.raises(ValueError, match=name):
        FastSpeech2(bad(), device="cpu")
    with pytest.raises(ValueError, match=name):
        FastSpeech2Trainer(bad(), device="cpu")
    with pytest.raises(ValueError, match=name):
        FastSpeech2Config(model=bad())


def test_valid_values_and_enums_are_accepted_and_become_strings():
    from everyvoice_amd.fs2 import FastSpeech2, apply_variance_settings, variance_settings

    class Level(enum.Enum):
        phone = "phone"
        frame = "frame"

    class Loss(enum.Enum):
        mse = "mse"
        mae = "mae"

    cfg = _config(pitch=dict(level=Level.frame, loss=Loss.mae), energy=dict(level="phone", loss="mae"))
    cfg.mel_loss = Loss.mae
    want = {"level": {"duration": "phone", "pitch": "frame", "energy": "phone"}, "loss": {"duration": "mse", "pitch": "mae", "energy": "mae", "mel": "mae"}}
    assert variance_settings(cfg) == want
    assert cfg.variance_predictors.pitch.level is Level.frame and cfg.mel_loss is Loss.mae  # (reading the settings leaves the configuration alone)
    assert apply_variance_settings(cfg) == want  # (what the constructors call: the strings are written back)
    assert cfg.variance_predictors.pitch.level == "frame" and cfg.variance_predictors.pitch.loss == "mae" and cfg.mel_loss == "mae"
    import json
    from dataclasses import asdict

    json.dumps(asdict(cfg))  # (a checkpoint's hyper-parameters are JSON only)
    with pytest.raises(RuntimeError, match="no CPU path"):  # a valid configuration gets as far as the device check
        FastSpeech2(cfg, device="cpu")
    assert variance_settings(_config())["level"] == {"duration": "phone", "pitch": "phone", "energy": "phone"}  # the defaults


def test_settings_survive_the_dict_override_and_checkpoint_forms():
    from dataclasses import asdict

    from everyvoice_amd.fs2 import FastSpeech2ModelConfig
    from everyvoice_amd.lightning import FastSpeech2 as Module
    from everyvoice_amd.lightning import FastSpeech2Config, parse_config_args

    cfg = FastSpeech2Config(model={"variance_predictors": {"pitch": {"level": "frame", "loss": "mae"}}, "mel_loss": "mae"})
    vp = cfg.model.variance_predictors
    assert (vp.pitch.level, vp.pitch.loss, vp.energy.level, vp.energy.loss, vp.duration.loss, cfg.model.mel_loss) == ("frame", "mae", "phone", "mse", "mse", "mae")
    # -c overrides: merged into the dumped config, which is rebuilt (and checked again)
    cfg.update_config(parse_config_args(["model.variance_predictors.energy.level=frame", "model.variance_predictors.duration.loss=mae"]))
    vp = cfg.model.variance_predictors
    assert (vp.pitch.level, vp.pitch.loss, vp.energy.level, vp.duration.loss, cfg.model.mel_loss) == ("frame", "mae", "frame", "mae", "mae")
    with pytest.raises(ValueError, match="variance_predictors.pitch.level"):
        FastSpeech2Config(**cfg.model_dump()).update_config(parse_config_args(["model.variance_predictors.pitch.level=utterance"]))
    # checkpoint hyper-parameters (JSON only) -> the module's config, and -> the inference model's config
    module = Module(cfg)
    ckpt = {"state_dict": {}}
    module.on_save_checkpoint(ckpt)
    back = Module.load_from_checkpoint(ckpt).config.model
    assert asdict(back) == asdict(cfg.model)
    hp_model = ckpt["hyper_parameters"]["config"]["model"]
    assert hp_model["variance_predictors"]["energy"]["level"] == "frame" and hp_model["mel_loss"] == "mae"
    from everyvoice_amd.lightning import _dataclass_from_dict

    assert asdict(_dataclass_from_dict(FastSpeech2ModelConfig, asdict(cfg.model))) == asdict(cfg.model)
    bad = {**ckpt, "hyper_parameters": {**ckpt["hyper_parameters"], "config": {**ckpt["hyper_parameters"]["config"], "model": {**hp_model, "mel_loss": "huber"}}}}
    with pytest.raises(TypeError, match="Unable to load config"):
        Module.load_from_checkpoint(bad)


def _batch(ref_cfg, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(max(1, L // 2), L + 1, (B,), generator=g)
    lens[0] = L
    pad = torch.arange(L)[None] >= lens[:, None]
    ids = torch.randint(1, ref_cfg.n_symbols, (B, L), generator=g).masked_fill(pad, 0)
    durs = torch.randint(0, 5, (B, L), generator=g)
    durs[:, 0] += 1
    durs = durs.masked_fill(pad, 0)
    mel_lens = durs.sum(1)
    T = int(mel_lens.max())
    mel = torch.randn(B, T, ref_cfg.n_mels, generator=g).masked_fill((torch.arange(T)[None] >= mel_lens[:, None])[..., None], 0.0)
    return dict(ids=ids, lens=lens, durations=durs, mel=mel, pitch=torch.randn(B, L, generator=g), energy=torch.randn(B, L, generator=g),
                pitch_frames=torch.randn(B, T, generator=g), energy_frames=torch.randn(B, T, generator=g),
                speakers=torch.randint(0, 3, (B,), generator=g))


def test_the_level_aware_reference_equals_the_oracle_at_phone_level_and_mse():
    from tests.fs2_levels_ref import training_losses_levels_ref

    ref_cfg = FastSpeech2ConfigRef.small()
    ref_cfg.n_speakers = 3
    ref_cfg.encoder.dropout = ref_cfg.decoder.dropout = ref_cfg.duration.dropout = ref_cfg.pitch.dropout = ref_cfg.energy.dropout = 0.0
    torch.manual_seed(3)
    model = FastSpeech2Ref(ref_cfg).train()
    batch = _batch(ref_cfg, 3, 14, seed=14)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    want = training_losses_ref(model, batch)
    want["total"].backward()
    want_grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.load_state_dict(state)  # (the BatchNorm statistics the first forward moved)
    model.zero_grad()
    got, margins = training_losses_levels_ref(model, batch)
    got["total"].backward()
    assert margins == {} and list(got) == list(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    for n, p in model.named_parameters():
        if n in want_grads:
            assert torch.equal(p.grad, want_grads[n]), n


def test_the_reference_moves_a_frame_level_predictor_behind_the_length_regulator():
    """(pitch: frame, energy: phone): the energy predictor does not see the pitch embedding, the pitch term is normalised by the
    frame count, and mae terms report their margin to the sign discontinuity."""
    from tests.fs2_levels_ref import forward_levels_ref, training_losses_levels_ref

    ref_cfg = FastSpeech2ConfigRef.small()
    ref_cfg.encoder.dropout = ref_cfg.decoder.dropout = ref_cfg.duration.dropout = ref_cfg.pitch.dropout = ref_cfg.energy.dropout = 0.0
    ref_cfg.pitch.level = "frame"
    torch.manual_seed(3)
    model = FastSpeech2Ref(ref_cfg).train()
    batch = _batch(ref_cfg, 3, 14, seed=14)
    batch.pop("speakers")
    phone_cfg = FastSpeech2ConfigRef.small()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    base = training_losses_ref(model, batch)
    model.load_state_dict(state)
    got, margins = training_losses_levels_ref(model, batch, kinds={"pitch": "mae", "mel": "mae"})
    assert torch.equal(got["duration"], base["duration"])
    assert not torch.equal(got["energy"], base["energy"]) and set(margins) == {"pitch", "mel", "postnet"} and min(margins.values()) >= 0.0
    with torch.no_grad():  # the energy term with the pitch embedding zeroed in the phone-level oracle = the frame-level model's energy term
        model.load_state_dict(state)
        model.cfg.pitch.level = "phone"
        keep = model.pitch_embedding.weight.clone()
        model.pitch_embedding.weight.zero_()
        assert torch.equal(training_losses_ref(model, batch)["energy"], got["energy"])
        model.pitch_embedding.weight.copy_(keep)
        model.cfg.pitch.level = "frame"
        model.load_state_dict(state)
    T = int(batch["durations"].sum(1).max())
    out = forward_levels_ref(model.eval(), batch["ids"], batch["lens"], durations=batch["durations"])
    assert tuple(out[3].shape) == (3, T) and tuple(out[4].shape) == (3, 14) and phone_cfg.pitch.level == "phone"
