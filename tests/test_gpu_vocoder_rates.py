"""Vocoders that upsample (output_sampling_rate = c x input_sampling_rate) and spec_type "mel" in training: the reconstruction loss,
whole GAN steps and the module / data side follow spectral.vocoder_output_transform -- the spectrogram the preprocessor stores as the
output-rate target.  References: oracle/mel_ref.py (torch.stft, its two filterbanks) and oracle/hifigan_ref.py, never the product.

Loss alone: float64 autograd of 45 * l1(f(y), f(y_hat)), f = the oracle transform at the derived parameters in float64 (the oracle's own
entry points mel_spectrogram_ref / torchaudio_mel_ref compute in fp32; ``_logspec64`` is their arithmetic on the oracle's filterbanks
in float64 and is held to them first).  Bounds: those of test_multi_resolution_stft_loss_value_and_gradient (the same DFT-as-GEMM against
FFT difference amplified by 1 / magnitude): value rel 2e-5, gradient |diff|_2 / |want|_2 <= 3e-3, max|diff| <= 1e-2 max|want|.
Measured (MI355X): DESIGN.md section 22."""

import json
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from everyvoice_amd.config import AudioConfig, HiFiGANConfig
from oracle import mel_ref
from oracle.hifigan_ref import (GeneratorRef, HiFiGANModelConfigRef, MultiPeriodDiscriminatorRef, MultiScaleDiscriminatorRef,
                                discriminator_loss_ref, feature_loss_ref, generator_loss_ref)
from tests.test_gpu_train_step import F32_G_GAIN, _bf16_operand_oracle, _grad_close, _params_close

pytestmark = pytest.mark.gpu

REPORT = True  # every figure is printed before it is asserted (pytest shows it with -s / -rA)


# ---- the oracle transform in float64 ----------------------------------------------------------------------------------------------
def _logspec64(x, t):
    """log(clamp(spec, 1e-5)) of x [B, S] (float64) through the oracle's transform ``t`` (vocoder_output_transform's dict) -> (log, linear)."""
    n_fft, win, hop, sr = t["n_fft"], t["win_length"], t["hop_length"], t["filter_sample_rate"]
    if t["spec_type"] == "mel-librosa":
        basis = torch.from_numpy(mel_ref.slaney_mel_basis(sr, n_fft, t["n_mels"], t["f_min"], t["f_max"])).to(x.dtype)
        lin = torch.matmul(basis, mel_ref.magnitude_spectrogram_ref(x, n_fft, win, hop))
    else:  # torchaudio_mel_ref's arithmetic: fb^T |STFT|^2 (spectrogram_ref's torch.stft call, in x's precision)
        fb = torch.from_numpy(mel_ref.htk_slaney_fbanks(sr, n_fft // 2 + 1, t["n_mels"], float(t["f_min"]), float(t["f_max"]))).to(x.dtype)
        spec = torch.stft(x, n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, dtype=x.dtype), center=True, pad_mode="reflect",
                          normalized=False, onesided=True, return_complex=True)
        lin = torch.matmul((spec.real**2 + spec.imag**2).transpose(-1, -2), fb).transpose(-1, -2)
    return torch.log(torch.clamp(lin, min=1e-5)), lin


def _logspec_oracle32(x, t):
    """The oracle's own entry points (fp32) at the same parameters."""
    n_fft, win, hop, sr = t["n_fft"], t["win_length"], t["hop_length"], t["filter_sample_rate"]
    if t["spec_type"] == "mel-librosa":
        return mel_ref.mel_spectrogram_ref(x, sr, n_fft, win, hop, t["n_mels"], t["f_min"], t["f_max"])
    return torch.log(torch.clamp(mel_ref.torchaudio_mel_ref(x, sr, n_fft, win, hop, t["n_mels"], float(t["f_min"]), float(t["f_max"])), min=1e-5))


def _tiny(c, win, spec_type, n_mels=10):
    return AudioConfig(input_sampling_rate=8000, output_sampling_rate=8000 * c, n_fft=32, fft_window_size=win, fft_hop_size=8, n_mels=n_mels,
                       f_max=4000, spec_type=spec_type)


# (id, AudioConfig, B, T): the tiny configs are the smallest at which each mechanism can go wrong -- the three sizes scaled by c, the
# short window scaled and centred, the input-rate filters -- in several blocks of the elementwise kernels; one case per type at the
# default sizes with c = 2.  Tiny "mel" at c = 1: 6 mel rows (with 10, empty HTK filters sit on the clamp, a kink of the comparison).
LOSS_CASES = []
for _st in ("mel-librosa", "mel"):
    for _win in (32, 24):
        for _c in (1, 2, 3):
            _n = 6 if (_st == "mel" and _c == 1) else 10
            LOSS_CASES.append((f"{_st}-win{_win}-c{_c}", _tiny(_c, _win, _st, _n), 2, 16 * 8 * _c))
    LOSS_CASES.append((f"{_st}-default-c2", AudioConfig(output_sampling_rate=44100, spec_type=_st), 2, 8192))


@pytest.mark.parametrize("case", LOSS_CASES, ids=[c[0] for c in LOSS_CASES])
def test_loss_value_and_gradient(cuda_device, case):
    from everyvoice_amd.spectral import vocoder_output_transform
    from everyvoice_amd.train.hifigan import MelLoss

    _, cfg, B, T = case
    t = vocoder_output_transform(cfg)
    g = torch.Generator().manual_seed(5)
    y = 0.3 * torch.tanh(torch.randn(B, T, generator=g))
    y_hat = y + 0.1 * torch.randn(B, T, generator=g)
    y64, yh64 = y.double(), y_hat.double().requires_grad_()
    (ly, lin_y), (lg, lin_g) = _logspec64(y64, t), _logspec64(yh64, t)
    # _logspec64 is the oracle's transform: its fp32 entry point agrees where fp32 can (away from the clamp; log of fp32 FFT noise below)
    want32 = _logspec_oracle32(y, t)
    solid = lin_y > 1e-3
    assert want32.shape == ly.shape and float((want32.double() - ly)[solid].abs().max()) <= 1e-5  # (measured <= 9e-7)
    # the comparison stays off the loss's kinks (asserted on the float64 oracle alone): the clamp at 1e-5 and |.| at 0
    assert float(torch.minimum(lin_y, lin_g.detach()).min()) >= 2e-5
    d = (ly - lg.detach()).abs()
    assert float((d < 1e-4).double().mean()) <= 1e-3
    want = 45.0 * F.l1_loss(lg, ly)
    want.backward()
    out = torch.zeros(1, device=cuda_device)
    grad = MelLoss(cfg, cuda_device).loss_and_grad(y.to(cuda_device), y_hat.to(cuda_device), 45.0, out)
    torch.cuda.synchronize()
    diff = grad.cpu().double() - yh64.grad
    rel_v = abs(float(out) - float(want)) / abs(float(want))
    rel_l2, rel_max = float(diff.norm() / yh64.grad.norm()), float(diff.abs().max() / yh64.grad.abs().max())
    if REPORT:
        print(f"LOSSERR {case[0]} value {float(want):.6f} rel {rel_v:.2e} grad l2 {rel_l2:.2e} max {rel_max:.2e} min-lin {float(torch.minimum(lin_y, lin_g.detach()).min()):.2e} "
              f"min-diff {float(d.min()):.2e}")
    assert grad.shape == (B, T)
    assert rel_v <= 2e-5
    assert rel_l2 <= 3e-3
    assert rel_max <= 1e-2


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_power_spectrum_op_codes(cuda_device, n):
    """Elementwise codes 26 / 27 at the block boundaries of the kernel: one fp32 rounding per operation, as torch's fp32 on the CPU
    without contraction (a*a + b*b may contract into an fma on the device: one rounding fewer, within 1 ulp of the sum)."""
    from everyvoice_amd.train import ops

    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    got = ops.elementwise(ops.EW_POWER, a.to(cuda_device), b.to(cuda_device)).cpu()
    want = a.double() ** 2 + b.double() ** 2
    # the products round (2^-24 relative each, so 2^-24 of their sum), then the sum rounds (2^-24): 2^-23 to first order
    assert float(((got.double() - want).abs() / want).max()) <= 1.01 * 2 ** -23
    got = ops.elementwise(ops.EW_SCALED_MUL, a.to(cuda_device), b.to(cuda_device), p0=2.0).cpu()
    assert torch.equal(got, 2.0 * a * b)  # (the factor 2 is exact: one rounding, of a * b)


# ---- whole steps ---------------------------------------------------------------------------------------------------------------------
UP2_MODEL = dict(upsample_rates=[8, 8, 4, 2], upsample_kernel_sizes=[16, 16, 8, 4], upsample_initial_channel=128)
UP2_AUDIO = dict(output_sampling_rate=44100)
UP2_MEL = dict(sr=22050, n_fft=2048, win=2048, hop=512)  # the output transform: sizes x 2, filters for the INPUT rate


def _up2_config(**audio):
    return HiFiGANConfig(model=UP2_MODEL, preprocessing=dict(audio=dict(UP2_AUDIO, **audio)))


def _mel_term_librosa(x, **kw):
    return mel_ref.mel_spectrogram_ref(x, **kw)


def _mel_term_torchaudio(x):
    return torch.log(torch.clamp(mel_ref.torchaudio_mel_ref(x, 22050, 1024, 1024, 256, 80, 0.0, 8000.0), min=1e-5))


def _gan_step(cuda_device, precision, config, model_ref_cfg, mel_term, S, hop_in, g_gain):
    """One GAN step against the float64 oracle step, built as tests/test_gpu_train_step.py: _full_gan_step builds it (the same order,
    the same bounds); ``mel_term``: the oracle's log-spectrogram of the reconstruction loss, ``hop_in``: output samples per input frame."""
    from everyvoice_amd.train.hifigan import HiFiGANTrainer

    B = 2
    torch.manual_seed(1234)
    torch.set_num_threads(8)
    g_ref = GeneratorRef(model_ref_cfg).train()
    mpd_ref, msd_ref = MultiPeriodDiscriminatorRef().train(), MultiScaleDiscriminatorRef().train()
    with torch.no_grad():  # livelier than the N(0, 0.01) init (the fixture of test_gpu_train_step.py), times that file's gain per precision
        for n, p in g_ref.named_parameters():
            if n.endswith("weight_v"):
                p.mul_(8.0)
            if n.endswith("weight_g"):
                p.mul_(8.0 * g_gain)
    opt_kw = dict(lr=2e-4, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.01)
    tr = HiFiGANTrainer(config, device=cuda_device, precision=precision, **opt_kw)
    tr.load_reference_state(g_ref.state_dict(), mpd_ref.state_dict(), msd_ref.state_dict())
    tr.keep_grads = True
    loss_rel = 2e-4 if precision == "f32" else 2e-3

    gen = torch.Generator().manual_seed(11)
    y = 0.3 * torch.tanh(torch.randn(B, 1, S, generator=gen))
    mel = mel_ref.mel_spectrogram_ref(y.squeeze(1)[:, :: hop_in // 256])[:, :, : S // hop_in]  # a log-mel at the input rate, S / hop_in frames
    y32, mel32 = y, mel
    if precision == "f32":
        g_ref, mpd_ref, msd_ref = g_ref.double(), mpd_ref.double(), msd_ref.double()
        y, mel = y.double(), mel.double()
    d_params_ref = list(mpd_ref.parameters()) + list(msd_ref.parameters())
    opt_g, opt_d = torch.optim.AdamW(g_ref.parameters(), **opt_kw), torch.optim.AdamW(d_params_ref, **opt_kw)
    y_hat = g_ref(mel)
    assert y_hat.shape == y.shape
    opt_d.zero_grad()
    r1, g1, _, _ = mpd_ref(y, y_hat.detach())
    r2, g2, _, _ = msd_ref(y, y_hat.detach())
    loss_d = discriminator_loss_ref(r1, g1) + discriminator_loss_ref(r2, g2)
    loss_d.backward()
    d_grads = {"mpd." + k: v.grad.clone().float() for k, v in mpd_ref.named_parameters()}
    d_grads.update({"msd." + k: v.grad.clone().float() for k, v in msd_ref.named_parameters()})
    opt_d.step()
    opt_g.zero_grad()
    loss_mel = F.l1_loss(mel_term(y.squeeze(1)), mel_term(y_hat.squeeze(1))) * 45
    _, g1, fr1, fg1 = mpd_ref(y, y_hat)
    _, g2, fr2, fg2 = msd_ref(y, y_hat)
    loss_fm = feature_loss_ref(fr1, fg1) + feature_loss_ref(fr2, fg2)
    loss_adv = generator_loss_ref(g1) + generator_loss_ref(g2)
    (loss_adv + loss_fm + loss_mel).backward()
    g_grads = {k: v.grad.clone().float() for k, v in g_ref.named_parameters()}
    opt_g.step()
    y_hat = y_hat.float()
    g_ref, mpd_ref, msd_ref = g_ref.float(), mpd_ref.float(), msd_ref.float()

    out = tr.training_step(mel32.to(cuda_device), y32.to(cuda_device))
    got_y = tr.last_grads["y_hat"].cpu().view(B, 1, S)
    if REPORT:
        print(f"STEPERR {precision} y_hat max|diff| {float((got_y - y_hat.detach()).abs().max()):.2e} of {float(y_hat.detach().abs().max()):.2e}; "
              + " ".join(f"{k} {out[k]:.6f} vs {float(v.detach()):.6f} rel {abs(out[k] - float(v.detach())) / abs(float(v.detach())):.1e}"
                         for k, v in (("d", loss_d), ("g_adv", loss_adv), ("g_fm", loss_fm), ("g_mel", loss_mel))))
    if precision == "f32":
        torch.testing.assert_close(got_y, y_hat.detach(), rtol=1e-4, atol=1e-5)
    else:
        assert float((got_y - y_hat.detach()).abs().max()) <= 2e-2 * float(y_hat.detach().abs().max())
    assert out["d"] == pytest.approx(float(loss_d.detach()), rel=loss_rel)
    assert out["g_adv"] == pytest.approx(float(loss_adv.detach()), rel=loss_rel)
    assert out["g_fm"] == pytest.approx(float(loss_fm.detach()), rel=loss_rel)
    assert out["g_mel"] == pytest.approx(float(loss_mel.detach()), rel=loss_rel)
    if precision != "f32":  # _full_gan_step's bf16 bounds at 2 items (direction and size per tensor, median, share below 0.995)
        cosines, worst, failed = {"d": [], "g": []}, {"d": (1.0, 0.0), "g": (1.0, 0.0)}, []
        for grads, key in ((d_grads, "d"), (g_grads, "g")):
            for name, want in grads.items():
                got = tr.last_grads[key][name].cpu().reshape(want.shape).double().flatten()
                w = want.double().flatten()
                if float(w.norm()) < 1e-12:
                    continue
                cos = float(torch.dot(got, w) / (got.norm() * w.norm() + 1e-300))
                ratio = float(got.norm() / w.norm())
                cosines[key].append(cos)
                worst[key] = min(worst[key][0], cos), max(worst[key][1], abs(ratio - 1.0))
                floor, tol = (0.999, 0.015) if key == "d" else (0.988, 0.06)
                if not (cos >= floor and 1.0 - tol <= ratio <= 1.0 + tol):
                    failed.append(f"{key}.{name}: cos {cos:.4f} norm ratio {ratio:.3f}")
        gc = sorted(cosines["g"])
        med, low = gc[len(gc) // 2], sum(c < 0.995 for c in gc)
        print(f"STEPCOS worst (cosine, |norm ratio - 1|) d {worst['d']} g {worst['g']} g median {med:.4f} below 0.995: {low} of {len(gc)}")
        assert not failed, failed
        assert med >= 0.996 and low <= 0.20 * len(gc), (med, low, len(gc))
        return
    for name, want in d_grads.items():
        _grad_close(name, tr.last_grads["d"][name].cpu(), want)
    for name, want in g_grads.items():
        _grad_close(name, tr.last_grads["g"][name].cpu(), want, rel=2e-2)
    sd_g = tr.g_params.state_dict()
    for k, v in g_ref.state_dict().items():
        _params_close(k, sd_g[k].cpu(), v, g_grads.get(k))
    sd_d = tr.d_params.state_dict()
    ref_d = {"mpd." + k: v for k, v in mpd_ref.state_dict().items()}
    ref_d.update({"msd." + k: v for k, v in msd_ref.state_dict().items()})
    for k, v in ref_d.items():
        if k.endswith("weight_u") or k.endswith("weight_v") and "discriminators.0" in k and k.startswith("msd."):
            continue  # spectral-norm buffers
        if k in sd_d:
            _params_close(k, sd_d[k].cpu(), v, d_grads.get(k))


def test_gan_step_at_twice_the_rate_matches_oracle(cuda_device):
    """22.05 -> 44.1 kHz: 8 input frames in, 4096 output samples out; the 45 x mel-L1 term at 2048 / 2048 / 512 with 22.05 kHz filters."""
    _gan_step(cuda_device, "f32", _up2_config(), HiFiGANModelConfigRef(**UP2_MODEL), lambda x: _mel_term_librosa(x, **UP2_MEL), 4096, 512, F32_G_GAIN)


def test_gan_step_at_twice_the_rate_bf16_operands_match_rounded_oracle(cuda_device):
    with _bf16_operand_oracle():
        _gan_step(cuda_device, "bf16", _up2_config(), HiFiGANModelConfigRef(**UP2_MODEL), lambda x: _mel_term_librosa(x, **UP2_MEL), 4096, 512, 1.0 / 8.0)


def test_gan_step_with_spec_type_mel_matches_oracle(cuda_device):
    """spec_type "mel" at c = 1, default sizes: the reconstruction term is the torchaudio mel (power spectrum, HTK scale), log-clamped."""
    cfg = HiFiGANConfig(preprocessing=dict(audio=dict(spec_type="mel")))
    _gan_step(cuda_device, "f32", cfg, HiFiGANModelConfigRef(), _mel_term_torchaudio, 2048, 256, F32_G_GAIN)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_graph_replay_equals_eager_steps_at_twice_the_rate(cuda_device, precision):
    """use_graph=True at c = 2: two eager warm-up steps, then three captured replays end bitwise where five eager steps do."""
    from everyvoice_amd.train.hifigan import HiFiGANTrainer

    g = torch.Generator().manual_seed(18)
    B, frames = 2, 8
    ys = [(0.3 * torch.tanh(torch.randn(B, 1, frames * 512, generator=g))).to(cuda_device) for _ in range(5)]
    mels = [torch.randn(B, 80, frames, generator=g).to(cuda_device) for _ in range(5)]
    res = {}
    for graph in (False, True):
        tr = HiFiGANTrainer(_up2_config(), device=cuda_device, seed=5, precision=precision, use_graph=graph)
        losses = [tr.training_step(m, y) for m, y in zip(mels, ys)]
        if graph:
            assert tr._graph_failed is None, tr._graph_failed
            assert len(tr._graphs) == 1
        res[graph] = (losses, tr.state_dict(), tr.checkpoint()["optimizer_states"])
    assert res[True][0] == res[False][0]
    assert all(l["g_mel"] > 0 for l in res[True][0])
    for k in res[False][1]:
        assert torch.equal(res[False][1][k], res[True][1][k]), k
    for a, b in zip(res[False][2], res[True][2]):
        assert a["evmi_flat_adamw"]["step"] == b["evmi_flat_adamw"]["step"] == 5
        assert torch.equal(a["evmi_flat_adamw"]["exp_avg_sq"], b["evmi_flat_adamw"]["exp_avg_sq"])


def test_training_step_refuses_audio_at_the_input_rate(cuda_device):
    from everyvoice_amd.train.hifigan import HiFiGANTrainer

    tr = HiFiGANTrainer(_up2_config(), device=cuda_device, seed=5)
    g = torch.Generator().manual_seed(3)
    mel = torch.randn(2, 80, 8, generator=g).to(cuda_device)
    before = {k: v.clone() for k, v in tr.state_dict().items()}
    with pytest.raises(ValueError, match=r"output_sampling_rate 44100.*4096 expected"):
        tr.training_step(mel, (0.3 * torch.tanh(torch.randn(2, 1, 8 * 256, generator=g))).to(cuda_device))
    assert tr.global_step == 0 and all(torch.equal(v, before[k]) for k, v in tr.state_dict().items())  # nothing was launched
    out = tr.training_step(mel, (0.3 * torch.tanh(torch.randn(2, 1, 8 * 512, generator=g))).to(cuda_device))
    assert tr.global_step == 1 and all(np.isfinite(v) for v in out.values()) and out["g_mel"] > 0


# ---- module and data side, end to end at a small size -------------------------------------------------------------------------------------
def _write_wav(path, x, sr=22050):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.clip(np.round(np.asarray(x) * 32767), -32768, 32767).astype("<i2").tobytes())


def test_preprocess_dataset_module_at_twice_the_rate(tmp_path, cuda_device):
    """GpuPreprocessor at 22050 -> 44100 -> HiFiGANDataModule / SpecDataset with segments of 2048 output samples (4 input frames) -> one
    training step and one validation step of lightning.HiFiGAN; the stored output-rate spectrogram IS the loss's transform of the stored
    output-rate audio (the bound of tests/test_gpu_mel.py between the front end and oracle/mel_ref.py: |log-mel diff| <= 2e-3)."""
    from everyvoice_amd import pipeline
    from everyvoice_amd.dataset import HiFiGANDataModule
    from everyvoice_amd.lightning import HiFiGAN

    gen = torch.Generator().manual_seed(9)
    items = []
    for i, n in enumerate([9000, 9800, 11000, 12500]):  # 0.41 - 0.57 s (min_audio_length 0.4)
        _write_wav(tmp_path / f"u{i}.wav", 0.3 * torch.tanh(torch.randn(n, generator=gen)).numpy())
        items.append(dict(basename=f"u{i}", speaker="default", language="default", wav=tmp_path / f"u{i}.wav"))
    audio = dict(UP2_AUDIO, vocoder_segment_size=2048)
    kept = pipeline.GpuPreprocessor(AudioConfig(**audio), device=cuda_device, batch_items=4, pitch=False).process(items, tmp_path / "pre")
    assert len(kept) == 4
    rows = ["basename|speaker|language"] + [f"{k['basename']}|default|default" for k in kept]
    (tmp_path / "train.psv").write_text("\n".join(rows) + "\n")
    (tmp_path / "val.psv").write_text("\n".join(rows[:3]) + "\n")
    cfg = HiFiGANConfig(model=UP2_MODEL, preprocessing=dict(save_dir=tmp_path / "pre", audio=audio),
                        training=dict(training_filelist=tmp_path / "train.psv", validation_filelist=tmp_path / "val.psv", batch_size=2, train_data_workers=0,
                                      logger=dict(save_dir=tmp_path / "logs", name="exp")))
    json.dumps(cfg.model_dump(mode="json"))
    dm = HiFiGANDataModule(cfg)
    dm.prepare_data()
    dm.setup("fit")
    batch = next(iter(dm.train_dataloader()))
    assert batch[0].shape == (2, 80, 4) and batch[1].shape == (2, 2048) and batch[3].shape == (2, 80, 4)
    model = HiFiGAN(cfg, device=cuda_device, precision="f32", use_graph=False)
    out = model.training_step(batch, 0)
    assert all(np.isfinite(v) for v in out.values()) and out["g_mel"] > 0 and model.global_step == 1
    # validation: the value is the L1 between the ORACLE's output-transform log-mels of the generated and the stored audio
    vb = next(iter(dm.val_dataloader()))
    err = model.validation_step(vb, 0)
    wav = model.trainer_.generate(vb[0].to(cuda_device)).cpu()
    assert wav.shape[-1] == vb[1].shape[-1] == 2048
    want = float((mel_ref.mel_spectrogram_ref(wav[:, 0], **UP2_MEL) - mel_ref.mel_spectrogram_ref(vb[1], **UP2_MEL)).abs().mean())
    if REPORT:
        print(f"VALERR validation/mel_spec_error {err:.6f} oracle {want:.6f} diff {abs(err - want):.2e}")
    assert model.logged["validation/mel_spec_error"] == err and abs(err - want) <= 2e-3
    # target and loss are the same spectrogram
    worst = 0.0
    for k in kept:
        base = tmp_path / "pre"
        y = pipeline.load_wav(base / "audio" / f"{k['basename']}--default--default--audio-44100.wav")[0][0]
        spec = torch.load(base / "spec" / f"{k['basename']}--default--default--spec-44100-mel-librosa.pt", weights_only=True)
        frames = y.numel() // 512
        got = model.trainer_.mel_loss.logmel(y[None].to(cuda_device))[0].cpu()[:, :frames]
        assert spec.shape == got.shape == (80, frames)
        worst = max(worst, float((got - spec).abs().max()))
    if REPORT:
        print(f"TARGETERR stored spec-44100 vs the loss's transform of audio-44100: max|diff| {worst:.2e}")
    assert worst <= 2e-3
