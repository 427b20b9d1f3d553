"""torch-CPU restatement of FastSpeech2's variance adaptor with ``variance_predictors.{pitch,energy}.level`` = "phone" or "frame"
and "mse" / "mae" losses -- a test helper beside the oracle, like ``tests/gst_ref.py``: composed from the modules of
``oracle.fs2_ref.FastSpeech2Ref`` (whose own ``forward`` / ``training_losses_ref`` stay phone-level and mse).

The order is the ming024 / LightningFastSpeech2 one (PARITY UNPINNED like the rest of the restatement):
  1. encoder, then the speaker / language embeddings;  2. duration predictor on the symbol axis;
  3. pitch, then energy, where the level is "phone": predictor on the current symbol-axis tensor, then its bucket embedding;
  4. length regulator;
  5. pitch, then energy, where the level is "frame": predictor on the current frame-axis tensor (mask = the frame padding), then its
     bucket embedding at EVERY frame, padded ones included (value 0 there);
  6. positional term (which zeroes the padding), decoder, mel_linear, postnet.
Training buckets the targets, inference buckets prediction * control.  The levels are read from ``model.cfg.{pitch,energy}.level``.
"""

import torch
import torch.nn.functional as F

from oracle.heavy_ref import expand_ref

MSE = {"duration": "mse", "pitch": "mse", "energy": "mse", "mel": "mse"}


def _levels(model):
    return {"pitch": model.cfg.pitch.level, "energy": model.cfg.energy.level}


def _encode(model, ids, lens, speakers, languages):
    L = ids.shape[1]
    pad = torch.arange(L)[None, :] >= lens[:, None]
    x = model.text_input_layer(ids) + model.position_embedding(L)[None]
    x = x.masked_fill(pad[..., None], 0.0)
    x, _ = model.encoder(x, lens)
    if model.speaker_embedding is not None:
        x = x + model.speaker_embedding(speakers)[:, None, :].masked_fill(pad[..., None], 0.0)
    if model.language_embedding is not None:
        x = x + model.language_embedding(languages)[:, None, :].masked_fill(pad[..., None], 0.0)
    return x, pad


def _variance(model, name):
    return getattr(model, name + "_predictor"), getattr(model, name + "_embedding"), getattr(model, name + "_bins")


def training_losses_levels_ref(model, batch: dict, kinds: dict | None = None, weights: dict | None = None, aligner=None, hard=None):
    """-> (losses, margins).  Teacher-forced training forward for any of the four level combinations; ``kinds``: "mse" / "mae" for
    "duration", "pitch", "energy" and "mel" (mel and postnet terms).  Every term is weight * sum f(pred - target) / count over the valid
    positions, f = x^2 or |x|; count = symbols for a symbol-axis term, frames for a frame-axis one, frames * n_mels for the mel terms.
    ``margins[term]`` = min |pred - target| over the valid elements of every mae term: the mae gradient is sign(pred - target), so a
    comparison against another arithmetic is only meaningful where no element sits at the discontinuity."""
    kinds = {**MSE, **(kinds or {})}
    w = {"mel": 1.0, "postnet": 1.0, "pitch": 0.1, "energy": 0.1, "duration": 0.1, "attn_ctc": 0.1, "attn_bin": 0.0}
    w.update(weights or {})
    levels = _levels(model)
    margins = {}

    def term(name, kind, pred, target, valid, count):
        d = pred - target
        if kind == "mae":
            margins[name] = float(d.detach().abs()[valid].min())
        return w[name] * ((d ** 2).sum() if kind == "mse" else d.abs().sum()) / count

    ids, lens = (batch["pfs"] if getattr(model, "pfs", False) else batch["ids"]), batch["lens"]
    B, L = ids.shape[:2]
    pad = torch.arange(L)[None, :] >= lens[:, None]
    losses = {}
    if aligner is not None:
        from oracle.alignment_ref import binarization_loss_ref, forward_sum_loss_ref
        from oracle.mas_ref import maximum_path_batch_ref

        mel_lens_in = batch["mel_lens"]
        Tm = int(mel_lens_in.max())
        soft, logprob = aligner(batch["mel"][:, :Tm].transpose(1, 2), model.text_input_layer(ids).masked_fill(pad[..., None], 0.0).transpose(1, 2), lens,
                                batch.get("attn_prior"))
        if hard is None:
            hard, _ = maximum_path_batch_ref(torch.log(soft.detach()).numpy(), mel_lens_in.numpy(), lens.numpy())
            hard = torch.from_numpy(hard)
        durations = hard.sum(1).long()
        losses["attn_ctc"] = w["attn_ctc"] * forward_sum_loss_ref(logprob, lens, mel_lens_in)
        if w["attn_bin"] > 0:
            losses["attn_bin"] = w["attn_bin"] * binarization_loss_ref(hard, soft)
        cum = torch.cumsum(durations, 1)

        def phone_level(key):  # average_data_by_durations: mean over the symbol's frames, 1e-7 for none
            fr = F.pad(torch.cumsum(batch[key + "_frames"][:, :Tm], 1), (1, 0))
            sums = torch.gather(fr, 1, cum) - torch.gather(fr, 1, cum - durations)
            return torch.where(durations > 0, sums / durations.clamp_min(1), torch.full_like(sums, 1e-7))

        batch = dict(batch, durations=durations)
        for key in ("pitch", "energy"):
            if levels[key] == "phone" and key not in batch:
                batch[key] = phone_level(key)
    durations = batch["durations"]
    x, _ = _encode(model, ids, lens, batch.get("speakers"), batch.get("languages"))
    durations = durations.clamp_min(0).masked_fill(pad, 0)
    n_tok = lens.sum()
    log_d = model.duration_predictor(x, pad)
    losses["duration"] = term("duration", kinds["duration"], log_d, torch.log(durations.float() + 1.0), ~pad, n_tok)
    for name in ("pitch", "energy"):
        if levels[name] == "phone":
            predictor, embedding, bins = _variance(model, name)
            target = batch[name].masked_fill(pad, 0.0)
            losses[name] = term(name, kinds[name], predictor(x, pad), target, ~pad, n_tok)
            x = x + embedding(torch.bucketize(target, bins))
    mel_lens = durations.sum(1)
    T = int(mel_lens.max())
    frames = torch.stack([F.pad(torch.repeat_interleave(x[b], durations[b], dim=0), (0, 0, 0, T - int(mel_lens[b]))) for b in range(B)])
    fpad = torch.arange(T)[None, :] >= mel_lens[:, None]
    n_frames = mel_lens.sum()
    for name in ("pitch", "energy"):
        if levels[name] == "frame":
            predictor, embedding, bins = _variance(model, name)
            target = batch[name + "_frames"][:, :T].masked_fill(fpad, 0.0)
            losses[name] = term(name, kinds[name], predictor(frames, fpad), target, ~fpad, n_frames)
            frames = frames + embedding(torch.bucketize(target, bins))
    y = (frames + model.position_embedding(T)[None]).masked_fill(fpad[..., None], 0.0)
    y, _ = model.decoder(y, mel_lens)
    mel = model.mel_linear(y).masked_fill(fpad[..., None], 0.0)
    target = batch["mel"][:, :T]
    n_el = mel_lens.sum() * mel.shape[2]
    valid = (~fpad)[..., None].expand_as(mel)
    losses["mel"] = term("mel", kinds["mel"], mel, target, valid, n_el)
    if model.postnet is not None:
        post = (mel + model.postnet(mel)).masked_fill(fpad[..., None], 0.0)
        losses["postnet"] = term("postnet", kinds["mel"], post, target, valid, n_el)
    losses["total"] = sum(losses.values())
    return losses, margins


@torch.no_grad()
def forward_levels_ref(model, ids, lens, duration_control=1.0, pitch_control=1.0, energy_control=1.0, durations=None, speakers=None,
                       languages=None, guard=False):
    """Inference forward for any level combination -> (mel, postnet mel, durations, pitch, energy, mel_lens); pitch / energy are
    [B, T] for a frame-level predictor and [B, L] otherwise.  ``guard``: assert that the inputs sit on no decision boundary a
    summation-order difference could cross -- no predicted duration within 1e-3 of a rounding boundary, no frame-level prediction
    times its control within 1e-3 of a bin edge."""
    B, L = ids.shape[:2]
    levels = _levels(model)
    controls = {"pitch": pitch_control, "energy": energy_control}
    x, pad = _encode(model, ids, lens, speakers, languages)
    log_d = model.duration_predictor(x, pad)
    out = {}
    for name in ("pitch", "energy"):
        if levels[name] == "phone":
            predictor, embedding, bins = _variance(model, name)
            out[name] = predictor(x, pad) * controls[name]
            x = x + embedding(torch.bucketize(out[name], bins))
    if durations is None:
        raw = torch.exp(log_d) - 1.0
        if guard:
            assert bool((((raw - torch.floor(raw) - 0.5).abs() > 1e-3) | pad).all()), "test input sits on a rounding boundary: pick another seed"
        durations = torch.clamp(torch.round(raw) * duration_control, min=0).long()
    durations = durations.masked_fill(pad, 0)
    mel_lens = durations.sum(1)
    T = int(mel_lens.max())
    frames = torch.zeros(B, T, x.shape[2])
    for b in range(B):
        e = torch.from_numpy(expand_ref(x[b].numpy(), durations[b].numpy()))
        frames[b, : e.shape[0]] = e
    fpad = torch.arange(T)[None, :] >= mel_lens[:, None]
    for name in ("pitch", "energy"):
        if levels[name] == "frame":
            predictor, embedding, bins = _variance(model, name)
            out[name] = predictor(frames, fpad) * controls[name]
            if guard:
                edge = (out[name][..., None] - bins).abs().min(-1).values
                assert bool(((edge > 1e-3) | fpad).all()), f"a frame-level {name} value sits on a bin edge: pick another seed"
            frames = frames + embedding(torch.bucketize(out[name], bins))
    y = (frames + model.position_embedding(T)[None]).masked_fill(fpad[..., None], 0.0)
    y, _ = model.decoder(y, mel_lens)
    mel = model.mel_linear(y).masked_fill(fpad[..., None], 0.0)
    post = mel + model.postnet(mel) if model.postnet is not None else mel
    post = post.masked_fill(fpad[..., None], 0.0)
    return mel, post, durations, out["pitch"], out["energy"], mel_lens
