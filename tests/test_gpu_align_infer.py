"""The aligner at inference on the GPU: ``evmi_align_durations_f32`` alone on planted inputs, on a ragged batch and
in a captured graph; ``FastSpeech2.align`` against the oracle's aligner in float64; teacher-forced synthesis from a preprocessed folder
that holds spectrograms and no durations.  The float64 references are tests/align_ref.py's, computed once per process."""

import numpy as np
import pytest
import torch

import align_ref as R
from everyvoice_amd import _lib

pytestmark = pytest.mark.gpu


def cbt(x, dev):
    """[A, N] numpy -> [A, 1, N] on the device (one item, channel-major)."""
    return torch.from_numpy(np.ascontiguousarray(x))[:, None, :].contiguous().to(dev)


def i32(values, dev):
    return torch.tensor(list(values), dtype=torch.int32, device=dev)


def fused(r, dev):
    from everyvoice_amd.train import ops

    L, T = r["k"].shape[1], r["q"].shape[1]
    prior = None if r["prior"] is None else torch.from_numpy(r["prior"])[None].contiguous().to(dev)
    return ops.align_durations(cbt(r["q"], dev), cbt(r["k"], dev), prior, i32([L], dev), i32([T], dev), r["temperature"])[0].cpu().to(torch.int64)


def chain(r, dev):
    """Today's way to the same durations: soft attention -> log -> the monotonic search."""
    from everyvoice_amd.heavy import maximum_path
    from everyvoice_amd.train import ops

    L, T = r["k"].shape[1], r["q"].shape[1]
    prior = None if r["prior"] is None else torch.from_numpy(r["prior"])[None].contiguous().to(dev)
    soft, _ = ops.align_attention_fwd(cbt(r["q"], dev), cbt(r["k"], dev), prior, i32([L], dev), r["temperature"])
    return maximum_path(ops.elementwise(16, soft), i32([T], dev), i32([L], dev))[1][0].cpu()


# =====================================================================================================================
# the kernel alone
# =====================================================================================================================
@pytest.mark.parametrize("setting", list(R.SETTINGS))
@pytest.mark.parametrize("L,T", R.SHAPES)
def test_planted_durations_are_found_exactly(cuda_device, L, T, setting):
    """The float64 optimum is the planted path and beats every single-boundary shift by >= 1.0 (prior, temperature 0.05: fp32
    accumulation error ~1e-2) or >= 0.02 (the model's temperature without the prior: ~1e-6): the fp32 search has to find it, and so has
    today's chain."""
    r = R.planted_reference(L, T, setting)
    assert r["margin"] >= R.SETTINGS[setting][2] and np.array_equal(r["optimum"], r["planted"])
    want = torch.from_numpy(r["planted"])
    assert torch.equal(fused(r, cuda_device), want)
    assert torch.equal(chain(r, cuda_device), want)


@pytest.mark.parametrize("L,T", R.SHAPES)
def test_model_setting_structure_and_score_bound(cuda_device, L, T):
    """The model's temperature with the prior: paths ~1e-4 apart exist, so no equality -- the structure of a duration row, and the float64
    score of the returned path within 2 T 2^-24 max|Q| of the float64 optimum (align_ref.score_bound)."""
    r = R.planted_reference(L, T, "model")
    got = fused(r, cuda_device).numpy()
    assert R.structure_ok(got, T, L), got
    gap = R.path_score(r["value"], r["optimum"]) - R.path_score(r["value"], got)
    print(f"L {L} T {T}: optimum - returned = {gap:.3e}, bound {R.score_bound(T, r['q_max']):.3e}")
    assert gap <= R.score_bound(T, r["q_max"]), (gap, R.score_bound(T, r["q_max"]))


RAGGED = [(1, 3), (37, 221), (150, 907), (64, 64), (50, 20)]  # (L_b, T_b); the last one has fewer frames than tokens
L_PAD, T_PAD, GUARD = 150, 907, 64


def _ragged_inputs(dev):
    from oracle.attention_prior_ref import attention_prior_ref

    A, B = R.A_PLANTED, len(RAGGED)
    q = torch.full((A, B, T_PAD), float("nan"))
    k = torch.full((A, B, L_PAD), float("nan"))
    prior = torch.full((B, T_PAD, L_PAD), float("nan"), dtype=torch.float64)
    items = []
    for b, (Lb, Tb) in enumerate(RAGGED):
        if Tb < Lb:  # no planted path: any finite numbers
            g = torch.Generator().manual_seed(b)
            qb, kb, pb = torch.randn(A, Tb, generator=g).numpy(), torch.randn(A, Lb, generator=g).numpy(), np.full((Tb, Lb), 0.5)
        else:
            qb, kb, _ = R.planted_case(Lb, Tb)
            pb = attention_prior_ref(Tb, Lb)
        q[:, b, :Tb], k[:, b, :Lb], prior[b, :Tb, :Lb] = torch.from_numpy(qb), torch.from_numpy(kb), torch.from_numpy(pb)
        items.append({"q": qb, "k": kb, "prior": pb, "temperature": 0.05})
    return q.to(dev), k.to(dev), prior.to(dev), items


def _guarded_call(q, k, prior, text_lens, mel_lens, temperature):
    """The call with sentinels around (and in) the duration rows and around the workspace -> (durations [B, L], guards untouched)."""
    dev = q.device
    A, B, T = q.shape
    L = k.shape[2]
    n = _lib.load().evmi_align_durations_ws_bytes(B, T, L)
    dbuf = torch.full((GUARD + B * L + GUARD,), -7, dtype=torch.int32, device=dev)
    wbuf = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    dur, ws = dbuf[GUARD : GUARD + B * L].view(B, L), wbuf[GUARD : GUARD + n]
    assert ws.data_ptr() % 16 == 0
    tl, ml = i32(text_lens, dev), i32(mel_lens, dev)
    rc = _lib.load().evmi_align_durations_f32(q.data_ptr(), k.data_ptr(), prior.data_ptr(), tl.data_ptr(), ml.data_ptr(),
                                              dur.data_ptr(), ws.data_ptr(), n, A, B, T, L, temperature, _lib.current_stream_ptr(dev))
    assert rc == _lib.EVMI_OK, _lib.load().evmi_last_error()
    torch.cuda.synchronize(dev)
    untouched = bool((dbuf[:GUARD] == -7).all() and (dbuf[GUARD + B * L :] == -7).all() and (wbuf[:GUARD] == 0xA5).all()
                     and (wbuf[GUARD + n :] == 0xA5).all())
    return dur.cpu().to(torch.int64), untouched


def test_ragged_batch_rows_equal_the_items_alone(cuda_device):
    """NaN in every padded region of q, k and prior, sentinels around the durations and the workspace: each row is bit for bit the item run
    alone (the same q / k bits go in), zero beyond its tokens; the item with fewer frames than tokens gets zeros."""
    q, k, prior, items = _ragged_inputs(cuda_device)
    got, untouched = _guarded_call(q, k, prior, [Lb for Lb, _ in RAGGED], [Tb for _, Tb in RAGGED], 0.05)
    assert untouched
    for b, (Lb, Tb) in enumerate(RAGGED):
        if Tb < Lb:
            assert not got[b].any()
            continue
        alone = fused(items[b], cuda_device)
        assert torch.equal(got[b, :Lb], alone) and not got[b, Lb:].any(), b
        assert torch.equal(alone, torch.from_numpy(R.planted_case(Lb, Tb)[2])), b


def test_ragged_batch_clamps_lengths_and_zeroes_empty_items(cuda_device):
    """Lengths outside [0, L] / [0, T] are clamped (the padding must then hold numbers: item 2 is the full rectangle); a zero-length or
    zero-frame item gets a row of zeros."""
    q, k, prior, items = _ragged_inputs(cuda_device)
    got, untouched = _guarded_call(q, k, prior, [0, 37, 10_000, 64, -3], [3, -5, 10_000, 0, 20], 0.05)
    assert untouched
    assert not got[0].any() and not got[1].any() and not got[3].any() and not got[4].any()
    assert torch.equal(got[2], fused(items[2], cuda_device))


def test_captured_call_follows_the_lengths_in_device_memory(cuda_device):
    from everyvoice_amd.train import ops

    dev = cuda_device
    q, k, prior, items = _ragged_inputs(dev)
    q, k, prior = torch.nan_to_num(q), torch.nan_to_num(k), torch.nan_to_num(prior, nan=0.5)  # shorter lengths than the padding are tried
    B = len(RAGGED)
    first, second = ([1, 37, 150, 64, 50], [3, 221, 907, 64, 20]), ([1, 30, 100, 10, 20], [2, 200, 600, 64, 50])
    tl, ml = i32(first[0], dev), i32(first[1], dev)
    out = torch.full((B, L_PAD), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(ops.align_durations_ws_bytes(B, T_PAD, L_PAD), dtype=torch.uint8, device=dev)
    eager = [ops.align_durations(q, k, prior, i32(t, dev), i32(m, dev), 0.05).cpu() for t, m in (first, second)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.align_durations(q, k, prior, tl, ml, 0.05, out=out, ws=ws)
    for (t, m), want in zip((first, second, first), (eager[0], eager[1], eager[0])):
        tl.copy_(i32(t, dev))
        ml.copy_(i32(m, dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out.cpu(), want)
    assert not torch.equal(eager[0], eager[1]) and eager[1].sum(1).tolist() == second[1]


# =====================================================================================================================
# the model
# =====================================================================================================================
def _model(dev, width=256, aligner=True, seed=11):
    from everyvoice_amd.fs2 import ConformerConfig, FastSpeech2, FastSpeech2ModelConfig, VariancePredictorConfig, VariancePredictors

    if width == 256:
        c = FastSpeech2ModelConfig()
    else:
        vp = lambda: VariancePredictorConfig(input_dim=width)  # noqa: E731
        c = FastSpeech2ModelConfig(encoder=ConformerConfig(layers=2, input_dim=width, feedforward_dim=2 * width),
                                   decoder=ConformerConfig(layers=2, input_dim=width, feedforward_dim=2 * width),
                                   variance_predictors=VariancePredictors(energy=vp(), duration=vp(), pitch=vp()))
    return FastSpeech2(c, device=dev).init_random(seed, aligner=aligner)


@pytest.fixture(scope="module")
def default_model(cuda_device):
    return _model(cuda_device)


def _utterances(seed=5):
    g = torch.Generator().manual_seed(seed)
    lens, mel_lens = torch.tensor([40, 23, 31]), torch.tensor([240, 150, 200])
    ids = torch.zeros(3, 40, dtype=torch.long)
    for b in range(3):
        ids[b, : lens[b]] = torch.randint(1, 80, (int(lens[b]),), generator=g)
    mel = torch.randn(3, 240, 80, generator=g)
    return ids, lens, mel, mel_lens


def _oracle_values(model, ids, lens, mel, mel_lens):
    """Per item: (value [T_b, L_b] float64 from the oracle's aligner run in float64 on the model's weights, optimum, max |Q|)."""
    from oracle.alignment_ref import AlignerRef
    from oracle.attention_prior_ref import attention_prior_ref

    c = model.config
    ref = AlignerRef(c.encoder.input_dim, c.n_mels).double()
    ref.load_state_dict({name[len("attention."):]: t.cpu().double() for name, t in model.aligner.items()})
    pad = torch.arange(ids.shape[1])[None, :] >= lens[:, None]
    emb = model.table.cpu().double()[ids].masked_fill(pad[:, :, None], 0.0).transpose(1, 2)  # [B, D, L]
    frames = mel.double().masked_fill((torch.arange(mel.shape[1])[None, :] >= mel_lens[:, None])[:, :, None], 0.0).transpose(1, 2)
    with torch.no_grad():
        q, k = ref.query_proj(frames).numpy(), ref.key_proj(emb).numpy()
    out = []
    for b in range(ids.shape[0]):
        Lb, Tb = int(lens[b]), int(mel_lens[b])
        value = R.cell_values(q[b][:, :Tb], k[b][:, :Lb], ref.temperature, attention_prior_ref(Tb, Lb))
        out.append((value, *R.maximum_path_f64(value, Tb, Lb)))
    return out


def _check_against_oracle(model):
    ids, lens, mel, mel_lens = _utterances()
    refs = _oracle_values(model, ids, lens, mel, mel_lens)
    batch = model.align(ids, lens, mel, mel_lens).cpu()
    assert batch.dtype == torch.int64 and tuple(batch.shape) == tuple(ids.shape)
    for b, (value, optimum, q_max) in enumerate(refs):
        Lb, Tb = int(lens[b]), int(mel_lens[b])
        alone = model.align(ids[b : b + 1, :Lb], lens[b : b + 1], mel[b : b + 1, :Tb], mel_lens[b : b + 1]).cpu()[0]
        for what, got in (("batch", batch[b].numpy()), ("alone", alone.numpy())):
            assert R.structure_ok(got, Tb, Lb), (what, b, got)
            gap = R.path_score(value, optimum[:Lb]) - R.path_score(value, got[:Lb])
            print(f"item {b} {what}: optimum - returned = {gap:.3e}, bound {R.score_bound(Tb, q_max):.3e}")
            assert gap <= R.score_bound(Tb, q_max), (what, b, gap)


def test_model_align_against_the_oracle_in_float64(default_model):
    assert default_model.has_aligner
    _check_against_oracle(default_model)


def test_model_align_at_encoder_width_128(cuda_device):
    _check_against_oracle(_model(cuda_device, width=128))


def test_model_align_in_bf16_mode_is_the_fp32_one(cuda_device, default_model):
    """The projections run in fp32 in both precision modes."""
    from everyvoice_amd.fs2 import FastSpeech2

    ids, lens, mel, mel_lens = _utterances()
    bf = FastSpeech2(default_model.config, device=cuda_device, precision="bf16").init_random(11, aligner=True)
    assert torch.equal(bf.align(ids, lens, mel, mel_lens), default_model.align(ids, lens, mel, mel_lens))


def test_model_align_refusals(cuda_device, default_model):
    ids, lens, mel, mel_lens = _utterances()
    plain = _model(cuda_device, width=128, aligner=False)
    assert not plain.has_aligner
    with pytest.raises(ValueError, match="no aligner"):
        plain.align(ids, lens, mel, mel_lens)
    with pytest.raises(ValueError, match="mel"):
        default_model.align(ids, lens, mel[:, :, :79], mel_lens)
    with pytest.raises(ValueError, match="mel"):
        default_model.align(ids, lens, mel[0], mel_lens)
    with pytest.raises(ValueError, match="item 1"):
        default_model.align(ids, lens, mel, torch.tensor([240, 22, 200]))


# =====================================================================================================================
# teacher-forced synthesis
# =====================================================================================================================
def _preprocessed(tmp_path, n_mels=80):
    g = torch.Generator().manual_seed(3)
    rows, frames = [], {}
    for i, (n_sym, n_frm) in enumerate([(12, 70), (20, 131), (7, 33)]):
        base = f"utt{i}"
        rows.append({"basename": base, "ids": torch.randint(1, 80, (n_sym,), generator=g).tolist(), "speaker": "default", "language": "default"})
        path = tmp_path / "spec" / f"{base}--default--default--spec-22050-mel-librosa.pt"
        path.parent.mkdir(parents=True, exist_ok=True)
        torch.save(torch.randn(n_mels, n_frm, generator=g), path)
        frames[base] = n_frm
    return rows, frames


def test_teacher_forced_specs_without_duration_files(tmp_path, default_model):
    from everyvoice_amd.pipeline import generate_teacher_forced_specs

    rows, frames = _preprocessed(tmp_path)
    assert not (tmp_path / "duration").exists()
    preds = generate_teacher_forced_specs(default_model, rows, tmp_path, batch_size=2, write_durations=True)
    specs = {}
    for p in preds:
        specs[p["basename"]] = torch.load(p["spec"], weights_only=True)
        assert specs[p["basename"]].shape == (80, frames[p["basename"]]) and p["frames"] == frames[p["basename"]]
        d = torch.load(tmp_path / "duration" / f"{p['basename']}--default--default--duration.pt", weights_only=True)
        assert int(d.sum()) == frames[p["basename"]] and d.shape[0] == len(rows[int(p["basename"][3:])]["ids"]) and bool((d >= 1).all())
    again = generate_teacher_forced_specs(default_model, rows, tmp_path, batch_size=2)  # (now from the duration files)
    for p in again:
        assert torch.equal(torch.load(p["spec"], weights_only=True), specs[p["basename"]])


def test_teacher_forcing_without_durations_or_aligner_names_both_files(tmp_path, cuda_device, default_model):
    from everyvoice_amd.pipeline import generate_teacher_forced_specs

    rows, _ = _preprocessed(tmp_path)
    with pytest.raises(FileNotFoundError) as e:
        generate_teacher_forced_specs(_model(cuda_device, width=128, aligner=False), rows, tmp_path)
    assert "utt0--default--default--duration.pt" in str(e.value) and "utt0--default--default--spec-22050-mel-librosa.pt" in str(e.value)
    (tmp_path / "spec" / "utt1--default--default--spec-22050-mel-librosa.pt").unlink()   # a model with an aligner and no spectrogram
    with pytest.raises(FileNotFoundError) as e:
        generate_teacher_forced_specs(default_model, rows, tmp_path)
    assert "utt1--default--default--duration.pt" in str(e.value) and "utt1--default--default--spec-22050-mel-librosa.pt" in str(e.value)
