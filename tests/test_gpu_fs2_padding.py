"""``model.mask_padding`` (csrc/fs2_lens_ops.hip, fs2.py, train/fs2.py): the two kernels alone, the inference model
against the oracle run on every item ALONE, and the training step against torch-CPU autograd of the masked restatement
tests/fs2_masked_ref.py (which tests/test_fs2_padding_host.py validates on the CPU).

Tolerances are the ones the unmasked tests of the same code use: test_gpu_fs2.py's 2e-4 (small) / 5e-4 (default) of a tensor's largest
entry in fp32 and 5e-2 in bf16; test_gpu_fs2_train.py's 2e-4 for an operator, and for the step 2e-4 (losses), 2e-3 (gradients, relative
L2), 1e-4 (BatchNorm statistics), in bf16 2e-2 / cosine 0.99 / norm within 5 %."""

import json

import pytest
import torch
import torch.nn.functional as F

from fs2_masked_ref import item_differences, masked_padding, oracle_model, ragged_batch, solo
from oracle.fs2_ref import FastSpeech2ConfigRef, FastSpeech2Ref, training_losses_ref
from tests.test_gpu_fs2 import _product_config
from tests.test_gpu_fs2_train import _l2close, _oracle_from, _ref_cfg, _shaped_batch, _trainer

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _close(got, want, rel, what=""):
    scale = float(want.abs().max()) + 1e-12
    err = float((got.cpu() - want).abs().max())
    print(f"{what}: err {err:.3e} / scale {scale:.3e} = {err / scale:.3e} (tolerance {rel:.0e})")
    assert err <= rel * scale, f"{what}: err {err:.3e} vs scale {scale:.3e}"


# ---- 1. the kernels alone --------------------------------------------------------------------------------------------------------------
# lengths below the reach of the k = 9 kernel (pad 4), equal to it, at T - 1, a full and an empty item; 300 columns: two 256-column tiles,
# six rows: a second workgroup with two idle waves
KERNEL_SHAPES = [(20, 6, 41, [41, 40, 5, 4, 1, 0]), (3, 2, 300, [300, 257])]


def _operands(C, B, T, k, lens, dev, seed):
    g = torch.Generator().manual_seed(seed)
    valid = (torch.arange(T)[None] < torch.tensor(lens)[:, None])[None].expand(C, B, T)
    mk = lambda: torch.randn(C, B, T, generator=g)
    x, dy = mk(), mk()
    nan, zero = (lambda t: torch.where(valid, t, torch.full((), NAN)).to(dev)), (lambda t: torch.where(valid, t, torch.zeros(())).to(dev))
    w, b = torch.randn(C, 1, k, generator=g), torch.randn(C, generator=g)
    return dict(x=x, dy=dy, x_nan=nan(x), x_zero=zero(x), dy_nan=nan(dy), dy_zero=zero(dy), w=w, b=b, valid=valid,
                lens=torch.tensor(lens, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("C,B,T,lens", KERNEL_SHAPES)
def test_forward_kernel_with_lengths(cuda_device, C, B, T, lens, k, act):
    from everyvoice_amd.fs2 import _dwconv

    o = _operands(C, B, T, k, lens, cuda_device, seed=k * 10 + act)
    w, b = o["w"].view(C, k).contiguous().to(cuda_device), o["b"].to(cuda_device)
    got = _dwconv(o["x_nan"], w, b, k, act, o["lens"]).cpu()
    want = _dwconv(o["x_zero"], w, b, k, act).cpu()
    valid = o["valid"]
    assert torch.isfinite(got).all()
    assert torch.equal(got[valid], want[valid])
    assert not got[~valid].any()
    # every length = T: the bits of the kernel it stands beside, on the raw input
    full = torch.full((B,), T, dtype=torch.int32, device=cuda_device)
    x = o["x"].to(cuda_device)
    assert torch.equal(_dwconv(x, w, b, k, act, full), _dwconv(x, w, b, k, act))
    # lengths outside [0, T] are clamped
    wild = torch.tensor([T + 7, -3] + [T] * (B - 2), dtype=torch.int32, device=cuda_device)
    clamped = torch.tensor([T, 0] + [T] * (B - 2), dtype=torch.int32, device=cuda_device)
    assert torch.equal(_dwconv(x, w, b, k, act, wild), _dwconv(x, w, b, k, act, clamped))


@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("C,B,T,lens", KERNEL_SHAPES)
def test_backward_kernel_with_lengths(cuda_device, C, B, T, lens, k):
    from everyvoice_amd.train import ops

    dev = cuda_device
    o = _operands(C, B, T, k, lens, dev, seed=k)
    w = o["w"].to(dev)
    dw, db = torch.zeros(C, 1, k, device=dev), torch.zeros(C, device=dev)
    dx = ops.dwconv_bwd(o["x_nan"], w, o["dy_nan"], dw, db, k, lens=o["lens"])
    dw0, db0 = torch.zeros_like(dw), torch.zeros_like(db)
    dx0 = ops.dwconv_bwd(o["x_zero"], w, o["dy_zero"], dw0, db0, k)
    torch.cuda.synchronize()
    valid = o["valid"]
    dx, dx0 = dx.cpu(), dx0.cpu()
    assert torch.isfinite(dx).all() and torch.equal(dx[valid], dx0[valid]) and not dx[~valid].any()
    # dw / db: float64 autograd of the masked operation
    v64 = valid.permute(1, 0, 2)
    x64 = torch.where(v64, o["x"].permute(1, 0, 2).double(), torch.zeros((), dtype=torch.float64))
    w64, b64 = o["w"].double().requires_grad_(), o["b"].double().requires_grad_()
    y = torch.where(v64, F.conv1d(x64, w64, b64, padding=(k - 1) // 2, groups=C), torch.zeros((), dtype=torch.float64))
    y.backward(torch.where(v64, o["dy"].permute(1, 0, 2).double(), torch.zeros((), dtype=torch.float64)))
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    _close(dw.double(), w64.grad, 2e-4, "dw")
    _close(db.double(), b64.grad, 2e-4, "db")
    # the dw-only call form (no dx) gives the same sums
    dw1, db1 = torch.zeros_like(dw), torch.zeros_like(db)
    assert ops.dwconv_bwd(o["x_nan"], w, o["dy_nan"], dw1, db1, k, need_dx=False, lens=o["lens"]) is None
    torch.cuda.synchronize()
    assert torch.equal(dw1, dw) and torch.equal(db1, db)
    # every length = T: dx carries the bits of the existing kernel
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    x, dy = o["x"].to(dev), o["dy"].to(dev)
    a = ops.dwconv_bwd(x, w, dy, torch.zeros_like(dw), torch.zeros_like(db), k, lens=full)
    b_ = ops.dwconv_bwd(x, w, dy, torch.zeros_like(dw), torch.zeros_like(db), k)
    torch.cuda.synchronize()
    assert torch.equal(a, b_)


# ---- 2. the inference model ------------------------------------------------------------------------------------------------------------
TOL = {("small", "f32"): 2e-4, ("default", "f32"): 5e-4, ("default", "bf16"): 5e-2}
NAMES = ("mel", "postnet mel", "pitch", "energy")


def _setup(name, precision, dev, mutate=None):
    """(oracle, product with the flag, product without it, oracle configuration): test_gpu_fs2.py's ``_models`` at seed 3; in bf16 with
    the smooth embedding tables of ``test_fs2_default_config_bf16_operands``.  ``mutate(ref_cfg)`` changes the configuration first."""
    from everyvoice_amd.fs2 import FastSpeech2

    ref_cfg = FastSpeech2ConfigRef.small() if name == "small" else FastSpeech2ConfigRef()
    if mutate is not None:
        mutate(ref_cfg)
    ref = oracle_model(ref_cfg, seed=3)
    if precision == "bf16":
        g = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for emb in (ref.pitch_embedding, ref.energy_embedding):
                n, d = emb.weight.shape
                emb.weight.copy_(torch.linspace(-1.0, 1.0, n)[:, None] * torch.randn(1, d, generator=g))
    models = []
    for flag in (True, False):
        cfg = _product_config(ref_cfg)
        cfg.mask_padding = flag
        models.append(FastSpeech2(cfg, device=dev, precision=precision).load_state_dict(ref.state_dict()))
    return ref, models[0], models[1], ref_cfg


def _inputs(name, ref_cfg, seed=11):
    return ragged_batch(ref_cfg.n_symbols, [12, 7, 5] if name == "small" else [40, 23], seed=seed)


def _alone(fn, ids, lens, **per_item):
    return [(lambda i, n, kw: fn(i, n, **kw))(*solo(ids, lens, b, **per_item)) for b in range(len(lens))]


def _check_items(out, alone, lens, tol, what):
    """Every item of the batch against its solo reference: integer outputs equal, the four tensors within ``tol``, zeros beyond."""
    out = [t.cpu() for t in out]
    assert torch.equal(out[5], torch.cat([a[5].cpu() for a in alone])), what
    for b, a in enumerate(alone):
        assert torch.equal(out[2][b, : int(lens[b])], a[2][0].cpu()) and not out[2][b, int(lens[b]):].any(), (what, b)
    diffs = item_differences(out, [[t.cpu() for t in a] for a in alone], lens)
    for b, row in enumerate(diffs):
        print(f"{what}: item {b} (mel, postnet mel, pitch, energy) = " + ", ".join(f"{v:.3e}" for v in row) + f" (tolerance {tol:.0e})")
    for b, row in enumerate(diffs):
        assert max(row) <= tol, (what, b, row)
    fpad = torch.arange(out[0].shape[1])[None, :] >= out[5][:, None]
    assert not out[0][fpad].any() and not out[1][fpad].any()
    return diffs


@pytest.mark.parametrize("name,precision", list(TOL))
def test_every_item_of_a_batch_is_the_oracle_on_that_item_alone(cuda_device, name, precision):
    ref, on, off, ref_cfg = _setup(name, precision, cuda_device)
    ids, lens, durs = _inputs(name, ref_cfg)
    tol = TOL[name, precision]
    alone = _alone(ref, ids, lens, durations=durs)
    # not vacuous: on these inputs the oracle's own batch differs from its solo runs by 1e-2 or more on every short item
    plain = item_differences(ref(ids, lens, durations=durs), alone, lens)
    print("oracle batch vs solo:", plain)
    assert all(min(row) >= 1e-2 for row in plain[1:]), plain
    _check_items(on(ids, lens, durations=durs), alone, lens, tol, f"{name} {precision} flag on")
    # ... and the product without the flag follows the oracle's batch, so it misses the solo tolerance there
    missed = item_differences([t.cpu() for t in off(ids, lens, durations=durs)], alone, lens)
    print("flag off vs solo:", missed)
    for row in missed[1:]:
        assert (min(row) if precision == "f32" else max(row)) > tol, missed


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_an_item_does_not_depend_on_its_neighbours_to_the_bit(cuda_device, precision):
    """Item 1 of [x0, x1, x2] and of [x0, x1, y2] (y2: another text of another length; x0 stays the longest, so the padded shape and
    every launch are the same).  Holds without the flag as well -- items never mix in inference, the flag is about an item's OWN
    padding -- which is asserted too, so that the claim is about masking and not about dispatch."""
    ref, on, off, ref_cfg = _setup("small", precision, cuda_device)
    ids, lens, durs = _inputs("small", ref_cfg)
    ids2, lens2, durs2 = ids.clone(), lens.clone(), durs.clone()
    g = torch.Generator().manual_seed(99)
    lens2[2] = 9
    ids2[2] = torch.randint(1, ref_cfg.n_symbols, (12,), generator=g).masked_fill(torch.arange(12) >= 9, 0)
    durs2[2] = torch.randint(1, 4, (12,), generator=g).masked_fill(torch.arange(12) >= 9, 0)
    assert int(durs2.sum(1).argmax()) == 0 == int(durs.sum(1).argmax()) and int(durs2[2].sum()) != int(durs[2].sum())
    for model in (on, off):
        a, b = model(ids, lens, durations=durs), model(ids2, lens2, durations=durs2)
        assert a[0].shape == b[0].shape
        for i in (0, 1, 3, 4):
            assert torch.equal(a[i][1], b[i][1]) and torch.equal(a[i][0], b[i][0]), (model.config.mask_padding, i)
        assert not torch.equal(a[1][2], b[1][2])


@pytest.mark.parametrize("name,precision", list(TOL))
def test_a_batch_against_the_products_own_solo_runs(cuda_device, name, precision):
    """Across shapes the dense layers pick tiles and K splits by problem size, so not to the bit: both sides are within the oracle
    tolerance of the same solo oracle run, hence within twice that of each other."""
    ref, on, off, ref_cfg = _setup(name, precision, cuda_device)
    ids, lens, durs = _inputs(name, ref_cfg)
    alone = _alone(on, ids, lens, durations=durs)
    _check_items(on(ids, lens, durations=durs), alone, lens, 2 * TOL[name, precision], f"{name} {precision} batch vs own solo")


def test_predicted_durations(cuda_device):
    """No ``durations=``: the duration predictor's own k = 3 convolutions are masked too, so every item gets the durations of its solo
    oracle run (checked where no value sits within 1e-3 of a rounding boundary, as test_fs2_small_predicted_durations_and_controls does)."""
    ref, on, off, ref_cfg = _setup("small", "f32", cuda_device)
    with torch.no_grad():
        ref.duration_predictor.linear.bias.fill_(1.2)  # durations of a few frames instead of 0
    on.load_state_dict(ref.state_dict())
    ids, lens, _ = _inputs("small", ref_cfg)
    kw = dict(duration_control=1.0, pitch_control=1.3, energy_control=0.8)
    alone = []
    for b in range(len(lens)):
        i, n, _ = solo(ids, lens, b)
        x = ref.text_input_layer(i) + ref.position_embedding(int(n))[None]
        x, _ = ref.encoder(x, n)
        raw = torch.exp(ref.duration_predictor(x, torch.zeros(1, int(n), dtype=torch.bool))) - 1.0
        assert ((raw - torch.floor(raw) - 0.5).abs() > 1e-3).all(), "test input sits on a rounding boundary: pick another seed"
        alone.append(ref(i, n, **kw))
    assert all(int(a[5]) > 0 for a in alone) and len({int(a[5]) for a in alone}) > 1
    _check_items(on(ids, lens, **kw), alone, lens, TOL["small", "f32"], "predicted durations")


def _frame_level(ref_cfg):
    ref_cfg.pitch.level = "frame"


def _dense_predictors(ref_cfg):
    ref_cfg.duration.depthwise = ref_cfg.pitch.depthwise = ref_cfg.energy.depthwise = False


@pytest.mark.parametrize("mutate,seed", [(_frame_level, 12), (_dense_predictors, 11)], ids=["pitch_level_frame", "depthwise_false"])
def test_other_predictor_configurations(cuda_device, mutate, seed):
    """A frame-level pitch predictor (masked with ``mel_lens`` on the regulated frames, which hold no zeros beyond the length once
    a bucket embedding has been added) and ``depthwise: false`` predictors (``evmi_mask_cols_f32`` in front of every k = 3 convolution):
    against the level-aware restatement tests/fs2_levels_ref.py run on every item alone (its guard: no frame-level value within 1e-3
    of a bin edge -- seed 11 has one)."""
    from fs2_levels_ref import forward_levels_ref

    ref, on, off, ref_cfg = _setup("small", "f32", cuda_device, mutate)
    ids, lens, durs = _inputs("small", ref_cfg, seed)
    fn = lambda i, n, **kw: forward_levels_ref(ref, i, n, guard=True, **kw)
    alone = _alone(fn, ids, lens, durations=durs)
    got = on(ids, lens, durations=durs)
    if ref_cfg.pitch.level == "frame":
        assert got[3].shape == got[0].shape[:2]  # [B, T]
    _check_items(got, alone, lens, 2e-4, "configuration")
    # the masked restatement on the batch says the same
    with masked_padding(ref):
        want = forward_levels_ref(ref, ids, lens, guard=True, durations=durs)
    for i in (0, 1, 3, 4):
        _close(got[i], want[i], 2e-4, f"batch against the masked restatement, {NAMES[i if i < 2 else i - 1]}")


def test_multispeaker_model_with_style_tokens(cuda_device):
    """Speaker embedding + Global Style Token module (both masked: ``gst_mask_padding`` with ``style_lens``): the oracle on every
    item alone, with the sum of the item's speaker row and its style embedding (tests/gst_ref.py on the reference alone) in the
    oracle's speaker slot."""
    from everyvoice_amd.fs2 import FastSpeech2
    from gst_ref import GSTRef, randomize_

    B = 3
    ref_cfg = FastSpeech2ConfigRef.small()
    ref_cfg.n_speakers = B
    ref = oracle_model(ref_cfg, seed=3)
    cfg = _product_config(ref_cfg)
    cfg.multispeaker, cfg.n_speakers, cfg.use_global_style_token_module, cfg.gst_mask_padding, cfg.mask_padding = True, 4, True, True, True
    torch.manual_seed(5)
    gst = randomize_(GSTRef(cfg.encoder.input_dim, cfg.n_mels, cfg.gst_num_heads, cfg.gst_num_tokens, cfg.gst_ref_enc_filters), torch.Generator().manual_seed(6)).eval()
    g = torch.Generator().manual_seed(7)
    table = torch.randn(4, cfg.encoder.input_dim, generator=g) * 0.3
    sd = dict(ref.state_dict())
    sd["speaker_embedding.weight"] = table
    sd.update({"gst." + k: v for k, v in gst.state_dict().items()})
    model = FastSpeech2(cfg, device=cuda_device).load_state_dict(sd)
    ids, lens, durs = _inputs("small", ref_cfg)
    speakers = torch.tensor([2, 0, 3])
    style_lens = torch.tensor([41, 23, 30])
    style_mel = torch.randn(B, 41, cfg.n_mels, generator=g)
    for b in range(B):
        style_mel[b, int(style_lens[b]):] = 0.0
    with torch.no_grad():
        ref.speaker_embedding.weight.copy_(torch.stack([table[speakers[b]] + gst(style_mel[b : b + 1, : int(style_lens[b])])[0] for b in range(B)]))
    alone = [ref(*solo(ids, lens, b)[:2], durations=durs[b : b + 1, : int(lens[b])], speakers=torch.tensor([b])) for b in range(B)]
    got = model(ids, lens, durations=durs, speakers=speakers, style_mel=style_mel, style_lens=style_lens)
    _check_items(got, alone, lens, 2e-4, "multispeaker + style tokens")


# ---- 3. training -----------------------------------------------------------------------------------------------------------------------
def _masked_trainer(ref_cfg, dev, mask=True, **kw):
    tr = _trainer(ref_cfg, dev, **kw)
    tr.config.mask_padding = mask  # (read at every step)
    return tr


def _ragged_train_batch(ref_cfg, lens, seed):
    ids, lens, durs = ragged_batch(ref_cfg.n_symbols, lens, seed, lo=0, hi=5)
    g = torch.Generator().manual_seed(seed + 1)
    durs[:, 0] += 1
    B, L = ids.shape
    mel_lens = durs.sum(1)
    T = int(mel_lens.max())
    mel = torch.randn(B, T, ref_cfg.n_mels, generator=g).masked_fill((torch.arange(T)[None] >= mel_lens[:, None])[..., None], 0.0)
    return dict(ids=ids, lens=lens, durations=durs, mel=mel, pitch=torch.randn(B, L, generator=g), energy=torch.randn(B, L, generator=g))


def _masked_oracle_step(tr, ref_cfg, batch):
    ref = _oracle_from(tr, ref_cfg)
    plain = {k: float(v) for k, v in training_losses_ref(ref, batch).items()}
    ref = _oracle_from(tr, ref_cfg)  # (the unmasked pass moved the running statistics)
    with masked_padding(ref):
        want = training_losses_ref(ref, batch)
        want["total"].backward()
    return ref, want, plain


def test_training_step_against_autograd_of_the_masked_restatement(cuda_device):
    """test_gpu_fs2_train.py's step test with the flag: every loss, every parameter gradient, the BatchNorm running statistics and the
    parameters after one clipped AdamW step."""
    ref_cfg = _ref_cfg(0.0, 0)
    tr = _masked_trainer(ref_cfg, cuda_device)
    batch = _ragged_train_batch(ref_cfg, [14, 9, 5], seed=14)
    ref, want, plain = _masked_oracle_step(tr, ref_cfg, batch)
    # the flag matters on this batch: the unmasked oracle's losses are elsewhere
    assert abs(plain["mel"] - float(want["mel"])) > 1e-3 * float(want["mel"]) and abs(plain["pitch"] - float(want["pitch"])) > 1e-3 * float(want["pitch"])
    got = tr.forward_backward(batch)
    for k, v in want.items():
        print(f"loss {k}: got {float(got[k]):.7f} want {float(v):.7f} (unmasked oracle {plain[k]:.7f})")
        assert float(got[k]) == pytest.approx(float(v), rel=2e-4), k
    grads = tr.params.gradients()
    named = dict(ref.named_parameters())
    assert set(grads) == set(named)
    for name, p in named.items():
        _l2close(grads[name], p.grad if p.grad is not None else torch.zeros_like(p), 2e-3, name)
    for name, buf in ref.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var"):
            _close(tr.state_dict()[name], buf, 1e-4, name)
    # one optimiser step: clip_grad_norm_(1.0) + AdamW at the Noam learning rate of step 1
    o = tr.training.optimizer
    noise = {n for n, p in named.items() if p.grad is None or float(p.grad.norm()) < 1e-5 * p.numel() ** 0.5}
    assert all(n.endswith(".bias") for n in noise) and len(noise) <= 2 * ref_cfg.encoder.layers + ref_cfg.postnet_layers
    torch.nn.utils.clip_grad_norm_(ref.parameters(), tr.training.gradient_clip_val)
    torch.optim.AdamW(ref.parameters(), lr=tr.learning_rate(1), betas=tuple(o.betas), eps=o.eps, weight_decay=o.weight_decay).step()
    tr2 = _masked_trainer(ref_cfg, cuda_device)
    tr2.training_step(batch)
    sd = tr2.state_dict()
    for name, p in ref.named_parameters():
        if name not in noise:
            diff = (sd[name].cpu() - p.detach()).abs()
            assert float((diff > 1e-6 + 2e-3 * tr.learning_rate(1)).float().mean()) < 0.01, name


def test_training_step_with_dense_predictors(cuda_device):
    """``depthwise: false``: the ``masked`` tape operator in front of every dense k = 3 convolution of the predictors -- losses and
    gradients of one fp32 step against autograd of the masked restatement."""
    ref_cfg = _ref_cfg(0.0, 0)
    _dense_predictors(ref_cfg)
    tr = _masked_trainer(ref_cfg, cuda_device)
    batch = _ragged_train_batch(ref_cfg, [14, 9, 5], seed=14)
    ref, want, plain = _masked_oracle_step(tr, ref_cfg, batch)
    assert abs(plain["pitch"] - float(want["pitch"])) > 1e-3 * float(want["pitch"])
    got = tr.forward_backward(batch)
    for k, v in want.items():
        assert float(got[k]) == pytest.approx(float(v), rel=2e-4), k
    grads = tr.params.gradients()
    named = dict(ref.named_parameters())
    assert set(grads) == set(named)
    for name, p in named.items():
        _l2close(grads[name], p.grad if p.grad is not None else torch.zeros_like(p), 2e-3, name)


def test_training_step_bf16_follows_the_masked_restatement(cuda_device):
    """precision="bf16" at test_gpu_fs2_train.py's bf16 tolerance: losses within 2e-2, the whole gradient within 5 % in norm and
    cosine >= 0.99 of the fp32 autograd of the masked restatement."""
    from everyvoice_amd.train import ops

    ref_cfg = _ref_cfg(0.0, 0)
    tr = _masked_trainer(ref_cfg, cuda_device, precision="bf16")
    batch = _ragged_train_batch(ref_cfg, [14, 9, 5], seed=14)
    ref, want, _ = _masked_oracle_step(tr, ref_cfg, batch)
    with ops.mode(operands="bf16"):
        got = tr.forward_backward(batch)
    for k, v in want.items():
        assert float(got[k]) == pytest.approx(float(v), rel=2e-2, abs=1e-4), k
    grads = tr.params.gradients()
    pairs = [(grads[n].cpu().double().flatten(), p.grad.double().flatten()) for n, p in ref.named_parameters() if p.grad is not None]
    g_, w_ = torch.cat([a for a, _ in pairs]), torch.cat([b for _, b in pairs])
    cos, ratio = float(torch.dot(g_, w_) / (g_.norm() * w_.norm())), float(g_.norm() / w_.norm())
    print(f"bf16 gradient: cosine {cos:.5f}, norm ratio {ratio:.4f}")
    assert cos >= 0.99 and 0.95 <= ratio <= 1.05, (cos, ratio)


def test_graph_replay_follows_each_batchs_lengths_bitwise(cuda_device):
    """use_graph=True: the step captured on one batch and replayed on two others of the same padded shape and other lengths is bit-equal
    to the eager step -- the kernels read the lengths from device memory."""
    ref_cfg = _ref_cfg(0.1, 0)
    eager, graph = (_masked_trainer(ref_cfg, cuda_device, use_graph=flag) for flag in (False, True))
    batches = [_shaped_batch(ref_cfg, seed, False, cuda_device) for seed in (5, 6, 7)]
    assert len({tuple(b["lens"].tolist()) for b in batches}) == 3 and len({tuple(b["durations"].sum(1).tolist()) for b in batches}) == 3
    used = []
    for step in range(6):
        b = batches[step % 3]
        le, lg = eager.training_step(b), graph.training_step(b)
        used.append(graph.last_step_was_graph)
        for k in le:
            assert torch.equal(le[k], lg[k]), (step, k, float(le[k]), float(lg[k]))
    assert graph._graph_failed is None and used == [False, False, True, True, True, True] and len(graph._graphs) == 1
    assert torch.equal(eager.params.flat, graph.params.flat) and torch.equal(eager.params.m, graph.params.m) and torch.equal(eager.params.v, graph.params.v)
    se, sg = eager.state_dict(), graph.state_dict()
    assert all(torch.equal(se[k], sg[k]) for k in se), "BatchNorm statistics / counters differ"


def test_flag_off_is_the_step_of_a_trainer_without_the_field(cuda_device):
    """mask_padding=False: the bits of a trainer whose configuration never heard of the field (it is deleted from the instance, so any
    read of it falls back to the class default and any masked launch would show as different bits)."""
    ref_cfg = _ref_cfg(0.1, 0)
    batches = [_shaped_batch(ref_cfg, seed, False, cuda_device) for seed in (5, 6)]
    off, old, on = _masked_trainer(ref_cfg, cuda_device, mask=False), _trainer(ref_cfg, cuda_device), _masked_trainer(ref_cfg, cuda_device)
    del old.config.__dict__["mask_padding"]
    for b in batches:
        lo, ll, _ = off.training_step(b), old.training_step(b), on.training_step(b)
        assert all(torch.equal(lo[k], ll[k]) for k in lo)
    assert torch.equal(off.params.flat, old.params.flat) and torch.equal(off.params.m, old.params.m)
    so, sl = off.state_dict(), old.state_dict()
    assert all(torch.equal(so[k], sl[k]) for k in so)
    assert not torch.equal(on.params.flat, off.params.flat)  # the batches have padding, so the flag does change the step


def test_checkpoint_carries_the_flag_into_the_inference_model(cuda_device):
    """A masked trainer's checkpoint builds a masked inference model: it agrees with the trainer's own weights loaded into a model
    with the flag set by hand, to the bit, and differs from one without it."""
    from everyvoice_amd.fs2 import FastSpeech2

    ref_cfg = _ref_cfg(0.1, 0)
    tr = _masked_trainer(ref_cfg, cuda_device)
    tr.training_step(_shaped_batch(ref_cfg, 5, False, cuda_device))
    ck = tr.checkpoint()
    json.dumps(ck["hyper_parameters"])
    assert ck["hyper_parameters"]["config"]["mask_padding"] is True
    model = FastSpeech2.from_checkpoint(ck, device=cuda_device)
    assert model.config.mask_padding is True and model.encoder.mask_padding and model.pitch_predictor.mask_padding
    ids, lens, durs = ragged_batch(ref_cfg.n_symbols, [12, 7, 5], seed=11)
    got = model(ids, lens, durations=durs)
    ck["hyper_parameters"]["config"].pop("mask_padding")  # a checkpoint from before the field: False
    old = FastSpeech2.from_checkpoint(ck, device=cuda_device)
    assert old.config.mask_padding is False
    assert not torch.equal(old(ids, lens, durations=durs)[1], got[1])
    # an item alone: within twice the oracle tolerance of the batch (section 2)
    alone = _alone(model, ids, lens, durations=durs)
    _check_items(got, alone, lens, 4e-4, "model from the checkpoint, batch vs own solo")
