"""FastSpeech2 at Conformer widths whose head dimension is none of 32 / 64 / 128, whole model against oracle/fs2_ref.py.

Two configurations built from ``FastSpeech2ConfigRef.small()``: input_dim 96 with 2 heads (head dimension 48: one and a half chunks of
the attention kernels' 32 channels) and input_dim 192 with 1 head (192: the fp32 backward shares a tile between two waves).  Neither
width is a power of two, so the dense layers, LayerNorm and the feed-forward chain run at widths the suite did not reach before.
Inference follows tests/test_gpu_fs2.py::test_fs2_small_given_durations, training
tests/test_gpu_fs2_train.py::test_training_step_losses_gradients_and_update, with their tolerances."""

import pytest
import torch

from oracle.fs2_ref import FastSpeech2ConfigRef, FastSpeech2Ref, randomize_norm_stats_, training_losses_ref
from tests.test_gpu_fs2 import _batch, _close, _models, _product_config
from tests.test_gpu_fs2_train import _l2close, _oracle_from, _train_batch, _trainer

pytestmark = pytest.mark.gpu

WIDTHS = [(96, 2, 192), (192, 1, 384)]  # (input_dim, heads, feedforward_dim)


def _ref_cfg(input_dim, heads, feedforward_dim, dropout=None):
    c = FastSpeech2ConfigRef.small()
    for conf in (c.encoder, c.decoder):
        conf.input_dim, conf.heads, conf.feedforward_dim = input_dim, heads, feedforward_dim
    for v in (c.duration, c.pitch, c.energy):
        v.input_dim = input_dim
    if dropout is not None:
        c.encoder.dropout = c.decoder.dropout = dropout
        c.duration.dropout = c.pitch.dropout = c.energy.dropout = dropout
    return c


@pytest.mark.parametrize("input_dim,heads,feedforward_dim", WIDTHS)
def test_fs2_inference_f32(cuda_device, input_dim, heads, feedforward_dim):
    from everyvoice_amd.fs2 import FastSpeech2

    ref_cfg = _ref_cfg(input_dim, heads, feedforward_dim)
    ref, model = _models(ref_cfg, cuda_device, seed=input_dim)
    B, L = 3, 12
    ids, lens, g = _batch(20, B, L, seed=7)
    durs = torch.randint(0, 6, (B, L), generator=g)
    durs[:, 0] += 1
    want = ref(ids, lens, durations=durs)
    got = model(ids, lens, durations=durs)
    assert torch.equal(got[2].cpu(), want[2])          # durations: integers, bit-exact
    assert torch.equal(got[5].cpu(), want[5])          # mel lengths
    for i in (3, 4, 0, 1):                             # pitch, energy, decoder mel, postnet mel
        _close(got[i].cpu(), want[i])
    fpad = torch.arange(got[1].shape[1])[None, :] >= want[5][:, None]  # padded frames are exactly zero
    assert float(got[1].cpu()[fpad].abs().sum()) == 0.0 and float(got[0].cpu()[fpad].abs().sum()) == 0.0
    # a checkpoint round trip: the configuration (widths included) and the state dict into a fresh model, the same output bits
    again = FastSpeech2.from_checkpoint(model.to_checkpoint(ref.state_dict()), device=cuda_device)
    assert again.config.encoder.input_dim == input_dim and again.config.decoder.heads == heads
    got2 = again(ids, lens, durations=durs)
    for a, b in zip(got, got2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("input_dim,heads,feedforward_dim", WIDTHS)
def test_fs2_inference_bf16_operands(cuda_device, input_dim, heads, feedforward_dim):
    """precision="bf16" against the fp32 oracle, 5e-2 of each tensor's scale, with bucket embeddings that are a smooth function of the
    bin (tests/test_gpu_fs2.py::test_fs2_default_config_bf16_operands says why)."""
    from everyvoice_amd.fs2 import FastSpeech2

    ref_cfg = _ref_cfg(input_dim, heads, feedforward_dim)
    torch.manual_seed(3)
    ref = FastSpeech2Ref(ref_cfg).eval()
    g = torch.Generator().manual_seed(4)
    randomize_norm_stats_(ref, g)
    with torch.no_grad():
        ramp = torch.linspace(-1.0, 1.0, ref_cfg.pitch.n_bins)[:, None]
        ref.pitch_embedding.weight.copy_(ramp * torch.randn(1, input_dim, generator=g))
        ref.energy_embedding.weight.copy_(ramp * torch.randn(1, input_dim, generator=g))
    model = FastSpeech2(_product_config(ref_cfg), device=cuda_device, precision="bf16").load_state_dict(ref.state_dict())
    B, L = 3, 12
    ids, lens, g = _batch(20, B, L, seed=7)
    durs = torch.randint(0, 6, (B, L), generator=g)
    durs[:, 0] += 1
    want = ref(ids, lens, durations=durs)
    got = model(ids, lens, durations=durs)
    assert torch.equal(got[2].cpu(), want[2]) and torch.equal(got[5].cpu(), want[5])
    for i in (3, 4, 0, 1):
        _close(got[i].cpu(), want[i], rel=5e-2)


@pytest.mark.parametrize("input_dim,heads,feedforward_dim", WIDTHS)
def test_fs2_training_step(cuda_device, input_dim, heads, feedforward_dim):
    """Losses (rel 2e-4) and every parameter's gradient (L2, rel 2e-3) of one step against autograd of the oracle in fp32; then the same
    step with bf16 operands against the fp32 one: losses rel 2e-2, the flat gradient cosine >= 0.99 and norm within 5 %."""
    from everyvoice_amd.train import ops

    ref_cfg = _ref_cfg(input_dim, heads, feedforward_dim, dropout=0.0)
    B, L = 3, 14
    tr = _trainer(ref_cfg, cuda_device)
    batch = _train_batch(ref_cfg, B, L, seed=L)
    ref = _oracle_from(tr, ref_cfg)
    want = training_losses_ref(ref, batch)
    want["total"].backward()
    got = tr.forward_backward(batch)
    for k, v in want.items():
        assert float(got[k]) == pytest.approx(float(v), rel=2e-4), k
    grads = tr.params.gradients()
    named = dict(ref.named_parameters())
    assert set(grads) == set(named)
    for name, p in named.items():
        _l2close(grads[name], p.grad if p.grad is not None else torch.zeros_like(p), 2e-3, name)
    g32 = tr.params.grad.clone().double()

    tr16 = _trainer(ref_cfg, cuda_device, precision="bf16")
    with ops.mode(operands="bf16"):  # what training_step does around forward_backward
        got16 = tr16.forward_backward(batch)
    for k, v in got.items():
        assert float(got16[k]) == pytest.approx(float(v), rel=2e-2, abs=1e-4), k
    g16 = tr16.params.grad.double()
    cos, ratio = float(torch.dot(g32, g16) / (g32.norm() * g16.norm())), float(g16.norm() / g32.norm())
    assert cos >= 0.99 and 0.95 <= ratio <= 1.05, (cos, ratio)
    assert float((g32 - g16).abs().max()) > 0.0  # the bf16 kernels did run
