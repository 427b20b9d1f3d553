"""``model.mask_padding`` restated on top of the oracle's own modules, in torch.

Inside ``with masked_padding(model):`` every layer of an ``oracle.fs2_ref.FastSpeech2Ref`` whose output at a column depends on other
columns takes the columns at or beyond an item's length as absent:
  * the depthwise convolution of every Conformer convolution module reads zero there, and its BatchNorm takes its statistics (training
    mode) over the valid columns only and is zero beyond them;
  * every convolution of the three variance predictors reads zero there (layer 0 included);
  * every postnet convolution reads zero there; its BatchNorm as above.
Columns are removed by a select, never by a multiplication.  The lengths are the ones the oracle itself passes around: ``lengths`` of a
``ConformerRef`` call, the complement of a predictor's padding mask, and for the postnet (which gets no lengths) those of the decoder
call in front of it.  Nothing else is touched: ``FastSpeech2Ref.forward`` and ``training_losses_ref`` run as they are, in fp32 or, after
``model.double()``, in fp64; autograd goes through."""

import torch
from gst_masked_ref import masked_batchnorm
from torch import nn

from oracle.fs2_ref import ConformerRef, FastSpeech2Ref, PostNetRef, VariancePredictorRef, randomize_norm_stats_


class masked_padding:
    def __init__(self, model: nn.Module):
        self.model, self.lens, self._handles, self._swapped = model, None, [], []

    def _valid(self, T):  # [B, 1, T]
        return (torch.arange(T)[None, :] < self.lens[:, None])[:, None, :]

    def _zero_input(self, module, args):  # x [B, C, T]
        x = args[0]
        return (torch.where(self._valid(x.shape[2]), x, torch.zeros((), dtype=x.dtype)),) + tuple(args[1:])

    def _set_conformer_lens(self, module, args):
        self.lens = args[1]

    def _set_predictor_lens(self, module, args):
        self.lens = (~args[1]).sum(1)

    def _swap_batchnorm(self, bn):
        bn.forward = lambda x: masked_batchnorm(bn, x, self._valid(x.shape[2]), act=None)
        self._swapped.append(bn)

    def __enter__(self):
        pre = lambda m, fn: self._handles.append(m.register_forward_pre_hook(fn))
        for m in self.model.modules():
            if isinstance(m, ConformerRef):
                pre(m, self._set_conformer_lens)
                for layer in m.conformer_layers:
                    pre(layer.conv_module.sequential[2], self._zero_input)
                    self._swap_batchnorm(layer.conv_module.sequential[3])
            elif isinstance(m, VariancePredictorRef):
                pre(m, self._set_predictor_lens)
                for conv in m.convs:
                    pre(conv, self._zero_input)
            elif isinstance(m, PostNetRef):
                for seq in m.convolutions:
                    pre(seq[0], self._zero_input)
                    self._swap_batchnorm(seq[1])
        return self.model

    def __exit__(self, *exc):
        for h in self._handles:
            h.remove()
        for bn in self._swapped:
            del bn.forward  # (the instance attribute: the class's forward is back)
        self._handles, self._swapped = [], []
        return False


def solo(ids, lens, b, **per_item):
    """Item ``b`` of a batch as a batch of its own, trimmed to its length: (ids [1, n], lens [1], keyword tensors trimmed alike)."""
    n = int(lens[b])
    return ids[b : b + 1, :n], lens[b : b + 1], {k: (v[b : b + 1, :n] if v.dim() > 1 else v[b : b + 1]) for k, v in per_item.items() if v is not None}


# ---- what the tests of the flag share ----------------------------------------------------------------------------------------------
def oracle_model(ref_cfg, seed=3):
    """The setup of tests/test_gpu_fs2.py's ``_models``, without the product."""
    torch.manual_seed(seed)
    ref = FastSpeech2Ref(ref_cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    randomize_norm_stats_(ref, g)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return ref


def ragged_batch(n_symbols, lens, seed, lo=1, hi=6):
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(lens)
    B, L = len(lens), int(lens.max())
    pad = torch.arange(L)[None] >= lens[:, None]
    ids = torch.randint(1, n_symbols, (B, L), generator=g).masked_fill(pad, 0)
    durs = torch.randint(lo, hi, (B, L), generator=g).masked_fill(pad, 0)
    return ids, lens, durs


def item_differences(batch_out, solo_outs, lens):
    """Per item: max |batch - solo| / max |solo| of (mel, postnet mel, pitch, energy) over the item's own extent (the solo tensor's:
    symbols for a phone-level predictor, frames for a frame-level one); whatever the batch holds beyond it must be zero."""
    rows = []
    for b, solo in enumerate(solo_outs):
        row = []
        for i in (0, 1, 3, 4):
            want = solo[i][0].cpu()
            got = batch_out[i][b].cpu()
            assert not got[want.shape[0]:].any(), (b, i)
            row.append(float((got[: want.shape[0]] - want).abs().max() / (want.abs().max() + 1e-12)))
        rows.append(row)
    return rows
