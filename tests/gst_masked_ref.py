"""Length-masked restatement of the Global Style Token module in plain torch, on the modules of
``tests/gst_ref.py`` -- a test helper.  Any dtype (the tests use float64), autograd throughout.

A reference with ``n`` valid frames inside ``T >= n`` rows: rows at or beyond ``n`` are absent whatever they hold (they are removed by a
select, never multiplied by zero, so NaN padding stays out of values and gradients).  Layer ``i`` maps ``n_i`` valid rows to
``n_{i+1} = (n_i - 1) // 2 + 1``; the convolution sees zero at rows >= n_i and writes zero at rows >= n_{i+1}; BatchNorm takes its
statistics over the valid positions of all items (count = sum_b n_{i+1}[b] * bins, running variance unbiased over that count) and is
zero at invalid positions; the GRU runs per item on the truncated sequence; the token attention is per item already."""

import torch
import torch.nn.functional as F


def valid_rows(n: torch.Tensor, layers: int):
    out = []
    for _ in range(layers):
        n = (n - 1) // 2 + 1
        out.append(n)
    return out


def row_mask(n: torch.Tensor, H: int) -> torch.Tensor:
    """[B, 1, H, 1] bool: row < n[b]."""
    return (torch.arange(H)[None, :] < n[:, None])[:, None, :, None]


def select(mask: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    return torch.where(mask, x, torch.zeros((), dtype=x.dtype))


def masked_batchnorm(bn, x: torch.Tensor, mask: torch.Tensor, act=F.relu) -> torch.Tensor:
    """x [B, C, H, W], mask [B, 1, H, 1] (or any shape broadcastable to x): the definition above.  Follows ``bn.training``; in training
    mode updates ``bn.running_mean`` / ``running_var`` / ``num_batches_tracked`` as ``nn.BatchNorm2d`` does."""
    m = mask.expand_as(x)
    shape = (1, -1) + (1,) * (x.dim() - 2)
    dims = [d for d in range(x.dim()) if d != 1]
    if bn.training:
        count = m[:, 0].sum().to(x.dtype)
        xs = select(m, x)
        mean = xs.sum(dims) / count
        var = select(m, (x - mean.view(shape)) ** 2).sum(dims) / count
        with torch.no_grad():
            bn.running_mean.mul_(1 - bn.momentum).add_(bn.momentum * mean.to(bn.running_mean.dtype))
            bn.running_var.mul_(1 - bn.momentum).add_(bn.momentum * (var * count / torch.clamp(count - 1, min=1)).to(bn.running_var.dtype))
            bn.num_batches_tracked += 1
    else:
        mean, var = bn.running_mean.to(x.dtype), bn.running_var.to(x.dtype)
    y = (x - mean.view(shape)) / torch.sqrt(var.view(shape) + bn.eps) * bn.weight.view(shape) + bn.bias.view(shape)
    return select(m, act(y) if act is not None else y)


def masked_encoder(enc, mel: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """``ReferenceEncoderRef`` on mel [B, T, n_mels] with lens [B] (int64, 1 <= lens <= T) -> the state after each item's last valid
    step [B, E / 2]."""
    n = lens.to(torch.int64)
    x = select(row_mask(n, mel.shape[1]), mel.unsqueeze(1))
    for conv, bn in zip(enc.convs, enc.bns):
        x = conv(x)
        n = (n - 1) // 2 + 1
        x = masked_batchnorm(bn, x, row_mask(n, x.shape[2]))
    x = x.transpose(1, 2)
    x = x.reshape(x.shape[0], x.shape[1], -1)
    return torch.cat([enc.gru(x[b : b + 1, : int(n[b])])[1][0] for b in range(x.shape[0])])


def masked_forward(gst, mel: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """``GSTRef`` with length masking -> style embeddings [B, E]."""
    return gst.stl(masked_encoder(gst.encoder, mel, lens))
