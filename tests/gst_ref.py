"""torch.nn restatement of the Global Style Token module (arXiv 1803.09017; the layout KinglittleQ/GST-Tacotron and mozilla/TTS
share) -- a test helper, like ``tests/sox_oracle.py``: plain ``nn.Conv2d`` / ``nn.BatchNorm2d`` / ``nn.GRU``, three bias-free
``nn.Linear`` and one parameter, under the state-dict names ``everyvoice_amd.fs2.gst_state_dict_shapes`` lists.

``GSTRef(E, n_mels)(mel [B, T, n_mels]) -> style embedding [B, E]``.  The mel is consumed as given (zero padding included)."""

import torch
import torch.nn as nn
import torch.nn.functional as F


class ReferenceEncoderRef(nn.Module):
    def __init__(self, E=256, n_mels=80, filters=(32, 32, 64, 64, 128, 128)):
        super().__init__()
        chans = [1] + list(filters)
        self.convs = nn.ModuleList([nn.Conv2d(chans[i], chans[i + 1], kernel_size=3, stride=2, padding=1) for i in range(len(filters))])
        self.bns = nn.ModuleList([nn.BatchNorm2d(c, eps=1e-5, momentum=0.1) for c in filters])
        bins = n_mels
        for _ in filters:
            bins = (bins - 1) // 2 + 1
        self.gru = nn.GRU(input_size=filters[-1] * bins, hidden_size=E // 2, batch_first=True)

    def forward(self, mel):  # [B, T, n_mels]
        x = mel.unsqueeze(1)
        for conv, bn in zip(self.convs, self.bns):
            x = F.relu(bn(conv(x)))
        x = x.transpose(1, 2)  # [B, T', C, bins]
        x = x.reshape(x.shape[0], x.shape[1], -1)
        _, h = self.gru(x)
        return h[0]  # the last hidden state [B, E / 2]


class _TokenAttentionRef(nn.Module):
    def __init__(self, query_dim, key_dim, E, heads):
        super().__init__()
        self.heads, self.E = heads, E
        self.W_query = nn.Linear(query_dim, E, bias=False)
        self.W_key = nn.Linear(key_dim, E, bias=False)
        self.W_value = nn.Linear(key_dim, E, bias=False)

    def forward(self, query, tokens):  # [B, query_dim], [N, key_dim]
        B, N, h = query.shape[0], tokens.shape[0], self.heads
        d = self.E // h
        q = self.W_query(query).view(B, h, d)
        k = self.W_key(tokens).view(N, h, d)
        v = self.W_value(tokens).view(N, h, d)
        p = torch.softmax(torch.einsum("bhd,nhd->bhn", q, k) / d ** 0.5, dim=-1)
        return torch.einsum("bhn,nhd->bhd", p, v).reshape(B, self.E)  # heads concatenated


class StyleTokenLayerRef(nn.Module):
    def __init__(self, E=256, heads=8, tokens=10):
        super().__init__()
        self.embed = nn.Parameter(torch.randn(tokens, E // heads) * 0.5)
        self.attention = _TokenAttentionRef(E // 2, E // heads, E, heads)

    def forward(self, ref):
        return self.attention(ref, torch.tanh(self.embed))


class GSTRef(nn.Module):
    def __init__(self, E=256, n_mels=80, heads=8, tokens=10, filters=(32, 32, 64, 64, 128, 128)):
        super().__init__()
        self.encoder = ReferenceEncoderRef(E, n_mels, filters)
        self.stl = StyleTokenLayerRef(E, heads, tokens)

    def forward(self, mel):
        return self.stl(self.encoder(mel))


def randomize_(model: nn.Module, gen: torch.Generator):
    """Lively biases and non-trivial BatchNorm statistics / affine parameters (as ``oracle.fs2_ref.randomize_norm_stats_`` does for
    BatchNorm1d), so that eval-mode folding is exercised."""
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=gen) * 0.5 + 0.75)
                m.weight.copy_(torch.rand(m.num_features, generator=gen) * 0.5 + 0.75)
                m.bias.copy_(torch.randn(m.num_features, generator=gen) * 0.1)
        for n, p in model.named_parameters():
            if "bias" in n and "bns" not in n:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
    return model
