"""The stand-alone pieces of the FastSpeech2 training step on the device: the tape operators of the embeddings, the length regulator
and the positional term against torch autograd, and a SideBranch on its stream against the same chain inline.

The operators' inputs and upstream gradients are small integers stored as fp32, so every sum is exact in any order and the comparisons
are ``torch.equal``.  The positional sinusoid is no integer: its reference is the kernel's own term on a zero tensor (0 + s = s exactly;
the term itself is pinned by the model's parity tests), added by torch -- one rounding, as in the kernels.  Shapes: two items of unequal
length (a padded tail), L = 5 and T = 9 (multiples of nothing), D = 2 (the embedding kernel wants an even D), tables of four rows with
repeated indices."""

import pytest
import torch

pytestmark = pytest.mark.gpu

D, B, L, T, ROWS = 2, 2, 5, 9, 4


@pytest.fixture(scope="module")
def dev(cuda_device):
    return torch.device(cuda_device)


def _ints(gen, *shape, lo=-3, hi=4):
    return torch.randint(lo, hi, shape, generator=gen).float()


class _Fix:
    """The inputs every operator test shares (made once, never written)."""

    def __init__(self, dev):
        from everyvoice_amd.train import fs2 as tfs2
        from everyvoice_amd.train.layers import ParamGroup

        gen = torch.Generator().manual_seed(5)
        self.dev = dev
        self.lens = torch.tensor([5, 3], dtype=torch.int32, device=dev)
        dur = torch.tensor([[2, 1, 3, 1, 2], [3, 2, 1, 0, 0]], dtype=torch.int32, device=dev)
        self.cum = torch.cumsum(dur, 1, dtype=torch.int32).contiguous()
        self.mel_lens = dur.sum(1).to(torch.int32).contiguous()  # [9, 6]
        self.ids = torch.tensor([[1, 3, 1, 0, 2], [3, 3, 2, 0, 0]], dtype=torch.int32, device=dev)  # (0 inside an item: the padding row)
        self.inv_freq = (1.0 / (10000 ** (torch.arange(0.0, D, 2.0) / D))).to(dev)
        g = self.group = ParamGroup(dev)
        self.table = tfs2.Table(g, "table.weight", ROWS, D)
        self.linear = tfs2.Dense(g, "text_input_layer.weight", None, 43, D, linear=True)
        g.finalize()
        self.table_w, self.linear_w = _ints(gen, ROWS, D).to(dev), _ints(gen, D, 43).to(dev)
        g.load("table.weight", self.table_w)
        g.load("text_input_layer.weight", self.linear_w)
        self.feats = torch.randint(0, 2, (43, B, L), generator=gen).float().to(dev)
        self.x, self.dy_l, self.dy_t = _ints(gen, D, B, L).to(dev), _ints(gen, D, B, L).to(dev), _ints(gen, D, B, T).to(dev)
        self.h = _ints(gen, D, B, T).to(dev)
        self.style = _ints(gen, B, D).to(dev)
        self.values = torch.randint(0, ROWS, (B, L), generator=gen).float().to(dev)
        self.bins = torch.tensor([0.5, 1.5, 2.5], device=dev)
        self.valid_l = (torch.arange(L, device=dev)[None, :] < self.lens[:, None]).float()      # [B, L]
        self.valid_t = (torch.arange(T, device=dev)[None, :] < self.mel_lens[:, None]).float()  # [B, T]
        self.pos_l = tfs2._add_posemb_(torch.zeros(D, B, L, device=dev), self.lens, self.inv_freq)
        self.pos_t = tfs2._add_posemb_(torch.zeros(D, B, T, device=dev), self.mel_lens, self.inv_freq)


@pytest.fixture(scope="module")
def fx(dev):
    return _Fix(dev)


def _run(fx, build, dy):
    """-> (output, the Var's tape after backward from `dy`); the group's gradients are zeroed first."""
    from everyvoice_amd.train.autograd import Tape

    fx.group.zero_grad()
    tape = Tape()
    y = build(tape)
    out = y.data.clone()
    y.grad = dy.clone()
    tape.backward()
    torch.cuda.synchronize(fx.dev)
    return out


def _leaf(t):
    return t.clone().requires_grad_(True)


@pytest.mark.parametrize("position", [False, True])
def test_text_embedding_of_symbol_ids(fx, position):
    from everyvoice_amd.train import fs2 as tfs2

    out = _run(fx, lambda tape: tfs2.embed_text(tape, fx.ids, fx.lens, fx.table, fx.inv_freq if position else None), fx.dy_l)
    w = _leaf(fx.table_w)
    ref = torch.nn.functional.embedding(fx.ids.long(), w, padding_idx=0).permute(2, 0, 1) * fx.valid_l
    if position:
        ref = ref + fx.pos_l
    ref.backward(fx.dy_l)
    assert torch.equal(out, ref.detach())
    assert torch.equal(fx.table.grad(), w.grad)


@pytest.mark.parametrize("position", [False, True])
def test_text_embedding_of_phonological_features(fx, position):
    from everyvoice_amd.train import fs2 as tfs2

    out = _run(fx, lambda tape: tfs2.embed_text(tape, fx.feats, fx.lens, fx.linear, fx.inv_freq if position else None), fx.dy_l)
    w = _leaf(fx.linear_w)
    ref = torch.einsum("dc,cbl->dbl", w, fx.feats) * fx.valid_l
    if position:
        ref = ref + fx.pos_l
    ref.backward(fx.dy_l)
    assert torch.equal(out, ref.detach())
    assert torch.equal(fx.linear.effective()[1].view(D, 43), w.grad)


def test_item_embedding_of_a_table(fx):
    from everyvoice_amd.train import fs2 as tfs2
    from everyvoice_amd.train.autograd import Var

    items = torch.tensor([2, 2], dtype=torch.int32, device=fx.dev)  # (both items in one row: their gradients collide)
    x = Var(fx.x)
    out = _run(fx, lambda tape: tfs2.add_item_embedding(tape, x, items, fx.lens, fx.table.data(), fx.table.grad()), fx.dy_l)
    xr, w = _leaf(fx.x), _leaf(fx.table_w)
    ref = xr + w[items.long()].t()[:, :, None] * fx.valid_l
    ref.backward(fx.dy_l)
    assert torch.equal(out, ref.detach()) and torch.equal(x.grad, xr.grad) and torch.equal(fx.table.grad(), w.grad)


def test_item_embedding_of_the_style_matrix(fx):
    from everyvoice_amd.train import fs2 as tfs2
    from everyvoice_amd.train.autograd import Var

    rows = torch.arange(B, device=fx.dev, dtype=torch.int32)
    x, style = Var(fx.x), Var(fx.style)
    out = _run(fx, lambda tape: tfs2.add_item_embedding(tape, x, rows, fx.lens, style.data, style), fx.dy_l)
    xr, sr = _leaf(fx.x), _leaf(fx.style)
    ref = xr + sr.t()[:, :, None] * fx.valid_l
    ref.backward(fx.dy_l)
    assert torch.equal(out, ref.detach()) and torch.equal(x.grad, xr.grad) and torch.equal(style.grad, sr.grad)
    assert not fx.group.grad.any()  # (the sink is the Var: no parameter gradient is touched)


def test_bucket_embedding(fx):
    from everyvoice_amd.train import fs2 as tfs2
    from everyvoice_amd.train.autograd import Var

    x = Var(fx.x)
    out = _run(fx, lambda tape: tfs2.add_bucket_embedding(tape, x, fx.values, fx.bins, fx.table), fx.dy_l)
    xr, w = _leaf(fx.x), _leaf(fx.table_w)
    ref = xr + w[torch.bucketize(fx.values, fx.bins)].permute(2, 0, 1)  # (every position, padded ones included)
    ref.backward(fx.dy_l)
    assert torch.equal(out, ref.detach()) and torch.equal(x.grad, xr.grad) and torch.equal(fx.table.grad(), w.grad)


@pytest.mark.parametrize("position", [False, True])
def test_length_regulator(fx, position):
    from everyvoice_amd.train import fs2 as tfs2
    from everyvoice_amd.train.autograd import Var

    x = Var(fx.x)
    out = _run(fx, lambda tape: tfs2.length_regulate(tape, x, fx.cum, fx.mel_lens, T, fx.inv_freq if position else None), fx.dy_t)
    xr = _leaf(fx.x)
    t = torch.arange(T, device=fx.dev)
    symbol = torch.searchsorted(fx.cum.long(), t[None, :].expand(B, T).contiguous(), right=True).clamp_max(L - 1)  # first l with cum[l] > t
    ref = xr.gather(2, symbol[None].expand(D, B, T)) * fx.valid_t
    if position:
        ref = ref + fx.pos_t
    ref.backward(fx.dy_t)
    assert torch.equal(out, ref.detach()) and torch.equal(x.grad, xr.grad)


def test_positional_term_in_place(fx):
    from everyvoice_amd.train import fs2 as tfs2
    from everyvoice_amd.train.autograd import Var

    h = Var(fx.h.clone())
    out = _run(fx, lambda tape: tfs2.add_position_(tape, h, fx.mel_lens, fx.inv_freq), fx.dy_t)
    hr = _leaf(fx.h)
    ref = hr * fx.valid_t + fx.pos_t
    ref.backward(fx.dy_t)
    assert torch.equal(out, ref.detach()) and torch.equal(h.data, out) and torch.equal(h.grad, hr.grad)


def test_a_branch_on_its_stream_leaves_the_bits_of_the_chain_inline_eager_and_captured(dev):
    """dense -> [branch: silu -> dense, on an alias] / [chain: dense -> silu], backward through the alias: the branch inline, on its
    stream, and on its stream inside a graph capture (which ends in an error if a forked stream is not joined)."""
    from everyvoice_amd.train import fs2 as tfs2
    from everyvoice_amd.train import ops
    from everyvoice_amd.train.autograd import Tape, Var
    from everyvoice_amd.train.layers import ParamGroup
    from everyvoice_amd.train.step import SideBranch

    C, Bb, Tt = 8, 2, 64
    gen = torch.Generator().manual_seed(3)
    g = ParamGroup(dev)
    layers = [tfs2.Dense(g, f"l{i}.weight", f"l{i}.bias", C, C) for i in range(3)]
    g.finalize()
    for i in range(3):
        g.load(f"l{i}.weight", torch.randn(C, C, 1, generator=gen))
        g.load(f"l{i}.bias", torch.randn(C, generator=gen))
    x_data, dy, dz = (torch.randn(C, Bb, Tt, generator=gen).to(dev) for _ in range(3))
    stream, branch = torch.cuda.Stream(dev), SideBranch(dev)

    def chain(enabled):
        g.zero_grad()
        tape = Tape()
        branch.begin(enabled)
        x = Var(x_data)
        h = tfs2.dense(tape, x, layers[0], ops.ACT_RELU)
        a = tfs2.joined_alias(tape, branch, h)
        z = branch.fork(lambda: tfs2.dense(branch.tape, tfs2.silu(branch.tape, a), layers[1]), done=False)
        y = tfs2.silu(tape, tfs2.dense(tape, h, layers[2]))
        y.grad, z.grad = dy, dz
        branch.backward()
        tape.backward()
        branch.close()
        branch.hand_over(z.data)
        assert branch._pending is None and branch.kept == [] and not branch.tape._ops
        return [y.data, z.data, x.grad, g.grad.clone()]

    def eager(enabled):
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            out = chain(enabled)
        torch.cuda.synchronize(dev)
        return [t.clone() for t in out]

    inline, on_stream = eager(False), eager(True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        static = chain(True)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert inline[2].abs().sum() > 0 and inline[3].abs().sum() > 0
    for want, got_eager, got_graph in zip(inline, on_stream, static):
        assert torch.equal(want, got_eager) and torch.equal(want, got_graph)
