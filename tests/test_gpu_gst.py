"""Global Style Token module (csrc/gst.hip, fs2.StyleTokens, train/fs2._StyleTokensT) against torch: every kernel entry point against
torch autograd of the same operator (2e-4 of the reference tensor's largest magnitude, the project's operator bound), the module and the
whole model against ``tests/gst_ref.py`` + ``oracle/fs2_ref.py`` (the oracle is not edited: the reference module's style matrix takes the
place of its speaker embedding), the training step against torch-CPU autograd (4e-3 relative L2, the whole-step bound of
test_gpu_fs2_train.py), bitwise reproducibility / graph replay / checkpoints with the module on, and the synthesis front end."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from gst_ref import GSTRef, randomize_
from oracle.fs2_ref import FastSpeech2ConfigRef, FastSpeech2Ref, randomize_norm_stats_, training_losses_ref
from tests.test_gpu_fs2 import _product_config
from tests.test_gpu_fs2_train import _l2close, _ref_cfg, _shaped_batch, _train_batch

pytestmark = pytest.mark.gpu

LAYERS = [(1, 32, 80), (32, 32, 40), (32, 64, 20), (64, 64, 10), (64, 128, 5), (128, 128, 3)]  # (c_in, c_out, mel bins in) of the six layers


def _close(got, want, rel=2e-4, what=""):
    scale = float(want.abs().max()) + 1e-12
    err = float((got.cpu() - want).abs().max())
    print(f"{what}: err {err:.3e} scale {scale:.3e} ratio {err / scale:.2e}")
    assert err <= rel * scale, f"{what}: err {err:.3e} vs scale {scale:.3e}"


def _cm(x):  # [B, C, H, W] -> channel-major [C, B, H, W]
    return x.permute(1, 0, 2, 3).contiguous()


# ---- operators ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 17, 566, 947])
def test_conv2d_forward_input_gradient_weight_gradient(cuda_device, T, B):
    """All three entry points on the six layer shapes, at the frame count layer i sees for a T-frame reference."""
    from everyvoice_amd.train import ops

    dev = cuda_device
    g = torch.Generator().manual_seed(T * 10 + B)
    H = T
    for li, (cin, cout, W) in enumerate(LAYERS):
        x = torch.randn(B, cin, H, W, generator=g, requires_grad=True)
        w = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).requires_grad_()
        b = (torch.randn(cout, generator=g) * 0.1).requires_grad_()
        y = F.conv2d(x, w, b, stride=2, padding=1)
        OH, OW = ops.gst_conv_out(H), ops.gst_conv_out(W)
        assert y.shape == (B, cout, OH, OW)
        dy = torch.randn(y.shape, generator=g)
        y.backward(dy)
        xd, wd, bd, dyd = _cm(x.detach()).to(dev), w.detach().to(dev), b.detach().to(dev), _cm(dy).to(dev)
        tag = f"layer {li} T {T} B {B}"
        got = ops.gst_conv2d_fwd(xd, wd, bd)
        _close(got.permute(1, 0, 2, 3), y.detach(), what=tag + " fwd")
        _close(ops.gst_conv2d_fwd(xd, wd, bd, ops.ACT_RELU).permute(1, 0, 2, 3), F.relu(y.detach()), what=tag + " fwd+relu")
        _close(ops.gst_conv2d_fwd(xd, wd, None).permute(1, 0, 2, 3), y.detach() - b.detach().view(1, -1, 1, 1), what=tag + " fwd no bias")
        _close(ops.gst_conv2d_dgrad(dyd, wd, H, W).permute(1, 0, 2, 3), x.grad, what=tag + " dgrad")
        dw, db = torch.full_like(wd, 0.5), torch.full_like(bd, -1.0)  # accumulated into: start from known non-zero values
        ops.gst_conv2d_wgrad(xd, dyd, dw, db, accumulate=True)
        _close(dw - 0.5, w.grad, what=tag + " wgrad")
        _close(db + 1.0, b.grad, what=tag + " bgrad")
        dw2, db2 = torch.full_like(wd, 7.0), torch.full_like(bd, 7.0)
        ops.gst_conv2d_wgrad(xd, dyd, dw2, db2, accumulate=False)
        _close(dw2, w.grad, what=tag + " wgrad (overwrite)")
        _close(db2, b.grad, what=tag + " bgrad (overwrite)")
        H = OH


@pytest.mark.parametrize("H", [128, 32])
@pytest.mark.parametrize("T", [1, 2, 15])
def test_gru_forward_backward(cuda_device, T, H):
    """The recurrence against nn.GRU autograd.  The input weights are the identity, so the GRU's input IS the projected input gi and
    its gradient IS dgi; dW_hh / db_hh come out of dgh and hprev through the dense weight gradient, as in the trainer."""
    from everyvoice_amd.train import ops

    dev, B = cuda_device, 3
    g = torch.Generator().manual_seed(T + H)
    gru = nn.GRU(3 * H, H, batch_first=True)
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.eye(3 * H))
        gru.bias_ih_l0.zero_()
        gru.weight_hh_l0.copy_(torch.randn(3 * H, H, generator=g) / H ** 0.5)
        gru.bias_hh_l0.copy_(torch.randn(3 * H, generator=g) * 0.2)
    x = torch.randn(B, T, 3 * H, generator=g, requires_grad=True)
    _, hT = gru(x)
    dh = torch.randn(B, H, generator=g)
    hT[0].backward(dh)
    gi = x.detach().permute(2, 0, 1).contiguous().to(dev)  # [3H, B, T]
    whh, bhh = gru.weight_hh_l0.detach().to(dev), gru.bias_hh_l0.detach().to(dev)
    hlast, saved = ops.gst_gru_fwd(gi, whh, bhh)
    _close(hlast.t(), hT[0].detach(), what=f"gru T {T} H {H} h")
    _close(ops.gst_gru_fwd(gi, whh, bhh, save=False)[0].t(), hT[0].detach(), what="gru (inference form) h")
    dgi, dgh = ops.gst_gru_bwd(saved, whh, dh.t().contiguous().to(dev))
    _close(dgi.permute(1, 2, 0), x.grad, what="gru dgi")
    dw, db = torch.zeros(3 * H, H, 1, device=dev), torch.zeros(3 * H, device=dev)
    ops.conv1d_bwd(saved[2].view(H, 1, B * T), whh.view(3 * H, H, 1), dgh.view(3 * H, 1, B * T), 1, 0, 1, 1, need_dx=False, dw_out=dw, db_out=db, accumulate=True)
    ops.wgrad_join(dev)
    _close(dw[..., 0], gru.weight_hh_l0.grad, what="gru dW_hh")
    _close(db, gru.bias_hh_l0.grad, what="gru db_hh")


@pytest.mark.parametrize("E,heads,N,B", [(256, 8, 10, 3), (64, 8, 10, 4), (256, 8, 10, 1), (128, 4, 16, 2)])
def test_token_attention_forward_backward(cuda_device, E, heads, N, B):
    from everyvoice_amd.train import ops

    dev = cuda_device
    g = torch.Generator().manual_seed(E + N + B)
    d = E // heads
    q = torch.randn(B, E, generator=g, requires_grad=True)
    k = torch.randn(N, E, generator=g, requires_grad=True)
    v = torch.randn(N, E, generator=g, requires_grad=True)
    p = torch.softmax(torch.einsum("bhd,nhd->bhn", q.view(B, heads, d), k.view(N, heads, d)) / d ** 0.5, -1)
    out = torch.einsum("bhn,nhd->bhd", p, v.view(N, heads, d)).reshape(B, E)
    dout = torch.randn(B, E, generator=g)
    out.backward(dout)
    qd, kd, vd = (t.detach().t().contiguous().to(dev) for t in (q, k, v))  # channel-major [E, B] / [E, N]
    style, probs = ops.gst_attention_fwd(qd, kd, vd, heads)
    _close(style, out.detach(), what="attention style")
    _close(probs, p.detach(), what="attention probabilities")
    dq, dk, dv = ops.gst_attention_bwd(dout.to(dev), qd, kd, vd, probs, heads)
    _close(dq.t(), q.grad, what="attention dq")
    _close(dk.t(), k.grad, what="attention dk")
    _close(dv.t(), v.grad, what="attention dv")


# ---- the module and the model, inference -------------------------------------------------------------------------------------------
def _gst_cfg(ref_cfg):
    cfg = _product_config(ref_cfg)
    cfg.use_global_style_token_module = True
    return cfg


def _gst_ref_for(cfg, seed):
    torch.manual_seed(seed)
    ref = GSTRef(cfg.encoder.input_dim, cfg.n_mels, cfg.gst_num_heads, cfg.gst_num_tokens, cfg.gst_ref_enc_filters)
    return randomize_(ref, torch.Generator().manual_seed(seed + 1))


@pytest.mark.parametrize("T", [1, 17, 566, 947])
def test_module_forward_in_eval_mode(cuda_device, T):
    """Default size (E = 256, 80 mel bins), folded BatchNorm on randomised running statistics, against tests/gst_ref.py."""
    from everyvoice_amd.fs2 import FastSpeech2ModelConfig, StyleTokens

    cfg = FastSpeech2ModelConfig(use_global_style_token_module=True)
    ref = _gst_ref_for(cfg, 3).eval()
    mod = StyleTokens(cfg, {"gst." + k: v for k, v in ref.state_dict().items()}, torch.device(cuda_device))
    mel = torch.randn(3, T, 80, generator=torch.Generator().manual_seed(T)) * 2.0 - 4.0
    with torch.no_grad():
        want = ref(mel)
    _close(mod.forward(mel.to(cuda_device)), want, what=f"module T {T}")


def _model_pair(cuda_device, B, seed):
    """(oracle with the reference module's style matrix as its speaker table, reference module, product model with the module)."""
    from everyvoice_amd.fs2 import FastSpeech2

    ref_cfg = FastSpeech2ConfigRef.small()
    ref_cfg.n_speakers = B
    torch.manual_seed(seed)
    ref = FastSpeech2Ref(ref_cfg).eval()
    g = torch.Generator().manual_seed(seed + 1)
    randomize_norm_stats_(ref, g)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    ref_cfg.n_speakers = 0
    cfg = _gst_cfg(ref_cfg)
    gst = _gst_ref_for(cfg, seed + 2).eval()
    sd = {k: v for k, v in ref.state_dict().items() if not k.startswith("speaker_embedding.")}
    sd.update({"gst." + k: v for k, v in gst.state_dict().items()})
    return ref, gst, FastSpeech2(cfg, device=cuda_device).load_state_dict(sd), ref_cfg


def test_model_with_style_reference_against_the_oracle(cuda_device):
    B, L = 3, 12
    ref, gst, model, ref_cfg = _model_pair(cuda_device, B, seed=31)
    g = torch.Generator().manual_seed(9)
    lens = torch.tensor([L, 7, 9])
    ids = torch.randint(1, 20, (B, L), generator=g).masked_fill(torch.arange(L)[None] >= lens[:, None], 0)
    durs = torch.randint(0, 6, (B, L), generator=g)
    durs[:, 0] += 1
    style_mel = torch.randn(B, 41, ref_cfg.n_mels, generator=g)
    with torch.no_grad():
        ref.speaker_embedding.weight.copy_(gst(style_mel))
        want = ref(ids, lens, durations=durs, speakers=torch.arange(B))
    got = model(ids, lens, durations=durs, style_mel=style_mel)
    assert torch.equal(got[2].cpu(), want[2]) and torch.equal(got[5].cpu(), want[5])  # integer outputs
    for i, name in ((3, "pitch"), (4, "energy"), (0, "mel"), (1, "postnet mel")):  # test_gpu_fs2.py: 2e-4 of the largest magnitude
        _close(got[i], want[i], what=name)
    # predicted durations as well
    with torch.no_grad():
        want = ref(ids, lens, speakers=torch.arange(B))
    got = model(ids, lens, style_mel=style_mel)
    assert torch.equal(got[2].cpu(), want[2]) and torch.equal(got[5].cpu(), want[5])
    _close(got[1], want[1], what="postnet mel, predicted durations")
    # one reference for the whole batch equals the explicit batch of copies, bit for bit
    one = style_mel[:1]
    a = model(ids, lens, durations=durs, style_mel=one)
    b = model(ids, lens, durations=durs, style_mel=one.expand(B, -1, -1).contiguous())
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[1], got[1])
    with pytest.raises(ValueError, match="style_mel"):
        model(ids, lens, durations=durs)
    with pytest.raises(ValueError, match="style_mel"):
        model(ids, lens, durations=durs, style_mel=style_mel[:2])
    plain = FastSpeech2Ref(ref_cfg)
    from everyvoice_amd.fs2 import FastSpeech2

    no_module = FastSpeech2(_product_config(ref_cfg), device=cuda_device).load_state_dict(plain.state_dict())
    with pytest.raises(ValueError, match="without the Global Style Token module"):
        no_module(ids, lens, durations=durs, style_mel=style_mel)


# ---- training ---------------------------------------------------------------------------------------------------------------------
def _gst_trainer(ref_cfg, cuda_device, seed=11, gst=True, **kw):
    from everyvoice_amd.train.fs2 import FastSpeech2Trainer

    cfg = _product_config(ref_cfg)
    cfg.learn_alignment = False
    cfg.use_global_style_token_module = gst
    for enc, rc in ((cfg.encoder, ref_cfg.encoder), (cfg.decoder, ref_cfg.decoder)):
        enc.dropout = rc.dropout
    for name in ("duration", "pitch", "energy"):
        getattr(cfg.variance_predictors, name).dropout = getattr(ref_cfg, name).dropout
    tr = FastSpeech2Trainer(cfg, device=cuda_device, seed=seed, **kw)
    g = torch.Generator().manual_seed(seed)
    sd = tr.state_dict()
    for n in tr.params.names():  # livelier than the default init (as test_gpu_fs2_train._trainer)
        if n.endswith("bias") or ".bias_" in n:
            sd[n] = torch.randn(sd[n].shape, generator=g) * 0.05
        elif n.endswith("weight_g") or (sd[n].dim() == 1 and n.endswith(".weight")):
            sd[n] = torch.rand(sd[n].shape, generator=g) * 0.5 + 0.75
    tr.load_state_dict(sd)
    return tr


class _StyleRows(nn.Module):
    """Stands where the oracle's speaker embedding stands: rows of the LIVE reference module's output, so gradients reach it."""

    def __init__(self, gst, mel):
        super().__init__()
        self.gst, self.mel = gst, mel

    def forward(self, ids):
        return self.gst(self.mel)[ids]


def _oracle_with_module(tr, ref_cfg, batch):
    B = batch["mel"].shape[0]
    ref_cfg.n_speakers = B
    ref = FastSpeech2Ref(ref_cfg).train()
    ref_cfg.n_speakers = 0
    c = tr.config
    gst = GSTRef(c.encoder.input_dim, c.n_mels, c.gst_num_heads, c.gst_num_tokens, c.gst_ref_enc_filters).train()
    sd = {k: v.detach().cpu() for k, v in tr.state_dict().items()}
    res = gst.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("gst.")}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    missing, unexpected = ref.load_state_dict(sd, strict=False)
    assert missing == ["speaker_embedding.weight"] and all(k.startswith("gst.") for k in unexpected), (missing, unexpected)
    ref.speaker_embedding = _StyleRows(gst, batch["mel"])
    return ref, gst


def test_trainer_state_dict_with_and_without_the_module(cuda_device):
    """Flag on: the gst.* tensors hold 485,024 parameters and load STRICTLY into the torch restatement (default size).  Flag off: the
    state dict has exactly the keys the oracle module has -- no gst. key, no new buffer."""
    ref_cfg = _ref_cfg(0.0, 0, default_size=True)
    on = _gst_trainer(ref_cfg, cuda_device)
    sd = on.state_dict()
    gst_sd = {k[4:]: v.cpu() for k, v in sd.items() if k.startswith("gst.")}
    names = set(on.params.names())
    assert sum(v.numel() for k, v in sd.items() if k.startswith("gst.") and k in names) == 485_024
    res = GSTRef().load_state_dict(gst_sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    off = _gst_trainer(ref_cfg, cuda_device, gst=False)
    assert set(off.state_dict()) == set(FastSpeech2Ref(ref_cfg).state_dict())
    assert not any(k.startswith("gst.") for k in off.state_dict())
    assert set(sd) - set(off.state_dict()) == {"gst." + k for k in GSTRef().state_dict()}


def test_training_step_with_the_module_against_torch_autograd(cuda_device):
    """Default model size, fp32: every loss, every gst.* gradient, every other gradient (the style path feeds the encoder's) and the
    BatchNorm running statistics of one step against torch-CPU autograd of the oracle with the reference module in its speaker slot.
    Bounds: the whole-step bounds of test_gpu_fs2_train.py (losses 2e-4, gradients 4e-3 relative L2, statistics 1e-4)."""
    ref_cfg = _ref_cfg(0.0, 0, default_size=True)
    tr = _gst_trainer(ref_cfg, cuda_device)
    batch = _train_batch(ref_cfg, 4, 40, seed=40)
    ref, gst = _oracle_with_module(tr, ref_cfg, batch)
    want = training_losses_ref(ref, dict(batch, speakers=torch.arange(4)))
    want["total"].backward()
    got = tr.forward_backward(batch)
    for k, v in want.items():
        print(f"loss {k}: got {float(got[k]):.7f} want {float(v):.7f}")
        assert float(got[k]) == pytest.approx(float(v), rel=2e-4), k
    grads = tr.params.gradients()
    named = {(n[len("speaker_embedding."):] if n.startswith("speaker_embedding.gst.") else n): p for n, p in ref.named_parameters()}
    assert set(grads) == set(named), set(grads) ^ set(named)
    assert sum(n.startswith("gst.") for n in named) == 32
    worst = {}
    for name, p in named.items():
        want_g = p.grad if p.grad is not None else torch.zeros_like(p)
        num, den = float((grads[name].cpu() - want_g).norm()), float(want_g.norm())
        worst[name] = num / (den + 1e-30)
    for name in sorted(worst, key=worst.get)[-8:]:
        print(f"gradient {name}: relative L2 {worst[name]:.3e}")
    for name, p in named.items():
        _l2close(grads[name], p.grad if p.grad is not None else torch.zeros_like(p), 4e-3, name)
    state = tr.state_dict()
    for name, buf in list(ref.named_buffers()):
        name = name[len("speaker_embedding."):] if name.startswith("speaker_embedding.gst.") else name
        if name.endswith("running_mean") or name.endswith("running_var"):
            _close(state[name], buf, 1e-4, what=name)
    assert int(state["gst.encoder.bns.0.num_batches_tracked"]) == 1


def test_bf16_precision_mode_with_the_module_follows_the_exact_step(cuda_device):
    """The bounds of test_training_step_bf16_operands_follow_the_exact_step, module on: losses within 2e-2, the flat gradient within 5 %
    in norm and cosine >= 0.99.  The module itself runs in fp32 in both modes."""
    from everyvoice_amd.train import ops

    ref_cfg = _ref_cfg(0.0, 0)
    batch = _train_batch(ref_cfg, 4, 23, seed=5)
    out = {}
    for prec in ("f32", "bf16"):
        tr = _gst_trainer(ref_cfg, cuda_device, precision=prec)
        with ops.mode(operands=prec):  # what training_step does around forward_backward
            losses = tr.forward_backward(batch)
        out[prec] = ({k: float(v) for k, v in losses.items()}, tr.params.grad.clone())
    for k, v in out["f32"][0].items():
        assert out["bf16"][0][k] == pytest.approx(v, rel=2e-2, abs=1e-4), k
    g32, g16 = out["f32"][1].double(), out["bf16"][1].double()
    cos = float(torch.dot(g32, g16) / (g32.norm() * g16.norm()))
    ratio = float(g16.norm() / g32.norm())
    print(f"bf16 vs f32 with the module: cosine {cos:.5f} norm ratio {ratio:.5f}")
    assert cos >= 0.99 and 0.95 <= ratio <= 1.05, (cos, ratio)
    assert float((g32 - g16).abs().max()) > 0.0


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_graph_replay_and_a_second_trainer_equal_the_eager_step_bitwise(cuda_device, precision):
    """The lockstep pattern of test_graph_replays_equal_eager_steps_bitwise with the module on (dropout on): an eager trainer, a
    second eager trainer from the same seed and a graph trainer stay on one trajectory bit for bit over six steps."""
    ref_cfg = _ref_cfg(0.1, 0)
    eager = _gst_trainer(ref_cfg, cuda_device, precision=precision, use_graph=False)
    twin = _gst_trainer(ref_cfg, cuda_device, precision=precision, use_graph=False)
    graph = _gst_trainer(ref_cfg, cuda_device, precision=precision, use_graph=True)
    # 150 frames: the reference encoder leaves three GRU steps (150 -> 75 -> 38 -> 19 -> 10 -> 5 -> 3), so the recurrent weights train
    batches = [_shaped_batch(ref_cfg, seed, False, cuda_device, T=150) for seed in (5, 6, 7)]
    used = []
    for step in range(6):
        b = batches[step % 3]
        le, lt, lg = eager.training_step(b), twin.training_step(b), graph.training_step(b)
        used.append(graph.last_step_was_graph)
        for k in le:
            assert torch.equal(le[k], lg[k]) and torch.equal(le[k], lt[k]), (step, k, float(le[k]), float(lt[k]), float(lg[k]))
    assert graph._graph_failed is None and used == [False, False, True, True, True, True]
    for other in (twin, graph):
        assert torch.equal(eager.params.flat, other.params.flat) and torch.equal(eager.params.m, other.params.m) and torch.equal(eager.params.v, other.params.v)
        se, so = eager.state_dict(), other.state_dict()
        assert all(torch.equal(se[k], so[k]) for k in se), "BatchNorm statistics / counters differ"
    # the module's parameters did move
    fresh = _gst_trainer(ref_cfg, cuda_device, precision=precision).state_dict()
    moved = eager.state_dict()
    for k in ("gst.encoder.convs.0.weight", "gst.encoder.convs.5.weight", "gst.encoder.gru.weight_hh_l0", "gst.stl.embed", "gst.stl.attention.W_key.weight"):
        assert not torch.equal(fresh[k], moved[k]), k
    assert int(moved["gst.encoder.bns.3.num_batches_tracked"]) == 6


def test_checkpoint_round_trip_with_the_module(cuda_device):
    ref_cfg = _ref_cfg(0.1)
    batch = _train_batch(ref_cfg, 2, 12, seed=4)
    a = _gst_trainer(ref_cfg, cuda_device)
    a.training_step(batch)
    ck = a.checkpoint()
    import json

    json.dumps(ck["hyper_parameters"])
    assert ck["hyper_parameters"]["config"]["use_global_style_token_module"] is True
    a.training_step(batch)
    b = _gst_trainer(ref_cfg, cuda_device).load_checkpoint(ck)  # (the same seed: it also keys the dropout masks)
    b.training_step(batch)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    # evaluation uses the module's running statistics and leaves them alone
    before = {k: v.clone() for k, v in a.state_dict().items() if k.startswith("gst.encoder.bns.")}
    losses = a.evaluate(batch)
    assert all(torch.isfinite(v).all() for v in losses.values())
    after = a.state_dict()
    assert all(torch.equal(v, after[k]) for k, v in before.items())
    # a module-free checkpoint does not load into a module-on trainer ...
    plain = _gst_trainer(ref_cfg, cuda_device, gst=False)
    kept = a.params.flat.clone()
    with pytest.raises(KeyError, match="gst."):
        a.load_checkpoint(plain.checkpoint())
    with pytest.raises(KeyError, match="gst."):
        a.load_state_dict(plain.state_dict(), strict=True)
    assert torch.equal(a.params.flat, kept)  # a refused state dict leaves the trainer as it was
    # ... and loads into a module-free one as before
    plain2 = _gst_trainer(ref_cfg, cuda_device, seed=5, gst=False).load_checkpoint(plain.checkpoint())
    assert torch.equal(plain.params.flat, plain2.params.flat)
    # the trained state loads into the inference model, which then wants a style reference
    from everyvoice_amd.fs2 import FastSpeech2

    model = FastSpeech2.from_checkpoint(a.checkpoint(), device=cuda_device)
    post = model(batch["ids"], batch["lens"], durations=batch["durations"], style_mel=batch["mel"])[1]
    assert torch.isfinite(post).all()


# ---- synthesis front end ---------------------------------------------------------------------------------------------------------
def test_synthesize_helper_with_a_wav_style_reference(cuda_device, tmp_path):
    import math

    from everyvoice_amd.config import AudioConfig
    from everyvoice_amd.fs2 import FastSpeech2, FastSpeech2ModelConfig
    from everyvoice_amd.pipeline import save_wav, style_reference_mel, synthesize_helper

    model = FastSpeech2(FastSpeech2ModelConfig(use_global_style_token_module=True), device=cuda_device).init_random(3)
    model.duration_predictor.b_lin.fill_(1.0)  # a few frames per token instead of the zeros a random duration predictor gives
    t = torch.arange(22050, dtype=torch.float32) / 22050.0
    save_wav(0.5 * torch.sin(2 * math.pi * 220.0 * t) * torch.linspace(1.0, 0.1, t.numel()), tmp_path / "a.wav", 22050)
    save_wav(0.4 * torch.sin(2 * math.pi * 440.0 * t) * torch.sin(math.pi * t) ** 2, tmp_path / "b.wav", 22050)
    t16 = torch.arange(16000, dtype=torch.float32) / 16000.0
    save_wav(0.5 * torch.sin(2 * math.pi * 220.0 * t16) * torch.linspace(1.0, 0.1, t16.numel()), tmp_path / "a16k.wav", 16000)
    texts = [[3, 4, 5, 6, 7, 8], [9, 10, 11]]

    def run(ref, out):
        _, _, preds, callbacks = synthesize_helper(model, texts, None, None, 1.0, 0, ["spec"], output_dir=tmp_path / out, style_reference=ref, batch_size=1)
        assert len(preds) == 2 and callbacks["spec"].last_file_written == preds[-1]["spec"]
        return [torch.load(p["spec"]) for p in preds]

    a1, a2, b = run(tmp_path / "a.wav", "a1"), run(str(tmp_path / "a.wav"), "a2"), run(tmp_path / "b.wav", "b")
    for x, y, z in zip(a1, a2, b):
        assert x.shape[0] == 80 and torch.isfinite(x).all()
        assert torch.equal(x, y)  # the same reference twice: identical files
        # another reference: another mel (the style enters in front of the duration predictor, so even its length may differ)
        assert x.shape != z.shape or not torch.equal(x, z)
    # a reference at another sampling rate goes through resample: the same tone at 16 kHz gives nearly the same style
    a16 = run(tmp_path / "a16k.wav", "a16")
    mel22 = style_reference_mel(tmp_path / "a.wav", AudioConfig(), cuda_device)
    mel16 = style_reference_mel(tmp_path / "a16k.wav", AudioConfig(), cuda_device)
    assert mel22.shape[2] == 80 and abs(mel22.shape[1] - mel16.shape[1]) <= 1 and mel22.shape[1] == 22050 // 256
    assert all(torch.isfinite(x).all() for x in a16)
    # a 1-D waveform is taken as well
    wave_mel = style_reference_mel(0.5 * torch.sin(2 * math.pi * 220.0 * t) * torch.linspace(1.0, 0.1, t.numel()), AudioConfig(), cuda_device)
    assert wave_mel.shape == mel22.shape and torch.isfinite(wave_mel).all()
    # ... at its own sampling rate through the public helper; the model's own audio configuration is the one used
    model.audio_config = AudioConfig()
    w16 = 0.5 * torch.sin(2 * math.pi * 220.0 * t16) * torch.linspace(1.0, 0.1, t16.numel())
    _, _, p16, _ = synthesize_helper(model, texts, None, None, 1.0, 0, ["spec"], output_dir=tmp_path / "w16", style_reference=w16,
                                     style_reference_sampling_rate=16000, batch_size=1)
    assert len(p16) == 2
    with pytest.raises(ValueError, match="style_mel"):
        synthesize_helper(model, texts, None, None, 1.0, 0, ["spec"], output_dir=tmp_path / "none")
