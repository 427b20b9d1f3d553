"""Length-masked Global Style Token module: the three masked operators against float64 torch on each item
truncated to its own length (padding filled with NaN), the inference and the training module against ``tests/gst_masked_ref.py``, and
the whole step -- against torch-CPU autograd, under graph replay on batches of other lengths, through a checkpoint into the inference
model.  Bounds: 2e-4 of the reference tensor's largest magnitude for operators and embeddings (``_close`` of test_gpu_gst.py), 4e-3
relative L2 for training gradients (the whole-step bound of test_gpu_fs2_train.py).

Measured on an MI355X (error / the reference's largest magnitude; every test prints its figures, the table is in DESIGN.md section 25):
convolution with rows <= 1.2e-6, BatchNorm with valid counts <= 1.5e-7, GRU with steps <= 2.6e-7, the inference module against float64
1.7e-7 and bit-equal to each reference alone (unmasked: 67 x / 101 x the bound away), the training module's embeddings 2.8e-7 and its live
gradients <= 1.8e-6 relative L2, padded to 130 vs 192: embeddings and statistics bit-equal, gradients within 2.6e-7."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from gst_masked_ref import masked_batchnorm, masked_forward
from gst_ref import GSTRef
from oracle.fs2_ref import FastSpeech2Ref, training_losses_ref
from tests.test_gpu_fs2_train import _l2close, _ref_cfg, _shaped_batch, _train_batch
from tests.test_gpu_gst import _close, _cm, _gst_ref_for, _gst_trainer

pytestmark = pytest.mark.gpu

NAN = float("nan")
LENS = (40, 97, 130)


def _i32(values, dev):
    return torch.tensor(values, dtype=torch.int32, device=dev)


# ---- operators ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,rows", [(17, (1, 2, 17)), (16, (16, 15, 3))])
@pytest.mark.parametrize("cin,cout,W", [(1, 32, 80), (128, 128, 3)])
def test_convolution_with_rows(cuda_device, cin, cout, W, H, rows):
    from everyvoice_amd.train import ops

    dev, B = cuda_device, 3
    g = torch.Generator().manual_seed(H * 100 + cin)
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) / (cin * 9) ** 0.5
    b = torch.randn(cout, generator=g, dtype=torch.float64) * 0.1
    OH, OW = ops.gst_conv_out(H), ops.gst_conv_out(W)
    poisoned = x.clone()
    for i, n in enumerate(rows):
        poisoned[i, :, n:] = NAN
    xd, wd, bd, rd = _cm(poisoned.float()).to(dev), w.float().to(dev), b.float().to(dev), _i32(rows, dev)
    for act in (ops.ACT_NONE, ops.ACT_RELU):
        for bias, bias_d in ((b, bd), (None, None)):
            got = ops.gst_conv2d_fwd(xd, wd, bias_d, act, rows=rd).permute(1, 0, 2, 3).cpu()
            assert got.shape == (B, cout, OH, OW) and torch.isfinite(got).all()
            want = torch.zeros(B, cout, OH, OW, dtype=torch.float64)
            for i, n in enumerate(rows):  # each item alone, truncated to its own length
                y = F.conv2d(x[i : i + 1, :, :n], w, bias, stride=2, padding=1)
                assert y.shape[2] == ops.gst_conv_out(n)
                want[i, :, : y.shape[2]] = F.relu(y[0]) if act == ops.ACT_RELU else y[0]
                assert not got[i, :, y.shape[2]:].any(), "rows beyond the valid ones must be zero"
            _close(got, want, what=f"conv rows {cin}->{cout} H {H} act {act} bias {bias is not None}")
    # every item full: the same bits as the entry point without lengths
    full = _cm(x.float()).to(dev)
    assert torch.equal(ops.gst_conv2d_fwd(full, wd, bd, ops.ACT_RELU, rows=_i32([H] * B, dev)), ops.gst_conv2d_fwd(full, wd, bd, ops.ACT_RELU))
    assert torch.equal(ops.gst_conv2d_fwd(full, wd, None, rows=_i32([H] * B, dev)), ops.gst_conv2d_fwd(full, wd, None))


@pytest.mark.parametrize("act", [0, 3])
def test_batchnorm_with_valid_counts(cuda_device, act):
    from everyvoice_amd.train import ops

    dev, C, B, T = cuda_device, 32, 3, 24
    valid = (3, 24, 10)
    g = torch.Generator().manual_seed(7 + act)
    x = (torch.randn(B, C, T, generator=g, dtype=torch.float64) * 1.5 + 0.3).requires_grad_()
    dy = torch.randn(B, C, T, generator=g, dtype=torch.float64)
    mask = (torch.arange(T)[None] < torch.tensor(valid)[:, None])[:, None, :]  # [B, 1, T]
    bn = nn.BatchNorm1d(C).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) * 0.5 + 0.75)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.1)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(C, generator=g) * 0.5 + 0.75)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    fn = F.relu if act == 3 else None
    y = masked_batchnorm(bn, x, mask, fn)
    y.backward(torch.where(mask, dy, torch.zeros((), dtype=torch.float64)))
    cnt = float(sum(valid))
    xs = torch.where(mask, x.detach(), torch.zeros((), dtype=torch.float64))
    mean = xs.sum((0, 2)) / cnt
    var = torch.where(mask, (x.detach() - mean[None, :, None]) ** 2, torch.zeros((), dtype=torch.float64)).sum((0, 2)) / cnt

    def cbt(t):  # [B, C, T] -> [C, B, T], NaN at the invalid columns
        return torch.where(mask, t.detach(), torch.full((), NAN, dtype=torch.float64)).permute(1, 0, 2).contiguous().float().to(dev)

    xd, dyd, vd = cbt(x), cbt(dy), _i32(valid, dev)
    gam, bet = bn.weight.detach().float().to(dev), bn.bias.detach().float().to(dev)
    rm, rv = rm0.float().to(dev), rv0.float().to(dev)
    out, m_, r_ = ops.batchnorm_fwd(xd, gam, bet, rm, rv, act, valid=vd, items=B)
    assert torch.isfinite(out).all() and not out.permute(1, 0, 2).cpu()[~mask.expand(B, C, T)].any()
    tag = f"batchnorm valid act {act}"
    _close(out.permute(1, 0, 2), y.detach(), what=tag + " y")
    _close(m_, mean, what=tag + " mean")
    _close(r_, 1.0 / torch.sqrt(var + bn.eps), what=tag + " rstd")
    _close(rm, bn.running_mean, what=tag + " running mean")
    _close(rv, bn.running_var, what=tag + " running var")
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    dx = ops.batchnorm_bwd(xd, gam, bet, m_, r_, dyd, dg, db, act, valid=vd, items=B)
    assert torch.isfinite(dx).all() and not dx.permute(1, 0, 2).cpu()[~mask.expand(B, C, T)].any()
    _close(dx.permute(1, 0, 2), x.grad, what=tag + " dx")
    _close(dg, bn.weight.grad, what=tag + " dgamma")
    _close(db, bn.bias.grad, what=tag + " dbeta")
    # evaluation mode: the running statistics normalise and stay
    bn.eval()
    with torch.no_grad():
        y_eval = masked_batchnorm(bn, x.detach(), mask, fn)
    rm_e, rv_e = bn.running_mean.float().to(dev), bn.running_var.float().to(dev)
    keep = (rm_e.clone(), rv_e.clone())
    out_e, m_e, r_e = ops.batchnorm_fwd(xd, gam, bet, rm_e, rv_e, act, momentum=-1.0, valid=vd, items=B)
    assert torch.isfinite(out_e).all() and torch.equal(rm_e, keep[0]) and torch.equal(rv_e, keep[1])
    _close(out_e.permute(1, 0, 2), y_eval, what=tag + " y (evaluation)")
    _close(m_e, bn.running_mean, what=tag + " mean (evaluation)")
    # every column valid: the existing pair (another, still fixed, order of the sums: within the bound, bit equality is reported)
    clean = x.detach().permute(1, 0, 2).contiguous().float().to(dev)
    dclean = dy.permute(1, 0, 2).contiguous().float().to(dev)
    full = _i32([T] * B, dev)
    ra, va, rb, vb = rm0.float().to(dev), rv0.float().to(dev), rm0.float().to(dev), rv0.float().to(dev)
    ya, ma, sa = ops.batchnorm_fwd(clean, gam, bet, ra, va, act, valid=full, items=B)
    yb, mb, sb = ops.batchnorm_fwd(clean, gam, bet, rb, vb, act)
    dga, dba, dgb, dbb = (torch.zeros(C, device=dev) for _ in range(4))
    dxa = ops.batchnorm_bwd(clean, gam, bet, ma, sa, dclean, dga, dba, act, valid=full, items=B)
    dxb = ops.batchnorm_bwd(clean, gam, bet, mb, sb, dclean, dgb, dbb, act)
    pairs = dict(y=(ya, yb), mean=(ma, mb), rstd=(sa, sb), running_mean=(ra, rb), running_var=(va, vb), dx=(dxa, dxb), dgamma=(dga, dgb), dbeta=(dba, dbb))
    print("valid == T everywhere, bit-equal to the existing pair:", {k: bool(torch.equal(a, b_)) for k, (a, b_) in pairs.items()})
    for k, (a, b_) in pairs.items():
        _close(a, b_.cpu(), what=tag + f" valid == T vs the existing pair: {k}")


@pytest.mark.parametrize("H", [32, 64, 128])
def test_gru_with_steps(cuda_device, H):
    from everyvoice_amd.train import ops

    dev, B, T = cuda_device, 3, 15
    steps = (1, 2, 15)
    g = torch.Generator().manual_seed(H)
    gru = nn.GRU(3 * H, H, batch_first=True).double()
    with torch.no_grad():  # identity input weights: the GRU's input IS gi and its gradient IS dgi (as in test_gpu_gst.py)
        gru.weight_ih_l0.copy_(torch.eye(3 * H))
        gru.bias_ih_l0.zero_()
        gru.weight_hh_l0.copy_(torch.randn(3 * H, H, generator=g) / H ** 0.5)
        gru.bias_hh_l0.copy_(torch.randn(3 * H, generator=g) * 0.2)
    x = torch.randn(B, T, 3 * H, generator=g, dtype=torch.float64, requires_grad=True)
    dh = torch.randn(B, H, generator=g, dtype=torch.float64)
    hT = torch.cat([gru(x[i : i + 1, :n])[1][0] for i, n in enumerate(steps)])  # each item alone on its truncated sequence
    hT.backward(dh)
    poisoned = x.detach().clone()
    for i, n in enumerate(steps):
        poisoned[i, n:] = NAN
    gi = poisoned.permute(2, 0, 1).contiguous().float().to(dev)  # [3H, B, T]
    whh, bhh, sd = gru.weight_hh_l0.detach().float().to(dev), gru.bias_hh_l0.detach().float().to(dev), _i32(steps, dev)
    hlast, saved = ops.gst_gru_fwd(gi, whh, bhh, steps=sd)
    _close(hlast.t(), hT.detach(), what=f"gru steps H {H} h")
    _close(ops.gst_gru_fwd(gi, whh, bhh, save=False, steps=sd)[0].t(), hT.detach(), what="gru steps (inference form) h")
    dgi, dgh = ops.gst_gru_bwd(saved, whh, dh.t().contiguous().float().to(dev), steps=sd)
    for t in (*saved, dgi, dgh):
        assert torch.isfinite(t).all()
        for i, n in enumerate(steps):
            assert not t[:, i, n:].any(), "saved tensors and dgi / dgh must be exactly zero beyond the steps"
    _close(dgi.permute(1, 2, 0), x.grad, what="gru steps dgi")  # (autograd leaves zero beyond the truncation as well)
    dw, db = torch.zeros(3 * H, H, 1, device=dev), torch.zeros(3 * H, device=dev)
    ops.conv1d_bwd(saved[2].view(H, 1, B * T), whh.view(3 * H, H, 1), dgh.view(3 * H, 1, B * T), 1, 0, 1, 1, need_dx=False, dw_out=dw, db_out=db, accumulate=True)
    ops.wgrad_join(dev)
    _close(dw[..., 0], gru.weight_hh_l0.grad, what="gru steps dW_hh")
    _close(db, gru.bias_hh_l0.grad, what="gru steps db_hh")
    # every item full: the same bits as the pair without step counts
    clean, full = x.detach().permute(2, 0, 1).contiguous().float().to(dev), _i32([T] * B, dev)
    ha, sa = ops.gst_gru_fwd(clean, whh, bhh, steps=full)
    hb, sb = ops.gst_gru_fwd(clean, whh, bhh)
    assert torch.equal(ha, hb) and all(torch.equal(a, b_) for a, b_ in zip(sa, sb))
    dhd = dh.t().contiguous().float().to(dev)
    assert all(torch.equal(a, b_) for a, b_ in zip(ops.gst_gru_bwd(sa, whh, dhd, steps=full), ops.gst_gru_bwd(sb, whh, dhd)))


# ---- the module -------------------------------------------------------------------------------------------------------------------
def _module_cfg(E):
    from everyvoice_amd.fs2 import ConformerConfig, FastSpeech2ModelConfig

    return FastSpeech2ModelConfig(encoder=ConformerConfig(input_dim=E), use_global_style_token_module=True)


def _padded_references(T, seed, fill, n_mels=80):
    """Three references of LENS frames inside [3, T, n_mels]; the padding holds ``fill``."""
    mel = torch.randn(len(LENS), T, n_mels, generator=torch.Generator().manual_seed(seed)) * 2.0 - 4.0
    for i, n in enumerate(LENS):
        mel[i, n:] = fill
    return mel


@pytest.mark.parametrize("E", [256, 64])
def test_inference_module_with_lengths(cuda_device, E):
    from everyvoice_amd.fs2 import StyleTokens

    dev = torch.device(cuda_device)
    cfg = _module_cfg(E)
    ref = _gst_ref_for(cfg, 3).eval()
    mod = StyleTokens(cfg, {"gst." + k: v for k, v in ref.state_dict().items()}, dev)
    mel, lens = _padded_references(192, E, NAN), _i32(LENS, dev)
    got = mod.forward(mel.to(dev), lens)
    assert torch.isfinite(got).all()
    with torch.no_grad():
        want64 = masked_forward(ref.double(), mel.double(), torch.tensor(LENS))
    _close(got, want64, what=f"E {E}: module with lengths vs the float64 restatement")
    scale = float(want64.abs().max())
    alone = torch.cat([mod.forward(mel[i : i + 1, :n].contiguous().to(dev)) for i, n in enumerate(LENS)]).cpu()
    for i, n in enumerate(LENS):
        err = float((got[i].cpu() - alone[i]).abs().max())
        print(f"E {E}: item {i} ({n} frames in 192) vs alone: err {err:.3e} ratio {err / scale:.2e}")
        assert err <= 2e-4 * scale
    # not vacuous: without lengths the zero-padded batch moves the shortest item by MORE than the bound
    zero = _padded_references(192, E, 0.0)
    assert torch.equal(torch.nan_to_num(mel, nan=0.0), zero)
    unmasked = mod.forward(zero.to(dev)).cpu()
    drift = float((unmasked[0] - alone[0]).abs().max())
    print(f"E {E}: unmasked shortest item vs alone: {drift:.3e} = {drift / (2e-4 * scale):.1f} x the bound")
    assert drift > 2e-4 * scale
    # one unpadded reference: masked and unmasked are the same computation, bit for bit
    one = mel[2:3, :130].contiguous().to(dev)
    assert torch.equal(mod.forward(one, _i32([130], dev)), mod.forward(one))


def _module_trainer(E, cuda_device):
    return _gst_trainer(_ref_cfg(0.0, 0, default_size=(E == 256)), cuda_device)


def _module_step(tr, mel, lens, dstyle, evaluation=False):
    """``_StyleTokensT.forward`` + its backward alone -> (style [B, E], {gst.* gradient}, {gst.* BatchNorm running statistics})."""
    from everyvoice_amd.train import fs2 as tfs2
    from everyvoice_amd.train.autograd import Tape

    dev = tr.device
    tr.params.zero_grad()
    tape = Tape()
    tfs2._EVAL[0] = evaluation
    try:
        style = tr.gst.forward(tape, mel.to(dev), None if lens is None else _i32(lens, dev))
    finally:
        tfs2._EVAL[0] = False
    if evaluation:
        return style.data.clone(), None, None
    style.grad = dstyle.to(dev)
    tape.backward()
    torch.cuda.synchronize()
    grads = {k: v.clone() for k, v in tr.params.gradients().items() if k.startswith("gst.")}
    stats = {k: v.clone() for k, v in tr.state_dict().items() if k.startswith("gst.") and "running_" in k}
    return style.data.clone(), grads, stats


@pytest.mark.parametrize("E", [256, 64])
def test_training_module_with_lengths(cuda_device, E):
    ref_cfg = _ref_cfg(0.0, 0, default_size=(E == 256))
    assert ref_cfg.encoder.input_dim == E
    a, b = _gst_trainer(ref_cfg, cuda_device), _gst_trainer(ref_cfg, cuda_device)  # the same seed: the same parameters
    c = a.config
    gst = GSTRef(c.encoder.input_dim, c.n_mels, c.gst_num_heads, c.gst_num_tokens, c.gst_ref_enc_filters).double().train()
    sd = {k[4:]: v.detach().cpu().double() if v.is_floating_point() else v.cpu() for k, v in a.state_dict().items() if k.startswith("gst.")}
    res = gst.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    mel192 = _padded_references(192, 5 + E, 0.0, c.n_mels)
    mel130 = mel192[:, :130].contiguous()
    dstyle = torch.randn(3, E, generator=torch.Generator().manual_seed(E))
    want = masked_forward(gst, mel192.double(), torch.tensor(LENS))
    want.backward(dstyle.double())
    style192, g192, s192 = _module_step(a, mel192, LENS, dstyle)
    style130, g130, s130 = _module_step(b, mel130, LENS, dstyle)
    _close(style192, want.detach(), what=f"E {E}: training module, style embeddings")
    named = {"gst." + n: p for n, p in gst.named_parameters()}
    assert set(named) == set(g192) and len(named) == 32
    # (a convolution bias in front of BatchNorm has a gradient of exactly zero in exact arithmetic: noise on both sides, left to
    # _l2close's floor and kept out of the printed figures)
    live = [n for n in named if not (".convs." in n and n.endswith(".bias"))]
    worst = {n: float((g192[n].cpu() - named[n].grad).norm() / (named[n].grad.norm() + 1e-30)) for n in live}
    for n in sorted(worst, key=worst.get)[-4:]:
        print(f"E {E}: gradient {n}: relative L2 {worst[n]:.3e}")
    for n, p in named.items():
        _l2close(g192[n], p.grad.float(), 4e-3, n)
    for n, buf in gst.named_buffers():
        if "running_" in n:
            _l2close(s192["gst." + n], buf.float(), 4e-3, n)
    # padded to 130 or to 192: the same embeddings, gradients and statistics (the weight gradient's slice split follows the position count,
    # so bit equality is not asked)
    _close(style130, style192.cpu(), what=f"E {E}: padded to 130 vs 192, style embeddings")
    pad_worst = max(float((g130[n] - g192[n]).norm() / (g192[n].norm() + 1e-30)) for n in live)
    stat_worst = max(float((s130[n] - s192[n]).norm() / (s192[n].norm() + 1e-30)) for n in s192)
    print(f"E {E}: padded to 130 vs 192: worst gradient relative L2 {pad_worst:.3e}, worst running statistic {stat_worst:.3e}, "
          f"style bit-equal {bool(torch.equal(style130, style192))}")
    for n in g192:
        _l2close(g130[n], g192[n].cpu(), 4e-3, n + " (130 vs 192)")
    for n in s192:
        _l2close(s130[n], s192[n].cpu(), 4e-3, n + " (130 vs 192)")
    # NaN in the padding changes nothing: not a bit
    c_ = _gst_trainer(ref_cfg, cuda_device)
    style_nan, g_nan, s_nan = _module_step(c_, _padded_references(192, 5 + E, NAN, c.n_mels), LENS, dstyle)
    assert torch.equal(style_nan, style192) and all(torch.equal(g_nan[n], g192[n]) for n in g192) and all(torch.equal(s_nan[n], s192[n]) for n in s192)


# ---- the whole model and step -------------------------------------------------------------------------------------------------------
class _MaskedStyleRows(nn.Module):
    """Stands where the oracle's speaker embedding stands: rows of the LIVE masked reference module's output."""

    def __init__(self, gst, mel, lens):
        super().__init__()
        self.gst, self.mel, self.lens = gst, mel, lens

    def forward(self, ids):
        return masked_forward(self.gst, self.mel, self.lens)[ids]


def _masked_trainer(ref_cfg, cuda_device, mask=True, **kw):
    """``_gst_trainer`` of test_gpu_gst.py with ``gst_mask_padding`` set: the flag is read at every step."""
    tr = _gst_trainer(ref_cfg, cuda_device, **kw)
    tr.config.gst_mask_padding = mask
    return tr


def test_training_step_with_masking_against_torch_autograd(cuda_device):
    """The small model of test_gpu_gst.py, fp32: every loss and every gradient of one step against torch-CPU autograd of the oracle with
    the masked reference module in its speaker slot (the items of the batch have different lengths)."""
    ref_cfg = _ref_cfg(0.0, 0)
    tr = _masked_trainer(ref_cfg, cuda_device)
    batch = _train_batch(ref_cfg, 4, 23, seed=5)
    mel_lens = batch["durations"].sum(1)
    B = 4
    ref_cfg.n_speakers = B
    ref = FastSpeech2Ref(ref_cfg).train()
    ref_cfg.n_speakers = 0
    c = tr.config
    gst = GSTRef(c.encoder.input_dim, c.n_mels, c.gst_num_heads, c.gst_num_tokens, c.gst_ref_enc_filters).train()
    sd = {k: v.detach().cpu() for k, v in tr.state_dict().items()}
    gst.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("gst.")}, strict=True)
    missing, unexpected = ref.load_state_dict(sd, strict=False)
    assert missing == ["speaker_embedding.weight"] and all(k.startswith("gst.") for k in unexpected)
    ref.speaker_embedding = _MaskedStyleRows(gst, batch["mel"], mel_lens)
    want = training_losses_ref(ref, dict(batch, speakers=torch.arange(B)))
    want["total"].backward()
    got = tr.forward_backward(batch)
    for k, v in want.items():
        print(f"loss {k}: got {float(got[k]):.7f} want {float(v):.7f}")
        assert float(got[k]) == pytest.approx(float(v), rel=2e-4), k
    grads = tr.params.gradients()
    named = {(n[len("speaker_embedding."):] if n.startswith("speaker_embedding.gst.") else n): p for n, p in ref.named_parameters()}
    assert set(grads) == set(named) and sum(n.startswith("gst.") for n in named) == 32
    want_g = {n: (p.grad if p.grad is not None else torch.zeros_like(p)) for n, p in named.items()}
    worst = {n: float((grads[n].cpu() - w).norm() / (w.norm() + 1e-30)) for n, w in want_g.items()}
    for n in sorted((n for n in worst if n.startswith("gst.") and not (".convs." in n and n.endswith(".bias"))), key=worst.get)[-4:]:
        print(f"gradient {n}: relative L2 {worst[n]:.3e}")
    for n, w in want_g.items():
        _l2close(grads[n], w, 4e-3, n)
    state = tr.state_dict()
    for n, buf in gst.named_buffers():
        if "running_" in n:
            _close(state["gst." + n], buf, 1e-4, what="gst." + n)


def test_graph_replay_follows_each_batchs_lengths_bitwise(cuda_device):
    """Under graph_buckets with use_graph=True the replayed masked step is bit-equal to the eager one on three batches of ONE padded
    shape and DIFFERENT lengths: the captured kernels read the lengths from device memory."""
    ref_cfg = _ref_cfg(0.1, 0)
    eager = _masked_trainer(ref_cfg, cuda_device, use_graph=False, graph_buckets=(8, 64))
    graph = _masked_trainer(ref_cfg, cuda_device, use_graph=True, graph_buckets=(8, 64))
    batches = [_shaped_batch(ref_cfg, seed, False, cuda_device, T=150) for seed in (5, 6, 7)]  # 150 frames: padded to 192
    assert len({tuple(b["durations"].sum(1).tolist()) for b in batches}) == 3
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
    # masking is really on: the same trajectory without it ends elsewhere
    plain = _masked_trainer(ref_cfg, cuda_device, mask=False, graph_buckets=(8, 64))
    for step in range(6):
        plain.training_step(batches[step % 3])
    assert not torch.equal(plain.params.flat, eager.params.flat)


def test_flag_off_is_the_step_of_a_trainer_without_the_field(cuda_device):
    """gst_mask_padding=False: the bits of a trainer whose configuration never heard of the field (it is deleted from the instance, so
    any read of it would fall back to the class default and any masked launch would show as different bits)."""
    ref_cfg = _ref_cfg(0.1, 0)
    batches = [_shaped_batch(ref_cfg, seed, False, cuda_device, T=150) for seed in (5, 6)]
    off = _masked_trainer(ref_cfg, cuda_device, mask=False)
    old = _gst_trainer(ref_cfg, cuda_device)
    del old.config.__dict__["gst_mask_padding"]
    on = _masked_trainer(ref_cfg, cuda_device)
    for b in batches:
        lo, ll, ln = off.training_step(b), old.training_step(b), on.training_step(b)
        assert all(torch.equal(lo[k], ll[k]) for k in lo)
    assert torch.equal(off.params.flat, old.params.flat) and torch.equal(off.params.m, old.params.m)
    assert not torch.equal(on.params.flat, off.params.flat)  # the batches have padding, so the flag does change the step


def test_checkpoint_carries_the_flag_into_the_inference_model(cuda_device):
    import json

    from everyvoice_amd.fs2 import FastSpeech2
    ref_cfg = _ref_cfg(0.1, 0)
    tr = _masked_trainer(ref_cfg, cuda_device)
    batch = _shaped_batch(ref_cfg, 5, False, cuda_device, T=150)
    tr.training_step(batch)
    ck = tr.checkpoint()
    json.dumps(ck["hyper_parameters"])
    assert ck["hyper_parameters"]["config"]["gst_mask_padding"] is True
    model = FastSpeech2.from_checkpoint(ck, device=cuda_device)
    assert model.config.gst_mask_padding is True
    # the trainer in evaluation mode and the inference model (folded BatchNorm) give the same embeddings for the padded batch + lengths
    mel_lens = batch["durations"].sum(1).tolist()
    mel = batch["mel"].clone()
    for i, n in enumerate(mel_lens):
        mel[i, n:] = NAN
    want, _, _ = _module_step(tr, mel, mel_lens, None, evaluation=True)
    got = model.gst.forward(mel.to(cuda_device), _i32(mel_lens, cuda_device))
    _close(got, want.cpu(), what="inference model vs the trainer's evaluation-mode embeddings")
    # ... through the public call: style_lens changes the output where the batch has padding
    ids, lens, durs = batch["ids"], batch["lens"], batch["durations"]
    zero = batch["mel"]
    with_lens = model(ids, lens, durations=durs, style_mel=zero, style_lens=torch.tensor(mel_lens))
    without = model(ids, lens, durations=durs, style_mel=zero)
    assert not torch.equal(with_lens[1], without[1])
    with pytest.raises(ValueError, match="style_lens"):
        model(ids, lens, durations=durs, style_mel=zero, style_lens=torch.tensor(mel_lens[:2]))
    with pytest.raises(ValueError, match="style_lens"):
        model(ids, lens, durations=durs, style_mel=zero, style_lens=torch.tensor([0] + mel_lens[1:]))


def test_one_reference_per_item_through_the_synthesis_front_end(cuda_device, tmp_path):
    import math

    from everyvoice_amd.config import AudioConfig
    from everyvoice_amd.fs2 import FastSpeech2, FastSpeech2ModelConfig
    from everyvoice_amd.pipeline import save_wav, style_reference_batch, style_reference_mel, synthesize_from_text

    t = torch.arange(22050, dtype=torch.float32) / 22050.0
    long_ = 0.5 * torch.sin(2 * math.pi * 220.0 * t) * torch.linspace(1.0, 0.1, t.numel())
    short = 0.4 * torch.sin(2 * math.pi * 440.0 * t[:9000])
    save_wav(short, tmp_path / "short.wav", 22050)
    alone = [style_reference_mel(r, AudioConfig(), cuda_device) for r in (long_, tmp_path / "short.wav")]
    mel, lens = style_reference_batch([long_, tmp_path / "short.wav"], AudioConfig(), cuda_device)
    assert lens.dtype == torch.int32 and lens.tolist() == [22050 // 256, 9000 // 256] and mel.shape == (2, 22050 // 256, 80)
    assert torch.equal(mel[0], alone[0][0]) and torch.equal(mel[1, : int(lens[1])], alone[1][0]) and not mel[1, int(lens[1]):].any()
    model = FastSpeech2(FastSpeech2ModelConfig(use_global_style_token_module=True), device=cuda_device).init_random(3)
    model.duration_predictor.b_lin.fill_(1.0)
    ids, tl = torch.tensor([[3, 4, 5, 6, 7, 8], [9, 10, 11, 0, 0, 0]]), torch.tensor([6, 3])
    both = synthesize_from_text(ids, tl, model, None, tmp_path / "both", ["a", "b"], output_types=("spec",), style_reference=[long_, tmp_path / "short.wav"])
    direct = model(ids, tl, style_mel=mel, style_lens=lens)  # what the helper must have called: the padded references WITH their lengths
    for i, rec in enumerate(both):
        spec = torch.load(rec["spec"])
        assert torch.isfinite(spec).all() and torch.equal(spec, direct[1][i, : int(direct[5][i])].t().cpu())
    assert not torch.equal(direct[1], model(ids, tl, style_mel=mel)[1])
    with pytest.raises(ValueError, match="one reference per item"):
        synthesize_from_text(ids, tl, model, None, tmp_path / "bad", ["a", "b"], output_types=("spec",), style_reference=[long_])
