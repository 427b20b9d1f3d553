"""The attention kernels for any head dimension up to 256 (csrc/attention_generic.hip), through the C ABI and train/ops.py.

Head dimensions: 8 (far below one 32-channel chunk), 48 (one and a half chunks), 100 (no multiple of 8: unaligned for the 8-channel
bf16 reads), 192 (six chunks; two waves share a query tile in the fp32 backward), 256 (the cap: four waves share a key tile in the
fp32 dK/dV kernel, two workgroups a head's output channels in the fp32 forward and the bf16 dK/dV kernel).  Sequence lengths and
item lengths as in tests/test_gpu_fs2_primitives.py::test_attention_cbt_tile_edges; bounds as derived there and in
tests/test_gpu_fs2_train.py, whose terms depend on the head dimension through gamma(dh) only."""

import math

import pytest
import torch

from everyvoice_amd import _lib
from helpers import E, NAN, U, assert_within, f32, gamma

pytestmark = pytest.mark.gpu

ATT_T = [1, 32, 33, 128, 129, 257]
HEAD_DIMS = [8, 48, 100, 192, 256]
BWD_SHAPES = [(96, 2, 3, 29), (200, 2, 2, 70), (192, 1, 2, 161), (512, 2, 2, 70)]  # (D, H, B, T): head dimensions 48, 100, 192, 256


def call(fn, *args):
    return fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else 0 if a is None else a for a in args])


def stream(dev):
    return _lib.current_stream_ptr(dev)


def lib():
    return _lib.load()


def _close(got, want, rel=2e-4):
    scale = float(want.abs().max()) + 1e-12
    err = float((got.cpu() - want).abs().max())
    assert err <= rel * scale, f"err {err:.3e} vs scale {scale:.3e}"


def _cbt(x):  # [B, C, T] -> [C, B, T]
    return x.permute(1, 0, 2).contiguous()


def _attention_ref(qkv, lens, H, keep_mask=None, p=0.0):
    """torch.nn.MultiheadAttention's arithmetic on [B, 3D, T]: key padding mask, softmax, dropout on the probabilities
    (tests/test_gpu_fs2_train.py::_attention_ref, restated)."""
    B, D3, T = qkv.shape
    D = D3 // 3
    dh = D // H
    q, k, v = [t.reshape(B, H, dh, T) for t in qkv.split(D, dim=1)]
    s = torch.einsum("bhdq,bhdk->bhqk", q, k) * dh ** -0.5
    s = s.masked_fill((torch.arange(T)[None, :] >= lens[:, None])[:, None, None, :], float("-inf"))
    pr = torch.softmax(s, -1)
    if keep_mask is not None:
        pr = pr * keep_mask / (1.0 - p)
    return torch.einsum("bhqk,bhdk->bhdq", pr, v).reshape(B, D, T)


def _keep_mask(dev, B, H, T, p, seed):
    """The kernels' dropout mask, read back through evmi_dropout_f32: element ((b T + q) T + k) of the stream seeded seed + head."""
    from everyvoice_amd.train import ops

    ones = torch.ones(B * T * T, device=dev)
    return torch.stack([(ops.dropout(ones, p, seed + h) > 0).float().view(B, T, T) for h in range(H)], dim=1).cpu()  # [B, H, Tq, Tk]


_REFS: dict = {}


def _reference(D, H, B, T, short_item):
    """(qkv, lens, dout, out, dqkv) of torch autograd without dropout, computed once per shape and shared by the fp32 and bf16 tests."""
    key = (D, H, B, T, short_item)
    if key not in _REFS:
        g = torch.Generator().manual_seed(D + T)
        qkv = torch.randn(B, 3 * D, T, generator=g, requires_grad=True)
        lens = torch.randint(T // 2, T + 1, (B,), generator=g)
        lens[0] = T
        if short_item:
            lens[-1] = 5  # an item shorter than one key tile
        do = torch.randn(B, D, T, generator=g)
        o = _attention_ref(qkv, lens, H)
        o.backward(do)
        _REFS[key] = (qkv.detach(), lens, do, o.detach(), qkv.grad.clone())
    return _REFS[key]


def _assert_gradient_blocks(got, want, D):
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        a, w = got[:, sl].double().flatten(), want[:, sl].double().flatten()
        cos, ratio = float(torch.dot(a, w) / (a.norm() * w.norm())), float(a.norm() / w.norm())
        assert cos >= 0.999 and 0.99 <= ratio <= 1.01, (name, cos, ratio)


# =====================================================================================================================
# fp32 forward (inference and training entry points) at the tile edges, against float64
# =====================================================================================================================
@pytest.mark.parametrize("T", ATT_T)
@pytest.mark.parametrize("dh", HEAD_DIMS)
def test_generic_forward_tile_edges(cuda_device, dh, T):
    """The bound of test_attention_cbt_tile_edges (scores: d_s = (gamma(dh) + 2 u) sum |q k| scale; probabilities eps = e^(2 d_s) - 1 +
    (tiles + 1) (E + u R + u); |o - o64| <= (2 (eps + gamma(len)) + 2 u) sum P |v|).  The log-sum-exp m + logf(l): it moves by at most
    max d_s with the scores, the normaliser l carries eps + gamma(len), logf costs E |log l| and the sum u |lse|.
    An item of length 0 has all-zero rows and lse = +inf."""
    dev, H = cuda_device, 2
    D = H * dh
    lens = sorted({n for n in (0, 1, 32, 33, T) if n <= T})
    B = len(lens)
    g = torch.Generator().manual_seed(dh * 1000 + T)
    qkv = torch.randn(3 * D, B, T, generator=g)
    x, lens_dev = qkv.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev)
    out_i = torch.full((D, B, T), NAN, device=dev)
    out_t = torch.full((D, B, T), NAN, device=dev)
    lse = torch.full((B, H, T), NAN, device=dev)
    assert call(lib().evmi_attention_generic_f32, x, lens_dev, out_i, B, T, D, H, stream(dev)) == _lib.EVMI_OK
    assert call(lib().evmi_mha_generic_fwd_f32, x, lens_dev, out_t, lse, B, T, D, H, 0.0, 0, None, stream(dev)) == _lib.EVMI_OK
    out_i, out_t, lse = out_i.cpu(), out_t.cpu(), lse.cpu()
    scale = f32(1.0 / math.sqrt(dh))
    q, k, v = (qkv[i * D : (i + 1) * D].double().view(H, dh, B, T).permute(2, 0, 3, 1) for i in range(3))  # [B, H, T, dh]
    for b, n in enumerate(lens):
        if n == 0:
            assert (out_i[:, b] == 0.0).all() and (out_t[:, b] == 0.0).all(), "an item without keys"
            assert (lse[b] == float("inf")).all()
            continue
        s = torch.einsum("htd,hkd->htk", q[b], k[b, :, :n]) * scale
        s_abs = torch.einsum("htd,hkd->htk", q[b].abs(), k[b, :, :n].abs()) * scale
        d_s = ((gamma(dh) + 2 * U) * s_abs).max(2, keepdim=True).values
        R = s.max(2, keepdim=True).values - s.min(2, keepdim=True).values
        tiles = (n + 31) // 32
        eps = torch.expm1(2 * d_s) + (tiles + 1) * (E + U * R + U)
        P = torch.softmax(s, 2)
        want = torch.einsum("htk,hkd->htd", P, v[b, :, :n])
        bound = (2 * (eps + gamma(n)) + 2 * U) * torch.einsum("htk,hkd->htd", P, v[b, :, :n].abs())
        for name, out in (("inference", out_i), ("training", out_t)):
            got = out[:, b].reshape(H, dh, T).permute(0, 2, 1)  # [H, T, dh]
            assert_within(got, want, bound, f"{name} forward dh {dh} T {T} len {n}")
        lse64 = torch.logsumexp(s, 2)  # [H, T]
        log_l = lse64 - s.max(2).values
        lse_bound = d_s[..., 0] + 2 * (eps[..., 0] + gamma(n)) + E * log_l.abs() + 2 * U * lse64.abs()
        assert_within(lse[b], lse64, lse_bound, f"lse dh {dh} T {T} len {n}")


# =====================================================================================================================
# guard bands: every tensor a view into one allocation, NaN around it
# =====================================================================================================================
@pytest.mark.parametrize("operands", ["f32", "bf16"])
@pytest.mark.parametrize("T", [33, 129])
@pytest.mark.parametrize("dh", [48, 100])
def test_generic_guard_bands(cuda_device, dh, T, operands):
    """qkv, dout, out and dqkv are views into ONE allocation with NaN in front of, between and behind them, the outputs pre-filled with
    NaN.  A load through a wrong index brings a NaN into the result (nothing leaves the allocation: no fault), a store through one
    overwrites a NaN outside the views.  All six kernels: inference forward, training forward, backward (dQ and dK/dV)."""
    dev, H, B, PAD = cuda_device, 2, 2, 1021
    D = H * dh
    qkv, lens, do, o, grad = _reference(D, H, B, T, False)
    sizes = [3 * D * B * T, D * B * T, D * B * T, D * B * T, 3 * D * B * T]  # qkv, dout, out (inference), out (training), dqkv
    buf = torch.full((sum(sizes) + PAD * (len(sizes) + 1),), NAN, device=dev)
    views, at = [], PAD
    for n in sizes:
        views.append(buf[at : at + n])
        at += n + PAD
    x, dout = views[0].view(3 * D, B, T), views[1].view(D, B, T)
    out_i, out_t, dqkv = views[2].view(D, B, T), views[3].view(D, B, T), views[4].view(3 * D, B, T)
    x.copy_(_cbt(qkv))
    dout.copy_(_cbt(do))
    lens_dev = lens.to(dev, torch.int32)
    lse, dsum = torch.full((B, H, T), NAN, device=dev), torch.full((B, H, T), NAN, device=dev)
    sfx, s = operands, stream(dev)
    L_ = lib()
    assert call(getattr(L_, "evmi_attention_generic_" + sfx), x, lens_dev, out_i, B, T, D, H, s) == _lib.EVMI_OK
    assert call(getattr(L_, "evmi_mha_generic_fwd_" + sfx), x, lens_dev, out_t, lse, B, T, D, H, 0.0, 0, None, s) == _lib.EVMI_OK
    assert call(getattr(L_, "evmi_mha_generic_bwd_" + sfx), x, lens_dev, out_t, dout, lse, dsum, dqkv, B, T, D, H, 0.0, 0, None, s) == _lib.EVMI_OK
    host = buf.cpu()
    inside = torch.zeros(host.numel(), dtype=torch.bool)
    at = PAD
    for n in sizes:
        inside[at : at + n] = True
        at += n + PAD
    assert torch.isnan(host[~inside]).all(), "a store outside the views"
    assert torch.isfinite(host[inside]).all(), "a NaN from outside the views (or an element left unwritten)"
    assert torch.equal(x.cpu(), _cbt(qkv)) and torch.equal(dout.cpu(), _cbt(do))
    got_grad = dqkv.cpu().permute(1, 0, 2)
    if operands == "f32":
        _close(out_i.cpu().permute(1, 0, 2), o)
        _close(out_t.cpu().permute(1, 0, 2), o)
        _close(got_grad, grad)
    else:
        _close(out_i.cpu().permute(1, 0, 2), o, 1e-2)
        _close(out_t.cpu().permute(1, 0, 2), o, 1e-2)
        _assert_gradient_blocks(got_grad, grad, D)


# =====================================================================================================================
# fp32 forward and backward against torch autograd
# =====================================================================================================================
@pytest.mark.parametrize("D,H,B,T", BWD_SHAPES)
def test_generic_training_forward_backward(cuda_device, D, H, B, T):
    """evmi_mha_generic_{fwd,bwd}_f32 through train/ops.py against torch autograd of the explicit attention: 2e-4 of the tensor's scale
    (only the summation order differs); a second backward gives the same bits (one writer per element, fixed summation order)."""
    from everyvoice_amd.train import ops

    assert ops.attention_entry("fwd", D // H, "f32") == "evmi_mha_generic_fwd_f32"
    qkv, lens, do, o, grad = _reference(D, H, B, T, False)
    dev = cuda_device
    x, lens32 = _cbt(qkv).to(dev), lens.to(dev, torch.int32)
    out, saved = ops.attention_train_fwd(x, lens32, H)
    _close(out.cpu().permute(1, 0, 2), o)
    dqkv = ops.attention_train_bwd(x, saved, _cbt(do).to(dev), H)
    _close(dqkv.cpu().permute(1, 0, 2), grad)
    again = ops.attention_train_bwd(x, saved, _cbt(do).to(dev), H)
    assert torch.equal(again, dqkv)


def test_generic_dropout_matches_torch_with_the_same_mask(cuda_device):
    """p = 0.3 at head dimension 100: the mask does not depend on the head dimension (read back through evmi_dropout_f32), forward
    and backward equal torch autograd with that mask."""
    from everyvoice_amd.train import ops

    D, H, B, T, p, seed = 200, 2, 2, 70, 0.3, 99
    g = torch.Generator().manual_seed(3)
    dev = cuda_device
    qkv = torch.randn(B, 3 * D, T, generator=g, requires_grad=True)
    lens = torch.tensor([T, T - 7])
    import dropout_ref

    keep = torch.from_numpy(dropout_ref.attention_keep(seed, B, H, T, p)).to(torch.float32)  # the generator restated on the host
    read_back = _keep_mask(dev, B, H, T, p, seed)
    assert keep.shape == read_back.shape and torch.equal(keep, read_back.to(torch.float32))  # ... is evmi_dropout_f32's stream, bit for bit
    assert abs(float(keep.mean()) - (1 - p)) < 0.03
    o = _attention_ref(qkv, lens, H, keep, p)
    do = torch.randn(B, D, T, generator=g)
    o.backward(do)
    x, lens32 = _cbt(qkv.detach()).to(dev), lens.to(dev, torch.int32)
    out, saved = ops.attention_train_fwd(x, lens32, H, p, seed=seed)
    _close(out.cpu().permute(1, 0, 2), o.detach())
    out2, _ = ops.attention_train_fwd(x, lens32, H, p, seed=seed)
    assert torch.equal(out, out2)
    dqkv = ops.attention_train_bwd(x, saved, _cbt(do).to(dev), H, p, seed=seed)
    _close(dqkv.cpu().permute(1, 0, 2), qkv.grad)
    again = ops.attention_train_bwd(x, saved, _cbt(do).to(dev), H, p, seed=seed)
    assert torch.equal(again, dqkv)


# =====================================================================================================================
# bf16 operands
# =====================================================================================================================
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("D,H,B,T", BWD_SHAPES)
def test_generic_training_bf16_operands(cuda_device, D, H, B, T, p):
    """evmi_mha_generic_{fwd,bwd}_bf16 against torch autograd in fp32 with the same dropout mask, the bounds of
    test_attention_training_bf16_operands: output within 1e-2 of its scale, dq / dk / dv cosine >= 0.999 and norm within 1 % (scores
    of unit variance after the 1 / sqrt(dh) scale and operand rounding of 2^-8 per term, at any head dimension).  The item of the
    three-item shape is shorter than a key tile."""
    from everyvoice_amd.train import ops

    dev = cuda_device
    qkv, lens, do, o, grad = _reference(D, H, B, T, B > 2)
    if p > 0:
        leaf = qkv.clone().requires_grad_()
        o = _attention_ref(leaf, lens, H, _keep_mask(dev, B, H, T, p, 7), p)
        o.backward(do)
        o, grad = o.detach(), leaf.grad
    x, lens32 = _cbt(qkv).to(dev), lens.to(dev, torch.int32)
    with ops.mode(operands="bf16"):
        assert ops.attention_entry("bwd", D // H) == "evmi_mha_generic_bwd_bf16"
        out, saved = ops.attention_train_fwd(x, lens32, H, p, seed=7)
        dqkv = ops.attention_train_bwd(x, saved, _cbt(do).to(dev), H, p, seed=7)
        again = ops.attention_train_bwd(x, saved, _cbt(do).to(dev), H, p, seed=7)
    assert torch.equal(dqkv, again)
    _close(out.cpu().permute(1, 0, 2), o, 1e-2)
    _assert_gradient_blocks(dqkv.cpu().permute(1, 0, 2), grad, D)


# =====================================================================================================================
# generic against specialised at a head dimension both take
# =====================================================================================================================
@pytest.mark.parametrize("operands,rel", [("f32", 2e-4), ("bf16", 1e-2)])
def test_generic_against_specialised_at_64(cuda_device, operands, rel):
    """D 128, H 2, T 161, p 0.1, the same seed: forward output, log-sum-exp and gradients of the two kernel families agree within the
    bound each holds against torch (no bit equality: their tiles are laid out and scheduled differently)."""
    dev, (D, H, B, T), p, seed = cuda_device, (128, 2, 2, 161), 0.1, 11
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3 * D, B, T, generator=g).to(dev)
    dout = torch.randn(D, B, T, generator=g).to(dev)
    lens = torch.tensor([T, 90], dtype=torch.int32, device=dev)
    res = {}
    for family in ("mha", "mha_generic"):
        out, lse = torch.full((D, B, T), NAN, device=dev), torch.full((B, H, T), NAN, device=dev)
        dsum, dqkv = torch.empty(B, H, T, device=dev), torch.full((3 * D, B, T), NAN, device=dev)
        fwd, bwd = getattr(lib(), f"evmi_{family}_fwd_{operands}"), getattr(lib(), f"evmi_{family}_bwd_{operands}")
        assert call(fwd, x, lens, out, lse, B, T, D, H, p, seed, None, stream(dev)) == _lib.EVMI_OK
        assert call(bwd, x, lens, out, dout, lse, dsum, dqkv, B, T, D, H, p, seed, None, stream(dev)) == _lib.EVMI_OK
        res[family] = (out.cpu(), lse.cpu(), dqkv.cpu())
    for got, want in zip(res["mha_generic"], res["mha"]):
        assert torch.isfinite(got).all()
        _close(got, want, rel)
