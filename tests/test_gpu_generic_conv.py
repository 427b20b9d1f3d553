"""The generic-shape bf16 MFMA convolution alone, through evmi_conv_generic_bf16 (csrc/conv_tc_generic.hip).

Yardstick: torch.nn.functional.conv1d in fp32 on the same bf16-rounded operands.  Tolerance: the project's own for this kind of
comparison, 2**-7 x max|want| (tests/test_gpu_train_tm.py: one bf16 rounding of the output plus the summation order).
Shapes (c_in, c_out, ks, dil, T): each the smallest at which one mechanism can fail; B = 2 everywhere.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROW_TILE = 256  # kGenericBN of csrc/conv_tc_generic.h
B = 2

SHAPES = {
    "all_tails_T_below_halo": (8, 8, 3, 1, 1),
    "cin_not_multiple_of_kstep_ragged_rows": (24, 24, 5, 2, 37),
    "n_mels_100_padded": (104, 192, 7, 1, 9),
    "cout_not_multiple_of_m_tile": (32, 40, 3, 1, 130),
    "v3_widest_halo": (256, 256, 7, 12, 70),
    "tile_boundary_inside_item": (64, 64, 9, 7, ROW_TILE + 1),
}


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _lrelu_bf(t, slope):
    return t if slope == 1.0 else _bf(F.leaky_relu(t, slope))


def _problem(name):
    c_in, c_out, ks, dil, T = SHAPES[name]
    g = torch.Generator().manual_seed(c_in + 3 * c_out + 5 * ks + 7 * dil + T)
    x = _bf(torch.randn(B, T, c_in, generator=g))
    if name == "n_mels_100_padded":
        x[:, :, 100:] = 0.0
    w = _bf(torch.randn(c_out, c_in, ks, generator=g) * (1.5 / (c_in * ks) ** 0.5))
    b = torch.randn(c_out, generator=g) * 0.1
    return x, w, b, g


def _laid(lib, w, dev):
    from everyvoice_amd import _lib

    c_out, c_in, ks = w.shape
    n = lib.evmi_conv_generic_weight_elems(c_in, c_out, ks)
    assert n >= c_out * c_in * ks and n % 8 == 0
    laid = torch.empty(n, dtype=torch.bfloat16, device=dev)
    wd = w.to(dev).contiguous()
    _lib.check(lib.evmi_conv_generic_relayout_f32(wd.data_ptr(), laid.data_ptr(), c_in, c_out, ks, _lib.current_stream_ptr()), "relayout")
    return laid


def _run(dev, x, w, b, dil, pad, n_rows=None, res=None, out0=None, pre=1.0, post=1.0, scale=1.0, row_stride=None, shift=0, limit=None):
    """x [B', T, c_in] (bf16-representable fp32), w [c_out, c_in, ks]; returns out as fp32 [B', limit]."""
    from everyvoice_amd import _lib

    lib = _lib.load()
    nb, T, c_in = x.shape
    c_out, _, ks = w.shape
    n_rows = T if n_rows is None else n_rows
    row_stride = c_out if row_stride is None else row_stride
    limit = n_rows * c_out if limit is None else limit
    laid = _laid(lib, w, dev)
    xd = x.to(dev, torch.bfloat16).contiguous()
    bd = b.to(dev)
    rd = res.to(dev, torch.bfloat16).contiguous() if res is not None else None
    out = (out0.to(dev, torch.bfloat16).contiguous() if out0 is not None
           else torch.full((nb, limit), float("nan"), dtype=torch.bfloat16, device=dev))
    _lib.check(lib.evmi_conv_generic_bf16(xd.data_ptr(), laid.data_ptr(), bd.data_ptr(), rd.data_ptr() if rd is not None else 0, out.data_ptr(),
                                          nb, T, n_rows, c_in, c_out, ks, dil, pad, row_stride, shift, limit, pre, post, scale,
                                          1 if out0 is not None else 0, _lib.current_stream_ptr()), "evmi_conv_generic_bf16")
    torch.cuda.synchronize()
    return out.float().cpu().view(nb, limit)


def _want(x, w, b, dil, pad, pre=1.0):
    return F.conv1d(_lrelu_bf(x, pre).transpose(1, 2), w, b, 1, pad, dil).transpose(1, 2)  # [B, T, c_out]


def _check(got, want, what=""):
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"{what}: max|diff| = {err:.3e}, bound = {2 ** -7 * scale:.3e}")
    assert torch.isfinite(got).all()
    assert err <= 2 ** -7 * scale


@pytest.mark.parametrize("name", list(SHAPES))
def test_generic_conv_vs_conv1d(cuda_device, name):
    c_in, c_out, ks, dil, T = SHAPES[name]
    x, w, b, _ = _problem(name)
    pad = dil * (ks - 1) // 2
    got = _run(cuda_device, x, w, b, dil, pad).view(B, T, c_out)
    _check(got, _want(x, w, b, dil, pad), name)


@pytest.mark.parametrize("name", ["cin_not_multiple_of_kstep_ragged_rows", "tile_boundary_inside_item"])
def test_generic_conv_epilogue(cuda_device, name):
    """pre / post slopes 0.1, a residual, out_scale 1/3 and accumulation onto a random out."""
    c_in, c_out, ks, dil, T = SHAPES[name]
    x, w, b, g = _problem(name)
    pad = dil * (ks - 1) // 2
    res = _bf(torch.randn(B, T, c_out, generator=g))
    out0 = _bf(torch.randn(B, T, c_out, generator=g))
    conv = _want(x, w, b, dil, pad, pre=0.1)
    # slopes alone
    got = _run(cuda_device, x, w, b, dil, pad, pre=0.1, post=0.1).view(B, T, c_out)
    _check(got, F.leaky_relu(conv, 0.1), name + " slopes")
    # residual, scale, running sum, activation of the result
    got = _run(cuda_device, x, w, b, dil, pad, res=res.view(B, -1), out0=out0.view(B, -1), pre=0.1, post=0.1, scale=1.0 / 3).view(B, T, c_out)
    _check(got, F.leaky_relu(out0 + (conv + res) / 3.0, 0.1), name + " res/scale/accumulate")


def test_generic_conv_upsampler_addressing(cuda_device):
    """ConvTranspose1d(u = 3, k = 7) in polyphase form: ceil(k / u) taps, u * c channels per input position, rows landing
    contiguously through out_row_stride / out_shift / out_limit."""
    u, k, cin, cout, T = 3, 7, 24, 8, 37
    p, nt = (k - u) // 2, (k + u - 1) // u
    g = torch.Generator().manual_seed(37)
    x = _bf(torch.randn(B, T, cin, generator=g))
    w = _bf(torch.randn(cin, cout, k, generator=g) * (1.5 / (cin * k / u) ** 0.5))
    b = torch.randn(cout, generator=g) * 0.1
    # with s = t + p, q = s // u, phi = s % u: tap j reads x[q - j] with w[ci][co][phi + j u]; as a convolution with pad nt - 1
    # that is tap nt - 1 - j
    wc = torch.zeros(u * cout, cin, nt)
    for phi in range(u):
        for j in range(nt):
            if phi + j * u < k:
                wc[phi * cout:(phi + 1) * cout, :, nt - 1 - j] = w[:, :, phi + j * u].t()
    n_rows = (T * u - 1 + p) // u + 1
    got = _run(cuda_device, x, wc, b.repeat(u), 1, nt - 1, n_rows=n_rows, row_stride=u * cout, shift=-p * cout, limit=T * u * cout)
    want = F.conv_transpose1d(x.transpose(1, 2), w, b, u, p).transpose(1, 2)
    assert want.shape == (B, T * u, cout)
    _check(got.view(B, T * u, cout), want, "upsampler (3, 7)")  # (an element never written would still be NaN)


@pytest.mark.parametrize("name", ["cin_not_multiple_of_kstep_ragged_rows", "tile_boundary_inside_item"])
def test_generic_conv_item_alone_equals_item_in_batch(cuda_device, name):
    c_in, c_out, ks, dil, T = SHAPES[name]
    x, w, b, _ = _problem(name)
    pad = dil * (ks - 1) // 2
    both = _run(cuda_device, x, w, b, dil, pad, pre=0.1)
    alone = _run(cuda_device, x[1:2], w, b, dil, pad, pre=0.1)
    assert torch.equal(both[1], alone[0])


def test_generic_conv_refuses_what_it_cannot_take(cuda_device):
    from everyvoice_amd import _lib

    lib = _lib.load()
    x, w, out = (torch.zeros(n, dtype=torch.bfloat16, device=cuda_device) for n in (64, 8192, 64))
    f = torch.zeros(64, device=cuda_device)
    args = lambda c_in, c_out, ks, dil: (x.data_ptr(), w.data_ptr(), f.data_ptr(), 0, out.data_ptr(), 1, 4, 4, c_in, c_out, ks, dil, 0,  # noqa: E731
                                         c_out, 0, 4 * c_out, 1.0, 1.0, 1.0, 0, _lib.current_stream_ptr())
    assert lib.evmi_conv_generic_bf16(*args(12, 8, 3, 1)) != _lib.EVMI_OK  # channels: multiples of 8
    assert lib.evmi_conv_generic_bf16(*args(8, 8, 3, 129)) != _lib.EVMI_OK  # halo 258 > 256
    assert lib.evmi_conv_generic_bf16(*args(8, 8, 3, 128)) == _lib.EVMI_OK  # halo 256: the limit itself
    torch.cuda.synchronize()
