"""The iSTFT output head alone, through evmi_istft_head_bf16 (csrc/istft_head_generic.hip; variant 0 at the specialised shape:
csrc/istft_head.hip).

Yardstick: float64 torch on the same rounded operands, ReflectionPad1d((1, 0)) -> conv1d(pad 3) -> exp / sin -> torch.istft.
Bound, per shape: e32 = the max-abs error against float64 of torch's own fp32 evaluation of the same chain on the CPU; the device must
stay within 16 x e32, floored at 1e-6 x max|want| (the MFMA chain sums up to 7 C products in one fixed order where the CPU convolution
sums in blocks, and the device expf / sinf / cosf are a few ulp).  Second anchor at the specialised shape: the generic kernel's error
is at most 2 x the specialised kernel's -- the same arithmetic in another order.
Shapes (C, n_fft, hop, L): each the smallest at which one mechanism can fail; B = 2 with different data per item; the output is
pre-filled with NaN and followed by a NaN guard band that must stay NaN.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B = 2
GUARD = 64


def _frame_tile(n_fft, hop):
    from everyvoice_amd import _lib

    return _lib.load().evmi_istft_head_frame_tile(n_fft, hop)  # frames per workgroup (csrc/istft_head_generic.h)


SHAPES = {
    "smallest": (8, 4, 1, 2),
    "ragged_kstep": (24, 8, 2, 37),
    "hop_not_dividing": (8, 12, 5, 40),
    "max_overlap": (8, 16, 1, 33),
    "three_m_tiles": (16, 32, 8, 9),
    "largest_head": (64, 128, 32, None),  # L = workgroup frame tile + 1: seam and halo recomputation at the widest head
    "largest_head_hop_half": (64, 128, 64, 5),
    "widest_input": (256, 128, 32, 5),
    "specialised_shape": (32, 16, 4, 70),
    "specialised_shape_L1": (32, 16, 4, 1),
}


def _shape(name):
    C, n_fft, hop, L = SHAPES[name]
    if L is None:
        L = _frame_tile(n_fft, hop) + 1
        assert L == 65  # 128 / 32: a 64-frame tile
    return C, n_fft, hop, L


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _chain(x, w, b, n_fft, hop):
    """x [B, L, C], w [n_fft + 2, C, 7], b [n_fft + 2] in one dtype -> wav [B, hop L]"""
    bins = n_fft // 2 + 1
    L = x.shape[1]
    xt = x.transpose(1, 2)
    xp = torch.cat([xt[:, :, 1:2] if L > 1 else xt[:, :, :1], xt], dim=2)  # ReflectionPad1d((1, 0)); L = 1 replicates
    z = F.conv1d(xp, w, b, padding=3)
    mag, phi = torch.exp(z[:, :bins]), torch.sin(z[:, bins:])
    window = torch.hann_window(n_fft, periodic=True, dtype=x.dtype)
    return torch.istft(mag * torch.exp(1j * phi), n_fft, hop_length=hop, win_length=n_fft, window=window, center=True)


_PROBLEMS: dict = {}


def _problem(name):
    """(x, w, bias, want float64, bound): computed once per shape and shared"""
    if name not in _PROBLEMS:
        C, n_fft, hop, L = _shape(name)
        g = torch.Generator().manual_seed(1000 * C + 10 * n_fft + hop + L)
        x = _bf(torch.randn(B, L, C, generator=g))
        w = _bf(torch.randn(n_fft + 2, C, 7, generator=g) * (7 * C) ** -0.5)
        b = torch.randn(n_fft + 2, generator=g) * 0.1
        want = _chain(x.double(), w.double(), b.double(), n_fft, hop)
        assert want.shape == (B, hop * L)
        e32 = float((_chain(x, w, b, n_fft, hop).double() - want).abs().max())
        bound = max(16.0 * e32, 1e-6 * float(want.abs().max()))
        _PROBLEMS[name] = (x, w, b, want, bound, e32)
    return _PROBLEMS[name]


def _run(dev, name, variant):
    from everyvoice_amd import _lib

    lib = _lib.load()
    C, n_fft, hop, L = _shape(name)
    x, w, b, _, _, _ = _problem(name)
    n = lib.evmi_istft_head_weight_elems(C, n_fft)
    assert n >= (n_fft + 2) * C * 7
    laid = torch.empty(n, dtype=torch.bfloat16, device=dev)
    xd = x.to(dev, torch.bfloat16).contiguous()
    wd, bd = w.to(dev).contiguous(), b.to(dev)
    out = torch.full((B * hop * L + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(lib.evmi_istft_head_bf16(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), laid.data_ptr(), out.data_ptr(), B, L, C, n_fft, hop,
                                        variant, _lib.current_stream_ptr()), "evmi_istft_head_bf16")
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.isnan(out[B * hop * L:]).all(), f"{name}: the guard band behind the output was written"
    return out[:B * hop * L].view(B, hop * L)


def _error(dev, name, variant):
    _, _, _, want, bound, e32 = _problem(name)
    got = _run(dev, name, variant)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = float((got.double() - want).abs().max())
    print(f"istft_head {name} variant {variant}: max|diff| = {err:.3e}, e32 = {e32:.3e}, bound = {bound:.3e}, "
          f"max|want| = {float(want.abs().max()):.3e}, err / bound = {err / bound:.3f}")
    return err, bound


@pytest.mark.parametrize("name", [n for n in SHAPES if not n.startswith("specialised")])
def test_generic_head_vs_float64(cuda_device, name):
    err, bound = _error(cuda_device, name, 0)
    assert err <= bound


@pytest.mark.parametrize("name", ["specialised_shape", "specialised_shape_L1"])
def test_both_kernels_at_the_specialised_shape(cuda_device, name):
    """Variant 0 (the specialised kernel) and variant 1 (the generic one) each against float64, and against each other."""
    err0, bound = _error(cuda_device, name, 0)
    err1, _ = _error(cuda_device, name, 1)
    assert err0 <= bound and err1 <= bound
    assert err1 <= 2.0 * err0


def test_items_differ():
    """(the yardstick itself: the two items of a problem hold different data, so a kernel that ignored the batch index would fail)"""
    _, _, _, want, _, _ = _problem("ragged_kstep")
    assert float((want[0] - want[1]).abs().max()) > 1e-3
