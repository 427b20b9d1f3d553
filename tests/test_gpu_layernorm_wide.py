"""LayerNorm backward and LayerNorm written as a packed bf16 input at 256 < C <= 1024 (csrc/fs2_train_ops.hip: the <32, 16> form up to
512 channels, layernorm_bwd_cbt_wide_kernel above; csrc/conv_cbt_bf16_pk.hip: layernorm_pack_wide_kernel).

Backward: widths on both sides of every switch (257: the first wide one; 511 / 512 / 513: around the change of kernel; 1023 / 1024: the
last), column counts one lane short of a workgroup, exactly one, one column into the second, and into a third.  Inputs carry an offset
(randn * 1.7 + 0.3: a variance computed as sum x^2 - n mean^2 would show).  Reference: F.layer_norm autograd in float64, the bound of
tests/test_gpu_fs2_train.py::test_layernorm_backward (2e-4 of each tensor's scale)."""

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_fs2_train import _close

pytestmark = pytest.mark.gpu

CANARY = 12345.5


def _reference(C, N):
    """(x, gamma, dy) in fp32, channel-major [C, 1, N], and the float64 gradients (dx [C, 1, N], dgamma, dbeta)."""
    g = torch.Generator().manual_seed(1000 * C + N)
    x = torch.randn(C, 1, N, generator=g) * 1.7 + 0.3
    gamma = torch.rand(C, generator=g) + 0.5
    dy = torch.randn(C, 1, N, generator=g) * 1.7 + 0.3
    xd = x.double().permute(1, 2, 0).requires_grad_()  # [1, N, C]
    gd, bd = gamma.double().requires_grad_(), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.layer_norm(xd, (C,), gd, bd).backward(dy.double().permute(1, 2, 0))
    return x, gamma, dy, xd.grad.permute(2, 0, 1).float(), gd.grad.float(), bd.grad.float()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("C", [257, 320, 384, 511, 512, 513, 1023, 1024])
def test_layernorm_backward_wide(cuda_device, C, N):
    from everyvoice_amd import _lib
    from everyvoice_amd.train import ops

    dev = cuda_device
    x, gamma, dy, want_dx, want_dg, want_db = _reference(C, N)
    xg, gg, dyg = x.to(dev), gamma.to(dev), dy.to(dev)
    start = torch.randn(C, 1, N, generator=torch.Generator().manual_seed(C)) * 0.5 + 0.25  # the input gradient so far (acc_into)

    def run(defer, accumulate):
        dgamma, dbeta = torch.full((C,), 1.0, device=dev), torch.full((C,), -2.0, device=dev)  # accumulated into: known non-zero starts
        acc = start.to(dev) if accumulate else None
        with ops.mode(ln_defer=defer):
            dx = ops.layernorm_bwd(xg, gg, dyg, dgamma, dbeta, acc_into=acc)
            if defer:
                assert torch.equal(dgamma.cpu(), torch.full((C,), 1.0))  # nothing reduced yet
            ops.wgrad_join(dev)
        assert acc is None or dx is acc
        return dx.cpu(), dgamma.cpu(), dbeta.cpu()

    got = {(defer, accumulate): run(defer, accumulate) for defer in (False, True) for accumulate in (False, True)}
    for (defer, accumulate), (dx, dgamma, dbeta) in got.items():
        _close(dx - (start if accumulate else 0.0), want_dx)
        _close(dgamma - 1.0, want_dg)
        _close(dbeta + 2.0, want_db)
    for accumulate in (False, True):  # the immediate and the deferred reduction: the same bits
        for a, b in zip(got[(False, accumulate)], got[(True, accumulate)]):
            assert torch.equal(a, b)
    for a, b in zip(got[(False, True)], run(False, True)):  # run to run: the same bits
        assert torch.equal(a, b)
    for a, b in zip(got[(True, False)], run(True, False)):
        assert torch.equal(a, b)

    # the entry point itself, dx and the workspace each between two canary blocks
    lib = _lib.load()
    n_ws, pad = lib.evmi_layernorm_bwd_cbt_f32_ws_elems(C, N), 4096
    assert n_ws == (N + 63) // 64 * 2 * C
    for accumulate in (0, 1):
        dx_buf = torch.full((pad + C * N + pad,), CANARY, device=dev)
        ws_buf = torch.full((pad + n_ws + pad,), CANARY, device=dev)
        dx, ws = dx_buf[pad:pad + C * N], ws_buf[pad:pad + n_ws]
        if accumulate:
            dx.copy_(start.to(dev).reshape(-1))
        dgamma, dbeta = torch.full((C,), 1.0, device=dev), torch.full((C,), -2.0, device=dev)
        rc = lib.evmi_layernorm_bwd_cbt_f32(xg.data_ptr(), gg.data_ptr(), dyg.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                            ws.data_ptr(), n_ws, C, N, 1e-5, accumulate, _lib.current_stream_ptr(dev))
        assert rc == 0, lib.evmi_last_error()
        torch.cuda.synchronize()
        for buf, n in ((dx_buf, C * N), (ws_buf, n_ws)):
            assert bool((buf[:pad] == CANARY).all()) and bool((buf[pad + n:] == CANARY).all())
        assert bool((ws != CANARY).all())  # every partial sum of every workgroup was written
        want = got[(False, bool(accumulate))]
        assert torch.equal(dx.cpu().reshape(C, 1, N), want[0]) and torch.equal(dgamma.cpu(), want[1]) and torch.equal(dbeta.cpu(), want[2])


@pytest.mark.parametrize("B,T", [(4, 112), (3, 64), (1, 193)])
@pytest.mark.parametrize("C", [288, 384, 512, 1024])
def test_layernorm_written_as_the_packed_input_wide(cuda_device, C, B, T):
    """tests/test_gpu_fs2_train.py::test_layernorm_written_as_the_packed_input_of_the_dense_layer_behind_it at c_in above 256: the
    fused LayerNorm -> dense against LayerNorm then the layer (which packs the same values), 2e-6 for y, dh, dw, db."""
    from everyvoice_amd.train import ops

    F_ = 2 * C
    g = torch.Generator().manual_seed(B + T + C)
    x = (torch.randn(C, B, T, generator=g) * 1.7 + 0.3).to(cuda_device)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(cuda_device), (torch.randn(C, generator=g) * 0.1).to(cuda_device)
    w = (torch.randn(F_, C, 1, generator=g) * C ** -0.5).to(cuda_device)
    b = (torch.randn(F_, generator=g) * 0.1).to(cuda_device)
    dy = torch.randn(F_, B, T, generator=g).to(cuda_device)
    with ops.mode(operands="bf16"):
        assert ops.ln_dense_fused_supported(B, T, C, F_)
        k1, k2 = {}, {}
        h = ops.layernorm(x, gamma, beta)
        y = ops.conv1d_fwd(h, w, b, 1, 0, 1, 1, keep=k1)
        y_f = ops.layernorm_dense_fwd(x, gamma, beta, w, b, k2)
        dw, db, ew, eb = torch.zeros_like(w), torch.zeros_like(b), torch.zeros_like(w), torch.zeros_like(b)
        dh, _, _ = ops.conv1d_bwd(h, w, dy, 1, 0, 1, 1, need_dx=True, dw_out=dw, db_out=db, accumulate=True, packed=k1)
        dh_f, _, _ = ops.conv1d_bwd(x, w, dy, 1, 0, 1, 1, need_dx=True, dw_out=ew, db_out=eb, accumulate=True, packed=k2)
        ops.wgrad_join(cuda_device)
        torch.cuda.synchronize()
    rel = lambda got, want: float((got - want).abs().max() / want.abs().max())  # noqa: E731
    for name, got, want in (("y", y_f, y), ("dh", dh_f, dh), ("dw", ew, dw), ("db", eb, db)):
        assert rel(got, want) <= 2e-6, (name, rel(got, want))


@pytest.mark.parametrize("C", [96, 192, 264])
def test_other_widths_keep_the_separate_operators(cuda_device, C):
    """No multiple of 32 above 256, and nothing up to 256 but 128 / 256: LayerNorm and the dense layer stay two operators."""
    from everyvoice_amd.train import ops

    with ops.mode(operands="bf16"):
        assert not ops.ln_dense_fused_supported(4, 112, C, 2 * C)
        assert not ops.ffn_packed_supported(4, 112, C, 2 * C, C)
        assert ops.ln_dense_fused_supported(4, 112, 256, 512) and ops.ln_dense_fused_supported(4, 112, 128, 256)
