"""Host-side argument refusals of the fp32 training primitives (csrc/train_ops.hip): every call below must return before any HIP
call is made, with the documented code and a message that names the entry point.  No GPU is needed -- the pointers handed over are
host memory (or NULL) and are never dereferenced, which is exactly what is asserted: a refusal that came after a launch would end
in EVMI_ERR_HIP on a machine without a device."""

import pytest
import torch

from everyvoice_amd import _lib

EVMI_ERR_INVALID_ARG = 1

_BUF = torch.zeros(64)  # 64-byte aligned host memory standing in for every device pointer
P = _BUF.data_ptr()
assert P % 16 == 0


def refused(name, *args, code=EVMI_ERR_INVALID_ARG, says=None):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == code, f"{name}{args}: returned {rc} ({msg!r}), wanted {code}"
    stem = says or name[len("evmi_"):].rsplit("_f32", 1)[0]
    assert stem in msg, f"{name}: evmi_last_error() = {msg!r} does not name the function ({stem!r})"
    return msg


# (entry point, arguments) -- one refused call each; P is a valid non-null pointer, 0 is NULL
CASES = [
    # period view: non-positive sizes, and a reflect pad >= T (T = 5, period = 11 pads 6 samples: index 2 (T - 1) - t < 0)
    ("evmi_period_view_f32", (P, P, 1, 5, 0, 0, None)),
    ("evmi_period_view_f32", (P, P, 1, 0, 3, 0, None)),
    ("evmi_period_view_f32", (P, P, 0, 5, 3, 0, None)),
    ("evmi_period_view_f32", (P, P, 1, 5, 11, 0, None)),
    ("evmi_period_view_f32", (P, P, 1, 5, 11, 1, None)),
    ("evmi_period_view_f32", (P, P, 1, 3, 6, 0, None)),   # pad == T exactly
    ("evmi_period_view_f32", (0, P, 1, 5, 3, 0, None)),
    # STFT framing: n_fft / 2 >= T, hop < 1
    ("evmi_stft_frames_f32", (P, P, 1, 8, 16, 4, 0, None)),
    ("evmi_stft_frames_f32", (P, P, 1, 8, 16, 4, 1, None)),
    ("evmi_stft_frames_f32", (P, P, 1, 100, 16, 0, 0, None)),
    ("evmi_stft_frames_f32", (P, P, 0, 100, 16, 4, 0, None)),
    ("evmi_avgpool4s2_f32", (P, P, 0, 8, 0, None)),
    ("evmi_avgpool4s2_f32", (P, P, 2, 0, 0, None)),
    ("evmi_avgpool4s2_f32", (P, P, 2, 0, 1, None)),
    # row reductions
    ("evmi_row_reduce_f32", (1, P, 0, P, 2, 8, 1.0, 0, None)),   # mode 1 reads b
    ("evmi_row_reduce_f32", (0, P, 0, P, 0, 8, 1.0, 0, None)),
    ("evmi_row_reduce_f32", (2, P, 0, P, 2, 0, 1.0, 0, None)),
    ("evmi_row_reduce_f32", (3, P, P, P, 2, 8, 1.0, 0, None)),
    ("evmi_row_reduce_f32", (0, 0, 0, P, 2, 8, 1.0, 0, None)),
    ("evmi_lrelu_bwd_rowsum_f32", (P, P, P, P, 0, 8, 0.1, 0, None)),
    ("evmi_lrelu_bwd_rowsum_f32", (P, P, P, P, 2, 0, 0.1, 0, None)),
    ("evmi_lrelu_bwd_rowsum_f32", (P, P, 0, P, 2, 8, 0.1, 0, None)),
    ("evmi_scalar_reduce_f32", (0, P, 0, P, 8, 1.0, 0.0, 0, None)),   # mode 0 reads b
    ("evmi_scalar_reduce_f32", (2, P, 0, P, 0, 1.0, 0.0, 0, None)),
    ("evmi_scalar_reduce_f32", (1, P, 0, P, -3, 1.0, 0.0, 0, None)),
    ("evmi_scalar_reduce_f32", (3, P, P, P, 8, 1.0, 0.0, 0, None)),
    # elementwise: size, op code, missing operands
    ("evmi_elementwise_f32", (5, P, 0, 0, P, 0, 1.0, 0.0, None)),
    ("evmi_elementwise_f32", (5, P, 0, 0, P, -1, 1.0, 0.0, None)),
    ("evmi_elementwise_f32", (25, P, P, P, P, 8, 1.0, 0.0, None)),
    ("evmi_elementwise_f32", (-1, P, P, P, P, 8, 1.0, 0.0, None)),
    ("evmi_elementwise_f32", (0, 0, 0, 0, P, 8, 1.0, 0.0, None)),
    ("evmi_normalize_vec_f32", (P, P, 0, 1e-12, None)),
    ("evmi_normalize_vec_f32", (P, P, -4, 1e-12, None)),
    # optimiser: kind, size, pointers, alignment
    ("evmi_optimizer_step_f32", (3, P, P, P, P, 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None, 0.0, None), "optimizer_step"),
    ("evmi_optimizer_step_f32", (-1, P, P, P, P, 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None, 0.0, None), "optimizer_step"),
    ("evmi_optimizer_step_f32", (0, P, P, P, P, 0, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None, 0.0, None), "optimizer_step"),
    ("evmi_optimizer_step_f32", (0, 0, P, P, P, 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None, 0.0, None), "optimizer_step"),
    ("evmi_optimizer_step_f32", (0, P, 0, P, P, 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None, 0.0, None), "optimizer_step"),
    ("evmi_optimizer_step_f32", (0, P, P, P, 0, 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None, 0.0, None), "optimizer_step"),
    ("evmi_optimizer_step_f32", (0, P, P, 0, P, 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None, 0.0, None), "optimizer_step"),   # AdamW needs m
    ("evmi_optimizer_step_f32", (1, P, P, 0, P, 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None, 0.0, None), "optimizer_step"),   # Adam needs m
    ("evmi_optimizer_step_f32", (0, P + 4, P, P, P, 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None, 0.0, None), "optimizer_step"),
    ("evmi_optimizer_step_f32", (0, P, P + 8, P, P, 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None, 0.0, None), "optimizer_step"),
    ("evmi_optimizer_step_f32", (0, P, P, P + 12, P, 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None, 0.0, None), "optimizer_step"),
    ("evmi_optimizer_step_f32", (2, P, P, 0, P + 4, 8, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None, 0.0, None), "optimizer_step"),
    ("evmi_optimizer_step_lrdev_f32", (0, P, P, P, P, 8, 0, 0.9, 0.99, 1e-8, 0.0, P, 0.0, None), "optimizer_step"),   # lr_dev NULL
    ("evmi_optimizer_step_lrdev_f32", (0, P, P, P, P, 8, P, 0.9, 0.99, 1e-8, 0.0, 0, 0.0, None), "optimizer_step"),   # step_dev NULL
    ("evmi_optimizer_step_lrdev_f32", (7, P, P, P, P, 8, P, 0.9, 0.99, 1e-8, 0.0, P, 0.0, None), "optimizer_step"),
    ("evmi_optimizer_step_lrdev_f32", (0, P, P, P, P, 0, P, 0.9, 0.99, 1e-8, 0.0, P, 0.0, None), "optimizer_step"),
    ("evmi_adamw_f32", (P, P, P, P, 0, 1e-3, 0.9, 0.99, 1e-8, 0.0, 1, None)),
    # row-wise helpers, layout changes, norms: non-positive sizes
    ("evmi_bias_add_rows_f32", (P, P, 0, 8, None)),
    ("evmi_bias_add_rows_f32", (P, P, 2, 0, None)),
    ("evmi_transpose_bct_cbt_f32", (P, P, 0, 2, 3, None)),
    ("evmi_transpose_bct_cbt_f32", (P, P, 2, 0, 3, None)),
    ("evmi_transpose_bct_cbt_f32", (P, P, 2, 2, 0, None)),
    ("evmi_reflect_pad_left1_f32", (P, P, 0, 4, 0, None)),
    ("evmi_reflect_pad_left1_f32", (P, P, 2, 1, 0, None)),   # one sample has nothing to reflect
    ("evmi_reflect_pad_left1_f32", (P, P, 2, 1, 1, None)),
    ("evmi_spectral_norm_grad_f32", (P, P, P, P, P, P, 0, 4, None)),
    ("evmi_spectral_norm_grad_f32", (P, P, P, P, P, P, 4, 0, None)),
    ("evmi_spectral_norm_grad_f32", (P, P, P, P, 0, P, 4, 4, None)),
    ("evmi_weight_norm_fwd_f32", (P, P, P, P, 0, 4, None)),
    ("evmi_weight_norm_fwd_f32", (P, P, P, P, 4, 0, None)),
    ("evmi_weight_norm_bwd_f32", (P, P, P, P, P, P, 0, 4, None)),
    ("evmi_weight_norm_bwd_f32", (P, P, P, P, P, P, 4, 0, None)),
    ("evmi_weight_norm_fwd_batched_f32", (P, P, P, P, 0, 0, 4, None)),
    ("evmi_weight_norm_fwd_batched_f32", (P, P, P, P, 2, 4, 4, None)),   # empty row range
    ("evmi_weight_norm_bwd_batched_f32", (P, P, P, P, P, 0, 0, 4, None)),
    ("evmi_weight_norm_bwd_batched_f32", (P, P, P, P, P, 2, 5, 4, None)),
    ("evmi_istft_polar_f32", (P, P, 0, 4, None)),
    ("evmi_istft_polar_bwd_f32", (P, P, P, 4, 0, None)),
    ("evmi_gemm_f32", (0, 0, 0, 4, 4, 1.0, P, 4, P, 4, 0.0, P, 4, None)),
    ("evmi_gemm_f32", (0, 0, 4, 4, 0, 1.0, P, 4, P, 4, 0.0, P, 4, None)),
    ("evmi_gemm_batched_f32", (0, 0, 4, 4, 4, 1.0, P, 4, 16, P, 4, 16, 0.0, P, 4, 16, 0, None)),
    ("evmi_ratio_accumulate_f32", (P, 0, 1.0, None)),
]


def _case_id(c):
    return c[0][len("evmi_"):] + "-" + "_".join("p" if a == P else ("pu" if isinstance(a, int) and a > P else str(a)) for a in c[1])


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_refused_on_the_host_with_the_documented_code(case):
    name, args = case[0], case[1]
    refused(name, *args, says=case[2] if len(case) > 2 else None)
    assert torch.count_nonzero(_BUF) == 0  # (nothing was written through the stand-in pointer)


# The FastSpeech2 forward and alignment entry points (csrc/fs2_ops.hip, csrc/align_train_ops.hip): non-positive sizes, an odd D of the
# sinusoid (its second half reads inv_freq[c - D / 2]: one past the table for the last channel), and the token limits of the header.
# (entry point, arguments, code, the name evmi_last_error() carries)
EVMI_ERR_UNSUPPORTED = 4
FS2_CASES = [
    ("evmi_fs2_add_posemb_f32", (P, P, P, 2, 4, 7, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_add_posemb_f32", (P, P, P, 2, 4, 1, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_add_posemb_f32", (P, P, P, 0, 4, 8, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_add_posemb_f32", (P, P, P, 2, 0, 8, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_add_posemb_f32", (P, P, P, 2, 4, 0, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_add_posemb_f32", (P, P, P, 2, -4, 8, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_embed_f32", (P, P, P, P, P, 2, 4, 7, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_mask_cols_f32", (P, P, 0, 2, 4, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_mask_cols_f32", (P, P, 8, 0, 4, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_mask_cols_f32", (P, P, 8, 2, -1, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_bucket_embed_add_f32", (P, P, P, P, 4, 0, 4, 8, 1.0, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_bucket_embed_add_f32", (P, P, P, P, 4, 2, 0, 8, 1.0, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_bucket_embed_add_f32", (P, P, P, P, 4, 2, 4, -8, 1.0, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_bucket_embed_add_f32", (P, P, P, P, 1, 2, 4, 8, 1.0, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_durations_i32", (P, P, P, 0, 4, 1.0, None), EVMI_ERR_INVALID_ARG, "fs2_durations"),
    ("evmi_fs2_durations_i32", (P, P, P, 2, -4, 1.0, None), EVMI_ERR_INVALID_ARG, "fs2_durations"),
    ("evmi_fs2_add_item_embedding_f32", (P, P, P, P, 0, 4, 8, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_add_item_embedding_f32", (P, P, P, P, 2, 0, 8, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_fs2_add_item_embedding_f32", (P, P, P, P, 2, 4, 0, None), EVMI_ERR_INVALID_ARG, None),
    ("evmi_layernorm_cbt_f32", (P, P, P, P, 1025, 2, 1e-5, None), EVMI_ERR_UNSUPPORTED, None),
    ("evmi_forward_sum_grad_f32", (P, P, P, P, P, P, 2 * 2049 + 2, 1, 2, 1024, -1.0, 1.0, None), EVMI_ERR_UNSUPPORTED, None),   # 2049 states
    ("evmi_forward_sum_grad_f32", (P, P, P, P, P, P, 2 * 19 + 2 - 1, 1, 2, 9, -1.0, 1.0, None), EVMI_ERR_INVALID_ARG, None),   # workspace one short
    ("evmi_forward_sum_loss_f32", (P, P, P, P, 1, 8, 3275, -1.0, None), EVMI_ERR_UNSUPPORTED, None),   # (5 L + 11) floats > 64 KiB
    ("evmi_monotonic_align_f32", (P, P, P, P, P, P, 1, 2, 8193, None), EVMI_ERR_UNSUPPORTED, None),    # 2 L floats > 64 KiB
]


@pytest.mark.parametrize("case", FS2_CASES, ids=[_case_id(c) for c in FS2_CASES])
def test_fs2_and_alignment_entry_points_refuse_on_the_host(case):
    name, args, code, says = case
    refused(name, *args, code=code, says=says)
    assert torch.count_nonzero(_BUF) == 0


def test_the_header_states_the_token_limits():
    from pathlib import Path

    text = " ".join((Path(__file__).resolve().parent.parent / "include" / "evmi.h").read_text().split())
    for phrase in ("L <= 1023", "L <= 3274", "L <= 8192"):
        assert phrase in text, phrase


# elementwise op codes and the operands they read besides `a`(the table beside ew_reads in csrc/train_ops.hip, restated)
_EW_READS_B = {1, 3, 4, 6, 7, 10, 11, 12, 15, 17, 18, 19, 22}
_EW_READS_C = {12, 20, 21, 22, 24}


@pytest.mark.parametrize("op", range(25))
def test_elementwise_refuses_a_missing_operand(op):
    if op in _EW_READS_B:
        assert "reads b" in refused("evmi_elementwise_f32", op, P, 0, P, P, 8, 1.0, 0.5, None)
    if op in _EW_READS_C:
        assert "reads c" in refused("evmi_elementwise_f32", op, P, P, 0, P, 8, 1.0, 0.5, None)
    # whatever it reads, an empty call is refused as well (before the launch that would have had a zero-size grid)
    refused("evmi_elementwise_f32", op, P, P, P, P, 0, 1.0, 0.5, None)


def test_the_header_states_the_enforced_preconditions():
    """include/evmi.h is the contract: the refusals above are written down where a binder reads them."""
    from pathlib import Path

    text = (Path(__file__).resolve().parent.parent / "include" / "evmi.h").read_text()
    for phrase in ("16-byte aligned", "shorter than T", "EVMI_ERR_INVALID_ARG before anything is launched"):
        assert phrase in text, phrase


def test_wrappers_leave_empty_tensors_alone():
    """fill_ / copy / zeros are called on whatever a model holds, including nothing (a zero-element bias): the library refuses
    n == 0, so the wrappers return an empty tensor untouched instead of calling it.  Host tensors: no launch happens."""
    from everyvoice_amd.train import ops

    e = torch.empty(0)
    assert ops.fill_(e, 3.0) is e
    assert ops.copy(e).numel() == 0
    out = torch.empty(0)
    assert ops.copy(e, out=out) is out
    assert ops.elementwise(ops.EW_SCALE, torch.empty(0, 4), p0=2.0).shape == (0, 4)
