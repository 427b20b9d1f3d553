"""Structural facts of the convolution operators' dispatch in everyvoice_amd/train/ops.py, read off the library calls they issue
(tools/ops_call_trace.py: the recorder stands in for the library, so this runs without a GPU).  No golden trace is pinned here."""

import importlib.util
import itertools
from pathlib import Path

import pytest

_spec = importlib.util.spec_from_file_location("ops_call_trace", Path(__file__).resolve().parent.parent / "tools" / "ops_call_trace.py")
trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(trace)

BF16 = dict(operands="bf16", packed=True, wgrad="mfma", dgrad="mfma", fwd="mfma", ffn_packed=True, resdrop=True)


def test_the_recorder_leaves_the_binding_as_it_found_it():
    from everyvoice_amd import _lib

    before = _lib.load, _lib.current_stream_ptr
    trace.run_case(trace.CASES["ffn_packed_infer[n=64]"], BF16, "packed")
    assert (_lib.load, _lib.current_stream_ptr) == before


@pytest.mark.parametrize("operands,packed", [("f32", True), ("f32", False), ("bf16", False)])
def test_no_fused_form_is_supported_off_the_packed_bf16_kernels(operands, packed):
    """Every *_supported predicate is false whenever packed_bf16() is false -- whatever the library answers, without asking it."""
    preds = [name for name in trace.CASES if name.startswith("predicates")]
    assert preds
    for name, (wgrad, dgrad, fwd) in itertools.product(preds, itertools.product(("mfma", "auto", "gemm"), ("mfma", "gemm"), ("mfma", "gemm"))):
        sw = dict(BF16, operands=operands, packed=packed, wgrad=wgrad, dgrad=dgrad, fwd=fwd)
        _, _, result = trace.run_case(trace.CASES[name], sw, "packed")
        shares, ffn_fused, ln_dense, resdrop, ffn_packed = result[:5]
        assert not (shares or ffn_fused or ln_dense or resdrop or ffn_packed), (name, sw, result)


def test_the_predicates_hold_where_the_packed_kernels_take_every_product():
    _, _, result = trace.run_case(trace.CASES["predicates[b=1,t=64,c_in=256,c_mid=1024,c_out=256]"], BF16, "packed")
    assert all(result[:5])
    _, _, result = trace.run_case(trace.CASES["predicates[b=1,t=64,c_in=16,c_mid=12,c_out=256]"], BF16, "packed")
    assert result[:5] == [True, True, False, True, False]  # (LayerNorm's pack takes 128 / 256 channels; bf16(a) is stored in channel octets)


@pytest.mark.parametrize("n", [64, 77])
def test_inference_chain_passes_null_for_the_seed_base_and_the_stored_pre_activation(n):
    """ffn_packed_infer draws no mask and stores no pre-activation, also where a seed base is set (run_case sets one)."""
    calls, _, _ = trace.run_case(trace.CASES[f"ffn_packed_infer[n={n}]"], BF16, "packed")
    assert [c[0] for c in calls] == ["evmi_layernorm_pack_bf16pk_w", "evmi_conv1d_cbt_bf16pk_ffn_up", "evmi_conv1d_cbt_bf16pk_resdrop"]
    up, down = calls[1][1], calls[2][1]
    assert up[4] == "NULL" and up[12:16] == [0.0, 0, "NULL", 1]
    assert down[12:18] == [0.0, 0, 0.0, 0, 1.0, "NULL"]
    train, _, _ = trace.run_case(trace.CASES[f"ffn_packed_fwd[n={n}]"], BF16, "packed")
    assert [c[0] for c in train] == [c[0] for c in calls]
    assert train[1][1][4] == "PTR" and train[1][1][14] == "seed_base" and train[2][1][17] == "seed_base"


def test_the_three_prepacked_weight_gradient_sites_issue_the_same_two_entry_points():
    pair = ["evmi_conv1d_wgrad_cbt_bf16pk_prepacked", "evmi_pkflat_rowsum"]
    for name, n_layers in (("conv1d_bwd_silu_dropout_dy[xp=True,db=True]", 1), ("conv1d_bwd_dropout_dy[xp=True,db=True,x_standin=False]", 1),
                           ("ffn_packed_bwd[n=64,db=True]", 2)):
        calls, _, _ = trace.run_case(trace.CASES[name], BF16, "packed")
        names = [c[0] for c in calls if c[0] in pair]
        assert names == pair * n_layers, (name, names)
        for c in calls:
            if c[0] == pair[1]:  # one job: the row sums of the packed output gradient the weight gradient in front of it read
                assert c[1][0] == 1 and len(c[1][1]) == 1
    calls, _, _ = trace.run_case(trace.CASES["ffn_packed_bwd[n=64,db=False]"], BF16, "packed")
    assert [c[0] for c in calls if c[0] in pair] == pair[:1] * 2
