"""The aligner at inference, host side (no GPU): the refusals of ``evmi_align_durations_f32`` -- decided before any device work, so they
hold with host pointers that are never dereferenced, as in tests/test_abi_arguments.py --, its workspace size, the aligner's key
table against the oracle's module, and the float64 restatement of tests/align_ref.py against the oracle's search on the planted
inputs the GPU tests use."""

import numpy as np
import pytest
import torch

import align_ref as R
from everyvoice_amd import _lib
from oracle.alignment_ref import AlignerRef
from oracle.mas_ref import maximum_path_ref

_BUF = torch.zeros(64)  # 64-byte aligned host memory standing in for every device pointer
P = _BUF.data_ptr()
assert P % 16 == 0
BIG = 1 << 40  # a workspace size no shape below exceeds

# evmi_align_durations_f32(q, k, prior, text_lens, mel_lens, dur, ws, ws_bytes, A, B, T, L, temperature, stream)
REFUSED = [
    ((0, P, P, P, P, P, P, BIG, 80, 2, 9, 5, 0.5, None), "INVALID", "null"),
    ((P, 0, P, P, P, P, P, BIG, 80, 2, 9, 5, 0.5, None), "INVALID", "null"),
    ((P, P, 0, 0, P, P, P, BIG, 80, 2, 9, 5, 0.5, None), "INVALID", "null"),   # (a NULL prior alone is no refusal: text_lens is)
    ((P, P, P, P, 0, P, P, BIG, 80, 2, 9, 5, 0.5, None), "INVALID", "null"),
    ((P, P, P, P, P, 0, P, BIG, 80, 2, 9, 5, 0.5, None), "INVALID", "null"),
    ((P, P, P, P, P, P, 0, BIG, 80, 2, 9, 5, 0.5, None), "INVALID", "null"),
    ((P, P, P, P, P, P, P, BIG, 0, 2, 9, 5, 0.5, None), "INVALID", "shape"),
    ((P, P, P, P, P, P, P, BIG, 80, 0, 9, 5, 0.5, None), "INVALID", "shape"),
    ((P, P, P, P, P, P, P, BIG, 80, 2, -1, 5, 0.5, None), "INVALID", "shape"),
    ((P, P, P, P, P, P, P, BIG, 80, 2, 9, 0, 0.5, None), "INVALID", "shape"),
    ((P, P, P, P, P, P, P, None, 80, 2, 9, 5, 0.5, None), "INVALID", "workspace"),    # one byte short (filled in below)
    ((P, P, P, P, P, P, P + 4, BIG, 80, 2, 9, 5, 0.5, None), "INVALID", "aligned"),
    ((P, P, P, P, P, P, P, BIG, 129, 2, 9, 5, 0.5, None), "UNSUPPORTED", "128"),
    ((P, P, P, P, P, P, P, BIG, 80, 2, 2000, 1025, 0.5, None), "UNSUPPORTED", "1024"),
]


@pytest.mark.parametrize("args,code,says", REFUSED, ids=[f"{c}-{s}-{i}" for i, (_, c, s) in enumerate(REFUSED)])
def test_refusals_before_any_device_work(args, code, says):
    lib = _lib.load()
    if args[7] is None:
        args = args[:7] + (lib.evmi_align_durations_ws_bytes(args[9], args[10], args[11]) - 1,) + args[8:]
    rc = lib.evmi_align_durations_f32(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == {"INVALID": _lib.EVMI_ERR_INVALID_ARG, "UNSUPPORTED": _lib.EVMI_ERR_UNSUPPORTED}[code], (rc, msg)
    assert "align_durations" in msg and says in msg, msg


def test_workspace_size_is_monotone_and_covers_a_byte_a_cell():
    ws = _lib.load().evmi_align_durations_ws_bytes
    for B, T, L in [(1, 1, 1), (3, 40, 17), (32, 566, 100), (2, 1100, 1023), (2, 1100, 1024)]:
        n = ws(B, T, L)
        assert B * T * L <= n <= B * T * (L + 15), (B, T, L, n)   # one byte a cell, rows padded to 16 bytes at the most
        assert ws(B + 1, T, L) >= n and ws(B, T + 1, L) >= n and ws(B, T, L + 1) >= n
    steps = [ws(2, 50, L) for L in range(1, 1025)]
    assert steps == sorted(steps)
    assert ws(0, 5, 5) == ws(5, 0, 5) == ws(5, 5, 0) == 0


@pytest.mark.parametrize("d_text,n_mels", [(256, 80), (128, 80), (64, 40)])
def test_aligner_key_table_is_the_oracles(d_text, n_mels):
    from everyvoice_amd.fs2 import ConformerConfig, FastSpeech2ModelConfig, aligner_state_dict_shapes
    from everyvoice_amd.train.fs2 import _AlignerT

    c = FastSpeech2ModelConfig(encoder=ConformerConfig(input_dim=d_text), n_mels=n_mels)
    ref = AlignerRef(d_text, n_mels, n_att=_AlignerT.n_att)
    want = {"attention." + name: tuple(t.shape) for name, t in ref.state_dict().items()}
    assert aligner_state_dict_shapes(c) == want
    assert ref.temperature == _AlignerT.temperature


@pytest.mark.parametrize("setting", list(R.SETTINGS))
@pytest.mark.parametrize("L,T", R.SHAPES)
def test_restatement_agrees_with_the_oracles_search_on_the_planted_inputs(L, T, setting):
    """The float64 dynamic programme of align_ref and the oracle's float32 one, fed the same values, find the same path; it is the
    planted one and beats every single-boundary shift by the margin the GPU tests rely on."""
    r = R.planted_reference(L, T, setting)
    assert r["margin"] >= R.SETTINGS[setting][2], r["margin"]
    assert np.array_equal(r["optimum"], r["planted"])
    path = maximum_path_ref(r["value"].astype(np.float32), T, L)
    assert np.array_equal(path.sum(0), r["optimum"])
    assert R.structure_ok(r["optimum"], T, L)
    assert abs(R.path_score(r["value"], r["optimum"])) <= T * r["q_max"] + 1e-9


def test_restatement_on_ties_and_infeasible_items():
    """Values on a grid of 0.5 tie often: the restatement still follows the oracle (same tie rule); no path -> zeros."""
    rng = np.random.default_rng(7)
    for T, L in [(7, 3), (40, 40), (33, 17), (64, 5)]:
        value = np.round(rng.standard_normal((T, L)) * 2) / 2
        dur, _ = R.maximum_path_f64(value, T, L)
        assert np.array_equal(dur, maximum_path_ref(value.astype(np.float32), T, L).sum(0))
    for t_y, t_x in [(0, 3), (3, 0), (2, 3)]:
        assert not R.maximum_path_f64(np.zeros((5, 5)), t_y, t_x)[0].any()
    # the single-boundary margin: a hand case.  Tokens 0 | 1 over 4 frames, durations (2, 2): moving the boundary either way costs 3
    value = np.array([[5.0, 0.0], [4.0, 1.0], [1.0, 4.0], [0.0, 6.0]])
    assert np.array_equal(R.maximum_path_f64(value, 4, 2)[0], [2, 2]) and R.shift_margin(value, [2, 2]) == 3.0
