"""Alignment scores, host side (no GPU): the two declarations and their symbols, the plan query, the refusals of
``evmi_align_scores_f32`` -- decided before any device work, so they hold with host pointers that are never dereferenced --, the
refusals of ``FastSpeech2.align`` and ``score_alignments`` that need no device, the float64 restatement of tests/align_scores_ref.py
against an explicit lattice, and THE CALIBRATION of the bound the GPU tests use, on every input they use."""

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import align_ref as R
import align_scores_ref as S
from everyvoice_amd import _lib

_BUF = torch.zeros(64)  # host memory standing in for every device pointer
P = _BUF.data_ptr()


def test_declared_in_the_header_and_exported():
    names = {name: params for name, _, params in _lib.declarations()}
    assert [t for t, _ in names["evmi_align_scores_plan"]] == ["int", "int", "int*", "int*"]
    assert [n for _, n in names["evmi_align_scores_f32"]] == ["q_dev", "k_dev", "prior_dev", "text_lens_dev", "mel_lens_dev", "dur_dev", "ctc_dev",
                                                             "path_dev", "symbol_dev", "A", "B", "T", "L", "temperature", "blank_logprob", "stream"]
    lib = _lib.load()
    assert lib.evmi_align_scores_plan is not None and lib.evmi_align_scores_f32 is not None
    assert lib.evmi_abi_version() == 2


def test_plan_query():
    """Host arithmetic: tiles are whole units of 8 frames, at most 64; the k image leaves the LDS once and for all as L grows; the
    largest launch still has a tile; the refusals are the launch's."""
    from everyvoice_amd.train import ops

    for A in (1, 3, 80, 128):
        inside = []
        for L in (1, 20, 64, 65, 255, 256, 257, 512, 1000, 1023):
            ty, klds = S.plan(A, L)
            assert ty % 8 == 0 and 8 <= ty <= 64, (A, L, ty)
            assert ops.align_scores_plan(A, L) == (ty, klds)
            inside.append(klds)
        assert inside == sorted(inside, reverse=True), (A, inside)
    assert S.plan(1, 1) == (64, True) and not S.plan(128, 1023)[1]
    sw = S.k_switch()
    assert S.plan(R.A_PLANTED, sw)[1] and not S.plan(R.A_PLANTED, sw + 1)[1] and sw + 444 <= 1100
    lib, ty, klds = _lib.load(), ctypes.c_int(-1), ctypes.c_int(-1)
    for args, code in (((0, 5), _lib.EVMI_ERR_INVALID_ARG), ((80, 0), _lib.EVMI_ERR_INVALID_ARG), ((129, 5), _lib.EVMI_ERR_UNSUPPORTED),
                       ((80, 1024), _lib.EVMI_ERR_UNSUPPORTED)):
        assert lib.evmi_align_scores_plan(*args, ctypes.byref(ty), ctypes.byref(klds)) == code
        assert (ty.value, klds.value) == (-1, -1)
    assert lib.evmi_align_scores_plan(80, 5, None, ctypes.byref(klds)) == _lib.EVMI_ERR_INVALID_ARG


# evmi_align_scores_f32(q, k, prior, text_lens, mel_lens, dur, ctc, path, symbol, A, B, T, L, temperature, blank_logprob, stream)
REFUSED = [
    ((0, P, P, P, P, P, P, P, P, 80, 2, 9, 5, 0.5, -1.0, None), "INVALID", "null"),
    ((P, 0, P, P, P, P, P, P, P, 80, 2, 9, 5, 0.5, -1.0, None), "INVALID", "null"),
    ((P, P, 0, 0, P, P, P, P, P, 80, 2, 9, 5, 0.5, -1.0, None), "INVALID", "null"),   # (a NULL prior alone is no refusal: text_lens is)
    ((P, P, P, P, 0, P, P, P, P, 80, 2, 9, 5, 0.5, -1.0, None), "INVALID", "null"),
    ((P, P, P, P, P, 0, P, P, P, 80, 2, 9, 5, 0.5, -1.0, None), "INVALID", "null"),
    ((P, P, P, P, P, P, 0, P, P, 80, 2, 9, 5, 0.5, -1.0, None), "INVALID", "null"),
    ((P, P, P, P, P, P, P, 0, P, 80, 2, 9, 5, 0.5, -1.0, None), "INVALID", "null"),
    ((P, P, P, P, P, P, P, P, 0, 80, 2, 9, 5, 0.5, -1.0, None), "INVALID", "null"),
    ((P, P, P, P, P, P, P, P, P, 0, 2, 9, 5, 0.5, -1.0, None), "INVALID", "shape"),
    ((P, P, P, P, P, P, P, P, P, 80, 0, 9, 5, 0.5, -1.0, None), "INVALID", "shape"),
    ((P, P, P, P, P, P, P, P, P, 80, 2, -1, 5, 0.5, -1.0, None), "INVALID", "shape"),
    ((P, P, P, P, P, P, P, P, P, 80, 2, 9, 0, 0.5, -1.0, None), "INVALID", "shape"),
    ((P, P, P, P, P, P, P, P, P, 129, 2, 9, 5, 0.5, -1.0, None), "UNSUPPORTED", "128"),
    ((P, P, P, P, P, P, P, P, P, 80, 2, 2000, 1024, 0.5, -1.0, None), "UNSUPPORTED", "1023"),
]


@pytest.mark.parametrize("args,code,says", REFUSED, ids=[f"{c}-{s}-{i}" for i, (_, c, s) in enumerate(REFUSED)])
def test_refusals_before_any_device_work(args, code, says):
    lib = _lib.load()
    rc = lib.evmi_align_scores_f32(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == {"INVALID": _lib.EVMI_ERR_INVALID_ARG, "UNSUPPORTED": _lib.EVMI_ERR_UNSUPPORTED}[code], (rc, msg)
    assert "align_scores" in msg and says in msg, msg


def _namespace_model(aligner=True):
    from everyvoice_amd.fs2 import FastSpeech2ModelConfig

    return SimpleNamespace(config=FastSpeech2ModelConfig(), device=torch.device("cpu"), _ready=True, has_aligner=aligner)


def test_align_refusals_before_any_launch():
    """The model object has no weights and no device: every refusal comes before the projections."""
    from everyvoice_amd.fs2 import AlignmentScores, FastSpeech2

    assert AlignmentScores._fields == ("ctc", "path", "symbol")
    model = _namespace_model()
    ids, lens, mel, mel_lens = torch.ones(2, 4, dtype=torch.long), torch.tensor([4, 3]), torch.zeros(2, 9, 80), torch.tensor([9, 7])
    good = torch.tensor([[2, 2, 2, 3], [1, 5, 1, 0]])
    align = lambda **kw: FastSpeech2.align(model, ids, lens, mel, mel_lens, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="no aligner"):
        FastSpeech2.align(_namespace_model(aligner=False), ids, lens, mel, mel_lens, return_scores=True)
    with pytest.raises(ValueError, match="return_scores"):
        align(durations=good)
    with pytest.raises(ValueError, match=r"expected \[2, 4\] integers"):
        align(durations=good[:, :3], return_scores=True)
    with pytest.raises(ValueError, match=r"expected \[2, 4\] integers"):
        align(durations=good.float(), return_scores=True)
    for bad, says in ((torch.tensor([[2, 2, 2, 3], [1, 5, 2, 0]]), "item 1.*8 frames.*has 7"), (torch.tensor([[2, 2, 2, 2], [1, 5, 1, 0]]), "item 0.*8 frames.*has 9"),
                      (torch.tensor([[2, 2, 2, 3], [1, 7, -1, 0]]), "item 1.*least entry -1"), (torch.tensor([[2, 2, 2, 3], [1, 5, 1, 9]]).int(), None)):
        if says is None:  # (beyond the item's symbols nothing is read: this row passes the check and reaches the projections)
            with pytest.raises(AttributeError):
                align(durations=bad, return_scores=True)
        else:
            with pytest.raises(ValueError, match=says):
                align(durations=bad, return_scores=True)
    with pytest.raises(ValueError, match="item 1"):
        FastSpeech2.align(model, ids, lens, mel, torch.tensor([9, 2]), return_scores=True)


def test_score_alignments_and_synthesis_refusals(tmp_path):
    from everyvoice_amd.pipeline import ALIGNMENT_SCORE_FIELDS, generate_teacher_forced_specs, score_alignments, synthesize_helper

    assert ALIGNMENT_SCORE_FIELDS == ("basename", "speaker", "language", "symbols", "frames", "seconds", "symbols_per_second", "attn_ctc", "attn_path",
                                      "worst_symbol", "worst_symbol_score")
    rows = [{"basename": "utt0", "ids": [1, 2, 3], "speaker": "default", "language": "default"}]
    with pytest.raises(ValueError, match="no aligner"):  # ... before any file is read: the folder does not exist
        score_alignments(_namespace_model(aligner=False), rows, tmp_path / "absent", out_path=tmp_path / "scores.psv")
    with pytest.raises(FileNotFoundError, match="utt0--default--default--spec-22050-mel-librosa.pt"):
        score_alignments(_namespace_model(), rows, tmp_path, out_path=tmp_path / "scores.psv")
    assert not (tmp_path / "scores.psv").exists()
    with pytest.raises(ValueError, match="alignment_scores needs a teacher_forcing_directory"):
        synthesize_helper(_namespace_model(), [[1, 2, 3]], None, None, 1.0, 0, ["spec"], output_dir=tmp_path / "out", alignment_scores=True)
    assert not (tmp_path / "out").exists()
    import inspect

    assert inspect.signature(generate_teacher_forced_specs).parameters["alignment_scores"].default is False
    assert inspect.signature(synthesize_helper).parameters["return_scores"].default is False  # (the reference's keyword: left alone)


# =====================================================================================================================
# the restatement
# =====================================================================================================================
@pytest.mark.parametrize("T,L", [(1, 1), (9, 1), (2, 2), (15, 5), (130, 63), (400, 65), (300, 257)])
def test_explicit_lattice_agrees_with_ctc_loss(T, L):
    from oracle.alignment_ref import forward_sum_loss_ref

    lp = torch.randn(T, L, generator=torch.Generator().manual_seed(1000 * L + T), dtype=torch.float64) * 2
    want = float(forward_sum_loss_ref(lp[None], torch.tensor([L]), torch.tensor([T]), S.BLANK))
    assert abs(S.ctc_lattice_f64(lp.numpy()) - want) <= 1e-12 * max(1.0, abs(want))


def test_restated_scores_on_a_hand_case():
    """Two symbols over three frames, no prior, temperature 1, one channel: every number by hand."""
    q, k = np.array([[0.0, 0.0, 2.0]], dtype=np.float32), np.array([[0.0, 2.0]], dtype=np.float32)
    soft, lp = S.attention(q, k, None, 1.0)
    assert np.array_equal(lp.numpy(), [[-0.0, -4.0], [-0.0, -4.0], [-4.0, -0.0]])
    near, far = -np.log1p(np.exp(-4.0)), -4.0 - np.log1p(np.exp(-4.0))
    ctc, path, symbol = S.scores_from(soft, lp, [2, 1])
    assert abs(path + near) < 1e-15 and np.allclose(symbol, [near, near], atol=1e-15)
    _, path, symbol = S.scores_from(soft, lp, [1, 2])
    assert abs(path + (2 * near + far) / 3) < 1e-15 and np.allclose(symbol, [near, (near + far) / 2], atol=1e-15)
    _, _, symbol = S.scores_from(soft, lp, [3, 0])
    assert np.isnan(symbol[1]) and abs(symbol[0] - (2 * near + far) / 3) < 1e-15
    assert abs(ctc - S.ctc_lattice_f64(lp.numpy())) < 1e-14
    # least_shift_ratio: from (2, 1) only "symbol 1 takes the last frame of symbol 0" can move; symbol 1's mean goes from near to (near + far) / 2
    assert abs(S.least_shift_ratio(soft.numpy(), [2, 1], np.array([1.0, 0.5])) - abs(far - near)) < 1e-12


# =====================================================================================================================
# the calibration
# =====================================================================================================================
@pytest.mark.parametrize("case", S.kernel_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_calibration(case):
    """On every input of the GPU tests: finite float64 scores with a positive CTC loss; 4 x err32 < 0.05 x ctc (a dropped, doubled or
    misplaced lattice state is an error of the order of the loss itself: 20 x outside the bound); moving any one boundary of the scored
    path by one frame moves a per-symbol score by at least 10 x that symbol's bound (a frame-to-symbol map off by one is seen)."""
    L, T, setting, A = case
    r = S.planted_scores(*case)
    assert np.isfinite([r["ctc"], r["path"]]).all() and np.isfinite(r["symbol"]).all() and r["ctc"] > 0
    assert R.structure_ok(r["dur"], T, L)
    if A == R.A_PLANTED and setting in ("prior", "model_temperature", "model"):
        assert np.array_equal(r["dur"], R.planted_reference(L, T, setting)["optimum"])
    print(f"calibration {case}: ctc {r['ctc']:.4f} err32 / ctc {r['ctc_err32'] / r['ctc']:.2e}; path {r['path']:.4f} err32 {r['path_err32']:.2e}; "
          f"symbol err32 max {r['symbol_err32'].max():.2e}; least shift ratio {r['shift_ratio']:.1f}")
    assert S.FACTOR * r["ctc_err32"] < 0.05 * r["ctc"], (r["ctc_err32"], r["ctc"])
    assert r["shift_ratio"] >= 10.0, r["shift_ratio"]


def test_the_cases_stand_on_both_sides_of_every_switch():
    cases = S.kernel_cases()
    shapes = {(L, T) for L, T, _, A in cases if A == R.A_PLANTED}
    ty, sw = S.plan(R.A_PLANTED, 20)[0], S.k_switch()
    asked = {(1, 1), (1, 9), (2, 2), (5, 15), (63, 130), (64, 64), (65, 400), (1000, 1000), (1023, 1100),
             (20, ty - 1), (20, ty), (20, ty + 1), (20, 2 * ty + 1), (sw, sw + 344), (sw + 1, sw + 444)}
    assert asked <= shapes
    # the product: every one of these shapes in every setting (both temperatures, with and without the prior)
    assert {"prior", "model_temperature", "model"} < set(S.SETTINGS) and {S.SETTINGS[s] for s in S.SETTINGS} == {(t, p) for t in (0.05, 0.0005) for p in (True, False)}
    assert {(L, T, s, R.A_PLANTED) for L, T in asked for s in S.SETTINGS} <= set(cases)
    assert any(L == sw and T > L for L, T in shapes) and any(L == sw + 1 for L, T in shapes)
    assert S.ACROSS_SWITCH in S.RAGGED and S.ACROSS_SWITCH[0] <= sw
    assert {A for *_, A in cases} == {3, R.A_PLANTED, 128}
    for name in S.SETTINGS:
        assert sum(1 for c in cases if c[2] == name) >= 15
    assert all((Lb, Tb, S.RAGGED_SETTING, R.A_PLANTED) in cases for Lb, Tb in S.RAGGED)
