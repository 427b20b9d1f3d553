"""STOI, host side (no GPU): the two declarations and their symbols, the plan arithmetic, the refusals of
``evmi_stoi_f32`` -- decided before any device work, so they hold with host pointers that are never dereferenced --, the band table, the
float64 restatement of tests/stoi_ref.py against values computed independently when the measure was specified, its properties, and the
pipeline's refusals."""

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stoi_ref as R
from everyvoice_amd import _lib

_BUF = torch.zeros(64)  # host memory standing in for every device pointer
P = _BUF.data_ptr()


def _plan(S):
    from everyvoice_amd.train import ops

    return ops.stoi_plan(S)


def test_declared_in_the_header_and_exported():
    names = {name: (ret, params) for name, ret, params in _lib.declarations()}
    assert names["evmi_stoi_plan"] == ("int", [("int", "S"), ("int*", "max_n"), ("int*", "f_cap"), ("int*", "j_cap")])
    assert [n for _, n in names["evmi_stoi_f32"][1]] == ["ref_dev", "deg_dev", "ref_lens_dev", "deg_lens_dev", "stoi_dev", "counts_dev", "segment_dev",
                                                        "frame_of_dev", "B", "S_ref", "S_deg", "stream"]
    lib = _lib.load()
    assert lib.evmi_stoi_plan is not None and lib.evmi_stoi_f32 is not None
    assert lib.evmi_abi_version() == 2


def test_plan_arithmetic_and_refusals():
    max_n = _plan(1)[0]
    assert max_n >= 110000 and (max_n - 256) % 128 == 0  # 11 s at 10 kHz; a whole number of frames
    for S, F in ((1, 0), (256, 0), (257, 1), (384, 1), (385, 2), (4096, 30), (4224, 31), (4225, 32), (20000, 155), (110000, 858), (max_n, (max_n - 256) // 128)):
        assert _plan(S) == (max_n, max(F, 1), max(F - 30, 1)), S
        assert R.stoi(np.zeros(S), np.zeros(S))["F"] == F
    assert _plan(max_n + 1) == _plan(max_n) == _plan(2 ** 31 - 1)  # beyond the limit: the limit's strides
    # 2 x 15 band values, an energy and an index per frame beside the transform's slots, inside 160 KiB
    assert 8 * 512 * 8 + 256 * 12 + 64 + (max_n - 256) // 128 * (2 * 15 * 4 + 8) <= 160 * 1024
    lib, a, b, c = _lib.load(), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    for S in (0, -5):
        assert lib.evmi_stoi_plan(S, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == _lib.EVMI_ERR_INVALID_ARG
        assert "shape" in lib.evmi_last_error().decode() and (a.value, b.value, c.value) == (-1, -1, -1)
    assert lib.evmi_stoi_plan(5, None, ctypes.byref(b), ctypes.byref(c)) == _lib.EVMI_ERR_INVALID_ARG
    assert lib.evmi_stoi_plan(5, ctypes.byref(a), None, ctypes.byref(c)) == _lib.EVMI_ERR_INVALID_ARG
    assert lib.evmi_stoi_plan(5, ctypes.byref(a), ctypes.byref(b), None) == _lib.EVMI_ERR_INVALID_ARG


# evmi_stoi_f32(ref, deg, ref_lens, deg_lens, stoi, counts, segment, frame_of, B, S_ref, S_deg, stream)
_NAMES = ["ref", "deg", "ref_lens", "deg_lens", "stoi", "counts", "segment", "frame_of", "B", "S_ref", "S_deg", "stream"]
_GOOD = [P] * 8 + [2, 9000, 9100, None]


def _with(**changes):
    args = list(_GOOD)
    for name, value in changes.items():
        args[_NAMES.index(name)] = value
    return tuple(args)


REFUSED = [(_with(**{name: 0}), "INVALID", "null") for name in _NAMES[:8]]
REFUSED += [(_with(**{name: bad}), "INVALID", "shape") for name, bad in (("B", 0), ("B", -1), ("S_ref", 0), ("S_deg", -3))]


@pytest.mark.parametrize("args,code,says", REFUSED, ids=[f"{c}-{s}-{i}" for i, (_, c, s) in enumerate(REFUSED)])
def test_refusals_before_any_device_work(args, code, says):
    lib = _lib.load()
    rc = lib.evmi_stoi_f32(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == _lib.EVMI_ERR_INVALID_ARG, (rc, msg)
    assert "stoi" in msg and says in msg, msg


def test_the_limit_is_the_plans_and_is_named():
    """The shorter padded row one sample beyond max_n is refused naming the limit; a longer row on one side alone is not what is
    refused (host pointers: a call inside the limits is never made here)."""
    lib, max_n = _lib.load(), _plan(1)[0]
    for S_ref, S_deg in ((max_n + 1, max_n + 1), (max_n + 1, 2 * max_n), (2 ** 31 - 1, max_n + 1)):
        assert lib.evmi_stoi_f32(*_with(S_ref=S_ref, S_deg=S_deg)) == _lib.EVMI_ERR_UNSUPPORTED
        msg = lib.evmi_last_error().decode()
        assert str(max_n) in msg and str(min(S_ref, S_deg)) in msg, msg


def test_band_table():
    from everyvoice_amd.pipeline import third_octave_bands

    assert third_octave_bands() == R.BAND_TABLE == R.bands()
    assert all(isinstance(v, int) for band in third_octave_bands() for v in band)


CLOSED_FORM = {0.0: 1.0, 0.1: 0.6462929873, 0.5: 0.5323158096, 2.0: 0.3924537495}


@pytest.fixture(scope="module")
def closed_form():
    return {g: R.stoi(*R.closed_form(g)) for g in CLOSED_FORM}


def test_closed_form_signals(closed_form):
    for g, want in CLOSED_FORM.items():
        r = closed_form[g]
        assert (r["F"], r["K"], r["J"]) == (155, 117, 87), g
        assert abs(r["stoi"] - want) <= 1e-9, (g, r["stoi"])
        assert len(r["segment"]) == 87 and len(r["frame_of"]) == 117 and abs(r["segment"].mean() - r["stoi"]) < 1e-12
        assert abs(r["margin"] - 0.2055) < 1e-4  # the nearest frame energy to the 40 dB threshold
        kept = r["frame_of"]
        assert (np.diff(kept) > 0).all() and 0 <= kept[0] and kept[-1] <= 154 and not ((kept >= 63) & (kept <= 91)).any()  # the silence


def test_properties(closed_form):
    x, y = R.closed_form(0.5)
    assert abs(R.stoi(x, 3.7 * y)["stoi"] - closed_form[0.5]["stoi"]) <= 1e-12  # scale invariance
    assert closed_form[0.1]["stoi"] > closed_form[0.5]["stoi"] > closed_form[2.0]["stoi"]
    r = R.stoi(x[:4096], y[:4096])
    assert (r["F"], r["J"]) == (30, 0) and np.isnan(r["stoi"])
    for n in (256, 0):
        r = R.stoi(x[:n], y[:n])
        assert (r["F"], r["K"], r["J"]) == (0, 0, 0) and np.isnan(r["stoi"]) and r["margin"] == float("inf")
    # only the first min(len) samples of either signal count
    assert R.stoi(x, y[:15000])["stoi"] == R.stoi(x[:15000], y[:15000])["stoi"]
    # an all-zero reference keeps every frame and scores 0
    r = R.stoi(np.zeros(6000), y[:6000])
    assert (r["F"], r["K"], r["J"]) == (45, 45, 15) and r["stoi"] == 0.0 and r["margin"] == 40.0
    # the float32 restatement finds the same frames and sits within 1e-5
    r32 = R.stoi(x.astype(np.float32), y.astype(np.float32), np.float32)
    assert np.array_equal(r32["frame_of"], closed_form[0.5]["frame_of"]) and abs(r32["stoi"] - closed_form[0.5]["stoi"]) < 1e-5


def test_pipeline_refusals_before_any_file_or_launch(tmp_path):
    from everyvoice_amd.pipeline import VOCODER_EVALUATION_FIELDS, Stoi, evaluate_vocoder, stoi

    assert Stoi._fields == ("stoi", "frames", "active", "segments", "segment_stoi", "frame_of")
    assert VOCODER_EVALUATION_FIELDS[:3] == ("basename", "speaker", "language") and VOCODER_EVALUATION_FIELDS[-1] == "note"
    wav, lens = torch.zeros(2, 5000), torch.tensor([5000, 4000])
    for bad_ref, bad_lens in ((torch.zeros(3, 5000), lens), (torch.zeros(5000), lens), (torch.zeros(2, 2, 5000), lens), (wav, torch.tensor([5000]))):
        with pytest.raises(ValueError, match="expected"):
            stoi(bad_ref, bad_lens, wav, lens, 10000)
    for rate in (0, -22050, 22050.5):
        with pytest.raises(ValueError, match="sample_rate"):
            stoi(wav, lens, wav, lens, rate)
    with pytest.raises(RuntimeError, match="GPU only"):
        stoi(wav, lens, wav[:, None], lens, 10000)
    vocoder = SimpleNamespace()  # no weights, no device: any use of it would raise AttributeError
    rows = [{"basename": "absent"}]
    with pytest.raises(FileNotFoundError, match="absent--default--default--spec-22050-mel-librosa.pt"):
        evaluate_vocoder(vocoder, rows, tmp_path)
    (tmp_path / "spec").mkdir()
    torch.save(torch.zeros(80, 10), tmp_path / "spec" / "absent--default--default--spec-22050-mel-librosa.pt")
    with pytest.raises(FileNotFoundError, match="absent--default--default--audio-22050.wav"):
        evaluate_vocoder(vocoder, rows, tmp_path)
