"""Mel-cepstral distortion along the warping path, host side (no GPU): the three declarations and their symbols,
the plan and workspace arithmetic, the refusals of ``evmi_dtw_cepstral_f32`` -- decided before any device work, so they hold with host
pointers that are never dereferenced --, the pipeline's refusals, the float64 restatement of tests/dtw_ref.py against brute-force
enumeration of every monotone path, the tie rule on a hand case, the basis, and THE CONDITIONS on every input tests/test_gpu_dtw.py
uses: exact float32 arithmetic and planted paths on the lattice cases, the calibration of the bound on the real-valued ones."""

import ctypes
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dtw_ref as D
from everyvoice_amd import _lib

_BUF = torch.zeros(64)  # host memory standing in for every device pointer
P = _BUF.data_ptr()


def _plan(K, Tb):
    from everyvoice_amd.train import ops

    return ops.dtw_plan(K, Tb)


def test_declared_in_the_header_and_exported():
    names = {name: (ret, params) for name, ret, params in _lib.declarations()}
    assert names["evmi_dtw_ws_bytes"] == ("long long", [("int", "B"), ("int", "Ta"), ("int", "Tb")])
    assert [t for t, _ in names["evmi_dtw_plan"][1]] == ["int", "int", "int*", "int*"]
    assert [n for _, n in names["evmi_dtw_cepstral_f32"][1]] == ["a_dev", "b_dev", "a_lens_dev", "b_lens_dev", "basis_dev", "dist_dev", "steps_dev", "lo_dev",
                                                                "hi_dev", "col_dev", "ws_dev", "ws_bytes", "B", "Ta", "Tb", "M", "K", "scale", "stream"]
    lib = _lib.load()
    assert lib.evmi_dtw_ws_bytes is not None and lib.evmi_dtw_plan is not None and lib.evmi_dtw_cepstral_f32 is not None
    assert lib.evmi_abi_version() == 2


def test_plan_and_workspace_arithmetic():
    from everyvoice_amd.train import ops

    chunks = set()
    for K in (1, 13, 24):
        for Tb in (1, 640, 1024):
            max_ta, chunk = _plan(K, Tb)
            assert max_ta >= 1024 and chunk >= 1, (K, Tb, max_ta, chunk)
            chunks.add(chunk)
    assert len(chunks) == 1
    assert all(_plan(K, 5)[0] >= _plan(K + 1, 5)[0] >= 1024 for K in range(1, 24))
    # one decision byte a cell, diagonal-major: Ta + Tb - 1 diagonals of Tb bytes padded to 16
    assert ops.dtw_ws_bytes(1, 1, 1) == 16 and ops.dtw_ws_bytes(3, 700, 257) == 3 * (700 + 257 - 1) * 272
    assert ops.dtw_ws_bytes(32, 1024, 1024) == 32 * 2047 * 1024
    assert ops.dtw_ws_bytes(0, 5, 5) == ops.dtw_ws_bytes(2, 0, 5) == ops.dtw_ws_bytes(2, 5, -1) == 0
    lib, max_ta, chunk = _lib.load(), ctypes.c_int(-1), ctypes.c_int(-1)
    for args, code, says in (((0, 5), _lib.EVMI_ERR_INVALID_ARG, "shape"), ((13, 0), _lib.EVMI_ERR_INVALID_ARG, "shape"),
                             ((25, 5), _lib.EVMI_ERR_UNSUPPORTED, "24 cepstra"), ((13, 1025), _lib.EVMI_ERR_UNSUPPORTED, "1024 frames")):
        assert lib.evmi_dtw_plan(*args, ctypes.byref(max_ta), ctypes.byref(chunk)) == code
        assert says in lib.evmi_last_error().decode() and (max_ta.value, chunk.value) == (-1, -1)
    assert lib.evmi_dtw_plan(13, 5, None, ctypes.byref(chunk)) == _lib.EVMI_ERR_INVALID_ARG
    assert lib.evmi_dtw_plan(13, 5, ctypes.byref(max_ta), None) == _lib.EVMI_ERR_INVALID_ARG


# evmi_dtw_cepstral_f32(a, b, a_lens, b_lens, basis, dist, steps, lo, hi, col, ws, ws_bytes, B, Ta, Tb, M, K, scale, stream)
_GOOD = [P] * 11 + [1 << 40, 2, 9, 5, 80, 13, 1.0, None]


def _with(**changes):
    names = ["a", "b", "a_lens", "b_lens", "basis", "dist", "steps", "lo", "hi", "col", "ws", "ws_bytes", "B", "Ta", "Tb", "M", "K", "scale", "stream"]
    args = list(_GOOD)
    for name, value in changes.items():
        args[names.index(name)] = value
    return tuple(args)


REFUSED = [(_with(**{name: 0}), "INVALID", "null") for name in ("a", "b", "a_lens", "b_lens", "basis", "dist", "steps", "lo", "hi", "col", "ws")]
REFUSED += [(_with(**{name: bad}), "INVALID", "shape") for name, bad in (("B", 0), ("Ta", 0), ("Tb", -3), ("M", 0), ("K", 0))]
REFUSED += [
    (_with(K=25), "UNSUPPORTED", "24 cepstra"),
    (_with(Tb=1025, Ta=1), "UNSUPPORTED", "1024 frames"),
    (_with(Ta=1200, K=24), "UNSUPPORTED", "LDS-resident side (Ta)"),
    (_with(Ta=100000, K=1), "UNSUPPORTED", "LDS-resident side (Ta)"),
    (_with(ws_bytes=2 * (9 + 5 - 1) * 16 - 1), "INVALID", "workspace too small"),
    (_with(ws=P + 4), "INVALID", "16-byte aligned"),
]


@pytest.mark.parametrize("args,code,says", REFUSED, ids=[f"{c}-{s.split()[0]}-{i}" for i, (_, c, s) in enumerate(REFUSED)])
def test_refusals_before_any_device_work(args, code, says):
    lib = _lib.load()
    rc = lib.evmi_dtw_cepstral_f32(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == {"INVALID": _lib.EVMI_ERR_INVALID_ARG, "UNSUPPORTED": _lib.EVMI_ERR_UNSUPPORTED}[code], (rc, msg)
    assert "dtw_cepstral" in msg and says in msg, msg


def test_the_limit_on_ta_is_the_plans():
    """One frame beyond max_ta is refused naming the limit; (host pointers: a call inside the limits is never made here)."""
    lib = _lib.load()
    for K in (1, 13, 24):
        max_ta = _plan(K, 5)[0]
        assert lib.evmi_dtw_cepstral_f32(*_with(Ta=max_ta + 1, K=K)) == _lib.EVMI_ERR_UNSUPPORTED
        assert str(max_ta) in lib.evmi_last_error().decode()


def test_pipeline_refusals_before_any_file_or_launch(tmp_path):
    from everyvoice_amd.fs2 import FastSpeech2ModelConfig
    from everyvoice_amd.pipeline import MelCepstralDistortion, evaluate_synthesis, mel_cepstral_basis, mel_cepstral_distortion

    assert MelCepstralDistortion._fields == ("mcd", "steps", "lo", "hi", "frame_mcd")
    model = SimpleNamespace(config=FastSpeech2ModelConfig(), device=torch.device("cpu"))  # no weights: any use of it would raise AttributeError
    rows = [{"basename": "absent", "ids": [1, 2, 3]}]
    for bad in (0, -1, 25, 80):
        with pytest.raises(ValueError, match="n_cepstra"):
            evaluate_synthesis(model, rows, tmp_path / "nothing", n_cepstra=bad)
    with pytest.raises(FileNotFoundError, match="absent--default--default--spec-22050-mel-librosa.pt"):
        evaluate_synthesis(model, rows, tmp_path / "nothing", n_cepstra=24)
    mel = torch.zeros(2, 7, 12)
    for bad in (0, 12, 25):
        with pytest.raises(ValueError, match="n_cepstra"):
            mel_cepstral_distortion(mel, torch.tensor([7, 7]), mel, torch.tensor([7, 7]), n_cepstra=bad)
    with pytest.raises(ValueError, match="expected"):
        mel_cepstral_distortion(mel, torch.tensor([7, 7]), torch.zeros(2, 7, 13), torch.tensor([7, 7]))
    with pytest.raises(RuntimeError, match="GPU only"):
        mel_cepstral_distortion(mel, torch.tensor([7, 7]), mel, torch.tensor([7, 7]), n_cepstra=5)
    with pytest.raises(ValueError, match="n_cepstra"):
        mel_cepstral_basis(13, 13)


def test_basis_is_orthonormal_and_leaves_c0_out():
    from everyvoice_amd.pipeline import MCD_DB_SCALE, mel_cepstral_basis

    for M, K in ((80, 13), (80, 24), (128, 24), (14, 13), (2, 1)):
        basis = mel_cepstral_basis(M, K)
        assert basis.dtype == torch.float32 and tuple(basis.shape) == (K, M)
        b64 = basis.double()
        assert float((b64 @ b64.T - torch.eye(K, dtype=torch.float64)).abs().max()) < 1e-6
        assert float(b64.sum(1).abs().max()) < 1e-5  # orthogonal to the constant row c0
        assert np.array_equal(basis.numpy(), D.dct_basis(M, K))
    m = np.arange(80)
    assert abs(float(mel_cepstral_basis(80, 13)[2, 5]) - np.sqrt(2 / 80) * np.cos(np.pi / 80 * (m[5] + 0.5) * 3)) < 1e-7
    assert MCD_DB_SCALE == D.MCD_SCALE


def test_float64_recurrence_against_every_monotone_path():
    rng = np.random.default_rng(0)
    for Na, Nb in itertools.product(range(1, 6), repeat=2):
        for trial in range(3):
            a, b = rng.normal(size=(Na, 4)), rng.normal(size=(Nb, 4))
            basis = rng.normal(size=(3, 4))
            r = D.dtw(a, b, basis, 1.0, np.float64)
            best = D.brute_force(r["c"])
            assert abs(r["D"][-1, -1] - best) <= 1e-12 * max(1.0, best), (Na, Nb, trial)
            assert D.is_path(r["lo"], r["hi"], Na) and r["steps"] == len(D.path_cells(r["lo"], r["hi"]))
            assert abs(D.path_cost64(a, b, basis, r["lo"], r["hi"]) - best) <= 1e-12 * max(1.0, best)
            assert max(Na, Nb) <= r["steps"] <= Na + Nb - 1
            assert r["dist"] == r["D"][-1, -1] / r["steps"]
            for j in range(Nb):
                assert abs(r["col"][j] - r["c"][r["lo"][j] : r["hi"][j] + 1, j].mean()) < 1e-12


def test_tie_rule_on_a_hand_case():
    """All costs equal: every predecessor ties, the diagonal is kept wherever it exists, and the rest follows the border."""
    c = np.ones((3, 5), dtype=np.float32)
    _, dec = D.recurrence(c)
    assert (dec[1:, 1:] == 0).all()
    steps, lo, hi = D.walk(dec)
    assert (steps, lo.tolist(), hi.tolist()) == (5, [0, 0, 0, 1, 2], [0, 0, 0, 1, 2])
    # up beats the diagonal only when strictly smaller; left beats up only when strictly smaller
    c = np.array([[1, 5, 1], [1, 1, 1], [1, 1, 1]], dtype=np.float32)  # D row 0: 1 6 7; D[1][0] = 2
    Dm, dec = D.recurrence(c)
    assert dec[1, 1] == 0 and Dm[1, 1] == 2  # diagonal 1, up 6, left 2
    assert dec[1, 2] == 2 and Dm[1, 2] == 3  # diagonal 6, up 7, left 2
    assert dec[2, 1] == 0 and Dm[2, 1] == 3  # diagonal D[1][0] = 2, up D[1][1] = 2 (a tie: not taken), left D[2][0] = 3
    c = np.array([[1, 0], [3, 1], [1, 1]], dtype=np.float32)  # D: 1 1 / 4 2 / 5 .
    Dm, dec = D.recurrence(c)
    assert dec[1, 1] == 0 and dec[2, 1] == 1 and Dm[2, 1] == 3  # diagonal 4, up 2, left 5
    nan = np.array([[1, np.nan], [1, 1]], dtype=np.float32)  # a comparison with NaN is false: the diagonal stays
    assert D.recurrence(nan)[1][1, 1] == 0
    steps, lo, hi = D.walk(np.full((4, 3), 7, dtype=np.uint8))  # any byte that is neither up nor left reads as the diagonal
    assert (steps, lo.tolist(), hi.tolist()) == (4, [0, 2, 3], [1, 2, 3])


# ---- the conditions on the inputs of tests/test_gpu_dtw.py --------------------------------------------------------------------------
def _lattice_keys():
    return D.lattice_keys(_plan(13, 64)[1])


def test_lattice_cases_are_exact_in_float32_and_planted():
    keys = _lattice_keys()
    chunk = _plan(13, 64)[1]
    sums = {Ta + Tb - 1 for Ta, Tb, *_ in keys}
    assert {chunk, chunk + 1, 2 * chunk, 2 * chunk + 1} <= sums  # both sides of a flush edge, one chunk and two
    assert {(Ta, Tb) for Ta, Tb, *_ in keys} >= set(D.LATTICE_SHAPES) and {(K, M) for _, _, K, M, _ in keys} == set(D.LATTICE_KM)
    unique, tied = 0, 0
    for key in keys:
        Ta, Tb, K, M, kind = key
        r = D.lattice_case(*key)
        a, b, basis = r["a"], r["b"], r["basis"]
        assert a.shape == (Ta, M) and b.shape == (Tb, M) and basis.shape == (K, M) and a.dtype == b.dtype == basis.dtype == np.float32
        assert set(np.unique(basis)) <= {-1.0, 0.0, 1.0} and 1 <= int((basis != 0).sum(1).max()) <= 8
        for x in (a, b):
            assert np.array_equal(x * 4, np.round(x * 4)) and np.abs(x).max() <= 1.0
            assert D.exact_in_float32(x, basis), key
        ca, cb = D.cepstra(a, basis, np.float64), D.cepstra(b, basis, np.float64)
        assert np.array_equal(ca, D.cepstra(a, basis, np.float32)) and np.array_equal(cb, D.cepstra(b, basis, np.float32))
        # cepstra on the quarter lattice within [-8, 8]: d_k^2 is a multiple of 1/16 up to 256, a sum of 24 of them stays below 2^24 / 16
        for cx in (ca, cb):
            assert np.array_equal(cx * 4, np.round(cx * 4)) and np.abs(cx).max() <= 8.0, key
        if Ta * Tb <= 300 * 300:  # ... and cell by cell, partial sum by partial sum, where that is quick
            assert D.costs_exact_in_float32(ca, cb), key
        want = D.lattice_expectation(key)
        assert D.is_path(want["lo"], want["hi"], Ta)
        if kind == "planted":
            assert want["dist"] == 0.0 and not want["col"].any(), key
            if r["plant"] is not None:
                assert np.array_equal(want["lo"], r["plant"][0]) and np.array_equal(want["hi"], r["plant"][1]), key
                unique += 1
            else:
                tied += 1
        else:
            assert want["dist"] > 0.0 and want["steps"] >= max(Ta, Tb)
    assert unique >= 30 and tied >= 6


def test_real_valued_cases_calibrate_the_bound():
    """err32 (the float32 restatement against float64) is far below the values: 4 x err32 < 1e-4 x value on every case, so the bound
    of the GPU tests separates a wrong path or a wrong cost from rounding.  The worst err32 / value is printed."""
    worst, same_path = 0.0, 0
    for Ta, Tb in D.REAL_SHAPES:
        r = D.real_case(Ta, Tb)
        assert r["a"].shape == (Ta, D.REAL_M) and r["b"].shape == (Tb, D.REAL_M) and np.isfinite(r["a"]).all() and np.isfinite(r["b"]).all()
        w64, w32 = D.real_expectation(Ta, Tb)
        err = abs(float(w32["dist"]) - float(w64["dist"]))
        assert 1.0 < w64["dist"] < 30.0, (Ta, Tb, w64["dist"])  # dB: a mel-like pair, neither identical nor unrelated
        assert 4 * err < 1e-4 * w64["dist"], (Ta, Tb, err, w64["dist"])
        worst = max(worst, err / float(w64["dist"]))
        same = np.array_equal(w32["lo"], w64["lo"]) and np.array_equal(w32["hi"], w64["hi"])
        same_path += same
        if same:
            col_err = np.abs(w32["col"].astype(np.float64) - w64["col"])
            assert (4 * col_err < 1e-4 * np.maximum(w64["col"], 1.0)).all(), (Ta, Tb, col_err.max())
        # the float32 path is optimal in float64 up to the same bound
        cost32 = D.path_cost64(r["a"], r["b"], r["basis"], w32["lo"], w32["hi"])
        assert cost32 - float(w64["D"][-1, -1]) <= D.bound(err, float(w64["D"][-1, -1])), (Ta, Tb)
        diagonal = int((w64["lo"][1:] == w64["hi"][:-1] + 1).sum())
        assert max(Ta, Tb) <= w64["steps"] < Ta + Tb - 1 and 0 < diagonal < w64["steps"] - 1  # a real warp: diagonal steps and runs
    print(f"worst err32 / value over {len(D.REAL_SHAPES)} cases: {worst:.2e}; float32 path == float64 path in {same_path}")
