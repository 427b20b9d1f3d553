"""Prosody steering of FastSpeech2, the part that needs no device: the restatement of the fit on fixed cases and
on the lattice where double sums are exact, the host-side refusals of the three entry points of csrc/fs2_prosody.hip (as in
tests/test_abi_arguments.py: host memory stands in for every device pointer and must come back untouched), and every refusal of
``fs2.check_prosody_arguments``."""

import math
import random

import pytest
import torch

from everyvoice_amd import _lib, fs2
from tests.fs2_prosody_ref import fit_ref

INVALID_ARG, UNSUPPORTED = _lib.EVMI_ERR_INVALID_ARG, _lib.EVMI_ERR_UNSUPPORTED
_BUF = torch.zeros(64)
P = _BUF.data_ptr()


# ---- the fit, restated ----------------------------------------------------------------------------------------------------------------
def test_fit_fixed_cases():
    assert fit_ref([1, 1, 1], 10) == [4, 3, 3]                      # 3.33 each: the one frame left goes to the lowest index
    assert fit_ref([0.5, 0.25, 0.25, 0.0], 7) == [3, 2, 2, 0]        # 3.5, 1.75, 1.75, 0: floors 3, 1, 1 and two frames for the two .75
    assert fit_ref([0.0] * 5, 3) == [1, 1, 1, 0, 0]                  # no weight anywhere: all equal, 0.6 each, ties to the lower index
    assert fit_ref([0.37], 11) == [11] and fit_ref([0.0], 4) == [4]  # one symbol takes everything
    assert fit_ref([1, 2, 3], 0, current=[5, 6, 7]) == [5, 6, 7]     # no target: the row stays
    assert fit_ref([3.0, 1.0], 1) == [1, 0] and fit_ref([1.0, 1.0], 1) == [1, 0]  # symbols of no frames are allowed


def test_fit_sums_to_the_target_on_the_lattice():
    """Weights that are multiples of 1/8 below 64: every double sum and product below is exact, so the result sums to the target and
    every duration is floor(x_l) or floor(x_l) + 1 of the exact share."""
    rng = random.Random(5)
    for _ in range(2000):
        n = rng.randint(1, 40)
        w = [rng.randint(0, 511) / 8.0 for _ in range(n)]
        target = rng.randint(1, 600)
        d = fit_ref(w, target)
        assert sum(d) == target and min(d) >= 0
        S = sum(w) or float(n)
        for wl, dl in zip(w if sum(w) else [1.0] * n, d):
            assert dl - math.floor(wl * target / S) in (0, 1)


def test_the_limit_is_the_headers():
    assert fs2.FIT_MAX_SYMBOLS == _lib.EVMI_FS2_FIT_MAX_SYMBOLS >= 4096 and _lib.EVMI_ABI_VERSION == 2
    names = [name for name, _, _ in _lib.declarations()]
    assert {"evmi_fs2_variance_apply_f32", "evmi_fs2_durations_ctl_i32", "evmi_fs2_fit_durations_i32"} <= set(names)


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------------------
def _apply(x=P, pred=P, forced=0, stride=0, control=0, cum=0, lens=P, bins=P, table=P, used=P, n_bins=4, B=2, L=5, n=5, D=8):
    return ("evmi_fs2_variance_apply_f32", (x, pred, forced, stride, control, cum, lens, bins, table, used, n_bins, B, L, n, D, 1.0, None))


def _ctl(log_d=P, lens=P, control=0, dur=P, weights=0, B=2, L=5):
    return ("evmi_fs2_durations_ctl_i32", (log_d, lens, control, dur, weights, B, L, 1.0, None))


def _fit(weights=P, lens=P, target=P, dur=P, B=2, L=5):
    return ("evmi_fs2_fit_durations_i32", (weights, lens, target, dur, B, L, None))


LIMIT = _lib.EVMI_FS2_FIT_MAX_SYMBOLS
ABI_CASES = [
    (_apply(x=0), INVALID_ARG), (_apply(lens=0), INVALID_ARG), (_apply(bins=0), INVALID_ARG), (_apply(table=0), INVALID_ARG),
    (_apply(used=0), INVALID_ARG), (_apply(pred=0), INVALID_ARG),  # (neither a prediction nor forced values)
    (_apply(B=0), INVALID_ARG), (_apply(L=0, cum=P), INVALID_ARG), (_apply(n=0), INVALID_ARG), (_apply(D=0), INVALID_ARG),
    (_apply(B=-1), INVALID_ARG), (_apply(D=-8), INVALID_ARG), (_apply(n_bins=1), INVALID_ARG),
    (_apply(L=4), INVALID_ARG),                          # without cum the control's rows are the columns' rows
    (_apply(forced=P, stride=4), INVALID_ARG),           # forced rows shorter than n
    (_ctl(log_d=0), INVALID_ARG), (_ctl(lens=0), INVALID_ARG), (_ctl(dur=0), INVALID_ARG), (_ctl(B=0), INVALID_ARG), (_ctl(L=0), INVALID_ARG),
    (_ctl(L=-3), INVALID_ARG),
    (_fit(weights=0), INVALID_ARG), (_fit(lens=0), INVALID_ARG), (_fit(target=0), INVALID_ARG), (_fit(dur=0), INVALID_ARG),
    (_fit(B=0), INVALID_ARG), (_fit(L=0), INVALID_ARG), (_fit(L=LIMIT + 1), UNSUPPORTED),
]


@pytest.mark.parametrize("case", ABI_CASES, ids=lambda c: c[0][0][len("evmi_fs2_"):])
def test_entry_points_refuse_on_the_host(case):
    (name, args), code = case
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == code, f"{name}{args}: returned {rc} ({msg!r}), wanted {code}"
    assert name[len("evmi_"):].rsplit("_", 1)[0] in msg, f"{name}: evmi_last_error() = {msg!r} does not name the function"
    assert torch.count_nonzero(_BUF) == 0  # (nothing was written through the stand-in pointer)


# ---- check_prosody_arguments -----------------------------------------------------------------------------------------------------------
B, L = 3, 7
OK_BL, OK_B = torch.ones(B, L), torch.ones(B)
FRAME = {"pitch": "frame", "energy": "frame"}


def test_what_is_accepted():
    check = fs2.check_prosody_arguments
    check(B, L)
    check(B, L, None, 1.2, 0.8, 1)
    check(B, L, None, OK_BL, OK_B, OK_BL.double())
    check(B, L, None, pitch=torch.zeros(B, L), energy=torch.zeros(B, L))
    check(B, L, FRAME, pitch=torch.zeros(B, 40), energy=torch.zeros(B, 1))  # (against T: behind the forward's host sync)
    check(B, L, None, OK_BL, target_frames=torch.tensor([40, 0, 9]))
    check(B, fs2.FIT_MAX_SYMBOLS, None, target_frames=torch.tensor([1, 1, 1], dtype=torch.int32))
    check(B, fs2.FIT_MAX_SYMBOLS + 1)  # (no target: no limit)


@pytest.mark.parametrize("name", ["duration_control", "pitch_control", "energy_control"])
@pytest.mark.parametrize("bad", [torch.ones(B, L + 1), torch.ones(B + 1), torch.ones(L), torch.ones(B, L, 1), torch.ones(B, L, dtype=torch.int64),
                                 torch.ones(B, dtype=torch.bool), [1.0] * B, None])
def test_a_control_of_another_shape_or_dtype_is_refused(name, bad):
    with pytest.raises(ValueError, match=name):
        fs2.check_prosody_arguments(B, L, **{name: bad})


@pytest.mark.parametrize("name", ["pitch", "energy"])
def test_forced_values_are_checked(name):
    check = fs2.check_prosody_arguments
    for bad in (torch.zeros(B, L + 1), torch.zeros(B, L - 1), torch.zeros(B + 1, L), torch.zeros(L), torch.zeros(B, L, dtype=torch.int64), [0.0] * L):
        with pytest.raises(ValueError, match=name):
            check(B, L, **{name: bad})
    for bad in (torch.zeros(B + 1, 40), torch.zeros(B, 0), torch.zeros(40)):
        with pytest.raises(ValueError, match=name):
            check(B, L, FRAME, **{name: bad})
    for control in (1.3, OK_BL, OK_B):  # forced together with a non-default control of the same variance
        with pytest.raises(ValueError, match=f"{name}_control"):
            check(B, L, **{name: torch.zeros(B, L), name + "_control": control})
    other = "energy" if name == "pitch" else "pitch"
    check(B, L, **{name: torch.zeros(B, L), other + "_control": 1.3, "duration_control": OK_BL})  # (another variance's control is fine)


def test_target_frames_are_checked():
    check = fs2.check_prosody_arguments
    with pytest.raises(ValueError, match="durations"):
        check(B, L, target_frames=torch.tensor([4, 0, 9]), durations=torch.ones(B, L, dtype=torch.long))
    with pytest.raises(ValueError, match="negative"):
        check(B, L, target_frames=torch.tensor([4, -1, 9]))
    for bad in (torch.tensor([4.0, 0.0, 9.0]), torch.tensor([4, 9]), torch.tensor([[4, 0, 9]]), torch.tensor([True, False, True]), [4, 0, 9], 12):
        with pytest.raises(ValueError, match="target_frames"):
            check(B, L, target_frames=bad)
    with pytest.raises(ValueError, match=str(fs2.FIT_MAX_SYMBOLS)):
        check(B, fs2.FIT_MAX_SYMBOLS + 1, target_frames=torch.tensor([4, 0, 9]))
