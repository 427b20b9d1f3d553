"""A dataset's SoX effect chain (``source_data[*].sox_effects``), applied on the device during preprocessing.

The reference hands the chain to SoX before resampling (everyvoice/preprocessor/preprocessor.py:187-194); its wizard writes
``channels 1`` plus any of ``norm -3.0``, the start-and-end trim ``silence 1 0.1 0.1%, reverse, silence 1 0.1 0.1%, reverse`` and the
gap removal ``silence 1 0.1 1.0% -1 0.4 1%`` (everyvoice/wizard/dataset.py:1084-1096).  This module parses such a chain on the host
(``parse_sox_effects``: once, before any file is read) and runs it on a zero-padded batch on the device (``apply_sox_effects``).
A chain is either reproduced or refused with a ValueError: an effect outside the four below is never dropped silently.

Supported (SoX 14.4 syntax):
  channels 1     the mix-down, which the pipeline always does first (a ``channels`` after another effect is refused)
  norm [dB]      peak normalise to 10^(dB/20) (dB defaults to 0).  SoX then re-quantises to 16 bits with random TPDF dither when it
                 writes its temporary file; that random step is NOT reproduced.
  reverse        each utterance reversed within its own length
  silence above_periods [duration threshold] [below_periods duration threshold]
                 above_periods in {0, 1}, below_periods in {1, -1}; durations in seconds (``0.1``) or samples (``4410s``),
                 thresholds ``X%`` or ``XdB`` / ``Xd``.  The algorithm ("SoX effect chains") follows SoX 14.4's silence
                 effect on its int32 sample scale; tests/sox_oracle.py restates it sample by sample.
"""

from __future__ import annotations

import functools
import math
import re
from dataclasses import dataclass

import torch

SUPPORTED = ("channels 1", "norm [dB]", "reverse",
             "silence {0|1} [duration threshold{%|d|dB}] [{1|-1} duration threshold{%|d|dB}]")
DEFAULT_CHAIN = [["channels", "1"]]
SAMPLE_MAX = 2**31 - 1  # SOX_SAMPLE_MAX: samples are taken on SoX's int32 scale, s = x * 2^31


@dataclass(frozen=True)
class Threshold:
    value: float
    unit: str  # "%" or "d"


@dataclass(frozen=True)
class Effect:
    name: str  # "norm", "reverse" or "silence" ("channels 1" is the mix-down and is not kept)
    db: float = 0.0  # norm
    above_periods: int = 0  # silence
    start: tuple | None = None  # (duration, Threshold): duration is ("s", seconds) or ("n", samples)
    below_periods: int = 0  # 0 = no stop part
    stop: tuple | None = None


def _refuse(effect, why: str):
    raise ValueError(f"SoX effect {effect!r}: {why}. Supported effects: " + "; ".join(SUPPORTED))


def _number(effect, s: str) -> float:
    try:
        v = float(s)
    except (TypeError, ValueError):
        _refuse(effect, f"{s!r} is not a number")
    if not math.isfinite(v):
        _refuse(effect, f"{s!r} is not a finite number")
    return v


def _duration(effect, s: str) -> tuple:
    if isinstance(s, str) and re.fullmatch(r"[0-9]+s", s):
        n = int(s[:-1])
        if n <= 0:
            _refuse(effect, f"duration {s!r} must be positive")
        return ("n", n)
    v = _number(effect, s)
    if v <= 0:
        _refuse(effect, f"duration {s!r} must be positive")
    return ("s", v)


def _threshold(effect, s: str) -> Threshold:
    m = re.fullmatch(r"(.+?)(%|dB|d)", s) if isinstance(s, str) else None
    if not m:
        _refuse(effect, f"threshold {s!r} needs a unit, '%' or 'dB'")
    return Threshold(_number(effect, m.group(1)), "%" if m.group(2) == "%" else "d")


def _periods(effect, s: str, allowed: tuple) -> int:
    if not isinstance(s, str) or not re.fullmatch(r"-?[0-9]+", s) or int(s) not in allowed:
        _refuse(effect, f"periods {s!r} must be one of {', '.join(str(a) for a in allowed)}")
    return int(s)


def parse_sox_effects(chain) -> list[Effect]:
    """``list[list[str]]`` (None and [] mean no effect) -> effect records, or ValueError naming the first effect that is not
    reproduced.  ``channels 1`` is accepted only before every other effect: the mix-down always comes first."""
    effects: list[Effect] = []
    for eff in chain or []:
        if not isinstance(eff, (list, tuple)) or not eff or not all(isinstance(a, str) for a in eff):
            _refuse(eff, "an effect is a non-empty list of strings")
        name, args = eff[0], list(eff[1:])
        if name == "channels":
            if args != ["1"]:
                _refuse(eff, "only 'channels 1' (mix-down to mono) is reproduced")
            if effects:
                _refuse(eff, "'channels 1' must come before every other effect (the chain would otherwise process stereo)")
        elif name == "norm":
            if len(args) > 1:
                _refuse(eff, "norm takes at most one argument, the peak level in dB")
            effects.append(Effect("norm", db=_number(eff, args[0]) if args else 0.0))
        elif name == "reverse":
            if args:
                _refuse(eff, "reverse takes no argument")
            effects.append(Effect("reverse"))
        elif name == "silence":
            if args and args[0] == "-l":
                _refuse(eff, "'silence -l' (leave the silence in) is not reproduced")
            if len(args) not in (1, 3, 4, 6):
                _refuse(eff, "wrong number of arguments")
            above = _periods(eff, args[0], (0, 1))
            rest = args[1:]
            start = None
            if above == 1:
                if len(rest) < 2:
                    _refuse(eff, "above_periods 1 needs a duration and a threshold")
                start, rest = (_duration(eff, rest[0]), _threshold(eff, rest[1])), rest[2:]
            below, stop = 0, None
            if rest:
                if len(rest) != 3:
                    _refuse(eff, "wrong number of arguments")
                below = _periods(eff, rest[0], (1, -1))
                stop = (_duration(eff, rest[1]), _threshold(eff, rest[2]))
            effects.append(Effect("silence", above_periods=above, start=start, below_periods=below, stop=stop))
        else:
            _refuse(eff, f"{name!r} is not reproduced")
    return effects


def duration_samples(duration: tuple, rate: int) -> int:
    """SoX's duration in samples: ``round(seconds * rate)`` (``Ns`` is N samples)."""
    kind, v = duration
    n = int(v) if kind == "n" else int(math.floor(v * rate + 0.5))
    if n < 1:
        raise ValueError(f"SoX silence duration {v} s is shorter than one sample at {rate} Hz")
    return n


def is_above(rms: int, thr: Threshold) -> bool:
    """SoX's threshold test on the truncated int32 RMS: ``rms / SAMPLE_MAX * 100 > X`` (%) or ``20 log10(rms / SAMPLE_MAX) > X`` (dB)."""
    r = rms / SAMPLE_MAX
    if thr.unit == "%":
        return r * 100.0 > thr.value
    return (20.0 * math.log10(r) if r > 0 else -math.inf) > thr.value


@functools.lru_cache(maxsize=64)
def rms_min(thr: Threshold) -> int:
    """The smallest int32 RMS that ``is_above`` calls above (2^31: none).  The test is monotone in the RMS, so the device compares
    integers and runs no transcendental function of its own."""
    if not is_above(SAMPLE_MAX, thr):
        return SAMPLE_MAX + 1
    lo, hi = 0, SAMPLE_MAX
    while lo < hi:
        mid = (lo + hi) // 2
        if is_above(mid, thr):
            hi = mid
        else:
            lo = mid + 1
    return lo


def silence_window(rate: int) -> int:
    """The RMS window: ``rate / 50`` samples (20 ms), floored."""
    return int(rate) // 50


def apply_sox_effects(x: torch.Tensor, lens: torch.Tensor, rate: int, effects: list[Effect]):
    """Run a parsed chain on a zero-padded batch: x [items, t_max] fp32 and lens [items] int32, both on the device.  Returns
    (x', lens') on the device (new tensors; the inputs are not modified): each utterance processed within its own length, zeros
    behind it, lengths never read back here.
    A ``silence`` directly followed by ``reverse`` is one pass (the gather writes the kept samples in reverse order)."""
    from . import _lib

    if not x.is_cuda:
        raise RuntimeError("everyvoice_amd.sox.apply_sox_effects computes on the GPU only (no CPU fallback)")
    lib = _lib.load()
    x = x.to(torch.float32).contiguous()
    lens = lens.to(x.device, torch.int32).clone()  # (rewritten in place by the silence kernels)
    items, t_max = x.shape
    stream = _lib.current_stream_ptr(x.device)
    i = 0
    while i < len(effects):
        e = effects[i]
        y = torch.empty_like(x)
        if e.name == "norm":
            _lib.check(lib.evmi_peak_normalize_f32(x.data_ptr(), y.data_ptr(), lens.data_ptr(), items, t_max, float(10.0 ** (e.db / 20.0)), stream),
                       "evmi_peak_normalize_f32")
        elif e.name == "reverse":
            _lib.check(lib.evmi_sox_reverse_f32(x.data_ptr(), y.data_ptr(), lens.data_ptr(), items, t_max, stream), "evmi_sox_reverse_f32")
        else:
            reverse = i + 1 < len(effects) and effects[i + 1].name == "reverse"
            window = silence_window(rate)
            d_start = duration_samples(e.start[0], rate) if e.above_periods else 0
            r_start = rms_min(e.start[1]) if e.above_periods else 0
            d_stop = duration_samples(e.stop[0], rate) if e.below_periods else 0
            r_stop = rms_min(e.stop[1]) if e.below_periods else 0
            n_ws = lib.evmi_sox_silence_ws_bytes(items, t_max, window, d_stop)
            if n_ws <= 0:
                raise RuntimeError(f"evmi_sox_silence_ws_bytes rejected items={items} t_max={t_max} rate={rate}")
            ws = torch.empty(n_ws, device=x.device, dtype=torch.uint8)
            _lib.check(lib.evmi_sox_silence_f32(x.data_ptr(), y.data_ptr(), lens.data_ptr(), ws.data_ptr(), n_ws, items, t_max, window,
                                                e.above_periods, d_start, r_start, e.below_periods, d_stop, r_stop, int(reverse), stream),
                       "evmi_sox_silence_f32")
            i += int(reverse)
        x = y
        i += 1
    return x, lens
