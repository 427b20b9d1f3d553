"""Plain numpy restatement of the SoX effect chains the preprocessor reproduces (everyvoice_amd/sox.py, csrc/sox_effects.hip):
what the device's parallel form is checked against.  One utterance at a time, float32 samples in [-1, 1).

There is no ``sox`` binary and no torchaudio on the machines this project is built and tested on, so parity with SoX itself is
pinned only by the reference's own expectation (the 440 Hz tone trimmed to 2.5 s, tests/test_sox_effects.py) and by the rules
below.  They were written from the description of SoX 14.4's ``silence.c``, without its source at hand; the rules marked
(unconfirmed) could not be checked against it.

  channels 1   the channels' mean (the pipeline's mix-down; float32, as torch's ``mean(0)``).
  norm dB      x / max|x| * float32(10^(dB/20)).  SoX re-quantises its output to 16 bits with TPDF dither; not restated.
  reverse      x[::-1].
  silence      walks the samples one by one, as SoX does:
    * sample scale: s = x * 2^31 (SoX's int32 samples; 16-bit input k is k << 16).
    * RMS: SoX keeps a running double sum over a ring of W = floor(rate / 50) squares (add the new square, subtract the one
      leaving); the window starts zero-filled and the divisor is always W; rms = (int32) sqrt(sum / W), truncated, with the
      current sample included.
    * threshold: above when rms / (2^31 - 1) * 100 > X (``X%``) or 20 log10(rms / (2^31 - 1)) > X (``XdB``).  (unconfirmed:
      SoX 14.4.2 may first mask the RMS to the input's precision, the top 16 bits for 16-bit files; not applied.)
    * durations: D = round(seconds * rate), or N for ``Ns``.
    * leading trim (above_periods 1): samples are dropped until D_start consecutive samples are above the start threshold;
      output starts at the first sample of that run; no such run -> empty output.
    * stop part (below_periods given), while copying: a run of D_stop consecutive samples below the stop threshold is discarded;
      a shorter below-run is kept, also one still open at the end.  below_periods 1: everything after that run is discarded.
      below_periods -1: the window is cleared (unconfirmed: zero-filled ring, sum 0) and the leading trim runs again from the
      next sample (with above_periods 0 (unconfirmed): copying resumes at the next sample).
"""

from __future__ import annotations

import math

import numpy as np

SAMPLE_MAX = 2**31 - 1


def _duration(s: str, rate: int) -> int:
    return int(s[:-1]) if s.endswith("s") else int(math.floor(float(s) * rate + 0.5))


def _threshold(s: str):
    if s.endswith("%"):
        return float(s[:-1]), "%"
    return float(s[:-2] if s.endswith("dB") else s[:-1]), "d"


def _above(rms: int, thr) -> bool:
    value, unit = thr
    r = rms / SAMPLE_MAX
    if unit == "%":
        return r * 100.0 > value
    return (20.0 * math.log10(r) if r > 0 else -math.inf) > value


def rms_trace(x: np.ndarray, rate: int, restarts=()) -> np.ndarray:
    """The int32 RMS SoX sees at every sample of x (float64 values before truncation), the window cleared after each index in
    ``restarts``.  Used by the tests to measure how far a decision lies from its threshold."""
    W = rate // 50
    ring, pos, total = [0.0] * W, 0, 0.0
    out = np.empty(len(x), dtype=np.float64)
    restarts = set(restarts)
    for i, v in enumerate(x.astype(np.float64).tolist()):
        s = v * 2147483648.0
        sq = s * s
        total = total - ring[pos] + sq
        ring[pos] = sq
        pos = (pos + 1) % W
        out[i] = math.sqrt(total / W)
        if i in restarts:
            ring, pos, total = [0.0] * W, 0, 0.0
    return out


def silence(x: np.ndarray, rate: int, args: list[str], trace: list | None = None) -> np.ndarray:
    """SoX ``silence`` on one mono utterance (float32) -> the kept samples (float32, unchanged).  ``trace``, when given, collects
    (sample index, rms before truncation, threshold test, threshold) of every decision that changed the state."""
    above_periods = int(args[0])
    rest = list(args[1:])
    start = stop = None
    if above_periods:
        start, rest = (_duration(rest[0], rate), _threshold(rest[1])), rest[2:]
    below_periods = int(rest[0]) if rest else 0
    if rest:
        stop = (_duration(rest[1], rate), _threshold(rest[2]))
    W = rate // 50
    ring, pos, total = [0.0] * W, 0, 0.0
    trimming = above_periods == 1
    run = 0  # consecutive samples above the start threshold (trimming) / below the stop threshold (copying)
    kept: list[int] = []  # indices of the output samples
    held: list[int] = []  # a below-run not yet long enough to be discarded
    xs = x.astype(np.float64).tolist()
    for i, v in enumerate(xs):
        s = v * 2147483648.0
        sq = s * s
        total = total - ring[pos] + sq
        ring[pos] = sq
        pos = (pos + 1) % W
        q = math.sqrt(total / W)
        rms = min(int(q), SAMPLE_MAX)
        if trimming:
            if _above(rms, start[1]):
                run += 1
                if run == start[0]:
                    kept.extend(range(i - start[0] + 1, i + 1))
                    trimming, run = False, 0
                    if trace is not None:
                        trace.append((i, q, "start", start[1]))
            else:
                run = 0
            continue
        if stop is None:
            kept.append(i)
            continue
        if _above(rms, stop[1]):
            kept.extend(held)
            kept.append(i)
            held, run = [], 0
            continue
        held.append(i)
        run += 1
        if run == stop[0]:
            if trace is not None:
                trace.append((i, q, "stop", stop[1]))
            held, run = [], 0
            if below_periods == 1:
                break
            ring, pos, total = [0.0] * W, 0, 0.0
            trimming = above_periods == 1
    if not trimming:
        kept.extend(held)
    return x[np.asarray(kept, dtype=np.int64)] if kept else x[:0]


def apply_chain(audio: np.ndarray, rate: int, chain) -> np.ndarray:
    """audio [channels, S] or [S] float32 -> mono float32 after the chain (mix-down first, then the effects in order)."""
    a = np.asarray(audio, dtype=np.float32)
    x = a.mean(0, dtype=np.float32) if a.ndim == 2 else a.copy()
    for eff in chain or []:
        name, args = eff[0], list(eff[1:])
        if name == "channels":
            continue
        if name == "norm":
            target = np.float32(10.0 ** (float(args[0]) / 20.0)) if args else np.float32(1.0)
            peak = np.abs(x).max() if x.size else np.float32(0)
            x = (x / peak * target).astype(np.float32)
        elif name == "reverse":
            x = x[::-1].copy()
        elif name == "silence":
            x = silence(x, rate, args)
        else:
            raise ValueError(f"oracle: {name!r} is not restated")
    return x
