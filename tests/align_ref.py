"""The aligner at inference, restated in float64 -- what tests/test_align_infer_host.py and tests/test_gpu_align_infer.py hold
``evmi_align_durations_f32`` and ``FastSpeech2.align`` to.

  value[t][l] = -temperature * sum_a (q[a][t] - k[a][l])^2  (+ log(prior[t][l] + 1e-8))
  Q[y][x]     = value[y][x] + max(Q[y-1][x-1], Q[y-1][x])  over the band max(0, L + y - T) <= x < min(L, y + 1), MAX_NEG = -1e9
  read back from (T - 1, L - 1): move to x - 1 when x == y or Q[y-1][x] < Q[y-1][x-1]

The same band and tie rule as ``oracle.mas_ref.maximum_path_ref`` (which works in float32), every sum in float64.
"""

from __future__ import annotations

import functools

import numpy as np

MAX_NEG = -1e9
A_PLANTED = 80


def cell_values(q, k, temperature: float, prior=None) -> np.ndarray:
    """q [A, T], k [A, L] (any float type) -> value [T, L] float64."""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    d = np.zeros((q.shape[1], k.shape[1]))
    for a in range(q.shape[0]):
        d += (q[a][:, None] - k[a][None, :]) ** 2
    v = -float(temperature) * d
    if prior is not None:
        v = v + np.log(np.asarray(prior, dtype=np.float64) + 1e-8)
    return v


def maximum_path_f64(value, t_y: int, t_x: int):
    """value [T, L] -> (durations [L] int64, zero from t_x on; max |Q| over the band).  An infeasible item (no token, no frame, fewer
    frames than tokens) gets zeros."""
    value = np.asarray(value, dtype=np.float64)
    T, L = value.shape
    dur = np.zeros(L, dtype=np.int64)
    if t_x <= 0 or t_y <= 0 or t_y < t_x:
        return dur, 0.0
    left = np.zeros((t_y, t_x), dtype=bool)
    prev = np.full(t_x, MAX_NEG)
    q_max = 0.0
    for y in range(t_y):
        lo, hi = max(0, t_x + y - t_y), min(t_x, y + 1)
        x = np.arange(lo, hi)
        v_cur = np.where(x == y, MAX_NEG, prev[x])
        v_prev = np.where(x == 0, 0.0 if y == 0 else MAX_NEG, prev[np.maximum(x - 1, 0)])
        cur = value[y, lo:hi] + np.maximum(v_prev, v_cur)
        left[y, lo:hi] = (x != 0) & ((x == y) | (v_cur < v_prev))
        prev = prev.copy()
        prev[lo:hi] = cur
        q_max = max(q_max, float(np.abs(cur).max()))
    index = t_x - 1
    for y in range(t_y - 1, -1, -1):
        dur[index] += 1
        if index != 0 and left[y, index]:
            index -= 1
    return dur, q_max


def path_score(value, dur) -> float:
    """Sum of value along the path that gives token l dur[l] consecutive frames (float64)."""
    dur = np.asarray(dur, dtype=np.int64)
    tokens = np.repeat(np.arange(len(dur)), dur)
    return float(np.asarray(value, dtype=np.float64)[np.arange(len(tokens)), tokens].sum())


def shift_margin(value, dur) -> float:
    """By how much the path of `dur` beats the best path that differs from it in ONE boundary moved by one frame (inf: no boundary
    can move, e.g. the diagonal)."""
    value, dur = np.asarray(value, dtype=np.float64), np.asarray(dur, dtype=np.int64)
    dur = dur[: int(np.flatnonzero(dur)[-1]) + 1] if dur.any() else dur[:0]
    first = np.cumsum(dur)[:-1]  # first frame of token l + 1
    tok = np.arange(len(first))
    gains = []
    later = dur[1:] >= 2     # token l takes the first frame of token l + 1
    gains.append((value[first, tok] - value[first, tok + 1])[later])
    earlier = dur[:-1] >= 2  # token l + 1 takes the last frame of token l
    gains.append((value[first - 1, tok + 1] - value[first - 1, tok])[earlier])
    gains = np.concatenate(gains)
    return float(-gains.max()) if gains.size else float("inf")


def score_bound(T: int, q_max: float) -> float:
    """How far below the float64 optimum the float64 score of a path found in fp32 may lie: the search adds one value a frame, each
    sum rounded once (2^-24 of at most max |Q|), so the fp32 score of any path is within T 2^-24 max |Q| of its float64 score; the path
    the fp32 search returns has the best fp32 score, hence at most twice that below the optimum."""
    return 2.0 * T * 2.0 ** -24 * q_max


def structure_ok(dur, t_y: int, t_x: int) -> bool:
    """The row sums to the frame count, every token up to t_x has a frame, nothing beyond."""
    dur = np.asarray(dur)
    return int(dur.sum()) == t_y and bool((dur[:t_x] >= 1).all()) and bool((dur[t_x:] == 0).all())


# ---- planted inputs -------------------------------------------------------------------------------------------------------------------
# (L, T): one token, the pure diagonal at a wave boundary, odd sizes either side of one wave of tokens (64) and of the largest k image the
# kernel keeps in LDS at 80 channels (256 tokens), and nearly all of its 1024 threads (1000, 1023) with a narrow band
SHAPES = [(1, 1), (1, 9), (2, 2), (5, 15), (63, 130), (64, 64), (65, 400), (255, 600), (256, 256), (257, 700), (1000, 1000), (1023, 1100)]
# (temperature, with the beta-binomial prior, least margin over a single-boundary shift asked of the inputs)
SETTINGS = {"prior": (0.05, True, 1.0), "model_temperature": (0.0005, False, 0.02)}
# ... and the model's own: its temperature WITH the prior.  The margins fall to ~1e-4, below what fp32 sums of |Q| ~ 4e3 resolve: no
# equality is asked there, only the structure and score_bound
MODEL_SETTING = (0.0005, True)


def planted_durations(rng, L: int, T: int) -> np.ndarray:
    """max(1, Poisson(6)) per token, then single frames taken from (tokens above one frame) or given to random tokens until the row
    sums to T; all ones when T == L."""
    assert T >= L >= 1
    d = np.maximum(1, rng.poisson(6.0, L)).astype(np.int64)
    while d.sum() != T:
        if d.sum() > T:
            cand = np.flatnonzero(d > 1)
            pick = rng.choice(cand, size=min(len(cand), int(d.sum() - T)), replace=False)
            d[pick] -= 1
        else:
            d[rng.integers(0, L, size=int(T - d.sum()))] += 1  # (a token drawn twice gets one frame: the loop goes on)
    return d


def planted_case(L: int, T: int, seed: int = 0, A: int = A_PLANTED):
    """k ~ N(0, 1) [A, L], planted durations [L] summing to T, q_t = k_{token(t)} + 0.05 noise [A, T]; q and k as float32."""
    rng = np.random.default_rng(1000 * L + T + seed)
    k = rng.standard_normal((A, L))
    dur = planted_durations(rng, L, T)
    q = k[:, np.repeat(np.arange(L), dur)] + 0.05 * rng.standard_normal((A, T))
    return q.astype(np.float32), k.astype(np.float32), dur


@functools.lru_cache(maxsize=None)
def planted_reference(L: int, T: int, setting: str) -> dict:
    """One planted case under one of SETTINGS (or "model": MODEL_SETTING) with its float64 reference, computed once per process and shared (read only):
    q, k (float32), prior ([T, L] float64 or None), planted, temperature, value (float64), optimum, q_max, margin."""
    from oracle.attention_prior_ref import attention_prior_ref

    temperature, with_prior = MODEL_SETTING if setting == "model" else SETTINGS[setting][:2]
    q, k, planted = planted_case(L, T)
    prior = attention_prior_ref(T, L) if with_prior else None
    value = cell_values(q, k, temperature, prior)
    optimum, q_max = maximum_path_f64(value, T, L)
    return {"q": q, "k": k, "prior": prior, "planted": planted, "temperature": temperature, "value": value, "optimum": optimum,
            "q_max": q_max, "margin": shift_margin(value, optimum)}
