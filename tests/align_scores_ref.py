"""The alignment scores restated -- what tests/test_align_scores_host.py and tests/test_gpu_align_scores.py hold
``evmi_align_scores_f32`` and ``FastSpeech2.align(return_scores=True)`` to.  Built from the oracle's ``alignment_attention_ref`` and
``forward_sum_loss_ref`` (the definition), in float64 for the reference and in float32 for the calibration:

  ctc       forward_sum_loss_ref of the item's attn_logprob (one item: no batch mean left)
  path      -mean over the frames of log(max(soft[y][p(y)], 1e-12)), p = the path where symbol x holds dur[x] consecutive frames
  symbol[x] mean of the same term over symbol x's own frames (NaN for a symbol without a frame)

THE BOUND follows tests/test_gpu_alignment_primitives.py: the CTC recurrence has no usable closed bound, so err32 = the error of this
same restatement evaluated in float32 on the CPU against its float64 evaluation, on the same input, and the kernel gets
4 x max(err32, 1e-6 x max(1, |value|)) -- per item for ctc and path, per symbol for symbol.  The floor is relative to max(1, |value|)
because the scores are logarithms: a value near 0 carries the absolute rounding of the lse it was subtracted from.  The host test
asserts what makes the bound meaningful (a wrong lattice state or a boundary off by one frame lies far outside it).

``ctc_lattice_f64`` is an explicit lattice, independent of ``F.ctc_loss``; the host test holds the two together.
"""

from __future__ import annotations

import functools

import numpy as np
import torch

import align_ref as R
from oracle.alignment_ref import alignment_attention_ref, forward_sum_loss_ref

BLANK = -1.0
FACTOR, FLOOR = 4.0, 1e-6
LOG_FLOOR = 1e-12
# (temperature, with the beta-binomial prior): align_ref's two SETTINGS and its MODEL_SETTING, and the fourth combination
SETTINGS = {"prior": (0.05, True), "model_temperature": (0.0005, False), "model": (0.0005, True), "sharp_no_prior": (0.05, False)}
FRAME_CHUNK = 128  # frames per call of alignment_attention_ref: its [A, T, L] intermediate stays small


def attention(q, k, prior, temperature, dtype=torch.float64):
    """q [A, T], k [A, L] float32 numpy, prior [T, L] float64 numpy or None -> (soft [T, L], attn_logprob [T, L]) in `dtype`, the
    oracle's, a block of frames at a time (a frame's row depends on no other frame)."""
    qt, kt = torch.from_numpy(q).to(dtype)[None], torch.from_numpy(k).to(dtype)[None]
    T, L = q.shape[1], k.shape[1]
    pt = None if prior is None else torch.from_numpy(prior)[None]
    soft, logprob = [], []
    for t0 in range(0, T, FRAME_CHUNK):
        s, lp = alignment_attention_ref(qt[:, :, t0 : t0 + FRAME_CHUNK], kt, torch.tensor([L]), None if pt is None else pt[:, t0 : t0 + FRAME_CHUNK],
                                        temperature)
        soft.append(s[0])
        logprob.append(lp[0])
    return torch.cat(soft), torch.cat(logprob)


def scores_from(soft, logprob, dur, blank=BLANK):
    """(ctc, path, symbol [L]) as Python floats / a float64 array, every step in the dtype of `soft` / `logprob`."""
    T, L = soft.shape
    ctc = float(forward_sum_loss_ref(logprob[None], torch.tensor([L]), torch.tensor([T]), blank))
    dur = np.asarray(dur, dtype=np.int64)
    assert dur.shape == (L,) and dur.sum() == T and (dur >= 0).all()
    tokens = torch.from_numpy(np.repeat(np.arange(L), dur))
    on_path = torch.log(torch.clamp(soft[torch.arange(T), tokens], min=LOG_FLOOR))
    path = float(-(on_path.sum() / T))
    sums = torch.zeros(L, dtype=soft.dtype).index_add_(0, tokens, on_path)
    with np.errstate(invalid="ignore", divide="ignore"):
        symbol = np.where(dur > 0, sums.double().numpy() / dur, np.nan)
    return ctc, path, symbol


def ctc_lattice_f64(logprob, blank=BLANK) -> float:
    """The CTC forward-sum loss of one item, written out: logprob [T, L] -> -log p(1 .. L) / L.  States blank, 1, blank, 2, ..., L,
    blank; a symbol state is entered from itself, the blank before it and the symbol before that (all labels differ)."""
    lp = np.asarray(logprob, dtype=np.float64)
    T, L = lp.shape
    ext = np.concatenate([np.full((T, 1), float(blank)), lp], axis=1)
    m = ext.max(1, keepdims=True)
    ext = ext - (m + np.log(np.exp(ext - m).sum(1, keepdims=True)))
    S = 2 * L + 1
    labels = np.zeros(S, dtype=np.int64)
    labels[1::2] = np.arange(1, L + 1)
    alpha = np.full(S, -np.inf)
    alpha[:2] = ext[0, labels[:2]]
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            one = np.concatenate([[-np.inf], alpha[:-1]])
            two = np.concatenate([[-np.inf, -np.inf], alpha[:-2]])
            two[0::2] = -np.inf
            alpha = np.logaddexp(np.logaddexp(alpha, one), two) + ext[t, labels]
        ll = np.logaddexp(alpha[-1], alpha[-2])
    return float(-ll / L)


def bound(err32, value):
    return FACTOR * np.maximum(err32, FLOOR * np.maximum(1.0, np.abs(value)))


def calibrated(q, k, prior, dur, temperature, keep_soft=False) -> dict:
    """The float64 scores of one item, err32 and the kernel's bound for each."""
    soft64, lp64 = attention(q, k, prior, temperature, torch.float64)
    ctc64, path64, sym64 = scores_from(soft64, lp64, dur)
    ctc32, path32, sym32 = scores_from(*attention(q, k, prior, temperature, torch.float32), dur)
    out = {"ctc": ctc64, "path": path64, "symbol": sym64, "ctc_err32": abs(ctc32 - ctc64), "path_err32": abs(path32 - path64),
           "symbol_err32": np.abs(sym32 - sym64)}
    for name in ("ctc", "path", "symbol"):
        out[name + "_bound"] = bound(out[name + "_err32"], out[name])
    if keep_soft:
        out["soft"], out["logprob"] = soft64.numpy(), lp64.numpy()
    return out


def least_shift_ratio(soft, dur, symbol_bound) -> float:
    """Move ONE boundary of the path by one frame (symbol l takes the first frame of l + 1, or l + 1 the last frame of l; the giver
    keeps at least one frame): the scores of the two symbols change.  -> over every such move, the larger of the two changes in units of
    that symbol's bound; the least of them (inf where no boundary can move)."""
    dur = np.asarray(dur, dtype=np.int64)
    L = len(dur)
    if L < 2:
        return float("inf")
    ls = np.log(np.maximum(soft, LOG_FLOOR))
    tokens = np.repeat(np.arange(L), dur)
    sums = np.bincount(tokens, weights=ls[np.arange(len(tokens)), tokens], minlength=L)
    mean = sums / dur
    first = np.cumsum(dur)[:-1]  # first frame of symbol l + 1
    lo, hi = np.arange(L - 1), np.arange(1, L)
    ratios = []
    for frame, taker, giver in ((first, lo, hi), (first - 1, hi, lo)):
        ok = dur[giver] >= 2
        d_taker = np.abs((sums[taker] + ls[frame, taker]) / (dur[taker] + 1) - mean[taker]) / symbol_bound[taker]
        d_giver = np.abs((sums[giver] - ls[frame, giver]) / np.maximum(dur[giver] - 1, 1) - mean[giver]) / symbol_bound[giver]
        ratios.append(np.maximum(d_taker, d_giver)[ok])
    ratios = np.concatenate(ratios)
    return float(ratios.min()) if ratios.size else float("inf")


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------------
def planted_inputs(L: int, T: int, setting: str, A: int = R.A_PLANTED) -> dict:
    """A planted case of align_ref under one of SETTINGS with its float64 optimum as the row to score (align_ref.planted_reference's
    inputs for its own settings at 80 channels)."""
    from oracle.attention_prior_ref import attention_prior_ref

    temperature, with_prior = SETTINGS[setting]
    q, k, _ = R.planted_case(L, T, A=A)
    prior = attention_prior_ref(T, L) if with_prior else None
    dur, _ = R.maximum_path_f64(R.cell_values(q, k, temperature, prior), T, L)
    return {"q": q, "k": k, "prior": prior, "temperature": temperature, "dur": dur}


@functools.lru_cache(maxsize=None)
def planted_scores(L: int, T: int, setting: str, A: int = R.A_PLANTED) -> dict:
    """planted_inputs with calibrated() and least_shift_ratio; computed once per process and shared (read only)."""
    r = planted_inputs(L, T, setting, A)
    c = calibrated(r["q"], r["k"], r["prior"], r["dur"], r["temperature"], keep_soft=True)
    c["shift_ratio"] = least_shift_ratio(c.pop("soft"), r["dur"], c["symbol_bound"])
    c.pop("logprob")
    return {**r, **c}


def plan(A: int, L: int):
    """(frames of one LDS tile, k image in LDS) of evmi_align_scores_f32: host arithmetic of the built library."""
    import ctypes

    from everyvoice_amd import _lib

    ty, klds = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.load().evmi_align_scores_plan(A, L, ctypes.byref(ty), ctypes.byref(klds))
    assert rc == _lib.EVMI_OK, _lib.load().evmi_last_error()
    return ty.value, bool(klds.value)


def k_switch(A: int = R.A_PLANTED) -> int:
    """The largest L whose k image sits in LDS at A channels (L + 1 reads k through the caches)."""
    inside = [L for L in range(1, 1024) if plan(A, L)[1]]
    assert inside and inside == list(range(1, inside[-1] + 1)) and inside[-1] < 1023, inside[-1:]
    return inside[-1]


def kernel_cases() -> list:
    """(L, T, setting, A) of the kernel-alone test: the issue's shapes in every setting, the frame tile's edges and both sides of the k
    switch from the plan query, 3 and 128 channels, and the items of the ragged batch."""
    shapes = [(1, 1), (1, 9), (2, 2), (5, 15), (63, 130), (64, 64), (65, 400), (1000, 1000), (1023, 1100)]  # (the last: B = 1, the L limit)
    ty = plan(R.A_PLANTED, 20)[0]
    shapes += [(20, ty - 1), (20, ty), (20, ty + 1), (20, 2 * ty + 1)]
    sw = k_switch()
    shapes += [(sw, sw), (sw, sw + 344), (sw + 1, sw + 444)]  # (256: align_ref's (256, 256), and (256, 600), (257, 700))
    cases = [(L, T, s, R.A_PLANTED) for L, T in shapes for s in SETTINGS]
    # (3 channels at the model's temperature give a nearly flat attention: no boundary is visible there, so the sharp settings)
    cases += [(37, 150, s, 3) for s in ("prior", "sharp_no_prior")] + [(130, 300, s, 128) for s in ("prior", "model")]
    cases += [(Lb, Tb, RAGGED_SETTING, R.A_PLANTED) for Lb, Tb in RAGGED if (Lb, Tb, RAGGED_SETTING, R.A_PLANTED) not in cases]
    return cases


RAGGED = [(37, 221), (1, 3), (150, 907), (64, 64)]  # (L_b, T_b) of the ragged batch, padded to (150, 907)
RAGGED_SETTING = "prior"
ACROSS_SWITCH = (150, 907)  # the ragged item that is also run in a batch padded beyond the k switch (its k image leaves the LDS there)
