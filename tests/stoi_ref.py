"""Intrusive STOI (Taal, Hendriks, Heusdens, Jensen 2011) restated in numpy from its definition, in float64 or
float32: the reference of tests/test_stoi_host.py and tests/test_gpu_stoi.py.  Written from the definition, not from the kernel: the
kept frames are overlap-added into a signal and framed again, the transform is a product with a DFT matrix, the segments are taken
one by one.  Signals at 10 kHz."""

from functools import lru_cache

import numpy as np

FS, FRAME, HOP, NFFT, BANDS, N, BETA_DB, RANGE_DB = 10000, 256, 128, 512, 15, 30, -15.0, 40.0
EPS = 2.220446049250313e-16
BAND_TABLE = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138),
              (138, 174), (174, 219)]


def bands():
    """[(first bin, one past the last bin)] of the 15 one-third-octave bands: centres 150 x 2^(b/3) Hz, edges x 2^(+-1/6), each snapped
    to the nearest of the 257 bins of linspace(0, 10000, 513)."""
    f = np.linspace(0.0, FS, NFFT + 1)[: NFFT // 2 + 1]
    out = []
    for b in range(BANDS):
        cf = 150.0 * 2.0 ** (b / 3.0)
        lo, hi = cf * 2.0 ** (-1.0 / 6.0), cf * 2.0 ** (1.0 / 6.0)
        out.append((int(np.argmin((f - lo) ** 2)), int(np.argmin((f - hi) ** 2))))
    return out


def window(dtype=np.float64):
    return np.hanning(FRAME + 2)[1:-1].astype(dtype)


def frames_of(x, w):
    """Rows w . x[128 i : 128 i + 256] for every i with 128 i < len(x) - 256 (the last admissible start is left out)."""
    starts = range(0, len(x) - FRAME, HOP)
    return np.array([w * x[s : s + FRAME] for s in starts], dtype=x.dtype).reshape(len(starts), FRAME)


@lru_cache(maxsize=None)
def _dft(dtype_name):
    t = np.arange(FRAME, dtype=np.float64)
    k = np.arange(NFFT // 2 + 1, dtype=np.float64)
    ang = 2.0 * np.pi * ((k[:, None] * t[None, :]) % NFFT) / NFFT
    return np.cos(ang).astype(dtype_name), np.sin(ang).astype(dtype_name)


def band_values(fr, dtype):
    """[15, frames]: sqrt of the power of the 512-point transform of each 256-sample frame summed over each band's bins."""
    c, s = _dft(np.dtype(dtype).name)
    re, im = fr @ c.T, fr @ s.T
    power = re * re + im * im
    return np.array([np.sqrt(power[:, lo:hi].sum(axis=1, dtype=dtype)) for lo, hi in bands()], dtype=dtype).reshape(BANDS, fr.shape[0])


def stoi(ref, deg, dtype=np.float64):
    """-> dict(stoi, F, K, J, segment [J], frame_of [K], margin): margin is the smallest distance in dB of any frame's energy to the
    40 dB threshold (inf without frames)."""
    dtype = np.dtype(dtype).type
    n = min(len(ref), len(deg))
    x, y = np.asarray(ref[:n], dtype=dtype), np.asarray(deg[:n], dtype=dtype)
    w = window(dtype)
    eps, nan = dtype(EPS), float("nan")
    xf, yf = frames_of(x, w), frames_of(y, w)
    F = xf.shape[0]
    assert F == (-(-(n - FRAME) // HOP) if n > FRAME else 0)
    empty = dict(stoi=nan, F=F, K=0, J=0, segment=np.zeros(0, dtype), frame_of=np.zeros(0, np.int32), margin=float("inf"))
    if F == 0:
        return empty
    e = dtype(20.0) * np.log10(np.sqrt((xf * xf).sum(axis=1, dtype=dtype)) + eps)
    slack = e.max() - dtype(RANGE_DB) - e
    keep = slack < 0
    kept = np.nonzero(keep)[0].astype(np.int32)
    K = len(kept)
    out = dict(empty, K=K, frame_of=kept, margin=float(np.abs(slack.astype(np.float64)).min()))
    if K < 2:
        return out

    def again(frames):
        sig = np.zeros((K - 1) * HOP + FRAME, dtype=dtype)
        for k, i in enumerate(kept):
            sig[k * HOP : k * HOP + FRAME] += frames[i]
        return frames_of(sig, w)

    X, Y = band_values(again(xf), dtype), band_values(again(yf), dtype)
    assert X.shape == (BANDS, K - 1)
    J = K - N if K >= N + 1 else 0
    out["J"] = J
    if J == 0:
        return out
    clip = dtype(1.0 + 10.0 ** (-BETA_DB / 20.0))
    rho = np.zeros((J, BANDS), dtype=dtype)
    for j, m in enumerate(range(N, K)):
        for b in range(BANDS):
            xs, ys = X[b, m - N : m], Y[b, m - N : m]
            c = np.sqrt((xs * xs).sum(dtype=dtype)) / (np.sqrt((ys * ys).sum(dtype=dtype)) + eps)
            yp = np.minimum(c * ys, xs * clip)
            xc, yc = xs - xs.mean(dtype=dtype), yp - yp.mean(dtype=dtype)
            xc = xc / (np.sqrt((xc * xc).sum(dtype=dtype)) + eps)
            yc = yc / (np.sqrt((yc * yc).sum(dtype=dtype)) + eps)
            rho[j, b] = (xc * yc).sum(dtype=dtype)
    out.update(stoi=float(rho.mean(dtype=dtype)), segment=rho.mean(axis=1, dtype=dtype))
    return out


# ---- the signals of the tests -----------------------------------------------------------------------------------------------------------
def closed_form(g, n=20000):
    """(x, x + g noise): a modulated three-tone signal with 0.4 s of silence, and a chirp-like noise."""
    i = np.arange(n, dtype=np.float64)
    t = i / FS
    x = (0.5 + 0.5 * np.sin(2 * np.pi * 3 * t)) * (np.sin(2 * np.pi * 220 * t) + 0.5 * np.sin(2 * np.pi * 880 * t) + 0.25 * np.sin(2 * np.pi * 2500 * t))
    x[8000:12000] = 0.0
    noise = np.sin(0.37 * i + 0.0123 * i * i)
    return x, x + g * noise


def noise_pair(seed, n, g=0.4, gap=None):
    """A seeded noise-like pair: white noise under a slow envelope (with a silent stretch where ``gap`` = (first, last) is given), and
    that plus g times other noise."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.float64)
    x = rng.standard_normal(n) * (0.6 + 0.4 * np.sin(2 * np.pi * 2.5 * i / FS))
    if gap is not None:
        x[gap[0] : gap[1]] = 0.0
    return x, x + g * rng.standard_normal(n)
