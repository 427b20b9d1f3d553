"""Mel-cepstral distortion along the dynamic-time-warping path, restated in numpy -- what tests/test_dtw_host.py and
tests/test_gpu_dtw.py hold ``evmi_dtw_cepstral_f32`` to.

``dtw(a, b, basis, scale, dtype)`` follows the header's definition in ``dtype`` (float64 or float32) with the same operation order and
tie rule; ``path_cost64`` prices any path in float64; ``brute_force`` enumerates every monotone path of a small rectangle.

The inputs of the GPU tests are built here so that the host file can assert their conditions without a GPU:
  lattice cases   a basis with entries in {-1, 0, 1}, at most 8 non-zeros a row, features on the quarter lattice in [-1, 1]: every
                  partial sum of ca, cb and s is exactly representable in float32 (``exact_in_float32``), so fmaf and multiply-add
                  agree and the float32 restatement is the bit oracle.  "planted": both sides repeat frames of one base sequence whose
                  adjacent cepstra differ; where only one side repeats, the zero-cost path is unique and equals the planted warp.
                  "random": two independent lattice sequences (non-zero costs, many exact ties).
  real cases      mel-like sequences (a random walk over frames plus noise), one side a resampled and jittered copy, the DCT basis.
                  THE BOUND on dist and col is section 15's: 4 x max(err32, 1e-6 x max(1, |value|)), err32 the float32 restatement's
                  error against float64 on the same case."""

from __future__ import annotations

import functools
import itertools
import math

import numpy as np

MCD_SCALE = 10.0 * math.sqrt(2.0) / math.log(10.0)
LATTICE_SCALE = 1.5
LATTICE_SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (63, 64), (64, 65), (65, 64), (128, 127), (257, 300), (700, 257), (1023, 1024), (1024, 1024)]
LATTICE_KM = [(1, 3), (13, 80), (24, 128)]
RANDOM_LATTICE_SHAPES = [(5, 1), (2, 2), (63, 64), (257, 300), (1024, 1024)]  # at K 13, M 80
REAL_SHAPES = [(97, 131), (585, 640), (1024, 947)]
REAL_K, REAL_M = 13, 80


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def _fma(x, y, acc, dtype):
    """fmaf in ``dtype``.  float32: the product of two float32 values is exact in float64, so one float64 add and one rounding to
    float32 give the fused result (up to a double rounding that the lattice cases never meet: their sums are exact)."""
    if dtype == np.float32:
        return (x.astype(np.float64) * y.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return x * y + acc


def cepstra(x, basis, dtype):
    """x [T, M], basis [K, M] -> [T, K]: acc = fma(basis[k][m], x[i][m], acc), m ascending from 0."""
    x, basis = np.asarray(x, dtype=dtype), np.asarray(basis, dtype=dtype)
    acc = np.zeros((x.shape[0], basis.shape[0]), dtype=dtype)
    for m in range(x.shape[1]):
        acc = _fma(np.broadcast_to(basis[None, :, m], acc.shape), np.broadcast_to(x[:, m, None], acc.shape), acc, dtype)
    return acc


def costs(ca, cb, dtype):
    """c[i][j] = sqrt(s), s = fma(d_k, d_k, s), d_k = ca[i][k] - cb[j][k], k ascending, s from 0."""
    s = np.zeros((ca.shape[0], cb.shape[0]), dtype=dtype)
    for k in range(ca.shape[1]):
        d = ca[:, None, k] - cb[None, :, k]
        s = _fma(d, d, s, dtype)
    return np.sqrt(s)


def recurrence(c):
    """D and the decision of every cell (0 diagonal, 1 up, 2 left) in c's dtype, one anti-diagonal at a time.  best = the diagonal
    where it exists, else +inf; then up if strictly smaller; then left if strictly smaller (a comparison with NaN is false)."""
    Na, Nb = c.shape
    dtype = c.dtype
    D = np.full((Na + 1, Nb + 1), np.inf, dtype=dtype)  # D[i + 1][j + 1]; the border stands for "does not exist"
    dec = np.zeros((Na, Nb), dtype=np.uint8)
    for s in range(Na + Nb - 1):
        i = np.arange(max(0, s - Nb + 1), min(Na, s + 1))
        j = s - i
        diag, up, left = D[i, j], D[i, j + 1], D[i + 1, j]
        best, d = diag.copy(), np.zeros(len(i), dtype=np.uint8)
        with np.errstate(invalid="ignore"):
            take = (i > 0) & (up < best)
            best[take], d[take] = up[take], 1
            take = (j > 0) & (left < best)
            best[take], d[take] = left[take], 2
        D[i + 1, j + 1] = c[i, j] if s == 0 else c[i, j] + best
        dec[i, j] = d
    return D[1:, 1:], dec


def walk(dec):
    """The path from (Na - 1, Nb - 1) back to (0, 0): (steps, lo [Nb], hi [Nb]).  Row 0 goes left, column 0 goes up."""
    Na, Nb = dec.shape
    i, j, steps = Na - 1, Nb - 1, 1
    lo, hi = np.zeros(Nb, dtype=np.int32), np.zeros(Nb, dtype=np.int32)
    hi[j] = i
    while i > 0 or j > 0:
        d = 2 if i == 0 else 1 if j == 0 else int(dec[i, j])
        if d == 1:
            i -= 1
        else:
            lo[j] = i
            if d != 2:
                i -= 1
            j -= 1
            hi[j] = i
        steps += 1
    lo[0] = 0
    return steps, lo, hi


def finish(c, D_end, steps, lo, hi, scale):
    dtype = c.dtype.type
    dist = dtype(scale) * D_end / dtype(steps)
    col = np.zeros(c.shape[1], dtype=c.dtype)
    for j in range(c.shape[1]):
        total = dtype(0)
        for i in range(lo[j], hi[j] + 1):
            total = total + c[i, j]
        col[j] = dtype(scale) * total / dtype(hi[j] - lo[j] + 1)
    return dist, col


def dtw(a, b, basis, scale, dtype):
    """-> dict(dist, steps, lo, hi, col, c, D) of one item a [Na, M], b [Nb, M] in ``dtype``."""
    c = costs(cepstra(a, basis, dtype), cepstra(b, basis, dtype), dtype)
    D, dec = recurrence(c)
    steps, lo, hi = walk(dec)
    dist, col = finish(c, D[-1, -1], steps, lo, hi, scale)
    return {"dist": dist, "steps": steps, "lo": lo, "hi": hi, "col": col, "c": c, "D": D}


def path_cells(lo, hi):
    """The cells of the path that lo / hi describe (steps (1,0), (0,1), (1,1)): column j holds rows lo[j] .. hi[j]."""
    return [(i, j) for j in range(len(lo)) for i in range(int(lo[j]), int(hi[j]) + 1)]


def is_path(lo, hi, Na):
    """lo / hi describe a monotone path from (0, 0) to (Na - 1, Nb - 1)."""
    lo, hi = np.asarray(lo).astype(np.int64), np.asarray(hi).astype(np.int64)
    return bool(lo[0] == 0 and hi[-1] == Na - 1 and (lo <= hi).all() and ((lo[1:] == hi[:-1]) | (lo[1:] == hi[:-1] + 1)).all())


def path_cost64(a, b, basis, lo, hi):
    """The float64 cost (unscaled sum of c) of the path lo / hi."""
    c = costs(cepstra(a, basis, np.float64), cepstra(b, basis, np.float64), np.float64)
    return float(sum(c[i, j] for i, j in path_cells(lo, hi)))


def brute_force(c):
    """Every monotone path of a small rectangle: the smallest total cost."""
    Na, Nb = c.shape

    @functools.lru_cache(maxsize=None)
    def totals(i, j):
        if i == 0 and j == 0:
            return (float(c[0, 0]),)
        out = []
        for pi, pj in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
            if pi >= 0 and pj >= 0:
                out.extend(t + float(c[i, j]) for t in totals(pi, pj))
        return tuple(out)

    return min(totals(Na - 1, Nb - 1))


def bound(err32, value):
    return 4.0 * np.maximum(err32, 1e-6 * np.maximum(1.0, np.abs(value)))


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------------
def lattice_basis(K, M, seed=0):
    """[K, M] float32 with entries in {-1, 0, 1}, between 1 and 8 non-zeros a row, the rows distinct where M allows."""
    rng = np.random.default_rng(1000 * K + M + seed)
    basis = np.zeros((K, M), dtype=np.float32)
    for k in range(K):
        nz = rng.choice(M, size=min(M, int(rng.integers(1, 9))), replace=False)
        basis[k, nz] = rng.choice([-1.0, 1.0], size=len(nz))
    return basis


def _lattice_frames(rng, n, M):
    return (rng.integers(-4, 5, size=(n, M)) / 4.0).astype(np.float32)


def _base_sequence(rng, n, M, basis):
    """n lattice frames whose adjacent cepstra differ."""
    x = _lattice_frames(rng, n, M)
    for _ in range(1000):
        cx = cepstra(x, basis, np.float64)
        same = np.nonzero((cx[1:] == cx[:-1]).all(axis=1))[0] + 1
        if len(same) == 0:
            return x
        x[same] = _lattice_frames(rng, len(same), M)
    raise AssertionError("no base sequence with distinct neighbours")


def _warp(rng, n_base, n):
    """A non-decreasing map of n frames onto all of n_base base frames (n >= n_base): which base frame each frame repeats."""
    extra = np.sort(rng.integers(0, n_base, size=n - n_base))
    return np.sort(np.concatenate([np.arange(n_base), extra])).astype(np.int64)


@functools.lru_cache(maxsize=None)
def lattice_case(Ta, Tb, K, M, kind="planted"):
    """-> dict(a, b, basis, scale, kind, plant).  planted: both sides repeat frames of one base sequence; where the shorter side is the
    base itself (Ta != Tb) ``plant`` is (lo, hi) of the unique zero-cost path, else (Ta == Tb: both repeat) None."""
    rng = np.random.default_rng(7 + 100003 * Ta + 1009 * Tb + 17 * K + M + (0 if kind == "planted" else 1))
    basis = lattice_basis(K, M)
    if kind == "random":
        return {"a": _lattice_frames(rng, Ta, M), "b": _lattice_frames(rng, Tb, M), "basis": basis, "scale": LATTICE_SCALE, "kind": kind, "plant": None}
    n_base = min(Ta, Tb) if Ta != Tb else max(1, (3 * Ta) // 4)
    base = _base_sequence(rng, n_base, M, basis)
    wa, wb = _warp(rng, n_base, Ta), _warp(rng, n_base, Tb)
    plant = None
    if Ta != Tb:  # cell (i, j) is on the planted path iff both frames repeat the same base frame
        lo = np.array([int(np.nonzero(wa == wb[j])[0][0]) for j in range(Tb)], dtype=np.int32)
        hi = np.array([int(np.nonzero(wa == wb[j])[0][-1]) for j in range(Tb)], dtype=np.int32)
        plant = (lo, hi)
    return {"a": base[wa].copy(), "b": base[wb].copy(), "basis": basis, "scale": LATTICE_SCALE, "kind": kind, "plant": plant}


def lattice_keys(diag_chunk):
    """(Ta, Tb, K, M, kind) of every lattice case of the GPU file: the listed shapes at the three (K, M), both sides of a diag_chunk
    edge (Ta + Tb - 1 == diag_chunk and diag_chunk + 1; 2 diag_chunk and 2 diag_chunk + 1), and the random ones."""
    h = diag_chunk // 2
    edges = [(h, h + 1), (h + 1, h + 1), (diag_chunk, diag_chunk + 1), (diag_chunk + 2, diag_chunk)]
    keys = [(Ta, Tb, K, M, "planted") for (Ta, Tb), (K, M) in itertools.product(LATTICE_SHAPES + edges, LATTICE_KM)]
    keys += [(Ta, Tb, 13, 80, "random") for Ta, Tb in RANDOM_LATTICE_SHAPES + edges[:2]]
    return keys + [key for key in ragged_keys() if key not in keys]


RAGGED = [(64, 65), (1, 5), (257, 300), (5, 1), (128, 127)]  # (Na, Nb) of the items of the ragged batch: K 13, M 80


def ragged_keys():
    return [(Na, Nb, 13, 80, "random" if i % 2 else "planted") for i, (Na, Nb) in enumerate(RAGGED)]


def exact_in_float32(x, basis):
    """Every partial sum of the cepstra of x is a float32 value (float64 arithmetic, checked at each m)."""
    x64, b64 = np.asarray(x, np.float64), np.asarray(basis, np.float64)
    acc = np.zeros((x64.shape[0], b64.shape[0]))
    for m in range(x64.shape[1]):
        acc = acc + b64[None, :, m] * x64[:, m, None]
        if not (acc == acc.astype(np.float32)).all():
            return False
    return True


def costs_exact_in_float32(ca, cb):
    """Every partial sum of s = sum_k (ca[i][k] - cb[j][k])^2 is a float32 value (float64 arithmetic, checked at each k)."""
    ca, cb = np.asarray(ca, np.float64), np.asarray(cb, np.float64)
    s = np.zeros((ca.shape[0], cb.shape[0]))
    for k in range(ca.shape[1]):
        d = ca[:, None, k] - cb[None, :, k]
        if not (d == d.astype(np.float32)).all():
            return False
        s = s + d * d
        if not (s == s.astype(np.float32)).all():
            return False
    return True


def dct_basis(n_mels, n_cepstra):
    """Orthonormal DCT-II rows 1 .. n_cepstra (what pipeline.mel_cepstral_basis builds), float32."""
    m, k = np.arange(n_mels, dtype=np.float64), np.arange(1, n_cepstra + 1, dtype=np.float64)
    return (math.sqrt(2.0 / n_mels) * np.cos(math.pi / n_mels * (m[None, :] + 0.5) * k[:, None])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def real_case(Ta, Tb):
    """Mel-like: b a random walk over frames (natural-log mel range) plus noise; a its resampled (to Ta frames, with a wandering
    rate) and jittered copy."""
    rng = np.random.default_rng(31 + 1009 * Ta + Tb)
    M = REAL_M
    walk_ = np.cumsum(rng.normal(0.0, 0.35, size=(Tb, M)), axis=0)
    walk_ = walk_ - walk_.mean(axis=0, keepdims=True)
    tilt = np.linspace(-2.0, -7.0, M)[None, :]
    b = np.clip(tilt + 0.6 * walk_ + rng.normal(0.0, 0.1, size=(Tb, M)), -11.5, 2.0)
    rate = np.cumsum(np.exp(rng.normal(0.0, 0.25, size=Ta)))
    pos = (rate - rate[0]) / max(rate[-1] - rate[0], 1e-9) * (Tb - 1)
    f = np.floor(pos).astype(np.int64).clip(0, Tb - 1)
    g = (f + 1).clip(0, Tb - 1)
    w = (pos - f)[:, None]
    a = (1 - w) * b[f] + w * b[g] + rng.normal(0.0, 0.15, size=(Ta, M))
    return {"a": a.astype(np.float32), "b": b.astype(np.float32), "basis": dct_basis(M, REAL_K), "scale": np.float32(MCD_SCALE)}


@functools.lru_cache(maxsize=None)
def real_expectation(Ta, Tb):
    """-> (float64 result, float32 result) of real_case(Ta, Tb)."""
    r = real_case(Ta, Tb)
    return dtw(r["a"], r["b"], r["basis"], float(r["scale"]), np.float64), dtw(r["a"], r["b"], r["basis"], r["scale"], np.float32)


@functools.lru_cache(maxsize=None)
def lattice_expectation(key):
    r = lattice_case(*key)
    return dtw(r["a"], r["b"], r["basis"], r["scale"], np.float32)
