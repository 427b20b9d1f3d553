"""The counter-based dropout generator of csrc/common.h restated on the host (test oracle only: numpy uint32 / uint64 arithmetic,
vectorised; nothing here calls the library).

    seed      a 64-bit stream key.  With a device-resident base the kernels use (value + base) & (2^63 - 1) (SeedArg::get).
    hash      dropout_hash(seed, j_lo, j_hi): a keyed two-round 32-bit mix.  k0 and k1 depend on the seed alone:
                  k0 = lo32(seed) * 0x9E3779B1 + 0x7F4A7C15
                  k1 = (hi32(seed) ^ (k0 >> 15)) * 0x85EBCA6B + 0xC2B2AE35
              and h = j_lo ^ k0; h += j_hi * 0x27D4EB2F; h ^= h >> 16; h *= 0x7FEB352D; h ^= k1; h ^= h >> 15; h *= 0x846CA68B;
              h ^= h >> 16, everything modulo 2^32.
    draw      ONE hash serves TWO elements: element i takes hash(seed, j = i >> 1) -- j_lo / j_hi are the halves of the 64-bit j -- and
              of it the low 16 bits where i is even, the high 16 bits where i is odd.  u = float(bits) * (1 / 65536): exact in fp32.
    keep      u >= p in fp32: the keep probability is 1 - ceil(65536 p) / 65536.

The attention kernels draw element (b T + q) T + k of the stream seed + head (`attention_keep`)."""

from __future__ import annotations

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def _mul32(a, b):
    return (_u32(a) * np.uint64(b)) & _M32  # (32 x 32 bits fit 64: no wrap before the mask)


def seed_get(value: int, base: int | None = None) -> int:
    """SeedArg::get(): the seed a kernel uses for argument `value` and the optional device-resident base."""
    if base is None:
        return int(value) & 0xFFFFFFFFFFFFFFFF
    return (int(value) + int(base)) & 0x7FFFFFFFFFFFFFFF  # (the 64-bit wrap of the sum does not reach the 63 bits kept)


def dropout_hash(seed: int, j_lo, j_hi=0) -> np.ndarray:
    """uint32 hash of the pair index (j_lo, j_hi) under `seed`; j_lo / j_hi broadcast."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0 = (_mul32(seed & 0xFFFFFFFF, 0x9E3779B1) + np.uint64(0x7F4A7C15)) & _M32
    k1 = _u32(seed >> 32) ^ (k0 >> np.uint64(15))
    k1 = (_mul32(k1, 0x85EBCA6B) + np.uint64(0xC2B2AE35)) & _M32
    h = _u32(j_lo) ^ k0
    h = (h + _mul32(j_hi, 0x27D4EB2F)) & _M32
    h ^= h >> np.uint64(16)
    h = _mul32(h, 0x7FEB352D)
    h ^= k1
    h ^= h >> np.uint64(15)
    h = _mul32(h, 0x846CA68B)
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def dropout_bits(h, odd) -> np.ndarray:
    """The 16 bits an element takes of its pair's hash: the low half (even element) or the high half (odd element)."""
    h = np.asarray(h, dtype=np.uint32)
    return np.where(np.asarray(odd).astype(bool), h >> np.uint32(16), h & np.uint32(0xFFFF)).astype(np.uint32)


def dropout_u16(h, odd) -> np.ndarray:
    return dropout_bits(h, odd).astype(np.float32) * np.float32(1.0 / 65536.0)


def element_bits(seed: int, i) -> np.ndarray:
    """The 16-bit draw of element(s) i (any integer array below 2^64) of stream `seed`."""
    i = np.asarray(i, dtype=np.uint64)
    j = i >> np.uint64(1)
    return dropout_bits(dropout_hash(seed, j & _M32, j >> np.uint64(32)), i & np.uint64(1))


def uniform01(seed: int, i) -> np.ndarray:
    return element_bits(seed, i).astype(np.float32) * np.float32(1.0 / 65536.0)


def keep_at(seed: int, i, p: float) -> np.ndarray:
    """bool: element(s) i of stream `seed` survive dropout with probability argument p (compared in fp32, as the kernels do)."""
    return np.float32(1.0 / 65536.0) * element_bits(seed, i).astype(np.float32) >= np.float32(p)


def keep_mask(seed: int, n: int, p: float) -> np.ndarray:
    """bool[n]: the first n elements of stream `seed`."""
    return keep_at(seed, np.arange(n, dtype=np.uint64), p)


def keep_rate(p: float) -> float:
    """The exact keep probability of a draw: 1 - ceil(65536 p) / 65536 (p as the fp32 the kernel receives)."""
    import math

    return 1.0 - math.ceil(65536.0 * float(np.float32(p))) / 65536.0


def attention_keep(seed: int, B: int, H: int, T: int, p: float) -> np.ndarray:
    """bool [B, H, Tq, Tk]: the attention kernels' mask -- element (b T + q) T + k of stream seed + h."""
    idx = np.arange(B * T * T, dtype=np.uint64)
    return np.stack([keep_at(seed_get(seed + h), idx, p).reshape(B, T, T) for h in range(H)], axis=1)
