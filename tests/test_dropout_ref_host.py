"""tests/dropout_ref.py -- the dropout generator of csrc/common.h restated in numpy -- checked on the host against a second statement of
the same arithmetic in plain Python integers, and for the properties the comments of common.h promise: one hash per pair of elements,
the keep rate 1 - ceil(65536 p) / 65536, streams of neighbouring seeds unrelated, the pair index's high word counted.  No GPU: the
comparison with the kernels is tests/test_gpu_fs2_train_primitives.py."""

import math

import numpy as np

import dropout_ref as R

M = 0xFFFFFFFF


def hash_py(seed, j_lo, j_hi):
    """dropout_hash in Python integers, one value at a time (nothing shared with the numpy form but the constants)."""
    k0 = ((seed & M) * 0x9E3779B1 + 0x7F4A7C15) & M
    k1 = ((seed >> 32) & M) ^ (k0 >> 15)
    k1 = (k1 * 0x85EBCA6B + 0xC2B2AE35) & M
    h = (j_lo ^ k0) & M
    h = (h + j_hi * 0x27D4EB2F) & M
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M
    h ^= k1
    h ^= h >> 15
    h = (h * 0x846CA68B) & M
    h ^= h >> 16
    return h


def test_numpy_form_equals_the_integer_form():
    rng = np.random.default_rng(0)
    seeds = [0, 1, 7, 99, 2**32 - 1, 2**32, 2**63 - 1, 2**64 - 1, 0x0123456789ABCDEF]
    for seed in seeds:
        j_lo = rng.integers(0, 2**32, 64, dtype=np.uint64)
        j_lo[:4] = [0, 1, 2**32 - 1, 2**31]
        for j_hi in (0, 1, 2**32 - 1):
            got = R.dropout_hash(seed, j_lo, j_hi)
            assert got.dtype == np.uint32
            assert [int(v) for v in got] == [hash_py(seed, int(j), j_hi) for j in j_lo]
    # element i -> pair i >> 1, halves of the 64-bit pair index, low / high 16 bits by parity
    for i in (0, 1, 2, 3, 2**33 - 1, 2**33, 2**33 + 1, 2**64 - 1):
        j = i >> 1
        h = hash_py(99, j & M, j >> 32)
        want = (h >> 16) if i & 1 else (h & 0xFFFF)
        assert int(R.element_bits(99, np.array([i], dtype=np.uint64))[0]) == want
        assert float(R.uniform01(99, np.array([i], dtype=np.uint64))[0]) == want / 65536.0


def test_seed_with_a_device_base_keeps_63_bits():
    assert R.seed_get(5) == 5 and R.seed_get(2**64 - 1) == 2**64 - 1
    assert R.seed_get(5, 0) == 5 and R.seed_get(5, 10) == 15
    assert R.seed_get(1, 2**63 - 1) == 0              # bit 63 of the sum is dropped
    assert R.seed_get(2**64 - 1, 2) == 1              # the sum wraps at 64 bits first: the same 63 bits
    assert R.seed_get(2**63 + 3, None) == 2**63 + 3   # without a base nothing is masked


def test_elements_2j_and_2j_plus_1_take_the_two_halves_of_one_hash():
    n = 4096
    j = np.arange(n // 2, dtype=np.uint64)
    h = R.dropout_hash(1234, j, 0)
    b = R.element_bits(1234, np.arange(n, dtype=np.uint64))
    assert np.array_equal(b[0::2], h & np.uint32(0xFFFF)) and np.array_equal(b[1::2], h >> np.uint32(16))
    assert np.array_equal((b[1::2].astype(np.uint32) << np.uint32(16)) | b[0::2], h)
    u = R.uniform01(1234, np.arange(n, dtype=np.uint64))
    assert u.dtype == np.float32 and np.array_equal(u.astype(np.float64) * 65536.0, b.astype(np.float64))  # exact: 16 bits times 2^-16
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0


def test_keep_rate_is_one_minus_ceil_65536_p_over_65536():
    """A draw is uniform over the 65536 values m / 65536 and survives where m / 65536 >= p, i.e. m >= ceil(65536 p): the keep rate is
    q = 1 - ceil(65536 p) / 65536.  The count of kept draws among n = 2^20 independent ones is Binomial(n, q) with standard deviation
    sqrt(n q (1 - q)); the test allows 6 of them (two-sided tail below 2e-9 per case, normal approximation valid at n q (1 - q) >= 15
    for every p here but the degenerate ones) plus one count.  p = 0 keeps everything and p = 65535.5 / 65536 only m = 65535."""
    n = 1 << 20
    for seed, p in ((7, 0.1), (8, 0.25), (9, 0.3), (10, 0.5), (11, 0.999), (12, 1.0 / 65536.0), (13, 1.5 / 65536.0)):
        q = R.keep_rate(p)
        assert q == 1.0 - math.ceil(65536.0 * float(np.float32(p))) / 65536.0
        kept = int(R.keep_mask(seed, n, p).sum())
        assert abs(kept - n * q) <= 6.0 * math.sqrt(n * q * (1.0 - q)) + 1.0, (p, kept, n * q)
    assert R.keep_mask(3, n, 0.0).all() and R.keep_rate(0.0) == 1.0
    # the comparison is the mask: keep == (bits >= ceil(65536 p)) element for element
    for p in (0.1, 0.3, 0.999):
        bits = R.element_bits(5, np.arange(n, dtype=np.uint64))
        assert np.array_equal(R.keep_mask(5, n, p), bits >= math.ceil(65536.0 * float(np.float32(p))))


def test_streams_of_neighbouring_seeds_are_neither_equal_nor_shifted_copies():
    """Two unrelated streams of 16-bit draws agree at a position with probability 2^-16: among n = 2^16 positions the number of
    agreements is Poisson(1) (P(>= 16) < 1e-13).  A stream that were the other one shifted by s would agree at n - |s| positions.
    Shifts up to 64 either way, for seeds that differ in the low word and across the 32-bit carry (the high word enters k1 only)."""
    n, reach = 1 << 16, 64
    i = np.arange(n + 2 * reach, dtype=np.uint64)
    for seed in (0, 7, 2**32 - 1, 2**40 + 5):
        a = R.element_bits(seed, i)
        b = R.element_bits(seed + 1, i)
        assert not np.array_equal(a, b)
        for s in range(-reach, reach + 1):
            same = int((a[reach : reach + n] == b[reach + s : reach + s + n]).sum())
            assert same < 16, (seed, s, same)
        # ... and on the pairs' hashes (a permutation inside the pair would hide from the 16-bit view)
        ha, hb = R.dropout_hash(seed, i, 0), R.dropout_hash(seed + 1, i, 0)
        for s in range(-reach, reach + 1):
            assert int((ha[reach : reach + n] == hb[reach + s : reach + s + n]).sum()) < 4, (seed, s)


def test_the_high_word_of_the_pair_index_changes_the_draw():
    """Elements i and i + 2^33 share j_lo and differ in j_hi: their draws agree with probability 2^-16 each (fewer than 16 of 2^16)."""
    n = 1 << 16
    i = np.arange(n, dtype=np.uint64)
    a = R.element_bits(21, i)
    for hi in (1, 2, 3):
        b = R.element_bits(21, i + np.uint64(hi << 33))
        assert int((a == b).sum()) < 16
        assert np.array_equal(b, R.dropout_bits(R.dropout_hash(21, i >> np.uint64(1), hi), i & np.uint64(1)))
    assert int((R.dropout_hash(21, i, 0) == R.dropout_hash(21, i, 1)).sum()) < 4


def test_attention_keep_indexes_query_major_per_head_stream():
    B, H, T, p, seed = 2, 3, 5, 0.3, 99
    m = R.attention_keep(seed, B, H, T, p)
    assert m.shape == (B, H, T, T) and m.dtype == bool
    for b, h, q, k in ((0, 0, 0, 0), (1, 2, 4, 3), (1, 0, 2, 4), (0, 1, 3, 1)):
        assert m[b, h, q, k] == R.keep_at(seed + h, np.array([(b * T + q) * T + k], dtype=np.uint64), p)[0]
