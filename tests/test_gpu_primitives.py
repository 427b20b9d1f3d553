"""The fp32 training primitives (csrc/train_ops.hip, csrc/gemm_f32.hip), one operator at a time, at the boundaries of the paths
their launchers select by shape.  Three kinds of assertion, in this order of preference:

(a) position probes -- a reduction over an input that is zero except for one 1.0 / 2.0 at index j must give the obvious value BIT
    FOR BIT; j runs over the boundaries of the path (workgroup strides, segments, split-K slabs, the last element).  A dropped
    or doubled element is an error of 100 %, no tolerance involved;
(b) random operands (fixed seed) against a float64 reference, with a bound evaluated per output element from the operation:
    u = 2^-24, gamma_n = n u / (1 - n u); a sum or dot product of n fp32 terms in ANY order (and with or without FMA contraction)
    has |error| <= gamma_n * sum |term|; r further fp32 roundings add (r + 1) u times the magnitudes they act on; one device math
    function (expf, logf, tanhf, sinf, cosf, powf) adds MATH_ULP ulp of its result.  Results below the smallest normal fp32 may be
    flushed: every bound carries TINY = 2^-126.  No bound is derived from what a kernel returned;
(c) torch.equal with the fp32 torch expression where the arithmetic is exact (data movement, selection, one correctly rounded
    operation).

The float64 references are plain torch on the CPU; no library call builds an expected value (one exception: the dropout MASK of the
softmax rows is read from the kernel's own output, and used only as a mask).  Every shape comment names the path it takes; the
selection rules are restated here from the launchers, not asked of the library."""

import math

import pytest
import torch
import torch.nn.functional as F

from everyvoice_amd import _lib

pytestmark = pytest.mark.gpu

from helpers import E, MATH_ULP, NAN, TINY, U, assert_within, bits, f32, gamma, same_bits  # noqa: F401  (shared with the other primitive files)


def ops_mod():
    from everyvoice_amd.train import ops

    return ops


# =====================================================================================================================
# row_reduce / lrelu_bwd_rowsum
# =====================================================================================================================
def nseg_of(rows, n):
    """evmi_row_reduce_f32 / evmi_lrelu_bwd_rowsum_f32: a row is split only when there are few long rows."""
    if rows < 512 and n > 16384:
        return min(64, (1024 + rows - 1) // rows, (n + 8191) // 8192)
    return 1


def reduction_positions(n, nseg=1):
    seg = -(-n // nseg)
    js = {0, 255, 256, 767, 768, 1023, 1024, seg - 1, seg, 2 * seg - 1, 2 * seg, (nseg - 1) * seg - 1, (nseg - 1) * seg, n - 2, n - 1}
    return sorted(j for j in js if 0 <= j < n)


# rows 1 / 3: every length (n <= 16384: one pass; 16385: nseg 3; 100003: nseg 13; 64 * 8192 + 1: nseg 64 with rows 1);
# rows 511: nseg 1 up to 16384, then min(64, ceil(1024 / 511) = 3, 3) = 3;  rows 512: never split.
# (A split into exactly two segments does not exist: n > 16384 gives ceil(n / 8192) >= 3 and rows < 512 gives ceil(1024 / rows) >= 3.)
ROW_N = [1, 255, 256, 257, 1023, 1024, 1025, 16384, 16385, 100003, 64 * 8192 + 1]
ROW_CASES = [(r, n) for r in (1, 3) for n in ROW_N] + [(r, n) for r in (511, 512) for n in ROW_N if n <= 16385]


def test_row_reduce_selection_rule_covers_the_segment_counts():
    got = {nseg_of(r, n) for r, n in ROW_CASES}
    assert {1, 3, 13, 64} <= got
    assert nseg_of(512, 16385) == 1 and nseg_of(511, 16385) == 3 and nseg_of(1, 16384) == 1 and nseg_of(1, 64 * 8192 + 1) == 64


@pytest.mark.parametrize("rows,n", ROW_CASES)
def test_row_reduce_position_probes(cuda_device, rows, n):
    """One 2.0 per row at a boundary index: out[r] = scale * f(2) exactly, in every mode, writing (NaN prefill) and accumulating."""
    ops = ops_mod()
    js = reduction_positions(n, nseg_of(rows, n))
    a = torch.zeros(rows, n, device=cuda_device)
    b = torch.full((rows, n), 0.5, device=cuda_device)
    scale = 0.75
    for lo in range(0, len(js), rows) if rows < len(js) else [0]:
        jr = torch.tensor([js[(lo + r) % len(js)] for r in range(rows)], device=cuda_device)
        rr = torch.arange(rows, device=cuda_device)
        a[rr, jr] = 2.0
        for mode, val in ((0, 2.0), (1, 1.0), (2, 4.0)):
            out = torch.full((rows,), NAN, device=cuda_device)
            ops.row_reduce(mode, a, b if mode == 1 else None, out, rows, n, scale=scale, accumulate=False)
            assert same_bits(out.cpu(), torch.full((rows,), val * scale)), (mode, jr.tolist(), out.cpu().tolist())
            acc = torch.full((rows,), 1.5, device=cuda_device)
            ops.row_reduce(mode, a, b if mode == 1 else None, acc, rows, n, scale=scale, accumulate=True)
            assert same_bits(acc.cpu(), torch.full((rows,), 1.5 + val * scale)), (mode, "accumulate", jr.tolist())
        a[rr, jr] = 0.0


@pytest.mark.parametrize("rows,n", ROW_CASES)
def test_row_reduce_random_against_float64(cuda_device, rows, n):
    ops = ops_mod()
    g = torch.Generator().manual_seed(rows * 1000003 + n)
    a, b = torch.randn(rows, n, generator=g), torch.randn(rows, n, generator=g)
    prev = torch.randn(rows, generator=g)
    ad, bd = a.to(cuda_device), b.to(cuda_device)
    scale = f32(-0.3)
    for mode in (0, 1, 2):
        terms = a.double() if mode == 0 else (a.double() * b.double() if mode == 1 else a.double() ** 2)
        want = scale * terms.sum(1)
        # n - 1 additions in any order + one product per term (modes 1, 2) + the multiplication by scale: gamma_{n + 1}
        bound = gamma(n + 1) * abs(scale) * terms.abs().sum(1)
        out = torch.full((rows,), NAN, device=cuda_device)
        ops.row_reduce(mode, ad, bd if mode == 1 else None, out, rows, n, scale=scale)
        assert_within(out, want, bound, f"row_reduce mode {mode}")
        acc = prev.clone().to(cuda_device)
        ops.row_reduce(mode, ad, bd if mode == 1 else None, acc, rows, n, scale=scale, accumulate=True)
        assert_within(acc, prev.double() + want, bound + U * (prev.double() + want).abs(), f"row_reduce mode {mode} accumulate")


@pytest.mark.parametrize("rows,n", ROW_CASES)
def test_lrelu_bwd_rowsum(cuda_device, rows, n):
    """dpre is one correctly rounded product: equal to torch's; its row sums: probes exact, random within gamma_n."""
    ops = ops_mod()
    slope = 0.125
    js = reduction_positions(n, nseg_of(rows, n))
    dy = torch.zeros(rows, 1, n, device=cuda_device)
    y = torch.ones(rows, 1, n, device=cuda_device)
    y[:, :, ::2] = -1.0  # even positions take the slope branch
    for lo in range(0, len(js), rows) if rows < len(js) else [0]:
        jr = torch.tensor([js[(lo + r) % len(js)] for r in range(rows)], device=cuda_device)
        rr = torch.arange(rows, device=cuda_device)
        dy[rr, 0, jr] = 2.0
        want = torch.where(jr.cpu() % 2 == 0, 2.0 * slope, 2.0)
        db = torch.full((rows,), NAN, device=cuda_device)
        dpre = ops.lrelu_bwd_rowsum(dy, y, slope, db, accumulate=False)
        assert same_bits(db.cpu(), want), (jr.tolist(), db.cpu().tolist())
        assert same_bits(dpre.cpu(), (dy * torch.where(y > 0, 1.0, slope)).cpu())
        db = torch.full((rows,), 1.5, device=cuda_device)
        ops.lrelu_bwd_rowsum(dy, y, slope, db, accumulate=True)
        assert same_bits(db.cpu(), 1.5 + want), ("accumulate", jr.tolist())
        dy[rr, 0, jr] = 0.0
    g = torch.Generator().manual_seed(rows * 7919 + n)
    dyr, yr = torch.randn(rows, 1, n, generator=g), torch.randn(rows, 1, n, generator=g)
    yr[0, 0, 0] = 0.0  # y == 0 is the slope side (y > 0 ? 1 : slope)
    prev = torch.randn(rows, generator=g)
    dpre_want = dyr * torch.where(yr > 0, 1.0, slope)  # fp32, one rounding per element: the same bits
    db = torch.full((rows,), NAN, device=cuda_device)
    dpre = ops.lrelu_bwd_rowsum(dyr.to(cuda_device), yr.to(cuda_device), slope, db, accumulate=False)
    assert same_bits(dpre.cpu(), dpre_want)
    terms = dpre_want.double().view(rows, n)
    bound = gamma(n) * terms.abs().sum(1)  # n - 1 additions of the (exactly known) fp32 products
    assert_within(db, terms.sum(1), bound, "lrelu_bwd_rowsum db")
    db = prev.clone().to(cuda_device)
    ops.lrelu_bwd_rowsum(dyr.to(cuda_device), yr.to(cuda_device), slope, db, accumulate=True)
    assert_within(db, prev.double() + terms.sum(1), bound + U * (prev.double() + terms.sum(1)).abs(), "lrelu_bwd_rowsum db accumulate")


# =====================================================================================================================
# scalar_reduce
# =====================================================================================================================
SCALAR_N = [1, 2047, 2048, 2049, 256 * 8 * 1024 - 1, 256 * 8 * 1024, 256 * 8 * 1024 + 1, 3 * 2 ** 21 + 7]


def scalar_grid(n):
    """evmi_scalar_reduce_f32: one workgroup per 2048 elements, at most 1024 of them; the stride of the loop is grid * 256."""
    return max(1, min(1024, (n + 2047) // 2048))


@pytest.mark.parametrize("n", SCALAR_N)
def test_scalar_reduce_position_probes(cuda_device, n):
    """A single element that differs from the background: the sum is that one term, exactly (double accumulation of zeros)."""
    ops = ops_mod()
    step = scalar_grid(n) * 256
    # below 256 * 8 * 1024 elements a thread makes at most 8 trips (two unrolled groups of 4); above, the remainder loop runs too
    js = sorted(j for j in {0, 255, 256, 1023, 1024, 2047, 2048, step - 1, step, 3 * step, 4 * step - 1, 4 * step, 7 * step, 8 * step - 1,
                            8 * step, 8 * step + 255, n - 257, n - 2, n - 1} if 0 <= j < n)
    zeros = torch.zeros(n, device=cuda_device)
    p = 0.5
    scale = 0.75
    for mode, background, val in ((0, 0.0, 2.0), (1, p, 4.0), (2, 0.0, 2.0)):
        a = torch.full((n,), background, device=cuda_device)
        for j in js:
            a[j] = background + 2.0
            out = torch.full((1,), NAN, device=cuda_device)
            ops.scalar_reduce(mode, a, zeros if mode == 0 else None, out, scale=scale, p=p)
            assert same_bits(out.cpu(), torch.tensor([val * scale])), (mode, j, out.item())
            acc = torch.full((1,), 1.5, device=cuda_device)
            ops.scalar_reduce(mode, a, zeros if mode == 0 else None, acc, scale=scale, p=p, accumulate=True)
            assert same_bits(acc.cpu(), torch.tensor([1.5 + val * scale])), (mode, j, "accumulate", acc.item())
            a[j] = background


@pytest.mark.parametrize("n", SCALAR_N)
def test_scalar_reduce_random_against_float64(cuda_device, n):
    ops = ops_mod()
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ad, bd = a.to(cuda_device), b.to(cuda_device)
    p, scale, prev = f32(0.3), f32(1.0 / 7.0), f32(-2.25)
    for mode, r in ((0, 1), (1, 3), (2, 0)):  # r: fp32 roundings inside one term (a - b; a - p twice and their product; none)
        terms = (a.double() - b.double()).abs() if mode == 0 else ((a.double() - p) ** 2 if mode == 1 else a.double())
        want = scale * terms.sum()
        # terms carry (r + 1) u each (their roundings, and one more for the fp32 value of the term itself where it is formed);
        # the accumulation is in double: n 2^-53 of the absolute sum; the result is cast to fp32 once (u |result|)
        bound = abs(scale) * terms.abs().sum() * ((r + 1) * U + n * 2.0 ** -53) + U * want.abs()
        out = torch.full((1,), NAN, device=cuda_device)
        ops.scalar_reduce(mode, ad, bd if mode == 0 else None, out, scale=scale, p=p)
        assert_within(out, want.reshape(1), bound.reshape(1), f"scalar_reduce mode {mode}")
        acc = torch.full((1,), prev, device=cuda_device)
        ops.scalar_reduce(mode, ad, bd if mode == 0 else None, acc, scale=scale, p=p, accumulate=True)
        assert_within(acc, (prev + want).reshape(1), (bound + U * (prev + want).abs()).reshape(1), f"scalar_reduce mode {mode} accumulate")


# =====================================================================================================================
# GEMM
# =====================================================================================================================
CANARY = -1234.5


class Mat:
    """A row-major matrix view inside a larger flat buffer: `off` floats in front of it, `pad` unused floats behind every row,
    everything outside the view filled with CANARY (or NaN inside, for an output that must be overwritten)."""

    def __init__(self, rows, cols, pad, off, device, values=None, fill=None):
        self.rows, self.cols, self.ld, self.off = rows, cols, cols + pad, off
        host = torch.full((off + rows * self.ld + 4,), CANARY)
        self.window = host[off : off + rows * self.ld].view(rows, self.ld)[:, :cols]
        if values is not None:
            self.window.copy_(values)
        elif fill is not None:
            self.window.fill_(fill)
        self.host = host
        self.dev = host.to(device)
        self.view = self.dev[off:]  # data_ptr() is the first element of the matrix

    def result(self):
        """(the window after the call, True if every float outside it is bitwise unchanged)"""
        after = self.dev.cpu()
        win = after[self.off : self.off + self.rows * self.ld].view(self.rows, self.ld)[:, : self.cols].clone()
        before = self.host.clone()
        outside_after = after.clone()
        before[self.off : self.off + self.rows * self.ld].view(self.rows, self.ld)[:, : self.cols] = 0.0
        outside_after[self.off : self.off + self.rows * self.ld].view(self.rows, self.ld)[:, : self.cols] = 0.0
        return win, same_bits(before, outside_after)


def run_gemm(device, ta, tb, M, N, K, alpha=1.0, beta=0.0, pads=(0, 0, 0), offs=(0, 0, 0), seed=0, a=None, b=None, what=""):
    """C = alpha op(A) op(B) + beta C through evmi_gemm_f32 on sub-matrix views, checked against float64 with the bound
        gamma_K |alpha| (|A| |B|)_ij + 3 u (|alpha (A B)_ij| + |beta C_ij|)
    (K products and K - 1 additions in any order, with or without FMA; then alpha *, beta *, + : three roundings), and the floats
    outside the M x N window bitwise unchanged.  beta == 0: C starts as NaN and must come out finite."""
    ops = ops_mod()
    g = torch.Generator().manual_seed(seed)
    alpha, beta = f32(alpha), f32(beta)
    a = torch.randn(M, K, generator=g) if a is None else a      # op(A)
    b = torch.randn(K, N, generator=g) if b is None else b      # op(B)
    c0 = torch.randn(M, N, generator=g)
    A = Mat(K, M, pads[0], offs[0], device, a.t()) if ta else Mat(M, K, pads[0], offs[0], device, a)
    B = Mat(N, K, pads[1], offs[1], device, b.t()) if tb else Mat(K, N, pads[1], offs[1], device, b)
    Cm = Mat(M, N, pads[2], offs[2], device, c0) if beta != 0.0 else Mat(M, N, pads[2], offs[2], device, fill=NAN)
    ops.gemm(A.view, B.view, Cm.view, ta=ta, tb=tb, alpha=alpha, beta=beta, M=M, N=N, K=K, lda=A.ld, ldb=B.ld, ldc=Cm.ld)
    got, untouched = Cm.result()
    ab = a.double() @ b.double()
    want = alpha * ab + (beta * c0.double() if beta != 0.0 else 0.0)
    bound = gamma(K) * abs(alpha) * (a.double().abs() @ b.double().abs()) + 3 * U * ((alpha * ab).abs() + (beta * c0.double()).abs())
    tag = f"gemm {what} ta={ta} tb={tb} M={M} N={N} K={K} alpha={alpha} beta={beta} pads={pads} offs={offs}"
    assert_within(got, want, bound, tag)
    assert untouched, tag + ": wrote outside the M x N window"
    return got


TRANS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("ta,tb", TRANS)
def test_gemm_small_shapes_crossed(cuda_device, ta, tb):
    """The MFMA tile kernel at partial tiles in M, N and K (K chunk 32): aligned views take the 16-byte loads, views with odd
    leading dimensions or an offset base the guarded scalars.  N == 1 with M * K >= 4096, alpha 1, beta 0 and unit ldb / ldc
    (M in {64, 65, 130} at K = 100, tight C) is the gemv path; K == 1 with M * N >= 4096 (not transposed) the rank-one kernel."""
    i = 0
    for M in (1, 31, 64, 65, 130):
        for N in (1, 31, 64, 65, 130):
            for K in (1, 2, 31, 32, 33, 100):
                alpha, beta = [(1.0, 0.0), (0.75, 1.0), (-1.5, -0.5), (1.0, 0.0)][i % 4]
                pads = [(0, 0, 0), (1, 3, 2), (4, 4, 4), (0, 0, 0)][(i // 4) % 4]
                run_gemm(cuda_device, ta, tb, M, N, K, alpha, beta, pads=pads, seed=i, what="cross")
                i += 1


@pytest.mark.parametrize("ta,tb", TRANS)
def test_gemm_unaligned_sub_matrix_views(cuda_device, ta, tb):
    """Base pointers 1, 2, 3 floats off 16-byte alignment (guarded scalar loads for every row) and a leading dimension = 2 mod 4
    from an aligned base (rows alternate between the vector and the scalar load); ldc > N with canaries in the gap."""
    for j, (M, N, K) in enumerate([(64, 64, 64), (65, 130, 100), (130, 31, 33)]):
        for off in (1, 2, 3):
            run_gemm(cuda_device, ta, tb, M, N, K, 1.25, 0.0, pads=(0, 0, 5), offs=(off, 0, 0), seed=10 * j + off, what="A offset")
            run_gemm(cuda_device, ta, tb, M, N, K, 1.0, -0.5, pads=(0, 0, 0), offs=(0, off, off), seed=10 * j + off, what="B, C offset")
        padA = (2 - (M if ta else K)) % 4  # ld = 2 (mod 4)
        padB = (2 - (K if tb else N)) % 4
        run_gemm(cuda_device, ta, tb, M, N, K, 1.0, 1.0, pads=(padA, padB, 3), seed=j, what="alternating rows")


@pytest.mark.parametrize("ta", [False, True])
def test_gemv_paths(cuda_device, ta):
    """N == 1, alpha 1, beta 0, ldb == ldc == 1: gemv_rows (A as stored) / gemv_cols (A transposed) from M * K >= 4096."""
    for M, K, pad in [(64, 64, 0),      # exactly at the threshold: gemv
                      (64, 64, 3),      # ... with lda > K (the threshold counts M * K, not the storage)
                      (63, 65, 0),      # 4095: the MFMA path
                      (1024, 5120, 0), (5120, 1024, 0), (1, 4096, 0), (4096, 1, 0)]:
        run_gemm(cuda_device, ta, False, M, 1, K, pads=(pad, 0, 0), seed=M + K, what="gemv")
    # position probes: row m of op(A) is one-hot at k = j_m, x[k] = k + 1 (exact in fp32): y[m] = j_m + 1, bit for bit
    for M, K in [(64, 64), (40, 5120)]:
        js = sorted({0, 31, 32, 63, 255, 256, 1023, 1024, K - 33, K - 32, K - 2, K - 1} & set(range(K)))
        a = torch.zeros(M, K)
        a[torch.arange(M), torch.tensor([js[m % len(js)] for m in range(M)])] = 1.0
        x = torch.arange(1, K + 1, dtype=torch.float32).view(K, 1)
        if M * K < 4096:
            continue
        got = run_gemm(cuda_device, ta, False, M, 1, K, a=a, b=x, what="gemv probe")
        assert same_bits(got, (a @ x)), "gemv position probe"


def test_rank_one_path(cuda_device):
    """K == 1, nothing transposed, M * N >= 4096: rank1_update; below, and with a transposition, the MFMA kernel."""
    for M, N in [(64, 64), (63, 65), (65, 64), (130, 300), (1, 4096), (4096, 1)]:
        for alpha, beta in [(1.0, 0.0), (-0.75, 0.5), (2.0, 1.0)]:
            run_gemm(cuda_device, False, False, M, N, 1, alpha, beta, pads=(2, 0, 3), seed=M * N, what="rank-1")
    run_gemm(cuda_device, True, False, 64, 64, 1, 1.5, 0.5, what="rank-1 shape, transposed A: MFMA")


def splitk_plan(K):
    """gemm_rm: K >= 8192 (and M * N <= 2^21): S = min(K / 4096, 128) equal slabs of kc = K / S, then a tail slab."""
    S = min(K // 4096, 128)
    kc = K // S
    return S, kc, K - S * kc


SPLITK = [8191,              # below the threshold: one plain GEMM
          8192,              # S 2, kc 4096, no tail
          8193,              # S 2, kc 4096, tail 1
          12289,             # S 3, kc 4096, tail 1
          4096 * 128,        # S 128, kc 4096, no tail
          4096 * 129 + 5]    # S 128 (capped), kc 4128, tail 5


def test_splitk_plan_restated():
    assert [splitk_plan(K) for K in SPLITK[1:]] == [(2, 4096, 0), (2, 4096, 1), (3, 4096, 1), (128, 4096, 0), (128, 4128, 5)]


@pytest.mark.parametrize("K", SPLITK)
@pytest.mark.parametrize("ta,tb", TRANS)
def test_gemm_split_k(cuda_device, ta, tb, K):
    M, N = 20, 33
    run_gemm(cuda_device, ta, tb, M, N, K, 0.5, -0.5, pads=(0, 0, 3), seed=K, what="split-K")
    run_gemm(cuda_device, ta, tb, M, N, K, 1.0, 0.0, pads=(1, 2, 0), seed=K + 1, what="split-K, beta 0 over NaN")
    # position probes along K: row m of op(A) one-hot at j_m, op(B)[k][n] = k + 1 (exact: K < 2^24): C[m][n] = j_m + 1
    S, kc, tail = splitk_plan(K) if K >= 8192 else (1, K, 0)
    js = sorted({0, 31, 32, 33, kc - 1, kc, 2 * kc - 1, S * kc - 1, S * kc, K - 2, K - 1} & set(range(K)))
    Mp, Np = len(js), 3
    a = torch.zeros(Mp, K)
    a[torch.arange(Mp), torch.tensor(js)] = 1.0
    b = torch.arange(1, K + 1, dtype=torch.float32).view(K, 1).repeat(1, Np)
    got = run_gemm(cuda_device, ta, tb, Mp, Np, K, a=a, b=b, what="split-K probe")
    assert same_bits(got, torch.tensor(js, dtype=torch.float32).view(Mp, 1).repeat(1, Np) + 1.0), "split-K position probe"


def test_gemm_long_k_with_a_large_output_takes_the_plain_path(cuda_device):
    """M * N = 2048 * 1025 > 2^21 with K = 8192: no split (the partial tiles would not fit the rule), one MFMA GEMM."""
    assert 2048 * 1025 > 2 ** 21
    run_gemm(cuda_device, False, True, 2048, 1025, 8192, 1.0, 0.0, seed=5, what="long K, large output")


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("K", [100, 8200])  # 8200: the per-problem split-K loop (S 2, kc 4100, no tail)
def test_gemm_batched(cuda_device, ta, tb, K):
    ops = ops_mod()
    M, N = 20, 33
    for batch in (1, 3, 16):
        g = torch.Generator().manual_seed(batch * 31 + K)
        a, b, c0 = torch.randn(batch, M, K, generator=g), torch.randn(batch, K, N, generator=g), torch.randn(batch, M, N, generator=g)
        sa, sb, sc = M * K + 1, K * N + 3, M * N + 2  # element strides that are not multiples of 4
        for alpha, beta in ((1.0, 0.0), (0.75, -0.5)):
            alpha, beta = f32(alpha), f32(beta)
            A = torch.full((batch, sa), CANARY)
            B = torch.full((batch, sb), CANARY)
            Cb = torch.full((batch, sc), CANARY)
            A[:, : M * K] = (a.transpose(1, 2) if ta else a).reshape(batch, -1)
            B[:, : K * N] = (b.transpose(1, 2) if tb else b).reshape(batch, -1)
            Cb[:, : M * N] = c0.reshape(batch, -1) if beta != 0.0 else NAN
            Ad, Bd, Cd = A.to(cuda_device), B.to(cuda_device), Cb.to(cuda_device)
            ops.gemm_groups(Ad, Bd, Cd, batch, M, N, K, M if ta else K, K if tb else N, N, sa, sb, sc, ta=ta, tb=tb, alpha=alpha, beta=beta)
            got = Cd.cpu()
            ab = a.double() @ b.double()
            want = alpha * ab + (beta * c0.double() if beta != 0.0 else 0.0)
            bound = gamma(K) * abs(alpha) * (a.double().abs() @ b.double().abs()) + 3 * U * ((alpha * ab).abs() + (beta * c0.double()).abs())
            assert_within(got[:, : M * N].reshape(batch, M, N), want, bound, f"gemm_groups batch={batch} K={K} ta={ta} tb={tb} beta={beta}")
            assert same_bits(got[:, M * N :], Cb[:, M * N :]), "gemm_groups wrote between the problems"


# =====================================================================================================================
# unfold / fold
# =====================================================================================================================
CONV_GEOMETRIES = [(41, 4, 20, 1), (5, 3, 2, 1), (15, 1, 7, 1), (11, 1, 25, 5), (3, 1, 1, 1), (16, 2, 3, 2)]  # (k, stride, pad, dil)
SWITCH_LENGTHS = [511, 512, 513, 1025]  # the per-row kernels start at 512 positions; 1025: a second tile of 1024 with one element


def conv_index(t_in, t_out, k, stride, pad, dil):
    ti = torch.arange(t_out)[None, :] * stride + torch.arange(k)[:, None] * dil - pad  # [k, t_out]
    return ti, (ti >= 0) & (ti < t_in)


def unfold_ref(x, t_out, k, stride, pad, dil):
    """col[(c k + j)][b][to] = x[c][b][to stride + j dil - pad] (0 outside), any dtype."""
    Cc, B, t_in = x.shape
    ti, ok = conv_index(t_in, t_out, k, stride, pad, dil)
    col = torch.where(ok, x[:, :, ti.clamp(0, t_in - 1)], torch.zeros((), dtype=x.dtype))  # [C, B, k, t_out]
    return col.permute(0, 2, 1, 3).reshape(Cc * k, B * t_out)


def fold_ref(dcol, Cc, B, t_in, t_out, k, stride, pad, dil):
    """The adjoint, written as a scatter-add."""
    ti, ok = conv_index(t_in, t_out, k, stride, pad, dil)
    d = dcol.reshape(Cc, k, B, t_out)
    dx = torch.zeros(Cc, B, t_in, dtype=dcol.dtype)
    for j in range(k):
        dx.index_add_(2, ti[j][ok[j]], d[:, j][:, :, ok[j]])
    return dx


@pytest.mark.parametrize("k,stride,pad,dil", CONV_GEOMETRIES)
@pytest.mark.parametrize("B", [1, 3])
def test_unfold_is_exact_at_the_kernel_switch(cuda_device, k, stride, pad, dil, B):
    ops = ops_mod()
    Cc = 2
    for t_out in SWITCH_LENGTHS:  # < 512: the flat kernel, >= 512: one workgroup row per (c, j, b)
        t_in = (t_out - 1) * stride + dil * (k - 1) + 1 - 2 * pad
        assert t_in >= 1 and ops.conv_out_len(t_in, k, stride, pad, dil) == t_out
        g = torch.Generator().manual_seed(t_out + k)
        x = torch.randn(Cc, B, t_in, generator=g)
        col, t_got = ops.unfold(x.to(cuda_device), k, stride, pad, dil, key="prim")
        assert t_got == t_out
        assert same_bits(col.cpu(), unfold_ref(x, t_out, k, stride, pad, dil)), (t_out, "unfold")


@pytest.mark.parametrize("k,stride,pad,dil", CONV_GEOMETRIES)
@pytest.mark.parametrize("B", [1, 3])
def test_fold_is_exact_on_integers_and_adjoint_to_unfold(cuda_device, k, stride, pad, dil, B):
    """Integer-valued dcol (a one-hot, and a superposition of many): every partial sum is an integer far below 2^24, so the fold is
    exact in any order.  Random floats: <unfold x, y> == <x, fold y> within gamma_k (a dx element sums at most k terms)."""
    ops = ops_mod()
    Cc = 2
    for t_in in SWITCH_LENGTHS:  # < 512: the flat kernel, >= 512: one workgroup row per (c, b)
        t_out = ops.conv_out_len(t_in, k, stride, pad, dil)
        g = torch.Generator().manual_seed(t_in * 3 + k)
        ints = torch.randint(-3, 4, (Cc * k, B * t_out), generator=g).float()
        onehot = torch.zeros(Cc * k, B * t_out)
        onehot[(Cc * k) // 2, (B * t_out) // 2] = 1.0
        onehot[Cc * k - 1, B * t_out - 1] = 1.0
        onehot[0, 0] = 1.0
        prev = torch.randint(-5, 6, (Cc, B, t_in), generator=g).float()
        for dcol in (onehot, ints):
            want = fold_ref(dcol, Cc, B, t_in, t_out, k, stride, pad, dil)
            out = torch.full((Cc, B, t_in), NAN, device=cuda_device)
            ops.fold(dcol.to(cuda_device), Cc, B, t_in, t_out, k, stride, pad, dil, out=out, accumulate=False)
            assert same_bits(out.cpu() + 0.0, want + 0.0), (t_in, "fold")  # (+ 0.0: an empty sum may be -0 or +0)
            acc = prev.clone().to(cuda_device)
            ops.fold(dcol.to(cuda_device), Cc, B, t_in, t_out, k, stride, pad, dil, out=acc, accumulate=True)
            assert same_bits(acc.cpu() + 0.0, prev + want + 0.0), (t_in, "fold accumulate")
        x, y = torch.randn(Cc, B, t_in, generator=g), torch.randn(Cc * k, B * t_out, generator=g)
        col, _ = ops.unfold(x.to(cuda_device), k, stride, pad, dil, key="prim")
        lhs = (col.cpu().double() * y.double()).sum()
        fy = ops.fold(y.to(cuda_device), Cc, B, t_in, t_out, k, stride, pad, dil)
        rhs = (x.double() * fy.cpu().double()).sum()
        # unfold moves data (exact); every fold element carries gamma_k of its absolute sum; the two dots are taken in double
        bound = (x.double().abs() * gamma(k) * fold_ref(y.double().abs(), Cc, B, t_in, t_out, k, stride, pad, dil)).sum()
        bound = bound + 2.0 ** -50 * (x.double().abs() * fold_ref(y.double().abs(), Cc, B, t_in, t_out, k, stride, pad, dil)).sum()
        assert abs(lhs - rhs) <= bound + TINY, (t_in, float(lhs), float(rhs), float(bound))
        assert_within(fy, fold_ref(y.double(), Cc, B, t_in, t_out, k, stride, pad, dil),
                      gamma(k) * fold_ref(y.double().abs(), Cc, B, t_in, t_out, k, stride, pad, dil), "fold")


# =====================================================================================================================
# data movement: dgrad_weights, bias_add_rows, transpose_bct_cbt
# =====================================================================================================================
def test_dgrad_weights_bias_add_transpose_are_exact(cuda_device):
    lib = _lib.load()
    st = _lib.current_stream_ptr(cuda_device)
    g = torch.Generator().manual_seed(11)
    # wt[g cin_g + ci][co][m] = w[g cout_g + co][ci][phi + stride (M - 1 - m)],  M = ceil((k - phi) / stride)
    for cin, cout, k, groups, stride in [(4, 6, 5, 1, 1), (8, 12, 41, 4, 4), (3, 5, 7, 1, 3), (16, 16, 3, 16, 2), (6, 4, 2, 2, 3)]:
        w = torch.randn(cout, cin // groups, k, generator=g)
        wd = w.to(cuda_device)
        for phi in range(min(stride, k)):
            Mm = (k - phi + stride - 1) // stride
            cin_g, cout_g = cin // groups, cout // groups
            want = torch.empty(cin, cout_g, Mm)
            for gi in range(groups):
                for ci in range(cin_g):
                    for m in range(Mm):
                        want[gi * cin_g + ci, :, m] = w[gi * cout_g : (gi + 1) * cout_g, ci, phi + stride * (Mm - 1 - m)]
            wt = torch.full((cin * cout_g * Mm + 4,), CANARY, device=cuda_device)
            _lib.check(lib.evmi_dgrad_weights_f32(wd.data_ptr(), wt.data_ptr(), cin, cout, k, groups, stride, phi, st))
            assert same_bits(wt.cpu()[:-4].view(cin, cout_g, Mm), want) and same_bits(wt.cpu()[-4:], torch.full((4,), CANARY))
        assert lib.evmi_dgrad_weights_f32(wd.data_ptr(), wt.data_ptr(), cin, cout, k, groups, stride, stride, st) == 1  # phase >= stride
    for rows, n in [(1, 1), (3, 255), (7, 257), (64, 1025), (2, 100003)]:
        y, bias = torch.randn(rows, n, generator=g), torch.randn(rows, generator=g)
        yd = torch.cat([y.reshape(-1), torch.full((4,), CANARY)]).to(cuda_device)
        bias_d = bias.to(cuda_device)
        _lib.check(lib.evmi_bias_add_rows_f32(yd.data_ptr(), bias_d.data_ptr(), rows, n, st))
        assert same_bits(yd.cpu()[:-4].view(rows, n), y + bias[:, None]) and same_bits(yd.cpu()[-4:], torch.full((4,), CANARY))
    for B, Cc, T in [(1, 1, 1), (3, 5, 7), (2, 80, 257), (4, 3, 1025)]:
        x = torch.randn(B, Cc, T, generator=g)
        out = torch.full((B * Cc * T + 4,), CANARY, device=cuda_device)
        xd = x.to(cuda_device)
        _lib.check(lib.evmi_transpose_bct_cbt_f32(xd.data_ptr(), out.data_ptr(), B, Cc, T, st))
        assert same_bits(out.cpu()[:-4].view(Cc, B, T), x.permute(1, 0, 2).contiguous()) and same_bits(out.cpu()[-4:], torch.full((4,), CANARY))


# =====================================================================================================================
# elementwise
# =====================================================================================================================
EW_N = [1, 255, 256, 257, 100003]
EXTREMES = [30.0, -30.0, 88.0, -88.0, 0.0, -0.0]


def _with_head(t, head):
    h = torch.tensor(head, dtype=torch.float32)[: t.numel()]
    t = t.clone()
    t[: h.numel()] = h
    return t


def _sig(z):
    return 1.0 / (1.0 + torch.exp(-z))


def ew_cases(op, n, g):
    """[(a, b, c, p0, p1, want, bound)] for one op code; want float64 with a bound, or an fp32 tensor with bound None (exact).
    r below counts the fp32 roundings of the formula in the table above ew_kernel; E is one math-function call."""
    rn = lambda: torch.randn(n, generator=g)  # noqa: E731
    pos = lambda: torch.rand(n, generator=g) * 3.9 + 0.1  # noqa: E731  [0.1, 4): the operand a formula divides by
    wide = lambda: _with_head(rn() * 3, EXTREMES)  # noqa: E731
    z32 = torch.zeros((), dtype=torch.float32)
    if op == 0:
        a, p0 = wide(), 0.125
        return [(a, None, None, p0, 0.0, torch.where(a > 0, a, a * p0), None)]
    if op == 1:
        a, b, p0 = rn(), wide(), 0.125
        return [(a, b, None, p0, 0.0, a * torch.where(b > 0, 1.0, p0), None)]
    if op == 2:
        a = wide()
        w = torch.tanh(a.double())
        return [(a, None, None, 0.0, 0.0, w, E * w.abs())]
    if op == 3:  # a (1 - t t): r = 3
        a, t = rn(), torch.tanh(wide())
        return [(a, t, None, 0.0, 0.0, a.double() * (1 - t.double() ** 2), 4 * U * a.double().abs() * (1 + t.double() ** 2))]
    if op == 4:  # p0 a + p1 b: r = 3
        a, b, p0, p1 = rn(), rn(), f32(0.3), f32(-1.7)
        return [(a, b, None, p0, p1, p0 * a.double() + p1 * b.double(), 4 * U * ((p0 * a.double()).abs() + (p1 * b.double()).abs()))]
    if op == 5:  # one product; p0 = 1 is the library's copy: exact
        a, p0 = wide(), f32(-0.3)
        return [(a, None, None, p0, 0.0, p0 * a.double(), 2 * U * (p0 * a.double()).abs()), (a, None, None, 1.0, 0.0, a.clone(), None)]
    if op == 6:
        a, b = rn(), rn()
        return [(a, b, None, 0.0, 0.0, a * b, None)]  # one correctly rounded product
    if op == 7:  # sign(a - b) p0: selection
        a, b, p0 = rn(), rn(), 0.75
        b[: n // 2] = a[: n // 2]
        a, b = _with_head(a, [0.0, -0.0, 1.0]), _with_head(b, [-0.0, 0.0, 1.0])
        d = a - b
        return [(a, b, None, p0, 0.0, torch.where(d > 0, p0, torch.where(d < 0, -p0, 0.0)) + z32, None)]
    if op == 8:  # 2 (a - p1) p0: r = 3, each relative to the running value
        a, p0, p1 = rn(), f32(0.37), f32(1.0)
        w = 2 * (a.double() - p1) * p0
        return [(a, None, None, p0, p1, w, 4 * U * w.abs())]
    if op == 9:  # log(max(a, p0)): about a quarter of the inputs sit below the clamp, one on it
        a, p0 = _with_head(torch.rand(n, generator=g) * 2, [0.5, 0.25, 1.0]), 0.5
        w = torch.log(a.double().clamp_min(p0))
        return [(a, None, None, p0, 0.0, w, E * w.abs())]
    if op == 10:  # b > p0 ? a / b : 0, b == p0 on the zero side
        a, b, p0 = rn(), _with_head(torch.rand(n, generator=g), [0.25, 0.0, 1.0]), 0.25
        return [(a, b, None, p0, 0.0, torch.where(b > p0, a / b, z32), None)]  # one correctly rounded quotient
    if op == 11:  # sqrt(a a + b b + p0): r = 5
        a, b, p0 = rn(), rn(), f32(1e-7)
        w = torch.sqrt(a.double() ** 2 + b.double() ** 2 + p0)
        return [(a, b, None, p0, 0.0, w, 6 * U * w)]
    if op == 12:  # a b / c: r = 2
        a, b, c = rn(), rn(), pos()
        w = a.double() * b.double() / c.double()
        return [(a, b, c, 0.0, 0.0, w, 3 * U * w.abs())]
    if op in (13, 15):  # v / (1 + exp(-z)): exp (E), 1 + (u), / (u) on the denominator side, the quotient's own rounding
        z = wide()
        a = z if op == 13 else rn()
        w = a.double() * _sig(z.double())
        return [(a, None if op == 13 else z, None, 0.0, 0.0, w, (E + 3 * U) * w.abs())]
    if op == 14:
        a = wide()
        return [(a, None, None, 0.0, 0.0, torch.clamp_min(a, 0.0) + z32, None)]
    if op == 16:
        a = pos()
        w = torch.log(a.double())
        return [(a, None, None, 0.0, 0.0, w, E * w.abs())]
    if op == 17:  # p0 (a - b) + p1 sign(a - b) / a: r = 4
        a, b, p0, p1 = pos(), pos(), f32(0.6), f32(0.02)
        b[: n // 3] = a[: n // 3]
        ad, bd = a.double(), b.double()
        return [(a, b, None, p0, p1, p0 * (ad - bd) + p1 * torch.sign(ad - bd) / ad, 5 * U * ((p0 * (ad - bd)).abs() + abs(p1) / ad))]
    if op == 18:  # a sg (1 + z (1 - sg)), sg = 1 / (1 + exp(-z)): es = E + 2 u on sg, then 1 - sg, z *, 1 +, and two products
        a, z = rn(), wide()
        ad, zd = a.double(), z.double()
        sg = _sig(zd)
        es = E + 2 * U
        t_abs = 1 + zd.abs() * (1 - sg)
        bound = ad.abs() * sg * (zd.abs() * (es * sg + 2 * U * (1 - sg)) + (es + 3 * U) * t_abs)
        bound = bound + TINY * ad.abs() * t_abs  # (sg itself is below the smallest normal at z = -88 and may be flushed)
        return [(a, z, None, 0.0, 0.0, ad * sg * (1 + zd * (1 - sg)), bound)]
    if op == 19:
        a, b = rn(), wide()
        return [(a, b, None, 0.0, 0.0, torch.where(b > 0, a, z32), None)]
    if op == 20:  # a min(1, p0 / (sqrt(c0) + 1e-6)): r = 4; a clipped norm (2 > p0 = 1) and an unclipped one (2 < p0 = 3: exactly a)
        a, c = rn(), torch.tensor([4.0])
        w = a.double() * (1.0 / (2.0 + f32(1e-6)))
        return [(a, None, c, 1.0, 0.0, w, 5 * U * w.abs()), (a, None, c, 3.0, 0.0, a.clone(), None)]
    if op == 21:
        a, c = rn(), torch.tensor([3.0])
        return [(a, None, c, 0.0, 0.0, a / 3.0, None)]  # one correctly rounded quotient
    if op == 22:  # op 17 with k0 = p0 / (sqrt(c0) sqrt(c1)) (r = 4 more); c0 == 0: k0 = 0, not NaN
        a, b, p0, p1 = pos(), pos(), f32(0.6), f32(0.02)
        b[: n // 3] = a[: n // 3]
        ad, bd = a.double(), b.double()
        out = []
        for c in (torch.tensor([2.0, 5.0]), torch.tensor([0.0, 5.0])):
            k0 = p0 / math.sqrt(float(c[0]) * float(c[1])) if float(c[0]) > 0 else 0.0
            out.append((a, b, c, p0, p1, k0 * (ad - bd) + p1 * torch.sign(ad - bd) / ad, 9 * U * ((k0 * (ad - bd)).abs() + abs(p1) / ad)))
        return out
    if op == 23:
        return [(rn(), None, None, f32(-2.5), 0.0, torch.full((n,), f32(-2.5)), None)]
    if op == 24:  # p0 a / c0: r = 2
        a, c, p0 = rn(), torch.tensor([3.0]), f32(0.3)
        w = p0 * a.double() / 3.0
        return [(a, None, c, p0, 0.0, w, 3 * U * w.abs())]
    raise AssertionError(op)


@pytest.mark.parametrize("op", range(25))
def test_elementwise_every_op_code(cuda_device, op):
    ops = ops_mod()
    for n in EW_N:
        g = torch.Generator().manual_seed(op * 1009 + n)
        for a, b, c, p0, p1, want, bound in ew_cases(op, n, g):
            dv = lambda t: None if t is None else t.to(cuda_device)  # noqa: E731
            ad = torch.cat([a, torch.full((4,), CANARY)]).to(cuda_device)[:n]
            out = torch.full((n + 4,), NAN, device=cuda_device)
            out[n:] = CANARY
            got = ops.elementwise(op, ad, dv(b), dv(c), out=out[:n], p0=p0, p1=p1)
            what = f"elementwise op {op} n {n} p0 {p0}"
            if bound is None:
                assert same_bits(got.cpu() + 0.0, want + 0.0), what  # (+ 0.0: the sign of a zero is not part of the contract)
            else:
                assert_within(got, want, bound, what)
            assert same_bits(out[n:].cpu(), torch.full((4,), CANARY)), what + ": wrote behind y"
            # the in-place form (out is a): what fill_ and copy rely on -- the same bits as out of place
            inplace = ops.elementwise(op, ad, dv(b), dv(c), out=ad, p0=p0, p1=p1)
            assert same_bits(inplace.cpu(), got.cpu()), what + " in place"


# =====================================================================================================================
# optimiser
# =====================================================================================================================
OPT_N = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027, 4 * 256 * 3 + 2]  # float4 body of n / 4 threads + a scalar tail of n % 4


class OptimizerBound:
    """Float64 replay of torch.optim.{AdamW, Adam, RMSprop} (the reference) that carries, next to the reference state, bounds on the
    fp32 kernel's error in m, v and p.  Per step, with G = |g| + wd |p| >= |g + wd p| (kinds 1, 2; G = |g| for AdamW):
      m: beta1 *, (1 - beta1) *, 1 -, + and the fma forming g + wd p           e_m <= beta1 e_m + 6 u (beta1 |m| + (1 - beta1) G)
      v: the same with g^2 (its relative error 2 e_g / |g| + u)                e_v <= beta2 e_v + 8 u (beta2 v + (1 - beta2) G^2)
      bias corrections 1 - powf(beta, step): powf within MATH_ULP ulp, amplified by beta^t / (1 - beta^t) through the subtraction
      p: the update c m / den, c = lr / bc1, den = sqrt(v) / sqrt(bc2) + eps; the moment errors propagate through it, every other
         operation (sqrt, *, +, /, /, *, -, the decay factor: <= 10 roundings) is relative to the update or to p."""

    def __init__(self, kind, p0, beta1, beta2, eps, wd, clip):
        self.kind, self.b1, self.b2, self.eps, self.wd, self.clip = kind, beta1, beta2, eps, wd, clip
        self.p = torch.nn.Parameter(p0.double().clone())
        kw = dict(lr=1.0, eps=eps, weight_decay=wd)
        self.opt = (torch.optim.AdamW([self.p], betas=(beta1, beta2), **kw) if kind == 0 else
                    torch.optim.Adam([self.p], betas=(beta1, beta2), **kw) if kind == 1 else
                    torch.optim.RMSprop([self.p], alpha=beta1, **kw))
        z = torch.zeros_like(p0, dtype=torch.float64)
        self.e_m, self.e_v, self.e_p, self.m_abs, self.v_abs, self.t = z.clone(), z.clone(), z.clone(), z.clone(), z.clone(), 0

    def step(self, g, lr):
        self.t += 1
        t, b1, b2 = self.t, self.b1, self.b2
        p_before = self.p.detach().clone()
        G = g.double().abs() + (self.wd * p_before.abs() if self.kind != 0 else 0.0)
        e_g = 2 * U * G + self.wd * self.e_p if self.kind != 0 else torch.zeros_like(G)
        for grp in self.opt.param_groups:
            grp["lr"] = lr
        self.p.grad = g.double().clone()
        self.opt.step()
        st = self.opt.state[self.p]
        if self.kind == 2:
            v = st["square_avg"]
            self.v_abs = b1 * self.v_abs + (1 - b1) * G * G
            self.e_v = b1 * self.e_v + 8 * U * self.v_abs + (1 - b1) * 2 * G * e_g
            gv = g.double() + self.wd * p_before
            den = v.sqrt() + self.eps
            upd = lr * gv.abs() / den
            rel_den = (self.e_v / (2 * v.sqrt()) + U * v.sqrt() + U * den) / den
            e_step = lr * e_g / den + upd * (rel_den + 3 * U) + U * self.p.detach().abs()
        else:
            m, v = st["exp_avg"], st["exp_avg_sq"]
            self.m_abs = b1 * self.m_abs + (1 - b1) * G
            self.v_abs = b2 * self.v_abs + (1 - b2) * G * G
            self.e_m = b1 * self.e_m + 6 * U * self.m_abs + (1 - b1) * e_g
            self.e_v = b2 * self.e_v + 8 * U * self.v_abs + (1 - b2) * 2 * G * e_g
            bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
            amp1, amp2 = b1 ** t / bc1, b2 ** t / bc2
            c = lr / bc1
            root = v.sqrt() / math.sqrt(bc2)
            den = root + self.eps
            upd = c * m.abs() / den
            rel_root = self.e_v / (2 * v) + 3 * U + 0.5 * (E * amp2 + U)
            rel_den = (root * rel_root + U * den) / den
            rel_c = E * amp1 + 2 * U
            e_step = c * self.e_m / den + upd * (rel_den + rel_c + 3 * U) + 3 * U * p_before.abs() + U * self.p.detach().abs()
        self.e_p = self.e_p * (1 + lr * self.wd) + e_step
        if self.clip > 0:
            with torch.no_grad():
                self.p.clamp_(-self.clip, self.clip)  # (the clamp is a contraction: it does not grow e_p)
        return self

    def moments(self):
        st = self.opt.state[self.p]
        return (None, st["square_avg"]) if self.kind == 2 else (st["exp_avg"], st["exp_avg_sq"])


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n", OPT_N)
def test_optimizer_step_kernel_against_torch_optim(cuda_device, kind, n):
    """Three steps from zero moments, in three configurations: (A) step from the host argument, weight decay; (B) step from the
    device counter, no decay, clip; (C) evmi_optimizer_step_lrdev_f32: rate and step from the device, a new rate every step."""
    lib = _lib.load()
    st = _lib.current_stream_ptr(cuda_device)
    b1, b2, eps = (f32(0.99), 0.0, f32(1e-8)) if kind == 2 else (f32(0.8), f32(0.99), f32(1e-8))
    lrs = [f32(2e-3), f32(1e-3), f32(3e-3)]
    for cfg, wd, clip in (("host", f32(0.01), 0.0), ("step_dev", 0.0, f32(0.05)), ("lrdev", f32(0.01), 0.0)):
        g = torch.Generator().manual_seed(kind * 100 + n)
        p0 = torch.randn(n, generator=g) * 0.1
        tail = torch.full((4,), CANARY)
        pd = torch.cat([p0, tail]).to(cuda_device)
        md = torch.cat([torch.zeros(n) if kind != 2 else torch.full((n,), CANARY), tail]).to(cuda_device)
        vd = torch.cat([torch.zeros(n), tail]).to(cuda_device)
        ref = OptimizerBound(kind, p0, b1, b2, eps, wd, clip)
        step_dev = torch.zeros(1, dtype=torch.int32, device=cuda_device)
        lr_dev = torch.zeros(1, device=cuda_device)
        for s in range(3):
            grad = torch.randn(n, generator=g)
            gd = torch.cat([grad, tail]).to(cuda_device)
            lr = lrs[s] if cfg == "lrdev" else lrs[0]
            step_dev.fill_(s + 1)
            if cfg == "lrdev":
                lr_dev.fill_(lr)
                _lib.check(lib.evmi_optimizer_step_lrdev_f32(kind, pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, lr_dev.data_ptr(),
                                                             b1, b2, eps, wd, step_dev.data_ptr(), clip, st))
            else:  # (with step_dev given the host argument is ignored: hand over a wrong one)
                _lib.check(lib.evmi_optimizer_step_f32(kind, pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, lr, b1, b2, eps, wd,
                                                       s + 1 if cfg == "host" else 77, None if cfg == "host" else step_dev.data_ptr(), clip, st))
            ref.step(grad, lr)
            what = f"optimizer kind {kind} n {n} {cfg} step {s + 1}"
            pg, mg, vg = pd.cpu(), md.cpu(), vd.cpu()
            assert_within(pg[:n], ref.p.detach(), ref.e_p, what + " p")
            m_ref, v_ref = ref.moments()
            assert_within(vg[:n], v_ref, ref.e_v, what + " v")
            if kind == 2:
                assert same_bits(mg, torch.full((n + 4,), CANARY)), what + ": RMSprop touched m"
            else:
                assert_within(mg[:n], m_ref, ref.e_m, what + " m")
            for name, t in (("p", pg), ("m", mg), ("v", vg), ("g", gd.cpu())):
                assert same_bits(t[n:], tail), what + f": wrote behind {name}"
            if clip > 0:
                assert float(pg[:n].abs().max()) <= clip, what + ": outside the clip range"
        if clip > 0:  # (the clip must have been active for the case to mean anything)
            assert n < 16 or bool((pg[:n].abs() == clip).any())


@pytest.mark.parametrize("n", OPT_N)
def test_adamw_kernel_against_torch_optim(cuda_device, n):
    ops = ops_mod()
    g = torch.Generator().manual_seed(n)
    b1, b2, eps, wd, lr = f32(0.8), f32(0.99), f32(1e-8), f32(0.01), f32(2e-3)
    p0 = torch.randn(n, generator=g) * 0.1
    tail = torch.full((4,), CANARY)
    pd, md, vd = (torch.cat([t, tail]).to(cuda_device) for t in (p0, torch.zeros(n), torch.zeros(n)))
    ref = OptimizerBound(0, p0, b1, b2, eps, wd, 0.0)
    for s in range(3):
        grad = torch.randn(n, generator=g)
        ops.adamw_step(pd[:n], grad.to(cuda_device), md[:n], vd[:n], lr, (b1, b2), eps, wd, s + 1)
        ref.step(grad, lr)
        assert_within(pd.cpu()[:n], ref.p.detach(), ref.e_p, f"adamw n {n} step {s + 1} p")
        assert_within(md.cpu()[:n], ref.moments()[0], ref.e_m, f"adamw n {n} m")
        assert_within(vd.cpu()[:n], ref.moments()[1], ref.e_v, f"adamw n {n} v")
        for t in (pd, md, vd):
            assert same_bits(t.cpu()[n:], tail)


def test_optimizer_bias_correction_at_a_large_device_step(cuda_device):
    """powf(beta, step) for a step counter far into training (10^6): beta^t underflows to 0, both corrections are exactly 1."""
    lib = _lib.load()
    st = _lib.current_stream_ptr(cuda_device)
    n, b1, b2, eps, lr = 1027, f32(0.8), f32(0.99), f32(1e-8), f32(1e-3)
    g = torch.Generator().manual_seed(4)
    p0, m0, v0, grad = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01, torch.randn(n, generator=g)
    pd, md, vd = p0.clone().to(cuda_device), m0.clone().to(cuda_device), v0.clone().to(cuda_device)
    step_dev = torch.full((1,), 1_000_000, dtype=torch.int32, device=cuda_device)
    gd = grad.to(cuda_device)
    _lib.check(lib.evmi_optimizer_step_f32(0, pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, lr, b1, b2, eps, 0.0,
                                           0, step_dev.data_ptr(), 0.0, st))
    m = b1 * m0.double() + (1 - b1) * grad.double()
    v = b2 * v0.double() + (1 - b2) * grad.double() ** 2
    upd = lr * m / (v.sqrt() + eps)
    # m: 4 roundings of beta1 |m0| + (1 - beta1) |g|; v: 5; the update: sqrt, +, /, * and the moments' relative errors; p: one subtraction
    e_m = 4 * U * (b1 * m0.double().abs() + (1 - b1) * grad.double().abs())
    e_v = 5 * U * v
    e_p = lr * e_m / (v.sqrt() + eps) + upd.abs() * (e_v / (2 * v) + 5 * U) + U * (p0.double() - upd).abs()
    assert_within(pd, p0.double() - upd, e_p, "optimizer at step 10^6")


# =====================================================================================================================
# weight norm
# =====================================================================================================================
def wn_fwd_ref(gv, v):
    """w = g v / ||v|| per row in float64, with bounds: ||v|| = sqrt of n products and n - 1 additions (gamma_{n+1} before the
    root, which halves it, + u for the root): (gamma_{n+1} + u) ||v||; w = v * (g / ||v||): the norm's error, a quotient, a product."""
    v64 = v.double().reshape(v.shape[0], -1)
    n = v64.shape[1]
    nrm = v64.norm(dim=1)
    w = gv.double().reshape(-1, 1) * v64 / nrm[:, None]
    return w, nrm, (gamma(n + 1) + 3 * U) * w.abs(), (gamma(n + 1) + U) * nrm


def wn_bwd_ref(gv, v, nrm32, dw):
    """dg = <dw, v> / ||v||, dv = g / ||v|| (dw - v <dw, v> / ||v||^2), the norm being an INPUT (fp32) of the backward kernel."""
    v64, dw64, nr, g64 = v.double().reshape(v.shape[0], -1), dw.double().reshape(v.shape[0], -1), nrm32.double(), gv.double().reshape(-1)
    n = v64.shape[1]
    dot = (dw64 * v64).sum(1)
    e_dot = gamma(n) * (dw64 * v64).abs().sum(1)  # n products, n - 1 additions, any order / contraction
    dg = dot / nr
    sc, k = g64 / nr, dot / (nr * nr)
    dv = sc[:, None] * (dw64 - v64 * k[:, None])
    e_k = e_dot / (nr * nr) + 3 * U * k.abs()  # nr * nr, the quotient (and the dot's error)
    inner_abs = dw64.abs() + (v64 * k[:, None]).abs()
    e_dv = sc.abs()[:, None] * (v64.abs() * e_k[:, None] + 2 * U * inner_abs) + 2 * U * sc.abs()[:, None] * inner_abs
    return dg, dv, e_dot / nr + U * dg.abs(), e_dv


@pytest.mark.parametrize("rows", [1, 7, 1024])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 5120])
def test_weight_norm_per_layer(cuda_device, rows, n):
    ops = ops_mod()
    g = torch.Generator().manual_seed(rows * 10007 + n)
    gv, v, dw = torch.randn(rows, 1, 1, generator=g), torch.randn(rows, n, 1, generator=g), torch.randn(rows, n, 1, generator=g)
    w, nrm = ops.weight_norm_fwd(gv.to(cuda_device), v.to(cuda_device))
    w_ref, n_ref, e_w, e_n = wn_fwd_ref(gv, v)
    assert_within(nrm, n_ref, e_n, "weight_norm_fwd norm")
    assert_within(w, w_ref.reshape(rows, n, 1), e_w.reshape(rows, n, 1), "weight_norm_fwd w")
    nrm32 = n_ref.float()  # the backward's norm input: the rounded reference, not the kernel's
    dg, dv = torch.full((rows, 1, 1), NAN, device=cuda_device), torch.full((rows, n, 1), NAN, device=cuda_device)
    ops.weight_norm_bwd(gv.to(cuda_device), v.to(cuda_device), nrm32.to(cuda_device), dw.to(cuda_device), dg, dv)
    dg_ref, dv_ref, e_dg, e_dv = wn_bwd_ref(gv, v, nrm32, dw)
    assert_within(dg, dg_ref.reshape(rows, 1, 1), e_dg.reshape(rows, 1, 1), "weight_norm_bwd dg")
    assert_within(dv, dv_ref.reshape(rows, n, 1), e_dv.reshape(rows, n, 1), "weight_norm_bwd dv")
    # position probes of the two row sums: v one-hot 2.0 at j: ||v|| = 2, w[j] = g exactly; dw one-hot 1.0 at j over v = 3: dot = 3
    js = sorted({0, 63, 64, 255, 256, 511, 512, n - 2, n - 1} & set(range(n)))
    R = len(js)
    vp = torch.zeros(R, n, 1)
    vp[torch.arange(R), torch.tensor(js), 0] = 2.0
    gp = torch.arange(1, R + 1, dtype=torch.float32).view(R, 1, 1)
    w, nrm = ops.weight_norm_fwd(gp.to(cuda_device), vp.to(cuda_device))
    assert same_bits(nrm.cpu(), torch.full((R,), 2.0)) and same_bits(w.cpu() + 0.0, vp / 2.0 * gp), "weight_norm_fwd probe"
    dg, dv = torch.full((R, 1, 1), NAN, device=cuda_device), torch.full((R, n, 1), NAN, device=cuda_device)
    ops.weight_norm_bwd(gp.to(cuda_device), torch.full((R, n, 1), 3.0, device=cuda_device), torch.full((R,), 2.0, device=cuda_device),
                        (vp / 2.0).to(cuda_device), dg, dv)
    assert same_bits(dg.cpu(), torch.full((R, 1, 1), 1.5)), "weight_norm_bwd probe"


WN_LAYERS = [(1, 5120), (4, 1), (7, 3), (5, 41 * 8), (3, 257), (2, 1024)]  # (rows, n_per_row): a one-row layer, one-element rows, ...


def _wn_table(device):
    """The flat layouts of train/layers.py (WNBatch), restated: per layer bias-free [g | v] in the parameter buffer, w in the
    effective-weight buffer, one norm per row; every tensor starts on a multiple of four floats."""
    up4 = lambda x: (x + 3) // 4 * 4  # noqa: E731
    L = len(WN_LAYERS)
    tab = torch.zeros(6, L + 1, dtype=torch.int64)
    off = w_off = r0 = 0
    for i, (rows, n) in enumerate(WN_LAYERS):
        tab[0, i], tab[1, i], tab[2, i], tab[3, i], tab[4, i], tab[5, i] = r0, n, off, off + up4(rows), w_off, r0
        off += up4(rows) + up4(rows * n)
        w_off += up4(rows * n)
        r0 += rows
    tab[0, L] = r0
    return tab, off, w_off, r0


def test_weight_norm_batched_equals_per_layer_on_every_bucket_range(cuda_device):
    """The batched kernels over [row_lo, row_hi) for every pair of layer boundaries: rows in range bitwise equal to the per-layer
    entry points ("same arithmetic"), rows outside untouched (canary), the gradient sink zeroed in range only."""
    ops = ops_mod()
    lib = _lib.load()
    st = _lib.current_stream_ptr(cuda_device)
    tab, n_flat, n_eff, n_rows = _wn_table(cuda_device)
    L = len(WN_LAYERS)
    g = torch.Generator().manual_seed(21)
    flat = torch.randn(n_flat, generator=g)
    dw_eff0 = torch.randn(n_eff, generator=g)
    flat_d, tab_d = flat.to(cuda_device), tab.to(cuda_device)
    per = []  # per-layer results (w, norm, dg, dv) from the per-layer entry points
    for i, (rows, n) in enumerate(WN_LAYERS):
        go, vo, wo = int(tab[2, i]), int(tab[3, i]), int(tab[4, i])
        gl, vl = flat_d[go : go + rows].view(rows, 1, 1), flat_d[vo : vo + rows * n].view(rows, n, 1)
        w, nrm = ops.weight_norm_fwd(gl, vl)
        w_ref, n_ref, e_w, e_n = wn_fwd_ref(gl.cpu(), vl.cpu())
        assert_within(w, w_ref.reshape(rows, n, 1), e_w.reshape(rows, n, 1), f"layer {i} w")
        dwl = dw_eff0[wo : wo + rows * n].view(rows, n, 1).to(cuda_device)
        dg, dv = torch.empty(rows, 1, 1, device=cuda_device), torch.empty(rows, n, 1, device=cuda_device)
        ops.weight_norm_bwd(gl, vl, nrm, dwl, dg, dv)
        per.append((w.cpu().reshape(-1), nrm.cpu(), dg.cpu().reshape(-1), dv.cpu().reshape(-1)))
    for lo_l in range(L):
        for hi_l in range(lo_l + 1, L + 1):
            row_lo, row_hi = int(tab[0, lo_l]), int(tab[0, hi_l])
            eff = torch.full((n_eff,), CANARY, device=cuda_device)
            norms = torch.full((n_rows,), CANARY, device=cuda_device)
            _lib.check(lib.evmi_weight_norm_fwd_batched_f32(flat_d.data_ptr(), eff.data_ptr(), norms.data_ptr(), tab_d.data_ptr(), L, row_lo, row_hi, st))
            eff_want, norms_want = torch.full((n_eff,), CANARY), torch.full((n_rows,), CANARY)
            for i in range(lo_l, hi_l):
                rows, n = WN_LAYERS[i]
                eff_want[int(tab[4, i]) : int(tab[4, i]) + rows * n] = per[i][0]
                norms_want[int(tab[5, i]) : int(tab[5, i]) + rows] = per[i][1]
            assert same_bits(eff.cpu(), eff_want) and same_bits(norms.cpu(), norms_want), f"fwd_batched layers [{lo_l}, {hi_l})"
            # backward over the same range: norms of ALL layers present (as after a full forward), gradient buffer canary
            norms_all = torch.cat([p[1] for p in per]).to(cuda_device)
            grad = torch.full((n_flat,), CANARY, device=cuda_device)
            sink = dw_eff0.clone().to(cuda_device)
            _lib.check(lib.evmi_weight_norm_bwd_batched_f32(flat_d.data_ptr(), grad.data_ptr(), norms_all.data_ptr(), sink.data_ptr(), tab_d.data_ptr(), L,
                                                            row_lo, row_hi, st))
            grad_want, sink_want = torch.full((n_flat,), CANARY), dw_eff0.clone()
            for i in range(lo_l, hi_l):
                rows, n = WN_LAYERS[i]
                grad_want[int(tab[2, i]) : int(tab[2, i]) + rows] = per[i][2]
                grad_want[int(tab[3, i]) : int(tab[3, i]) + rows * n] = per[i][3]
                sink_want[int(tab[4, i]) : int(tab[4, i]) + rows * n] = 0.0
            assert same_bits(grad.cpu(), grad_want), f"bwd_batched layers [{lo_l}, {hi_l}): gradients"
            assert same_bits(sink.cpu(), sink_want), f"bwd_batched layers [{lo_l}, {hi_l}): gradient sink"


# =====================================================================================================================
# spectral norm pieces, ratio_accumulate
# =====================================================================================================================
def test_normalize_vec(cuda_device):
    ops = ops_mod()
    g = torch.Generator().manual_seed(2)
    for n in (1, 63, 1023, 1024, 1025, 5120):  # one workgroup of 1024 threads: one, and up to five, elements per thread
        x = torch.randn(n, generator=g)
        y = ops.normalize_vec(x.to(cuda_device), torch.full((n,), NAN, device=cuda_device))
        want = x.double() / x.double().norm()
        assert_within(y, want, (gamma(n + 1) + 2 * U) * want.abs(), f"normalize_vec n {n}")  # the norm as in weight norm, then one quotient
        z = ops.normalize_vec(torch.zeros(n, device=cuda_device), torch.full((n,), NAN, device=cuda_device), eps=1e-12)
        assert same_bits(z.cpu() + 0.0, torch.zeros(n)), "zero vector: 0 / eps"
        for j in sorted({0, 63, 64, 1023, 1024, n - 1} & set(range(n))):  # one 2.0: ||x|| = 2, y[j] = 1 exactly
            x = torch.zeros(n)
            x[j] = 2.0
            y = ops.normalize_vec(x.to(cuda_device), torch.full((n,), NAN, device=cuda_device))
            assert same_bits(y.cpu() + 0.0, x / 2.0), (n, j)


@pytest.mark.parametrize("rows,cols", [(1, 1), (128, 15), (1024, 5120)])
def test_spectral_norm_grad(cuda_device, rows, cols):
    """gw += dw / sigma - (dot / sigma^2) u v^T: r = 7 roundings (/, *, /, *, *, -, +) on the magnitudes of the three terms."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(rows + cols)
    gw0, dw = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    u, v = F.normalize(torch.randn(rows, generator=g), dim=0), F.normalize(torch.randn(cols, generator=g), dim=0)
    sigma, dot = torch.tensor([f32(2.37)]), torch.tensor([f32(-11.3)])
    gw = torch.cat([gw0.reshape(-1), torch.full((4,), CANARY)]).to(cuda_device)
    dev = [t.to(cuda_device) for t in (dw, u, v, sigma, dot)]  # (held until the results are read)
    _lib.check(lib.evmi_spectral_norm_grad_f32(gw.data_ptr(), *(t.data_ptr() for t in dev), rows, cols, _lib.current_stream_ptr(cuda_device)))
    sg, dt = float(sigma), float(dot)
    t1, t2 = dw.double() / sg, (dt / (sg * sg)) * torch.outer(u.double(), v.double())
    assert_within(gw[:-4].view(rows, cols), gw0.double() + t1 - t2, 8 * U * (gw0.double().abs() + t1.abs() + t2.abs()), "spectral_norm_grad")
    assert same_bits(gw.cpu()[-4:], torch.full((4,), CANARY))


def test_spectral_norm_layer_against_torch(cuda_device):
    """One SNConv (1024 x 1024 x 5, the widest MSD layer): effective weight of a training-mode call and the gradient of weight_orig
    against torch.nn.utils.spectral_norm in float64.  The chain (gemv_cols, normalize, gemv_rows, normalize, a dot, W / sigma) is
    bounded norm-wise: with dv = ||v_gpu - v_ref|| <= 2 gamma_h ||W|^T |u||| / ||W^T u|| + gamma_{w + 2} and s2 = ||W||_2,
    sigma = ||W v|| moves by at most s2 dv + gamma_w || |W| |v| || (+ the dot and the normalisation: gamma_{h + 2})."""
    from everyvoice_amd.train.layers import ParamGroup, SNConv

    h, cin, k = 1024, 1024, 5
    wdt = cin * k
    g = torch.Generator().manual_seed(9)
    W = torch.randn(h, cin, k, generator=g) / math.sqrt(wdt)
    u0, v0 = F.normalize(torch.randn(h, generator=g), dim=0), F.normalize(torch.randn(wdt, generator=g), dim=0)
    # (a weight gradient with a component along W: <dW, W> is then large and the rank-one term dominates the result, so the test
    # is sensitive to u, v and the power of sigma in front of them)
    dW = torch.randn(h, cin, k, generator=g) + 40.0 * W
    gW0 = torch.randn(h, cin, k, generator=g)
    group = ParamGroup(cuda_device)
    layer = SNConv(group, "c", cin, h, k, pad=2)
    group.finalize()
    group.load("c.weight_orig", W)
    layer.u.copy_(u0)
    layer.v.copy_(v0)
    group.gradient(layer.i_w).copy_(gW0)
    w_eff, sink = layer.effective(training=True)
    sink.copy_(dW)
    layer.finish_grads()
    torch.cuda.synchronize()
    # torch, float64
    conv = torch.nn.Conv1d(cin, h, k, padding=2).double()
    with torch.no_grad():
        conv.weight.copy_(W.double())
    conv = torch.nn.utils.spectral_norm(conv)
    with torch.no_grad():
        conv.weight_u.copy_(u0.double())
        conv.weight_v.copy_(v0.double())
    conv.train()
    conv(torch.zeros(1, cin, 8, dtype=torch.float64))  # the pre-forward hook: one power iteration, weight = weight_orig / sigma
    w_ref = conv.weight
    (w_ref * dW.double()).sum().backward()
    gW_ref = gW0.double() + conv.weight_orig.grad
    Wm = W.double().view(h, wdt)
    u1, v1 = conv.weight_u.detach(), conv.weight_v.detach()
    sigma = float(u1 @ (Wm @ v1))
    s2 = float(torch.linalg.matrix_norm(Wm, 2))
    amp1 = float((Wm.abs().t() @ u0.double().abs()).norm() / (Wm.t() @ u0.double()).norm())
    amp2 = float((Wm.abs() @ v1.abs()).norm() / (Wm @ v1).norm())
    d_v = 2 * gamma(h) * amp1 + gamma(wdt + 2)
    rel_sigma = (s2 / sigma) * d_v + gamma(wdt) * amp2 + gamma(h + 2) + 4 * U
    assert_within(w_eff, w_ref.detach(), (rel_sigma + 2 * U) * w_ref.detach().abs(), "SNConv effective weight")
    # gradient, Frobenius norm: dw / sigma (rel_sigma), (dot / sigma^2) u v^T (2 rel_sigma + the two vectors' errors), 8 u of each term
    d_u = 2 * ((s2 / sigma) * d_v + gamma(wdt) * amp2) + gamma(h + 2)
    assert float((layer.v.cpu().double() - v1).norm()) <= d_v and float((layer.u.cpu().double() - u1).norm()) <= d_u  # the stored state
    dot = float((dW.double() * W.double()).sum())
    bound = (float(dW.double().norm()) / sigma) * (rel_sigma + 8 * U) + abs(dot) / sigma ** 2 * (2 * rel_sigma + d_u + d_v + 8 * U) + 8 * U * float(gW0.double().norm())
    err = float((group.gradient(layer.i_w).cpu().double() - gW_ref).norm())
    assert err <= bound, (err, bound)
    # (worst-case gamma_n at n = 1024 / 5120 is loose, a few 1e-3: the sharp checks of these kernels are the operator tests above;
    # this one pins the wiring -- which vector multiplies which side, sigma against sigma^2 -- at the layer's real size)
    rank_one = abs(dot) / sigma ** 2
    assert bound < 0.1 * rank_one, (bound, rank_one)


def test_ratio_accumulate(cuda_device):
    """out += w sqrt(c0 / c1) (a quotient, a root, a product, the addition: 4 u); c1 == 0 adds nothing."""
    lib = _lib.load()
    st = _lib.current_stream_ptr(cuda_device)
    for c0, c1, w, prev in [(3.7, 11.3, 0.5, 0.0), (3.7, 11.3, 0.25, -2.5), (1e-12, 5.0, 1.0, 1.0), (2.0, 0.0, 1.0, 0.625), (0.0, 2.0, 1.0, 0.625)]:
        c0, c1, w, prev = f32(c0), f32(c1), f32(w), f32(prev)
        out, sq = torch.tensor([prev, CANARY], device=cuda_device), torch.tensor([c0, c1], device=cuda_device)
        _lib.check(lib.evmi_ratio_accumulate_f32(out.data_ptr(), sq.data_ptr(), w, st))
        if c1 == 0.0:
            assert same_bits(out.cpu(), torch.tensor([prev, CANARY]))
            continue
        term = w * math.sqrt(c0 / c1)
        assert_within(out[:1], torch.tensor([prev + term], dtype=torch.float64), torch.tensor([4 * U * (abs(prev) + abs(term))], dtype=torch.float64), "ratio_accumulate")
        assert same_bits(out.cpu()[1:], torch.tensor([CANARY]))


# =====================================================================================================================
# pooling, views, framing: forward exact (or gamma_4), backward = the adjoint
# =====================================================================================================================
def adjoint_check(x, y, Ax_gpu, ATy_gpu, bound_terms, what):
    """<A x, y> == <x, A^T y> with both images from the GPU and the dots in double; bound_terms: the float64 sum of
    |x_i| * (bound on (A^T y)_i) + |y_j| * (bound on (A x)_j)."""
    lhs = (Ax_gpu.cpu().double().reshape(-1) * y.double().reshape(-1)).sum()
    rhs = (x.double().reshape(-1) * ATy_gpu.cpu().double().reshape(-1)).sum()
    scale = (Ax_gpu.cpu().double().abs().reshape(-1) * y.double().abs().reshape(-1)).sum()
    assert abs(lhs - rhs) <= bound_terms + 2.0 ** -45 * scale + TINY, (what, float(lhs), float(rhs), float(bound_terms))


def linear_adjoint64(fwd, x_shape, dy):
    """A^T dy by float64 autograd of the linear map fwd."""
    x = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    fwd(x).backward(dy.double())
    return x.grad


@pytest.mark.parametrize("t_in", [1, 2, 3, 4, 5, 50, 51, 8192, 8193])
def test_avgpool4s2_and_adjoint(cuda_device, t_in):
    ops = ops_mod()
    g = torch.Generator().manual_seed(t_in)
    Cc, B = 3, 2
    x = torch.randn(Cc, B, t_in, generator=g)
    pool = lambda t: F.avg_pool1d(t, 4, 2, padding=2, count_include_pad=True)  # noqa: E731
    y = ops.avgpool4s2(x.to(cuda_device))
    assert y.shape[2] == t_in // 2 + 1 == pool(x).shape[2]
    # up to four terms added in order, times 0.25 (exact): gamma_3 of the absolute sum
    e_y = gamma(3) * pool(x.double().abs())
    assert_within(y, pool(x.double()), e_y, "avgpool4s2")
    dy = torch.randn(y.shape, generator=g)
    dx = ops.avgpool4s2_bwd(dy.to(cuda_device), t_in)
    e_dx = gamma(3) * linear_adjoint64(pool, x.shape, dy.abs())
    assert_within(dx, linear_adjoint64(pool, x.shape, dy), e_dx, "avgpool4s2 backward")
    adjoint_check(x, dy, y, dx, (x.double().abs() * e_dx).sum() + (dy.double().abs() * e_y).sum(), "avgpool4s2")


def _period_T(period):
    """T with reflect pads 0, 1 and period - 1, each at the smallest legal T (pad < T) and at a long row."""
    out = set()
    for pad in (0, 1, period - 1):
        k = 1
        while k * period - pad <= pad or k * period - pad < 1:
            k += 1
        out.add(k * period - pad)           # the smallest T with this pad
        out.add((k + 700) * period - pad)
    return sorted(out)


@pytest.mark.parametrize("period", [2, 3, 5, 7, 11])
def test_period_view_and_adjoint(cuda_device, period):
    ops = ops_mod()
    lib = _lib.load()
    for T in _period_T(period):
        g = torch.Generator().manual_seed(T)
        B = 3
        H = -(-T // period)
        pad = H * period - T
        assert pad < T

        def view(t):
            tp = F.pad(t, (0, pad), mode="reflect") if pad else t
            return tp.view(1, B, H, period).permute(0, 1, 3, 2).reshape(1, B * period, H)

        x = torch.randn(1, B, T, generator=g)
        y = ops.period_view(x.to(cuda_device), period)
        assert same_bits(y.cpu(), view(x)), (period, T)
        dy = torch.randn(1, B * period, H, generator=g)
        dx = ops.period_view_bwd(dy.to(cuda_device), B, T, period)
        e_dx = gamma(1) * linear_adjoint64(view, x.shape, dy.abs())  # at most two terms: one addition
        assert_within(dx, linear_adjoint64(view, x.shape, dy), e_dx, "period_view backward")
        adjoint_check(x, dy, y, dx, (x.double().abs() * e_dx).sum(), "period_view")
    # a pad of T or more is refused, not launched (T = 5, period = 11 would read x[-2])
    buf = torch.zeros(64, device=cuda_device)
    assert lib.evmi_period_view_f32(buf.data_ptr(), buf.data_ptr(), 1, 5, 11, 0, None) == 1
    assert b"period_view" in lib.evmi_last_error()


@pytest.mark.parametrize("T", [2, 3, 257])
def test_reflect_pad_left1_and_adjoint(cuda_device, T):
    ops = ops_mod()
    g = torch.Generator().manual_seed(T)
    Cc, B = 5, 3
    padl = lambda t: F.pad(t, (1, 0), mode="reflect")  # noqa: E731
    x = torch.randn(Cc, B, T, generator=g)
    y = ops.reflect_pad_left1(x.to(cuda_device))
    assert same_bits(y.cpu(), padl(x))
    dy = torch.randn(Cc, B, T + 1, generator=g)
    dx = ops.reflect_pad_left1_bwd(dy.to(cuda_device))
    e_dx = gamma(1) * linear_adjoint64(padl, x.shape, dy.abs())
    assert_within(dx, linear_adjoint64(padl, x.shape, dy), e_dx, "reflect_pad_left1 backward")
    adjoint_check(x, dy, y, dx, (x.double().abs() * e_dx).sum(), "reflect_pad_left1")


@pytest.mark.parametrize("n_fft,hop", [(1024, 120), (2048, 240), (512, 50)])  # the trainer's multi-resolution STFT loss
def test_stft_frames_and_adjoint(cuda_device, n_fft, hop):
    ops = ops_mod()
    lib = _lib.load()
    for T in (n_fft // 2 + 1, 8192):  # the smallest legal T (reflect pad n_fft / 2 < T), and the training segment
        g = torch.Generator().manual_seed(T + n_fft)
        B = 2
        Fr = 1 + T // hop

        def frames(t):
            tp = F.pad(t[None], (n_fft // 2, n_fft // 2), mode="reflect")[0]
            return tp.unfold(1, n_fft, hop)[:, :Fr].permute(2, 0, 1).reshape(n_fft, B * Fr)

        x = torch.randn(B, T, generator=g)
        fr, f_got = ops.stft_frames(x.to(cuda_device), n_fft, hop)
        assert f_got == Fr and same_bits(fr.cpu(), frames(x)), (n_fft, T)
        dfr = torch.randn(n_fft, B * Fr, generator=g)
        dx = ops.stft_frames_bwd(dfr.to(cuda_device), B, T, n_fft, hop)
        terms = 3 * (n_fft // hop + 1)  # a sample is read by at most ceil(n_fft / hop) frames, itself and its two mirror images
        e_dx = gamma(terms) * linear_adjoint64(frames, x.shape, dfr.abs())
        assert_within(dx, linear_adjoint64(frames, x.shape, dfr), e_dx, "stft_frames backward")
        adjoint_check(x, dfr, fr, dx, (x.double().abs() * e_dx).sum(), "stft_frames")
    buf = torch.zeros(64, device=cuda_device)
    assert lib.evmi_stft_frames_f32(buf.data_ptr(), buf.data_ptr(), 1, n_fft // 2, n_fft, hop, 0, None) == 1  # pad == T: refused
    assert b"stft_frames" in lib.evmi_last_error()


# =====================================================================================================================
# iSTFT head
# =====================================================================================================================
@pytest.mark.parametrize("H", [1, 9, 513])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_istft_polar_and_backward(cuda_device, H, n):
    """s = exp(a) (cos, sin)(sin(b)).  Forward: exp (E), the inner sin (E, passed on by |d cos|, |d sin| <= 1, |sin b| <= 1), the outer
    function (E), one product: (3 E + 2 u) mag.  Backward against float64 autograd: two such products and a sum per output, the
    phase row one more factor cos(b) (E) and product."""
    ops = ops_mod()
    g = torch.Generator().manual_seed(H * 1000 + n)
    a = torch.cat([torch.randn(H, 1, n, generator=g), torch.randn(H, 1, n, generator=g) * 3.0])
    a[0, 0, 0] = 0.0
    ds = torch.randn(2 * H, 1, n, generator=g)
    s = ops.istft_polar(a.to(cuda_device), H)
    a64 = a.double().requires_grad_()
    mag, ph = torch.exp(a64[:H]), torch.sin(a64[H:])
    s_ref = torch.cat([mag * torch.cos(ph), mag * torch.sin(ph)])
    e_s = (3 * E + 2 * U) * torch.cat([mag, mag]).detach()
    assert_within(s, s_ref.detach(), e_s, "istft_polar")
    s_ref.backward(ds.double())
    da = ops.istft_polar_bwd(a.to(cuda_device), ds.to(cuda_device), H)
    amp = mag.detach() * (ds[:H].double().abs() + ds[H:].double().abs())
    e_da = torch.cat([(3 * E + 4 * U) * amp, (4 * E + 5 * U) * amp])
    assert_within(da, a64.grad, e_da, "istft_polar backward")


# =====================================================================================================================
# softmax rows (public ABI without a caller in this repository)
# =====================================================================================================================
@pytest.mark.parametrize("Tk", [1, 33, 64, 200])
def test_softmax_rows_and_backward(cuda_device, Tk):
    lib = _lib.load()
    st = _lib.current_stream_ptr(cuda_device)
    B, Tq = 4, 5
    lens = torch.tensor([1, Tk, max(1, Tk // 2), max(1, Tk - 1)], dtype=torch.int32)
    g = torch.Generator().manual_seed(Tk)
    S = torch.randn(B, Tq, Tk, generator=g) * 2.0  # (|s - max| stays far below 87: no valid probability underflows)
    valid = torch.arange(Tk)[None, None, :] < lens[:, None, None]
    S64 = S.double().masked_fill(~valid, float("-inf"))
    P_ref = torch.softmax(S64, dim=-1)
    spread = (S64.amax(-1, keepdim=True) - S64).masked_fill(~valid, 0.0)
    # exp(s - m): the subtraction (u |s - m| on the exponent) and expf (E), in the numerator and in every term of the sum; the sum
    # of len terms (gamma_len); 1 / sum and the product (2 u)
    rel = 2 * (U * spread.amax(-1, keepdim=True) + E) + gamma(Tk) + 3 * U
    e_P = rel * P_ref
    sd = torch.cat([S.reshape(-1), torch.full((4,), CANARY)]).to(cuda_device)
    lens_d = lens.to(cuda_device)
    _lib.check(lib.evmi_softmax_rows_f32(sd.data_ptr(), None, lens_d.data_ptr(), B, Tq, Tk, 0.0, 0, st))
    P_gpu = sd.cpu()[:-4].view(B, Tq, Tk)
    assert_within(P_gpu, P_ref, e_P, "softmax_rows")
    assert bool((P_gpu[~valid.expand_as(P_gpu)] == 0).all()) and same_bits(sd.cpu()[-4:], torch.full((4,), CANARY))
    # backward, p = 0: dS = scale P (d - sum_k P d), P an input (the rounded reference)
    P32 = P_ref.float()
    dP = torch.randn(B, Tq, Tk, generator=g)
    scale = f32(0.125)

    def bwd_ref(d64):
        P64 = P32.double()
        sabs = (P64 * d64).abs().sum(-1, keepdim=True)
        s = (P64 * d64).sum(-1, keepdim=True)
        # the dot (gamma_Tk of its absolute sum), the subtraction, the two products
        return scale * P64 * (d64 - s), abs(scale) * P64 * (gamma(Tk) * sabs + 3 * U * (d64.abs() + sabs))

    dd, P32d = dP.clone().to(cuda_device), P32.to(cuda_device)
    _lib.check(lib.evmi_softmax_bwd_rows_f32(P32d.data_ptr(), dd.data_ptr(), B * Tq, Tk, scale, 0.0, 0, st))
    want, e_dS = bwd_ref(dP.double())
    assert_within(dd, want, e_dS, "softmax_bwd_rows")
    # dropout: the mask is read from the kernel's own zeros (valid keys only: beyond lens the output is 0 by definition)
    p, seed = f32(0.25), 1234567
    sd = S.clone().to(cuda_device)
    dropped = torch.full((B * Tq * Tk + 4,), CANARY, device=cuda_device)
    _lib.check(lib.evmi_softmax_rows_f32(sd.data_ptr(), dropped.data_ptr(), lens_d.data_ptr(), B, Tq, Tk, p, seed, st))
    assert same_bits(sd.cpu(), P_gpu), "the probabilities do not depend on p"
    D = dropped.cpu()[:-4].view(B, Tq, Tk)
    assert same_bits(dropped.cpu()[-4:], torch.full((4,), CANARY))
    assert bool((P_gpu[valid.expand_as(P_gpu)] > 0).all())
    mask = (D != 0) & valid
    keep = 1.0 / (1.0 - p)
    # v * (1 / (1 - p)): the probability's own error, then 1 - p, the quotient, the product
    assert_within(D, P_ref * mask * keep, (rel + 3 * U) * P_ref * mask * keep, "softmax_rows dropped")
    if Tk >= 33:
        frac = float(mask.sum()) / float(valid.expand_as(mask).sum())
        assert 0.6 < frac < 0.9, frac  # keep probability 0.75 over >= 300 draws: +- 6 sigma
    dd = dP.clone().to(cuda_device)
    _lib.check(lib.evmi_softmax_bwd_rows_f32(P32d.data_ptr(), dd.data_ptr(), B * Tq, Tk, scale, p, seed, st))
    dm = dP.double() * mask * keep  # (where P32 == 0 the mask does not matter: the term and the result are 0)
    want, e_dS = bwd_ref(dm)
    e_dS = e_dS + abs(scale) * P32.double() * 3 * U * (dm.abs() + (P32.double() * dm).abs().sum(-1, keepdim=True))  # d * keep: 3 roundings
    assert_within(dd, want, e_dS, "softmax_bwd_rows with the same seed")
