"""The fused residual kernels alone: evmi_resblock_pair_bf16 (csrc/resblock_pair_kernel.h, six entries; resblock_pair_chunked_kernel.h,
the 128-channel entry) and evmi_resblock_branch_bf16 (resblock_branch_kernel.h, three entries), against the float64 reference of
tests/resblock_ref.py.

(a) - (c) run on LATTICE inputs: small integers on which every bf16 rounding point is exact and every fp32 sum is exact in any order
(resblock_ref.check_lattice asserts both for each case before it is used), so the kernels are compared with the UNROUNDED float64
reference in bits, with no tolerance: a wrong row at a tile seam, an intermediate that is not zero outside [0, T), a misplaced tap or
channel changes an integer.  A failure prints the first differing (item, row, channel) and the row modulo the tile's valid rows.
tt / bn come from the plan queries, never from this file.  Every run prefills `out` with NaN (when not accumulating), keeps sentinel
guard rows in front of and behind `out`, and keeps x and out apart.

(d) runs on random inputs against the reference that rounds where the kernels store.  Measured on MI355X, max|diff| / max|want|,
B = 2, T = tt + 1, dilation 3 (branches 1, 3, 5), slope 0.1, post 0.1, scale 1/3, accumulating:
    pair   c64 k3 2.11e-4   c64 k7 4.28e-4   c64 k11 8.87e-4   c32 k3 5.19e-8   c32 k7 8.01e-4   c32 k11 3.91e-4   c128 k3 2.76e-3
    branch c32 k3 2.60e-3   c32 k7 1.33e-3   c64 k3 1.23e-3
RANDOM_BOUND is twice the largest of them (2 x 2.762e-3 = 5.52e-3); 2**-7, the project's figure for one bf16 rounding plus the summation order, is the ceiling
such a bound may not pass.  (The 128-channel kernel stages conv2 + b2 in bf16 before the residual is added -- one rounding more than
the reference has.)

(f) the narrow (128-row) and wide (256-row) LDS-DMA tiles of evmi_conv_tc_tm_bf16 give the same bits (launch_conv_tc's claim).
"""

import ctypes as C

import pytest
import torch

import resblock_ref as R

pytestmark = pytest.mark.gpu

GUARD_ROWS = 64
SENTINEL = -24832.0  # bf16-representable, far from every value a run produces
RANDOM_BOUND = 2 * 2.762e-3  # twice the largest measured value of the docstring; below the 2**-7 ceiling


def _lib():
    from everyvoice_amd import _lib as L

    return L


def pair_plan(c, ks, dil):
    tt, bn, kc, n = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_longlong(-1)
    assert _lib().load().evmi_resblock_pair_plan(c, ks, dil, C.byref(tt), C.byref(bn), C.byref(kc), C.byref(n)) == 1, (c, ks, dil)
    return tt.value, bn.value, kc.value, n.value


def branch_plan(c, ks, dils):
    tt, bn = C.c_int(-1), C.c_int(-1)
    assert _lib().load().evmi_resblock_branch_plan(c, ks, 3, (C.c_int * 3)(*dils), C.byref(tt), C.byref(bn)) == 1, (c, ks, dils)
    return tt.value, bn.value


def _laid(w, kc, dev):
    """the image the generator ships: the library's own host relayout of fp32 [C][C][ks]"""
    c, _, ks = w.shape
    wf = w.to(torch.float32).contiguous()
    dst = torch.empty(c * c * ks, dtype=torch.bfloat16)
    _lib().check(_lib().load().evmi_resblock_pair_relayout_f32(wf.data_ptr(), dst.data_ptr(), c, ks, kc), "relayout")
    return dst.to(dev)


class _Out:
    """out [B][T][C] bf16 between two bands of sentinel rows; NaN inside unless a base is given"""

    def __init__(self, dev, B, T, c, base):
        self.buf = torch.full((2 * GUARD_ROWS + B * T, c), SENTINEL, dtype=torch.bfloat16, device=dev)
        self.body = self.buf[GUARD_ROWS:GUARD_ROWS + B * T].view(B, T, c)
        if base is None:
            self.body.fill_(float("nan"))
        else:
            self.body.copy_(base.to(dev, torch.bfloat16))
        self.ptr = self.body.data_ptr()
        assert self.ptr % 16 == 0

    def read(self):
        torch.cuda.synchronize()
        guards = torch.cat([self.buf[:GUARD_ROWS], self.buf[-GUARD_ROWS:]]).float().cpu()
        assert bool((guards == SENTINEL).all()), "rows outside out were written"
        return self.body.float().cpu().to(torch.float64)


def run_pair(dev, x, w1, b1, w2, b2, dil, slope, post=1.0, scale=1.0, base=None, n_cu=0):
    L = _lib()
    B, T, c = x.shape
    ks = w1.shape[2]
    kc = pair_plan(c, ks, dil)[2]
    xd = x.to(dev, torch.bfloat16).contiguous()
    l1, l2 = _laid(w1, kc, dev), _laid(w2, kc, dev)
    b1d, b2d = b1.to(dev, torch.float32), b2.to(dev, torch.float32)
    out = _Out(dev, B, T, c, base)
    L.check(L.load().evmi_resblock_pair_bf16(xd.data_ptr(), l1.data_ptr(), b1d.data_ptr(), l2.data_ptr(), b2d.data_ptr(), out.ptr, B, T, c, ks, dil,
                                             slope, post, scale, 0 if base is None else 1, n_cu, L.current_stream_ptr()), "evmi_resblock_pair_bf16")
    return out.read()


def run_branch(dev, x, ws, bs, dils, slope, post=1.0, scale=1.0, base=None, n_cu=0):
    L = _lib()
    B, T, c = x.shape
    ks = ws[0].shape[2]
    xd = x.to(dev, torch.bfloat16).contiguous()
    laid = [_laid(w, c, dev) for w in ws]
    bd = [b.to(dev, torch.float32) for b in bs]
    out = _Out(dev, B, T, c, base)
    L.check(L.load().evmi_resblock_branch_bf16(xd.data_ptr(), (C.c_void_p * 6)(*[t.data_ptr() for t in laid]), (C.c_void_p * 6)(*[t.data_ptr() for t in bd]),
                                               out.ptr, B, T, c, ks, 3, (C.c_int * 3)(*dils), slope, post, scale, 0 if base is None else 1, n_cu,
                                               L.current_stream_ptr()), "evmi_resblock_branch_bf16")
    return out.read()


def assert_bits(got, want, tt, what):
    """got: the kernel's bf16 output as float64; want: the float64 reference (representable: check_lattice).  Value equality of
    every element (NaN equals nothing), the first difference named."""
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    i, r, ch = (int(v) for v in bad[0])
    rows = sorted({int(v) for v in bad[:, 1]})
    msg = (f"{what}: {len(bad)} elements differ; first at item {i}, row {r} (row % tt = {r % tt}, tt = {tt}), channel {ch}: "
           f"got {float(got[i, r, ch])}, want {float(want[i, r, ch])}; rows that differ: {rows[:12]}{' ...' if len(rows) > 12 else ''}")
    print(msg)
    raise AssertionError(msg)


def _pair_cases():
    for c, ks in R.PAIR_ENTRIES:
        for dil in R.pair_dilations(c):
            yield c, ks, dil


# ---- (a) bits on the lattice, every table entry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,ks,dil", list(_pair_cases()))
def test_pair_bits_on_the_lattice(cuda_device, c, ks, dil):
    tt = pair_plan(c, ks, dil)[0]
    for T, acc, post, scale in R.pair_runs(c, ks, dil, tt):
        x, ws, bs, base = R.lattice(c, ks, R.B_LATTICE, T)
        base = base if acc else None
        want = R.check_lattice(x, ws, bs, (dil,), R.LATTICE_SLOPE, post, scale, base)
        got = run_pair(cuda_device, x, ws[0], bs[0], ws[1], bs[1], dil, R.LATTICE_SLOPE, post, scale, base)
        assert_bits(got, want, tt, f"pair c={c} k={ks} dil={dil} T={T} accumulate={acc} post={post} scale={scale}")


# ---- (b) the tile walk -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,ks,dil", R.WALK_PAIRS)
def test_pair_tile_walk(cuda_device, c, ks, dil):
    tt = pair_plan(c, ks, dil)[0]
    for B, T, n_cu in R.walk_problems(tt, ks):
        assert B * -(-T // tt) in (9, 40, 1)
        x, ws, bs, base = R.lattice(c, ks, B, T)
        want = R.check_lattice(x, ws, bs, (dil,), R.LATTICE_SLOPE, 0.5, 0.5, base)
        got = run_pair(cuda_device, x, ws[0], bs[0], ws[1], bs[1], dil, R.LATTICE_SLOPE, 0.5, 0.5, base, n_cu=n_cu)
        assert_bits(got, want, tt, f"pair c={c} k={ks} dil={dil} B={B} T={T} n_cu={n_cu}")


@pytest.mark.parametrize("c,ks", R.BRANCH_ENTRIES)
def test_branch_tile_walk(cuda_device, c, ks):
    dils = (1, 3, 5)
    tt = branch_plan(c, ks, dils)[0]
    for B, T, n_cu in R.walk_problems(tt, ks):
        assert B * -(-T // tt) in (9, 40, 1)
        x, ws, bs, base = R.lattice(c, ks, B, T, n_pairs=3, **R.BRANCH_LATTICE)
        want = R.check_lattice(x, ws, bs, dils, R.LATTICE_SLOPE, 0.5, 0.5, base)
        got = run_branch(cuda_device, x, ws, bs, dils, R.LATTICE_SLOPE, 0.5, 0.5, base, n_cu=n_cu)
        assert_bits(got, want, tt, f"branch c={c} k={ks} B={B} T={T} n_cu={n_cu}")


# ---- (c) branches ------------------------------------------------------------------------------------------------------------------------------
def _branch_cases():
    for c, ks in R.BRANCH_ENTRIES:
        for k, dils in enumerate(R.BRANCH_TRIPLES[(c, ks)]):
            yield c, ks, k, dils


@pytest.mark.parametrize("c,ks,k,dils", list(_branch_cases()))
def test_branch_bits_on_the_lattice(cuda_device, c, ks, k, dils):
    tt = branch_plan(c, ks, dils)[0]
    for T, acc, post, scale in R.branch_runs(tt, k):
        x, ws, bs, base = R.lattice(c, ks, R.B_LATTICE, T, n_pairs=3, **R.BRANCH_LATTICE)
        base = base if acc else None
        want = R.check_lattice(x, ws, bs, dils, R.LATTICE_SLOPE, post, scale, base)
        got = run_branch(cuda_device, x, ws, bs, dils, R.LATTICE_SLOPE, post, scale, base)
        assert_bits(got, want, tt, f"branch c={c} k={ks} dils={dils} T={T} accumulate={acc} post={post} scale={scale}")


@pytest.mark.parametrize("c,ks", R.BRANCH_ENTRIES)
def test_branch_equals_three_chained_pairs_in_bits(cuda_device, c, ks):
    """resblock_branch_kernel.h: "the two paths give the same bits" -- on random inputs, across a seam of both tilings"""
    dils = (1, 3, 5)
    T = pair_plan(c, ks, 1)[0] + 1
    assert T > branch_plan(c, ks, dils)[0] + 1
    x, ws, bs, base = R.random_problem(c, ks, 2, T, n_pairs=3)
    got = run_branch(cuda_device, x, ws, bs, dils, 0.1, 0.1, 1.0 / 3.0, base)
    y = x
    for p in range(3):
        last = p == 2
        y = run_pair(cuda_device, y, ws[2 * p], bs[2 * p], ws[2 * p + 1], bs[2 * p + 1], dils[p], 0.1, 0.1 if last else 1.0,
                     1.0 / 3.0 if last else 1.0, base if last else None)
    assert_bits(got, y, branch_plan(c, ks, dils)[0], f"branch vs pairs c={c} k={ks}")


# ---- (d) random inputs, tolerance --------------------------------------------------------------------------------------------------------------
def _check_random(got, want, what):
    assert bool(torch.isfinite(got).all())
    err = float((got - want).abs().max() / want.abs().max())
    print(f"{what}: max|diff| / max|want| = {err:.3e} (bound {RANDOM_BOUND:.3e})")
    assert RANDOM_BOUND <= 2 ** -7
    assert err <= RANDOM_BOUND


@pytest.mark.parametrize("c,ks", R.PAIR_ENTRIES)
def test_pair_random_inputs(cuda_device, c, ks):
    dil = 3
    T = pair_plan(c, ks, dil)[0] + 1
    x, ws, bs, base = R.random_problem(c, ks, 2, T)
    want = R.pair_ref(x, ws[0], bs[0], ws[1], bs[1], dil, 0.1, 0.1, 1.0 / 3.0, base, rounded=True)
    got = run_pair(cuda_device, x, ws[0], bs[0], ws[1], bs[1], dil, 0.1, 0.1, 1.0 / 3.0, base)
    _check_random(got, want, f"pair c={c} k={ks}")


@pytest.mark.parametrize("c,ks", R.BRANCH_ENTRIES)
def test_branch_random_inputs(cuda_device, c, ks):
    dils = (1, 3, 5)
    T = branch_plan(c, ks, dils)[0] + 1
    x, ws, bs, base = R.random_problem(c, ks, 2, T, n_pairs=3)
    want = R.branch_ref(x, ws, bs, dils, 0.1, 0.1, 1.0 / 3.0, base, rounded=True)
    got = run_branch(cuda_device, x, ws, bs, dils, 0.1, 0.1, 1.0 / 3.0, base)
    _check_random(got, want, f"branch c={c} k={ks}")


# ---- (e) item independence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,ks", [(32, 3), (64, 7), (128, 3)])
def test_pair_item_alone_gives_the_same_bits(cuda_device, c, ks):
    dil = 3
    T = pair_plan(c, ks, dil)[0] + 1
    x, ws, bs, base = R.random_problem(c, ks, 3, T)
    args = (ws[0], bs[0], ws[1], bs[1], dil, 0.1, 0.1, 0.5)
    batch = run_pair(cuda_device, x, *args, base)
    alone = run_pair(cuda_device, x[1:2], *args, base[1:2])
    assert_bits(alone, batch[1:2], T - 1, f"pair c={c} k={ks}: item 1 alone")


def test_branch_item_alone_gives_the_same_bits(cuda_device):
    c, ks, dils = 64, 3, (1, 3, 5)
    T = branch_plan(c, ks, dils)[0] + 1
    x, ws, bs, base = R.random_problem(c, ks, 3, T, n_pairs=3)
    batch = run_branch(cuda_device, x, ws, bs, dils, 0.1, 0.1, 0.5, base)
    alone = run_branch(cuda_device, x[1:2], ws, bs, dils, 0.1, 0.1, 0.5, base[1:2])
    assert_bits(alone, batch[1:2], T - 1, "branch c=64 k=3: item 1 alone")


# ---- (f) the narrow and the wide tile of the time-major convolution --------------------------------------------------------------------------
def test_conv_tc_narrow_and_wide_tiles_give_the_same_bits(cuda_device):
    """C = 128, k = 3 through evmi_conv_tc_tm_bf16: 2 x 300 rows run on the 128-row tiles (4 workgroups of 256-row tiles would not fill
    the chip), 2 x 32768 rows on the 256-row tiles (256 row tiles: launch_conv_tc's threshold).  Lattice inputs: both equal the exact
    result, and so each other on the rows whose taps lie inside the shorter sequence."""
    from everyvoice_amd.train.mrf_tm import TMBuf

    L = _lib()
    lib = L.load()
    c, ks, dil, B = 128, 3, 1, 2
    assert lib.evmi_conv_tc_supported(c, c, ks, dil)
    s = L.current_stream_ptr()
    x_long, w, b = R.conv_tc_lattice(c, ks, B, 32768)
    wd = w.to(cuda_device, torch.float32).contiguous()
    laid = torch.empty(c * c * ks // 2, device=cuda_device)
    L.check(lib.evmi_conv_tc_relayout_f32(wd.data_ptr(), laid.data_ptr(), c, c, ks, dil, 0, s), "relayout")
    bd = b.to(cuda_device, torch.float32)
    outs = {}
    for T in (300, 32768):
        x = x_long[:, :T].contiguous()
        want = R.check_conv_lattice(x, w, b, dil)
        xb, yb = TMBuf(c, B, T, cuda_device), TMBuf(c, B, T, cuda_device)
        xb.valid().copy_(x.to(cuda_device, torch.bfloat16))
        yb.valid().fill_(float("nan"))
        L.check(lib.evmi_conv_tc_tm_bf16(xb.ptr, laid.data_ptr(), bd.data_ptr(), 0, 0, yb.ptr, B, T, xb.Tp, xb.PL, c, c, ks, dil, 1.0, 1.0, 1.0, 1.0, s),
                "evmi_conv_tc_tm_bf16")
        torch.cuda.synchronize()
        got = yb.valid().float().cpu()
        whole = yb.store.view(torch.bfloat16).double().nan_to_num(0.0).abs().sum()
        assert float(whole.cpu()) == float(got.double().abs().sum()), "rows outside the valid ones were written"
        assert_bits(got.double(), want.double(), 128 if T == 300 else 256, f"conv_tc c=128 k=3 T={T}")
        outs[T] = got
    common = 300 - dil * (ks - 1) // 2  # rows whose taps lie inside the shorter sequence
    assert torch.equal(outs[300][:, :common], outs[32768][:, :common])
