"""Reference of the fused residual kernels (csrc/resblock_pair_kernel.h, resblock_pair_chunked_kernel.h, resblock_branch_kernel.h)
and the inputs their layer-level tests run on.  A helper module: tests/test_resblock_ref_host.py checks it without a GPU,
tests/test_gpu_resblock_fused.py compares the kernels with it.

The reference is the contract at the top of resblock_pair_kernel.h in float64, written with torch's conv1d and nothing else:

    out = post( [base] + out_scale * ( x + b2 + conv2( lrelu( b1 + conv1_dil( lrelu(x) ) ) ) ) )

Activations are [B][T][C], parameters [C][C][ks] (torch: [out][in][tap]); every convolution zero-pads ITS input ("same" padding), so
the intermediate is zero outside [0, T) -- not lrelu(b1).  A branch is three pairs chained, scale / post / base on the last only.

Two kinds of input:

* lattice(...): small integers on which every bf16 rounding point of the kernels is exact and every fp32 sum is exact in any order
  (x = 4 {-2..2}, w1 = 2 {-1, 0, 1}, w2 = 4 {-1, 0, 1}, b1 = 2 {..}, b2 = 4 {..}, slopes and scale 0.5: lrelu(x) is even, conv1 + b1
  is even, the intermediate an integer, conv2 + b2 and x multiples of 4, so is every y; the scaled sum is even, the base a multiple of 4,
  the output an integer).  check_lattice() ASSERTS both properties for the case at hand -- representable at every rounding point,
  sum of absolute products below 2**24 -- so a kernel can be compared with the unrounded float64 reference in bits, on either MFMA shape.
* random_problem(...): bf16-rounded normals, dense weights scaled 1.5 / sqrt(C ks), slope 0.1, for the tolerance test.
"""

import torch
import torch.nn.functional as F

F64 = torch.float64

# wrong variants of the pair reference (test_resblock_ref_host.py: each must be visible on the lattice inputs)
VARIANTS = ("t1_not_zeroed", "x_replicated", "conv2_dilated", "seam_shifted")


def bf16(t):
    """round to bf16 (nearest even), back in float64"""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def lrelu(t, slope):
    return torch.where(t > 0, t, t * slope)


def conv(x, w, dil, pad=None):
    """x [B][T][C], w [C][C][ks]; zero padding dil * (ks - 1) / 2 on both sides unless `pad` is given"""
    ks = w.shape[2]
    pad = dil * (ks - 1) // 2 if pad is None else pad
    return F.conv1d(x.transpose(1, 2), w, None, 1, pad, dil).transpose(1, 2)


def _bias(b):
    return b.view(1, 1, -1)


def pair_ref(x, w1, b1, w2, b2, dil, slope, post_slope=1.0, out_scale=1.0, base=None, rounded=False, variant=None, tt=None, stages=None):
    """One residual pair in float64.  rounded: round to bf16 where the kernels store (the activated input, the intermediate, the
    output).  variant: one of VARIANTS, a deliberately wrong form (tt: rows a tile stores, for "seam_shifted").  stages: a dict that
    receives every intermediate quantity (check_lattice reads it)."""
    x, w1, b1, w2, b2 = (t.to(F64) for t in (x, w1, b1, w2, b2))
    rnd = bf16 if rounded else (lambda t: t)
    ks = w1.shape[2]
    h2, h1 = (ks - 1) // 2, dil * (ks - 1) // 2
    xa = rnd(lrelu(x, slope))
    if variant == "x_replicated":
        xa_pad = F.pad(xa.transpose(1, 2), (h1, h1), mode="replicate").transpose(1, 2)
        c1 = conv(xa_pad, w1, dil, pad=0)
    else:
        c1 = conv(xa, w1, dil)
    t1 = rnd(lrelu(c1 + _bias(b1), slope))
    if variant == "t1_not_zeroed":
        # the intermediate of the rows just outside the sequence, computed from the zero-padded input as a tile would
        xa_wide = F.pad(xa, (0, 0, h2, h2))
        t1_wide = rnd(lrelu(conv(xa_wide, w1, dil) + _bias(b1), slope))
        c2 = conv(t1_wide, w2, 1, pad=0)
    elif variant == "conv2_dilated":
        c2 = conv(t1, w2, dil)
    else:
        c2 = conv(t1, w2, 1)
    c2b = c2 + _bias(b2)
    y = x + c2b
    pre = out_scale * y + (base.to(F64) if base is not None else 0.0)
    out = rnd(lrelu(pre, post_slope))
    if variant == "seam_shifted":
        out = out.clone()
        hi = min(2 * tt, out.shape[1])
        out[:, tt:hi] = out[:, tt - 1:hi - 1].clone()
    if stages is not None:
        stages.update(xa=xa, c1=c1, t1=t1, c2b=c2b, y=y, pre=pre, out=out,
                      abs1=conv(xa.abs(), w1.abs(), dil) + _bias(b1.abs()),
                      abs2=conv(t1.abs(), w2.abs(), 1) + _bias(b2.abs()) + x.abs())
    return out


def branch_ref(x, ws, bs, dils, slope, post_slope=1.0, out_scale=1.0, base=None, rounded=False, stages=None):
    """Three chained pairs: ws / bs = [w1, w2] / [b1, b2] of pair 0, 1, 2; scale, post and base on the last pair only; y(p) rounded
    between the pairs where the pair kernel stores it."""
    y = x.to(F64)
    n = len(dils)
    for p in range(n):
        last = p == n - 1
        st = {} if stages is not None else None
        y = pair_ref(y, ws[2 * p], bs[2 * p], ws[2 * p + 1], bs[2 * p + 1], dils[p], slope, post_slope if last else 1.0,
                     out_scale if last else 1.0, base if last else None, rounded, stages=st)
        if stages is not None:
            stages[p] = st
    return y


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _sparse_int(shape, lo, hi, density, g):
    v = torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    return v * (torch.rand(shape, generator=g) < density)


def _rows_exact(C, ks, n, g):
    """[C][C][ks] of {-1, 0, 1} with exactly n non-zero weights per output channel (no Poisson tail: the growth of a chain is bounded)"""
    pos = torch.rand(C, C * ks, generator=g).argsort(dim=1)[:, :n]
    sign = torch.randint(0, 2, (C, n), generator=g).to(F64) * 2 - 1
    return torch.zeros(C, C * ks, dtype=F64).scatter_(1, pos, sign).view(C, C, ks)


def lattice(C, ks, B, T, n_pairs=1, x_density=0.25, w_per_row=3.0, w1_unit=2, exact_rows=None, seed=0):
    """x [B][T][C], ws [2 n_pairs] x [C][C][ks], bs [2 n_pairs] x [C], base [B][T][C], all float64 integers on the lattice of the
    module docstring.  w_per_row: expected non-zero weights per output channel of one convolution; w1_unit: the step of conv1's
    weights (the activated input is even, so 1 keeps conv1 + b1 even as well)."""
    g = _gen(C, ks, n_pairs, seed)
    dens = w_per_row / (C * ks)
    ws, bs = [], []
    for _ in range(n_pairs):
        if exact_rows:  # (n1, n2): exactly that many non-zero weights per output channel of conv1 / conv2
            ws += [w1_unit * _rows_exact(C, ks, exact_rows[0], g), 4 * _rows_exact(C, ks, exact_rows[1], g)]
        else:
            ws += [w1_unit * _sparse_int((C, C, ks), -1, 1, dens * 1.5, g), 4 * _sparse_int((C, C, ks), -1, 1, dens * 1.5, g)]
        bs += [2 * torch.randint(-1, 2, (C,), generator=g).to(F64), 4 * torch.randint(-1, 2, (C,), generator=g).to(F64)]
    gx = _gen(C, ks, n_pairs, seed, B, 7)  # one stream of rows: a shorter T is a prefix of a longer one
    x = 4 * _sparse_int((B, 2048, C), -2, 2, x_density * 1.25, gx)[:, :T].contiguous()
    base = 4 * torch.randint(-2, 3, (B, 2048, C), generator=gx).to(F64)[:, :T].contiguous()
    return x, ws, bs, base


def _representable(name, t):
    assert torch.equal(bf16(t), t), f"lattice: {name} is not representable in bf16 (max |v| = {float(t.abs().max())})"


def check_lattice(x, ws, bs, dils, slope, post_slope, out_scale, base):
    """Asserts, for this very case, that bf16 arithmetic is exact: every quantity a kernel rounds (the activated input, the
    intermediate, conv2 + b2 -- the 128-channel kernel stages it in bf16 --, y(p), the output) is representable, and the sum of
    absolute products of every accumulation stays below 2**24, so fp32 sums are exact in any order.  Returns the float64 output."""
    stages = {}
    out = branch_ref(x, ws, bs, dils, slope, post_slope, out_scale, base, rounded=False, stages=stages)
    for t, name in ((x, "x"), (base, "base")) + tuple((w, "w") for w in ws):
        if t is not None:
            _representable(name, t)
    for p in range(len(dils)):
        st = stages[p]
        for name in ("xa", "t1", "c2b", "y", "out"):
            _representable(f"pair {p} {name}", st[name])
        worst = max(float(st["abs1"].max()), float(st["abs2"].max()), float(st["pre"].abs().max()) * 2)
        assert worst < 2 ** 24, f"lattice: absolute sum {worst} of pair {p} is not below 2**24"
    return out


def random_problem(C, ks, B, T, n_pairs=1, seed=0):
    """bf16-representable normals; dense weights scaled 1.5 / sqrt(C ks) as the neighbouring layer tests do"""
    g = _gen(C, ks, n_pairs, seed, 99)
    x = bf16(torch.randn(B, T, C, generator=g, dtype=F64))
    ws = [bf16(torch.randn(C, C, ks, generator=g, dtype=F64) * (1.5 / (C * ks) ** 0.5)) for _ in range(2 * n_pairs)]
    bs = [(torch.randn(C, generator=g, dtype=F64) * 0.1).to(torch.float32).to(F64) for _ in range(2 * n_pairs)]  # (fp32 on the device)
    base = bf16(torch.randn(B, T, C, generator=g, dtype=F64))
    return x, ws, bs, base


# ---- the cases of tests/test_gpu_resblock_fused.py (a): the host file checks the lattice assertions and the sensitivity on the same ---
PAIR_ENTRIES = [(64, 3), (64, 7), (64, 11), (32, 3), (32, 7), (32, 11), (128, 3)]
BRANCH_ENTRIES = [(32, 3), (32, 7), (64, 3)]
COMBOS = [(acc, post, scale) for acc in (0, 1) for post in (1.0, 0.5) for scale in (1.0, 0.5)]
LATTICE_SLOPE = 0.5


def pair_dilations(C):
    return (1, 5) if C == 128 else (1, 3, 5)


def pair_lengths(ks, tt):
    """the smallest T at which each mechanism is live: one row, shorter than the halo, the seam, a last tile of halo-deep rows"""
    h2 = (ks - 1) // 2
    return [1, h2 + 1, tt - 1, tt, tt + 1, 2 * tt + h2]


def branch_lengths(tt):
    return [1, tt - 1, tt, tt + 1, 2 * tt + 1]


def pair_runs(C, ks, dil, tt):
    """(T, accumulate, post_slope, out_scale) of the eight runs of one (entry, dilation): every combination once, every T at least once"""
    Ts = pair_lengths(ks, tt)
    shift = pair_dilations(C).index(dil) * 2
    return [(Ts[(i + shift) % len(Ts)],) + COMBOS[i] for i in range(len(COMBOS))]


def branch_runs(tt, k):
    Ts = branch_lengths(tt)
    return [(Ts[(i + 2 * k) % len(Ts)],) + COMBOS[i] for i in range(len(COMBOS))]


# The branch lattice: three chained pairs multiply the values (|y(p+1)| <= 5 |y(p)| + 12 with one weight per row and convolution),
# and the draw of one pair overflows the bf16 integer range at pair 2.  One non-zero weight per output channel and convolution, of
# step 1 in conv1 (its operand is even already), keeps check_lattice's assertions for every triple and length; every tap of every
# convolution still carries a weight (test_resblock_ref_host.py asserts it), and a row, tap or channel moved by one changes the output.
BRANCH_LATTICE = dict(x_density=0.25, w1_unit=1, exact_rows=(1, 1))
B_LATTICE = 3

# the tile walk: one k = 3 and one k = 11 pair entry (every branch entry with (1, 3, 5))
WALK_PAIRS = [(64, 3, 3), (32, 11, 5)]


def walk_problems(tt, ks):
    """(B, T, n_cu): 9 tiles on the device's grid and on 8 workgroups (five XCD ranges occupied, four workgroups walk two tiles with
    the register prefetch live); 40 tiles on 16 workgroups (the two slots of an XCD walk 3 and 2 tiles); one tile (seven empty ranges)"""
    return [(3, 2 * tt + ks, 0), (3, 2 * tt + ks, 8), (10, 3 * tt + 7, 16), (10, 3 * tt + 7, 0), (1, tt - 3, 0), (1, tt - 3, 8)]
# per branch entry: the generator's own triple, one with d0 > d1 (the tile loads by d0, the reach grows by every d), and the smallest
BRANCH_TRIPLES = {e: [(1, 3, 5), (3, 1, 5), (1, 1, 1)] for e in BRANCH_ENTRIES}


# ---- one plain convolution on the lattice (the narrow / wide tiles of the time-major convolution) ------------------------------------
def conv_tc_lattice(C, ks, B, T, seed=0):
    """x [B][T][C], w [C][C][ks], b [C]: small integers, three non-zero weights per output channel on average"""
    g = _gen(C, ks, seed, 5)
    w = _sparse_int((C, C, ks), -2, 2, 3.0 * 1.25 / (C * ks), g)
    b = torch.randint(-3, 4, (C,), generator=g).to(F64)
    x = _sparse_int((B, T, C), -4, 4, 0.3, _gen(C, ks, seed, B, 6)).to(torch.float32)
    return x, w, b


def check_conv_lattice(x, w, b, dil):
    """the same two assertions for bias + conv(x): returns the exact result, computed in fp32 (exact below 2**24 in any order)"""
    xf, wf, bf = x.to(torch.float32), w.to(torch.float32), b.to(torch.float32)
    worst = float((conv(xf.abs(), wf.abs(), dil) + _bias(bf.abs())).max())
    assert worst < 2 ** 24, f"lattice: absolute sum {worst} is not below 2**24"
    want = conv(xf, wf, dil) + _bias(bf)
    for name, t in (("x", xf), ("w", wf), ("out", want)):
        assert torch.equal(t.to(torch.bfloat16).to(torch.float32), t), f"lattice: {name} is not representable in bf16"
    return want
