"""The FastSpeech2 forward kernels (csrc/fs2_ops.hip), one entry point at a time, at the boundaries of the path the launcher picks:
the three template sizes of layernorm_cbt_kernel (switching at C = 64 / 256 / 1024) with column counts around its 64-column
workgroup, depthwise taps around an item's ends, bin edges, rounding ties of the durations, the length regulator's zero durations,
the attention kernel's query tile of 128 and key tile of 32, and the refusals.

Assertions as in tests/test_gpu_primitives.py: (a) position probes bit for bit, (b) float64 references with a bound evaluated per
element from the operation (gamma_n sum |term|, MATH_ULP per device math call; no bound comes from a kernel's output), (c) torch.equal
where the arithmetic is exact (selection, data movement, one correctly rounded operation)."""

import math

import pytest
import torch
import torch.nn.functional as F

from everyvoice_amd import _lib
from helpers import E, NAN, U, assert_within, f32, gamma, same_bits

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = 1, _lib.EVMI_ERR_UNSUPPORTED
SENTINEL = -1234.5


def call(fn, *args):
    """fn(...) with tensors passed as their pointers (None as NULL); the tensors stay referenced until the launch has been issued --
    a temporary `t.to(dev)` dropped earlier would hand its block to the next allocation."""
    return fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else 0 if a is None else a for a in args])


def stream(dev):
    return _lib.current_stream_ptr(dev)


def i32(values, dev):
    return torch.tensor(list(values), dtype=torch.int32, device=dev)


def lib():
    return _lib.load()


# =====================================================================================================================
# LayerNorm over channels
# =====================================================================================================================
# C 1, 3, 5, 64: layernorm_cbt_kernel<16> (C = 1 and 3 leave slices empty, 5 and 65 a short last slice; 64 fills 4 x 16);
# C 65, 255, 256: <64>;  C 257, 1023, 1024: <256> (1024 fills 4 x 256).  n_cols 1 / 63 / 64 / 65 / 130: one partly filled workgroup,
# one lane short, exactly one, one column into the second, a third workgroup with 2 columns.
LN_CASES = [(C, n) for C in (1, 3, 5, 64, 65, 255, 256, 257) for n in (1, 63, 64, 65, 130)] + [(C, n) for C in (1023, 1024) for n in (1, 65)]
LN_EPS = f32(1e-5)


def test_layernorm_template_rule_restated():
    cpt = lambda C: 16 if C <= 64 else 64 if C <= 256 else 256 if C <= 1024 else None  # noqa: E731
    assert {cpt(C) for C, _ in LN_CASES} == {16, 64, 256} and cpt(1025) is None
    assert [cpt(C) for C in (64, 65, 256, 257, 1024)] == [16, 64, 64, 256, 256]
    for C, _ in LN_CASES:  # every slice of ceil(C / 4) channels fits the thread's registers
        assert (C + 3) // 4 <= cpt(C)


@pytest.mark.parametrize("C,n_cols", LN_CASES)
def test_layernorm_cbt(cuda_device, C, n_cols):
    """Against float64 layer_norm.  mean: a sum of C terms and a division, d_m = gamma(C) sum|x| / C + u |mean|; deviations d = x - mean:
    d_d = d_m + u |d|; var = sum d^2 / C: the squares move by 2 |d| d_d + d_d^2, the sum costs gamma(C + 1) var; rstd = 1 / sqrtf(var +
    eps): half the relative error of its argument plus 3 roundings (sum, root, division: correctly rounded); y = d rstd gamma + beta:
    three more roundings and one of the result.  One column is constant: var = 0, rstd = 1 / sqrt(eps) multiplies whatever d is.
    Behind the last channel's row lie 64 floats that no column of the last workgroup may reach."""
    dev = cuda_device
    g = torch.Generator().manual_seed(C * 1000 + n_cols)
    x = torch.randn(C, n_cols, generator=g) * 2 + 0.5
    x[:, n_cols // 2] = 0.75
    gam, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    y = torch.full((C * n_cols + 64,), SENTINEL, device=dev)
    rc = call(lib().evmi_layernorm_cbt_f32, x.to(dev), gam.to(dev), beta.to(dev), y, C, n_cols, LN_EPS, stream(dev))
    assert rc == _lib.EVMI_OK
    y = y.cpu()
    assert (y[C * n_cols :] == SENTINEL).all(), "a column past n_cols was written"
    x64 = x.double()
    want = F.layer_norm(x64.t(), (C,), gam.double(), beta.double(), LN_EPS).t()
    mean = x64.mean(0, keepdim=True)
    d = x64 - mean
    var = (d * d).mean(0, keepdim=True)
    d_m = gamma(C) * x64.abs().sum(0, keepdim=True) / C + U * mean.abs()
    d_d = d_m + U * d.abs()
    d_var = (2 * d.abs() * d_d + d_d * d_d).mean(0, keepdim=True) + gamma(C + 1) * var
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    rel_rstd = 0.5 * d_var / (var + LN_EPS) + 3 * U
    core = (d.abs() * rel_rstd + d_d * (1 + rel_rstd)) * rstd * gam.double().abs()[:, None]
    bound = core + 3 * U * (d * rstd * gam.double()[:, None]).abs() + U * want.abs()
    assert_within(y[: C * n_cols].view(C, n_cols), want, bound, f"layernorm C {C} n_cols {n_cols}")


def test_layernorm_cbt_refuses_more_than_1024_channels(cuda_device):
    dev = cuda_device
    x, p = torch.zeros(1025, 2, device=dev), torch.zeros(1025, device=dev)
    y = torch.full((1025, 2), SENTINEL, device=dev)
    assert call(lib().evmi_layernorm_cbt_f32, x, p, p, y, 1025, 2, LN_EPS, stream(dev)) == UNSUPPORTED
    assert (y == SENTINEL).all()
    for C, n in ((0, 2), (4, 0)):
        assert call(lib().evmi_layernorm_cbt_f32, x, p, p, y, C, n, LN_EPS, stream(dev)) == INVALID_ARG


# =====================================================================================================================
# depthwise convolution
# =====================================================================================================================
# k 1: no neighbours; 3 / 9 / 31 with T 1, 2, k - 1 (every output sees both ends), k, 70 (interior outputs; C B T = 1050: 5 workgroups)
DW_CASES = sorted({(k, T) for k in (1, 3, 9, 31) for T in (1, 2, k - 1, k, 70) if T >= 1})
DW_B, DW_C = 3, 5


def run_dwconv(dev, x, w, bias, k, act):
    C, B, T = x.shape
    y = torch.full((C, B, T), NAN, device=dev)
    rc = call(lib().evmi_dwconv1d_cbt_f32, x.to(dev), w.to(dev), None if bias is None else bias.to(dev), y,
                                     C, B, T, k, (k - 1) // 2, act, stream(dev))
    assert rc == _lib.EVMI_OK
    return y.cpu()


@pytest.mark.parametrize("k,T", DW_CASES)
def test_dwconv1d_cbt(cuda_device, k, T):
    """Against float64 conv1d(groups = C) per item: bias and k products in one FMA chain, gamma(k + 1) of their magnitudes.  SiLU
    v / (1 + expf(-v)) has slope <= 1.1 in v and costs E + 3 u of its value (expf, the sum, the division); ReLU is exact."""
    g = torch.Generator().manual_seed(100 * k + T)
    x = torch.randn(DW_C, DW_B, T, generator=g)
    w, b = torch.randn(DW_C, k, generator=g), torch.randn(DW_C, generator=g)
    pad = (k - 1) // 2
    xb = x.double().permute(1, 0, 2)  # [B, C, T]
    for bias in (b, None):
        pre = F.conv1d(xb, w.double()[:, None, :], None if bias is None else bias.double(), padding=pad, groups=DW_C).permute(1, 0, 2)
        mag = F.conv1d(xb.abs(), w.double().abs()[:, None, :], None if bias is None else bias.double().abs(), padding=pad, groups=DW_C).permute(1, 0, 2)
        d_pre = gamma(k + 1) * mag
        for act in (0, 1, 2):
            got = run_dwconv(cuda_device, x, w, bias, k, act)
            if act == 0:
                want, bound = pre, d_pre
            elif act == 1:
                want = pre * torch.sigmoid(pre)
                bound = 1.1 * d_pre + (E + 3 * U) * want.abs()
            else:
                want, bound = pre.clamp_min(0), d_pre
            assert_within(got, want, bound, f"dwconv k {k} T {T} act {act} bias {bias is not None}")


@pytest.mark.parametrize("k,T", DW_CASES)
def test_dwconv1d_cbt_item_boundary_probe(cuda_device, k, T):
    """x = one 1.0 at the last frame of item 0 and one 2.0 at frame 0 of item 1; no bias, no activation: item 0 holds w[c][j] where
    t + j - pad = T - 1, item 1 holds 2 w[c][j] where t + j - pad = 0 (exact: one product with a power of two), everything else,
    item 2 included, is exactly 0.  A tap that crosses an item boundary (k > T makes every tap a candidate) puts a weight there."""
    g = torch.Generator().manual_seed(k + T)
    w = torch.randn(DW_C, k, generator=g)
    pad = (k - 1) // 2
    x = torch.zeros(DW_C, DW_B, T)
    x[:, 0, T - 1] += 1.0
    x[:, 1, 0] += 2.0  # (T = 1: two different items, still one impulse each)
    want = torch.zeros(DW_C, DW_B, T)
    for t in range(T):
        j0, j1 = T - 1 - t + pad, 0 - t + pad
        if 0 <= j0 < k:
            want[:, 0, t] = w[:, j0]
        if 0 <= j1 < k:
            want[:, 1, t] = 2.0 * w[:, j1]
    got = run_dwconv(cuda_device, x, w, None, k, 0)
    assert torch.equal(got, want), (got - want).abs().max()
    assert (got[:, 2] == 0.0).all()


# =====================================================================================================================
# embedding, positional sinusoid, column mask, per-item embedding
# =====================================================================================================================
# D 2: one frequency; 6: three (c < h and c >= h both several wide); 256: the model's.  L 1 / 255 / 257: D B L crosses workgroups at
# every D; 2048 (D 6 only): positions up to 2047, the argument of sinf reaches 2047 rad
EMB_CASES = [(D, L) for D in (2, 6, 256) for L in (1, 255, 257)] + [(6, 2048)]


def emb_lens(L):
    return [0, 1, L]


def inv_freq_of(D):
    from oracle.fs2_ref import PositionalEmbeddingRef

    return PositionalEmbeddingRef(D).inv_freq.clone()


def pe64(n, inv_freq):
    """(float64 sin | cos of the fp32-ROUNDED product float(l) * inv_freq -- the kernel's argument, exactly --, the same with |.|)"""
    ang = (torch.arange(n, dtype=torch.float32)[:, None] * inv_freq[None, :]).double()  # one correctly rounded fp32 product each
    return torch.cat([ang.sin(), ang.cos()], 1).t()  # [D, n]


@pytest.mark.parametrize("D,L", EMB_CASES)
def test_fs2_embed(cuda_device, D, L):
    """Table rows are selected exactly (inv_freq = NULL: the bare embedding); with the sinusoid: MATH_ULP of it and the rounding of the
    sum; padded columns are exactly 0 (the buffer starts as NaN)."""
    dev = cuda_device
    lens = emb_lens(L)
    B, V = len(lens), 11
    g = torch.Generator().manual_seed(D * L)
    ids = torch.randint(0, V, (B, L), generator=g, dtype=torch.int32)
    ids[2, 0], ids[2, -1] = V - 1, 0
    table = torch.randn(V, D, generator=g)
    inv_freq = inv_freq_of(D)
    valid = torch.arange(L)[None, :] < torch.tensor(lens)[:, None]  # [B, L]
    rows = table[ids.long()].permute(2, 0, 1)  # [D, B, L]
    for with_pe in (False, True):
        out = torch.full((D, B, L), NAN, device=dev)
        rc = call(lib().evmi_fs2_embed_f32, ids.to(dev), i32(lens, dev), table.to(dev),
                                      inv_freq.to(dev) if with_pe else 0, out, B, L, D, stream(dev))
        assert rc == _lib.EVMI_OK
        out = out.cpu()
        assert (out[:, ~valid] == 0.0).all()
        if not with_pe:
            assert torch.equal(out, rows * valid[None])
        else:
            pe = pe64(L, inv_freq)[:, None, :]
            want = (rows.double() + pe) * valid[None]
            assert_within(out, want, (E * pe.abs() + U * want.abs()) * valid[None], f"fs2_embed D {D} L {L}")


@pytest.mark.parametrize("D,L", EMB_CASES)
def test_fs2_add_posemb_mask_cols_item_embedding(cuda_device, D, L):
    dev = cuda_device
    lens = emb_lens(L)
    B = len(lens)
    g = torch.Generator().manual_seed(D + L)
    x = torch.randn(D, B, L, generator=g)
    valid = torch.arange(L)[None, :] < torch.tensor(lens)[:, None]
    inv_freq = inv_freq_of(D)
    # add_posemb: x + pe on the valid columns, exactly 0 on the padded ones
    xd = x.to(dev)
    assert call(lib().evmi_fs2_add_posemb_f32, xd, i32(lens, dev), inv_freq.to(dev), B, L, D, stream(dev)) == _lib.EVMI_OK
    got = xd.cpu()
    assert (got[:, ~valid] == 0.0).all()
    pe = pe64(L, inv_freq)[:, None, :]
    want = (x.double() + pe) * valid[None]
    assert_within(got, want, (E * pe.abs() + U * want.abs()) * valid[None], f"add_posemb D {D} L {L}")
    # mask_cols: selection
    xd = x.to(dev)
    assert call(lib().evmi_mask_cols_f32, xd, i32(lens, dev), D, B, L, stream(dev)) == _lib.EVMI_OK
    assert same_bits(xd.cpu(), torch.where(valid[None], x, torch.zeros(())))
    # add_item_embedding: one correctly rounded addition on the valid columns, the padded ones untouched
    table = torch.randn(4, D, generator=g)
    item = [3, 0, 2]
    xd = x.to(dev)
    assert call(lib().evmi_fs2_add_item_embedding_f32, xd, i32(item, dev), i32(lens, dev), table.to(dev), B, L, D,
                                                 stream(dev)) == _lib.EVMI_OK
    assert same_bits(xd.cpu(), torch.where(valid[None], x + table[item].t()[:, :, None], x))


def test_fs2_posemb_matches_oracle_at_position_2047(cuda_device):
    """With the oracle's inv_freq the kernel's sinusoid at the last of 2048 positions equals the oracle's position embedding within the
    bound of test_fs2_embed (zeros in, so the sum adds nothing)."""
    from oracle.fs2_ref import PositionalEmbeddingRef

    dev, D, L = cuda_device, 6, 2048
    ref = PositionalEmbeddingRef(D)
    x = torch.zeros(D, 1, L, device=dev)
    assert call(lib().evmi_fs2_add_posemb_f32, x, i32([L], dev), ref.inv_freq.to(dev), 1, L, D, stream(dev)) == _lib.EVMI_OK
    want = ref(L).t().double()  # [D, L]
    assert_within(x.cpu()[:, 0, 2047], want[:, 2047], E * want[:, 2047].abs() + U * want[:, 2047].abs(), "posemb vs oracle at 2047")
    assert_within(x.cpu()[:, 0], want, E * want.abs() + U * want.abs(), "posemb vs oracle")


# =====================================================================================================================
# variance bucketise + embedding add
# =====================================================================================================================
# n_bins 2: a single edge (the search loop does not run: lo == hi == ... one comparison); 3: two; 256 / 257: a full tree and one more
@pytest.mark.parametrize("control", [1.0, 1.3])
@pytest.mark.parametrize("n_bins", [2, 3, 256, 257])
def test_fs2_bucket_embed_add(cuda_device, n_bins, control):
    """Exact: x + table[bucketize(fp32(values * control), bins)] -- the bucket is the number of edges strictly below the value, the sum one
    correctly rounded addition.  values: every edge, its two fp32 neighbours, below the first and above the last edge, +-inf.
    (NaN is left out: torch.bucketize puts it past the last edge, the kernel's `bins[mid] < v` is false for it and gives bucket 0; the
    product never produces one -- the predictors' outputs are finite and control is a finite factor.)"""
    dev, D = cuda_device, 3
    bins = torch.linspace(-2.0, 3.0, n_bins - 1)
    inf = torch.tensor(float("inf"))
    values = torch.cat([bins, torch.nextafter(bins, inf), torch.nextafter(bins, -inf), torch.tensor([-2.5, -1e30, 3.5, 1e30, float("inf"), float("-inf"), 0.0])])
    if control != 1.0:  # the same set seen through the product: values whose fp32 product lands on / next to the edges
        c = torch.tensor(control, dtype=torch.float32)
        values = torch.cat([values, values / c, torch.nextafter(values / c, inf), torch.nextafter(values / c, -inf)])
    B, L = 1, len(values)
    g = torch.Generator().manual_seed(n_bins)
    x, table = torch.randn(D, B, L, generator=g), torch.randn(n_bins, D, generator=g)
    xd = x.to(dev)
    rc = call(lib().evmi_fs2_bucket_embed_add_f32, xd, values.to(dev), bins.to(dev), table.to(dev), n_bins, B, L, D,
                                             control, stream(dev))
    assert rc == _lib.EVMI_OK
    bucket = torch.bucketize(values * torch.tensor(control, dtype=torch.float32), bins)
    assert int(bucket.min()) == 0 and int(bucket.max()) == n_bins - 1
    assert set(bucket.tolist()) == set(range(n_bins)), "every bucket is hit"
    assert same_bits(xd.cpu(), x + table[bucket].t()[:, None, :])


# =====================================================================================================================
# durations
# =====================================================================================================================
DUR_CONTROLS = [0.5, 1.0, 1.3]


def durations_ref64(log_d, control):
    """The oracle's rule, clamp(round(exp(log_d) - 1) * control, min = 0).long(), in float64 with control as the c_float the kernel gets."""
    return torch.clamp(torch.round(torch.exp(log_d.double()) - 1.0) * f32(control), min=0).long()


def run_durations(dev, log_d, lens, control):
    B, L = log_d.shape
    dur = torch.full((B, L), -7, dtype=torch.int32, device=dev)
    assert call(lib().evmi_fs2_durations_i32, log_d.to(dev), i32(lens, dev), dur, B, L, control, stream(dev)) == _lib.EVMI_OK
    return dur.cpu()


@pytest.mark.parametrize("control", DUR_CONTROLS)
def test_fs2_durations_exact_values(cuda_device, control):
    """exp(-inf) - 1 = -1 and exp(-3) - 1 round to -1: clamped to 0; 0 -> 0; log 2 -> 1; log 3.5 -+ 1e-2 -> 2 | 3 on the two sides of the
    tie; then the product with control is truncated.  Padded tokens are 0.
    log_d = 20 is there for the range (4.85e8 frames, no overflow of the int): at that size one ulp of expf is 32 frames, so this one
    entry is held to MATH_ULP of the float64 value instead of to the integer."""
    vals = [float("-inf"), -3.0, 0.0, math.log(2.0), math.log(3.5) - 1e-2, math.log(3.5) + 1e-2, 20.0]
    rounded = [0, 0, 0, 1, 2, 3]
    want = [int(r * f32(control)) for r in rounded]
    log_d = torch.tensor([vals, vals], dtype=torch.float32)
    got = run_durations(cuda_device, log_d, [len(vals), 3], control)
    assert got[0, :6].tolist() == want, (got[0].tolist(), want)
    big = float(torch.round(torch.exp(torch.tensor(20.0, dtype=torch.float64)) - 1.0)) * f32(control)
    assert abs(int(got[0, 6]) - big) <= (E + 2 * U) * big + 1, (int(got[0, 6]), big)
    assert got[1, :3].tolist() == want[:3] and got[1, 3:].tolist() == [0, 0, 0, 0]
    assert durations_ref64(log_d[0, :6], control).tolist() == want


DUR_SEED, DUR_B, DUR_L = 4, 4, 1024
DUR_LENS = [1024, 0, 1, 700]


def durations_random_case(control):
    """log_d ~ N(1, 0.6^2): durations 0 .. about 15.  Left out: exp(log_d) - 1 within 1e-3 of a tie n + 1/2 (fp32 expf may round to the
    other side), and, for control != 1, a scaled value within 1e-3 of an integer WITHOUT being one (r * 1.3f: the fp32 product may round
    up to the integer that float64 truncates below; an exact integer -- every r * 0.5 with even r -- is exact in both)."""
    g = torch.Generator().manual_seed(DUR_SEED)
    log_d = torch.randn(DUR_B, DUR_L, generator=g) * 0.6 + 1.0
    v = torch.exp(log_d.double()) - 1.0
    keep = ((v - torch.floor(v)) - 0.5).abs() > 1e-3
    scaled = torch.round(v) * f32(control)
    off = (scaled - torch.round(scaled)).abs()
    keep &= (off == 0) | (off > 1e-3)
    valid = torch.arange(DUR_L)[None, :] < torch.tensor(DUR_LENS)[:, None]
    return log_d, torch.where(valid, durations_ref64(log_d, control), torch.zeros(DUR_B, DUR_L, dtype=torch.long)), keep


@pytest.mark.parametrize("control", DUR_CONTROLS)
def test_fs2_durations_exclusions_are_few(control):
    """No GPU: the reference alone leaves out at most 1 % of the 4096 elements (the seed was picked for that)."""
    _, want, keep = durations_random_case(control)
    assert keep.numel() == 4096 and int((~keep).sum()) <= 40, int((~keep).sum())
    assert int(want.max()) >= 8 and int((want == 0).sum()) > 0


@pytest.mark.parametrize("control", DUR_CONTROLS)
def test_fs2_durations_random(cuda_device, control):
    log_d, want, keep = durations_random_case(control)
    got = run_durations(cuda_device, log_d, DUR_LENS, control).long()
    assert int((~keep).sum()) <= 40
    assert torch.equal(got[keep], want[keep]), torch.nonzero((got != want) & keep)[:8].tolist()
    assert (got[1] == 0).all() and (got[2, 1:] == 0).all() and (got[3, 700:] == 0).all()


# =====================================================================================================================
# length regulator
# =====================================================================================================================
@pytest.mark.parametrize("slack", [0, 9])
@pytest.mark.parametrize("L", [1, 33])
@pytest.mark.parametrize("C", [1, 7])
def test_length_regulate_cbt(cuda_device, C, L, slack):
    """Exact against repeat_interleave per item, zero padded to T.  Durations with zeros in front, in the middle and at the end (the
    binary search over equal prefix sums), one item all zeros (cum[L - 1] = 0: nothing but padding); T = the largest total, or 9 more."""
    dev = cuda_device
    g = torch.Generator().manual_seed(C * 100 + L)
    B = 4
    dur = torch.randint(1, 6, (B, L), generator=g)
    if L > 1:
        dur[0, :3], dur[0, 15:18], dur[0, -2:] = 0, 0, 0
        dur[1, 0], dur[1, -1] = 0, 7
        dur[3] = 1
    dur[2] = 0
    x = torch.randn(C, B, L, generator=g)
    T = int(dur.sum(1).max()) + slack
    want = torch.zeros(C, B, T)
    for b in range(B):
        rep = torch.repeat_interleave(x[:, b], dur[b], dim=1)
        want[:, b, : rep.shape[1]] = rep
    cum = torch.cumsum(dur, 1).to(torch.int32)
    out = torch.full((C, B, T), NAN, device=dev)
    assert call(lib().evmi_length_regulate_cbt_f32, x.to(dev), cum.to(dev), out, C, B, L, T, stream(dev)) == _lib.EVMI_OK
    assert same_bits(out.cpu(), want)


# =====================================================================================================================
# fused self-attention at its tile edges
# =====================================================================================================================
# T 1: one query, one key;  32 | 33: one key tile, and one key into the second;  128 | 129: one query tile (4 waves x 32), and one query
# into a second workgroup;  257: three query tiles, nine key tiles.  lens from {0, 1, 32, 33, T}: no key, one, a full tile, one more, all.
ATT_T = [1, 32, 33, 128, 129, 257]


@pytest.mark.parametrize("T", ATT_T)
@pytest.mark.parametrize("dh", [32, 64, 128])
def test_attention_cbt_tile_edges(cuda_device, dh, T):
    """Against float64 softmax attention (every query row, padded ones included, attends to the keys below the item's length).
    score: the scaled query (u) in a dot product of dh terms: d_s = (gamma(dh) + 2 u) sum |q k| scale.  A probability expf(s - m) moves by
    e^(2 d_s) with the scores, costs E + u R (expf and its argument, R = the row's range) and then up to one correction factor per
    key tile, each E + u R + u: eps = 2 max d_s + (tiles + 1) (E + u R + u).  Numerator and denominator are sums of len such terms:
    (eps + gamma(len)) each, the final product 2 u:  |o - o64| <= (2 (eps + gamma(len)) + 2 u) sum_j P_j |v_j|.
    An item of length 0 has all-zero rows, not NaN."""
    dev, H = cuda_device, 2
    D = H * dh
    lens = sorted({n for n in (0, 1, 32, 33, T) if n <= T})
    B = len(lens)
    g = torch.Generator().manual_seed(dh * 1000 + T)
    qkv = torch.randn(3 * D, B, T, generator=g)
    out = torch.full((D, B, T), NAN, device=dev)
    assert call(lib().evmi_attention_cbt_f32, qkv.to(dev), i32(lens, dev), out, B, T, D, H, stream(dev)) == _lib.EVMI_OK
    out = out.cpu()
    assert torch.isfinite(out).all()
    scale = f32(1.0 / math.sqrt(dh))
    q, k, v = (qkv[i * D : (i + 1) * D].double().view(H, dh, B, T).permute(2, 0, 3, 1) for i in range(3))  # [B, H, T, dh]
    for b, n in enumerate(lens):
        got = out[:, b].reshape(H, dh, T).permute(0, 2, 1)  # [H, T, dh]
        if n == 0:
            assert (got == 0.0).all(), "an item without keys"
            continue
        s = torch.einsum("htd,hkd->htk", q[b], k[b, :, :n]) * scale
        s_abs = torch.einsum("htd,hkd->htk", q[b].abs(), k[b, :, :n].abs()) * scale
        d_s = ((gamma(dh) + 2 * U) * s_abs).max(2, keepdim=True).values
        R = s.max(2, keepdim=True).values - s.min(2, keepdim=True).values
        tiles = (n + 31) // 32
        eps = torch.expm1(2 * d_s) + (tiles + 1) * (E + U * R + U)
        P = torch.softmax(s, 2)
        want = torch.einsum("htk,hkd->htd", P, v[b, :, :n])
        bound = (2 * (eps + gamma(n)) + 2 * U) * torch.einsum("htk,hkd->htd", P, v[b, :, :n].abs())
        assert_within(got, want, bound, f"attention dh {dh} T {T} len {n}")


def test_attention_cbt_refusals(cuda_device):
    dev = cuda_device
    z, out = torch.zeros(3 * 48, 1, 4, device=dev), torch.full((48, 1, 4), SENTINEL, device=dev)
    lens = i32([4], dev)
    assert call(lib().evmi_attention_cbt_f32, z, lens, out, 1, 4, 48, 1, stream(dev)) == UNSUPPORTED  # d_head 48
    assert call(lib().evmi_attention_cbt_f32, z, lens, out, 1, 4, 48, 5, stream(dev)) == INVALID_ARG  # 48 % 5
    assert (out == SENTINEL).all()


# =====================================================================================================================
# refusals of the pointwise entry points
# =====================================================================================================================
def test_pointwise_entry_points_refuse_bad_shapes(cuda_device):
    """Non-positive sizes and (for the sinusoid, whose second half reads inv_freq[c - D / 2]) an odd D: EVMI_ERR_INVALID_ARG before
    any launch -- the buffers keep their sentinel."""
    dev, L_ = cuda_device, lib()
    x = torch.full((8, 2, 4), SENTINEL, device=dev)  # D 8 (or less), B 2, L 4
    lens, ids = i32([4, 2], dev), torch.zeros(2, 4, dtype=torch.int32, device=dev)
    table, inv_freq, vals, bins = torch.ones(4, 8, device=dev), torch.ones(4, device=dev), torch.zeros(2, 4, device=dev), torch.zeros(3, device=dev)
    dur = torch.full((2, 4), -7, dtype=torch.int32, device=dev)
    s = stream(dev)
    for B, L, D in ((0, 4, 8), (2, 0, 8), (2, 4, 0), (-1, 4, 8), (2, -4, 8), (2, 4, -8), (2, 4, 7), (2, 4, 1)):
        assert call(L_.evmi_fs2_add_posemb_f32, x, lens, inv_freq, B, L, D, s) == INVALID_ARG, (B, L, D)
        assert call(L_.evmi_fs2_embed_f32, ids, lens, table, inv_freq, x, B, L, D, s) == INVALID_ARG
        if D in (7, 1):
            continue  # the other entry points take any positive D
        assert call(L_.evmi_mask_cols_f32, x, lens, D, B, L, s) == INVALID_ARG, (B, L, D)
        assert call(L_.evmi_fs2_bucket_embed_add_f32, x, vals, bins, table, 4, B, L, D, 1.0, s) == INVALID_ARG
        assert call(L_.evmi_fs2_add_item_embedding_f32, x, ids, lens, table, B, L, D, s) == INVALID_ARG
        if D == 8:
            assert call(L_.evmi_fs2_durations_i32, vals, lens, dur, B, L, 1.0, s) == INVALID_ARG
    assert call(L_.evmi_fs2_bucket_embed_add_f32, x, vals, bins, table, 1, 2, 4, 8, 1.0, s) == INVALID_ARG  # n_bins
    assert call(L_.evmi_dwconv1d_cbt_f32, x, table, 0, x, 8, 2, 4, 3, 1, 3, s) == INVALID_ARG  # act 3
    assert call(L_.evmi_length_regulate_cbt_f32, x, ids, x, 8, 2, 4, 0, s) == INVALID_ARG  # T 0
    torch.cuda.synchronize()
    assert (x == SENTINEL).all() and (dur == -7).all()
