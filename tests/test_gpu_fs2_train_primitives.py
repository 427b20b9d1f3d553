"""The FastSpeech2 TRAINING kernels (csrc/fs2_train_ops.hip, the head-dimension-specialised kernels of csrc/attention_train.hip), one entry
point at a time, at the boundaries of the path its launcher picks: BatchNorm's 256- / 1024-thread kernels (BN_LONG_ROW = 8192 columns) and
the prefetch / tail loops of row_walk (multiples of 8 NT), the depthwise backward's unroll tiers (k <= 4 / <= 12 / <= 32) and its staged /
direct forms (40 KiB of LDS), the table backward's chunks of 4096 tokens and tiles of 256 rows, the elementwise kernels around their
workgroup and vector widths, the attention kernels' query block of 128 and key tile of 32 -- and the dropout mask of every kernel that
draws one against tests/dropout_ref.py, the generator restated on the host, bit for bit.

Assertions as in tests/test_gpu_primitives.py and tests/test_gpu_fs2_primitives.py: (a) position probes bit for bit, (b) float64 references
with a bound evaluated per element from the operation (gamma_n sum |term|, MATH_ULP per device math call; no bound comes from a kernel's
output), (c) torch.equal where the arithmetic is exact (integer-valued inputs, selection, one correctly rounded operation).  The long sums
of these kernels (BatchNorm's statistics, the depthwise partial sums across waves and items) are accumulated in double: a double sum of n
fp32 values is off by n 2^-52 of the magnitudes (D64 below), so those sums cost ONE fp32 rounding where the result is stored, not
gamma(n).  Bounds are first order in u (the dropped second-order terms are below 1e-6 of the kept ones at these sizes).  Outputs start as
NaN / a sentinel with a guard band behind them; accumulated outputs (dgamma, dbeta, dw, db, dtable) start from known non-zero values.
Every case list has a host test (`*_rule_restated`) that restates the launcher's selection and shows that the list reaches each branch."""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

import dropout_ref
from everyvoice_amd import _lib
from helpers import E, NAN, U, assert_within, f32, gamma, same_bits

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = 1, _lib.EVMI_ERR_UNSUPPORTED
SENTINEL = -1234.5
GUARD = 64
UB = 2.0 ** -8  # unit roundoff of bf16


def call(fn, *args):
    """fn(...) with tensors passed as their pointers (None as NULL); the tensors stay referenced until the launch has been issued."""
    return fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else 0 if a is None else a for a in args])


def stream(dev):
    return _lib.current_stream_ptr(dev)


def i32(values, dev):
    return torch.tensor(list(values), dtype=torch.int32, device=dev)


def lib():
    return _lib.load()


def guarded(n, dev, fill=NAN):
    """n elements of `fill` with GUARD sentinels behind them."""
    t = torch.full((n + GUARD,), fill, device=dev)
    t[n:] = SENTINEL
    return t


def guard_ok(t, n):
    return bool((t[n:] == SENTINEL).all())


def d64(n):
    """relative error of a double-precision sum of n terms (of the terms' magnitudes)"""
    return n * 2.0 ** -52


# =====================================================================================================================
# BatchNorm1d, training mode: evmi_batchnorm_{fwd,bwd}_cbt_f32 and the _valid pair
# =====================================================================================================================
BN_C = 3
BN_EPS, BN_MOM = f32(1e-5), f32(0.1)
BN_LONG_ROW = 8192
# row_walk: thread i takes a prefetch trip (eight values NT apart) while i + 7 NT < N, then single values while i < N.
# 1 / 2: N = 1 (the unbiased variance's rule) and the smallest batch; 255 / 256 / 257: one trip of the 256 threads, a lane short, a lane
# over (tail loop alone); 2047: threads 0 .. 254 take one prefetch trip and nothing else, thread 255 seven single values; 2048 = 8 x 256:
# every thread exactly one prefetch trip; 2049: thread 0 one more value behind it; 8191: the last row of the 256-thread kernels (four
# prefetch trips, or three and a tail); 8192 = BN_LONG_ROW = 8 x 1024: the first row of the 1024-thread kernels, one prefetch trip and
# no tail; 8193: and a tail of one; 16385: two prefetch trips and a tail.
BN_COLS = (1, 2, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 16385)
BN_CASES = [(n, 0) for n in BN_COLS] + [(n, a) for n in (257, 8193) for a in (2, 3, 4)]
# (B, T): the issue's three -- 72 columns; 8192 and 8193 columns across BN_LONG_ROW with items shorter than 8 x 1024 (tail loops only) --
# and two that reach the prefetch loop INSIDE an item: (3, 2100) at 256 threads (T >= 2048, 6300 columns), (1, 8193) at 1024 threads.
BNV_SHAPES = ((3, 24), (2, 4096), (3, 2731), (3, 2100), (1, 8193))
BNV_PATTERNS = ("full", "mixed", "clamped", "zero", "single")
BN_RELU_SEED = {}  # (n_cols, act) -> seed, where the default seed leaves a pre-activation too close to 0 (none does)


def bn_threads(n_cols):
    return 1024 if n_cols >= BN_LONG_ROW else 256


def bn_walk(n, nt, tid=0):
    """(trips of row_walk's prefetch loop, trips of its tail loop) of thread `tid` of nt over n values"""
    i, pre, tail = tid, 0, 0
    while i + 7 * nt < n:
        i, pre = i + 8 * nt, pre + 1
    while i < n:
        i, tail = i + nt, tail + 1
    return pre, tail


def bn_walk_kinds(n, nt):
    """{(takes prefetch trips, takes single values)} over the threads of one row_walk"""
    return {(p > 0, t > 0) for p, t in (bn_walk(n, nt, tid) for tid in range(nt))}


def bnv_valid(pattern, B, T):
    v = {"full": [T] * 3, "mixed": [0, T, 1], "clamped": [-5, T + 7, 3], "zero": [0] * 3, "single": [0, 1, 0]}[pattern]
    if B == 1:
        v = {"full": [T], "mixed": [T - 1], "clamped": [T + 7], "zero": [-5], "single": [1]}[pattern]
    return v[:B]


def bn_act64(z, act):
    return z * torch.sigmoid(z) if act == 2 else z.clamp_min(0) if act == 3 else torch.tanh(z) if act == 4 else z


def bn_fwd_ref(x, gam, bet, rm, rv, act, training=True):
    """float64 BatchNorm forward of x [C, n] (n = 0: the kernels divide by 1 and every sum is empty) with the error bound of each output.
    mean = (float)(double sum / N): d_m = u |mean| + D64 mean|x|.  d = v - mean in fp32: d_d = d_m + u |d|.  Squares in fp32, summed in
    double: d_ss = sum(2 |d| d_d + d_d^2 + u (|d| + d_d)^2) + D64 ss; var = (float)(ss / N) adds u var.  rstd = 1 / sqrtf(var + eps): a
    relative r on the argument moves it by at most r / (2 (1 - r)^1.5), plus the three roundings of sum, root, division.  ga = gamma rstd
    (one rounding) and z = d ga + beta (one or two roundings: the compiler may contract): the bound takes two, on the product and the sum.
    SiLU z / (1 + expf(-z)): slope <= 1.1, E + 3 u of its value; tanhf: slope <= 1, E of its value; ReLU and the identity: exact -- ReLU
    only where |z| > d_z, which `relu_clear` reports (a property of the inputs alone; the rule test asserts it for every committed case).
    Evaluation mode: mean = running_mean exactly, var = running_var exactly."""
    C, n = x.shape
    N = max(n, 1)
    if training:
        mean = x.sum(1) / N
        d = x - mean[:, None]
        ss = (d * d).sum(1)
        var = ss / N
        d_m = U * mean.abs() + d64(n) * x.abs().sum(1) / N
        d_d = d_m[:, None] + U * d.abs()
        dd = d.abs() + d_d
        d_ss = (2 * d.abs() * d_d + d_d * d_d + U * dd * dd).sum(1) + d64(n) * ss
        d_var = d_ss / N + U * var
        unb = ss / max(n - 1, 1)  # the unbiased variance of the running statistic; N = 1: divided by 1
        d_unb = d_ss / max(n - 1, 1) + U * unb
    else:
        mean, var = rm.clone(), rv.clone()
        d = x - mean[:, None]
        d_m, d_var = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        d_d = U * d.abs()
    r = d_var / (var + BN_EPS)
    assert (r < 0.01).all()
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    rel_rstd = 0.5 * r / (1 - r) ** 1.5 + 3 * U
    rel_g = rel_rstd + 2 * U
    z = d * (rstd * gam)[:, None] + bet[:, None]
    core = (gam.abs() * rstd)[:, None]
    d_z = core * (d_d * (1 + rel_g[:, None]) + d.abs() * rel_g[:, None]) + U * (d * (rstd * gam)[:, None]).abs() + U * z.abs()
    y = bn_act64(z, act)
    d_y = {0: d_z, 3: d_z, 2: 1.1 * d_z + (E + 3 * U) * y.abs(), 4: d_z + E * y.abs()}[act]
    out = dict(y=y, d_y=d_y, z=z, d_z=d_z, mean=mean, d_mean=d_m, rstd=rstd, d_rstd=rel_rstd * rstd,
               relu_clear=bool((z.abs() > d_z).all()) if n else True)
    if training:
        # (1 - m) rm + m stat: (1 - m) is one rounding, each product one, the sum one
        out["rm"] = (1 - BN_MOM) * rm + BN_MOM * mean
        out["d_rm"] = 2 * U * ((1 - BN_MOM) * rm).abs() + BN_MOM * d_m + U * (BN_MOM * mean).abs() + U * out["rm"].abs()
        out["rv"] = (1 - BN_MOM) * rv + BN_MOM * unb
        out["d_rv"] = 2 * U * ((1 - BN_MOM) * rv).abs() + BN_MOM * d_unb + U * (BN_MOM * unb).abs() + U * out["rv"].abs()
    return out


def bn_bwd_ref(x, gam, bet, mean, rstd, dy, act, g0, b0):
    """float64 BatchNorm backward as the kernel defines it from ITS inputs (x, gamma, beta, the saved fp32 mean and rstd, dy):
    xh = (x - mean) rstd, z = xh gamma + beta, dz = dy act'(z), s1 = sum dz, s2 = sum dz xh, dx = gamma rstd (dz - s1 / N - xh s2 / N);
    dbeta = b0 + s1, dgamma = g0 + s2 (accumulated into).  Bounds: xh two roundings; z as in the forward; act' exact for the identity and
    for ReLU where |z| > d_z (`relu_clear`); SiLU's s (1 + z (1 - s)) with |act''| <= 0.5 in z and its five operations on s = 1 / (1 +
    expf(-z)) (relative E + 2 u); tanh's 1 - t^2 with t = tanhf(z) off by E |t| and (1 - t^2) d_z.  s1, s2: double sums of fp32 terms (the product dz xh
    is rounded to fp32 first), stored through one fp32 rounding and one addition to the start value; m1 = (float)(s1 / N), m2 alike;
    dx: the inner difference loses u of each of its three terms, the two outer products 2 u of the result."""
    C, n = x.shape
    N = max(n, 1)
    xh = (x - mean[:, None]) * rstd[:, None]
    d_xh = 2 * U * xh.abs()
    ga, be = gam[:, None], bet[:, None]
    z = xh * ga + be
    d_z = ga.abs() * d_xh + U * (xh * ga).abs() + U * z.abs()
    if act == 2:
        s = torch.sigmoid(z)
        es = E + 2 * U
        rr = 1 + z * (1 - s)
        g = s * rr
        d_g = 0.5 * d_z + es * s * rr.abs() + s * (z.abs() * (es * s + 2 * U * (1 - s)) + U * rr.abs()) + U * g.abs()
    elif act == 4:
        t = torch.tanh(z)
        g = 1 - t * t
        d_t = E * t.abs() + g * d_z
        d_g = 2 * t.abs() * d_t + U * t * t + U * g.abs()
    elif act == 3:
        g, d_g = (z > 0).double(), torch.zeros_like(z)
    else:
        g, d_g = torch.ones_like(z), torch.zeros_like(z)
    dz = dy * g
    d_dz = dy.abs() * d_g + U * dz.abs()
    s1, s2 = dz.sum(1), (dz * xh).sum(1)
    d_s1 = d_dz.sum(1) + d64(n) * dz.abs().sum(1)
    d_s2 = (xh.abs() * d_dz + dz.abs() * d_xh + U * (dz * xh).abs()).sum(1) + d64(n) * (dz * xh).abs().sum(1)
    dbeta, dgamma = b0 + s1, g0 + s2
    d_dbeta = d_s1 + U * s1.abs() + U * dbeta.abs()
    d_dgamma = d_s2 + U * s2.abs() + U * dgamma.abs()
    m1, m2 = s1 / N, s2 / N
    d_m1, d_m2 = d_s1 / N + U * m1.abs(), d_s2 / N + U * m2.abs()
    inner = dz - m1[:, None] - xh * m2[:, None]
    d_inner = (d_dz + d_m1[:, None] + xh.abs() * d_m2[:, None] + m2.abs()[:, None] * d_xh
               + U * ((dz - m1[:, None]).abs() + (xh * m2[:, None]).abs() + inner.abs()))
    dx = (gam * rstd)[:, None] * inner
    d_dx = (gam * rstd).abs()[:, None] * d_inner + 2 * U * dx.abs()
    return dict(dx=dx, d_dx=d_dx, dgamma=dgamma, d_dgamma=d_dgamma, dbeta=dbeta, d_dbeta=d_dbeta,
                relu_clear=bool((z.abs() > d_z).all()) if n else True)


@functools.lru_cache(maxsize=None)
def bn_case(n_cols, act, const_channel=False):
    """inputs (fp32) and both references of one plain case; computed once, shared by the rule test and the GPU tests"""
    g = torch.Generator().manual_seed(BN_RELU_SEED.get((n_cols, act), 7000 + 10 * n_cols + act))
    x = torch.randn(BN_C, n_cols, generator=g) * 2 + 0.5
    if const_channel:
        x[1] = 0.75
    gam, bet = torch.rand(BN_C, generator=g) + 0.5, torch.randn(BN_C, generator=g) * 0.3
    rm, rv = torch.randn(BN_C, generator=g), torch.rand(BN_C, generator=g) + 0.5
    dy = torch.randn(BN_C, n_cols, generator=g)
    fwd = bn_fwd_ref(x.double(), gam.double(), bet.double(), rm.double(), rv.double(), act)
    mean_f, rstd_f = fwd["mean"].float(), fwd["rstd"].float()  # the backward's saved statistics: the references', rounded
    bwd = bn_bwd_ref(x.double(), gam.double(), bet.double(), mean_f.double(), rstd_f.double(), dy.double(), act, 1.0, -2.0)
    return dict(x=x, gam=gam, bet=bet, rm=rm, rv=rv, dy=dy, fwd=fwd, bwd=bwd, mean_f=mean_f, rstd_f=rstd_f)


def test_batchnorm_rule_restated():
    nts = {n: bn_threads(n) for n in BN_COLS}
    assert [nts[n] for n in (8191, 8192, 8193)] == [256, 1024, 1024] and set(nts.values()) == {256, 1024}
    walks = {n: (bn_walk(n, nts[n]), bn_walk(n, nts[n], nts[n] - 1)) for n in BN_COLS}  # (the first thread's, the last thread's)
    assert walks[2047] == ((1, 0), (0, 7)) and walks[2048] == ((1, 0), (1, 0)) and walks[2049] == ((1, 1), (1, 0))  # 8 x 256
    assert walks[8191] == ((4, 0), (3, 7)) and walks[8192] == ((1, 0), (1, 0)) and walks[8193] == ((1, 1), (1, 0))  # 8 x 1024
    assert walks[16385] == ((2, 1), (2, 0)) and walks[1] == ((0, 1), (0, 0)) and walks[257] == ((0, 2), (0, 1))
    kinds = {nt: set().union(*[bn_walk_kinds(n, nt) for n in BN_COLS if nts[n] == nt]) for nt in (256, 1024)}
    # 256 threads: a thread takes the tail loop alone, the prefetch loop alone, both, nothing; 1024 threads: every row has N >= 8192 > 1023
    # + 7 x 1024, so every thread takes a prefetch trip first (the tail alone and the idle thread: the _valid pair's short items below)
    assert kinds[256] == {(False, False), (False, True), (True, False), (True, True)} and kinds[1024] == {(True, False), (True, True)}
    assert {a for _, a in BN_CASES} == {0, 2, 3, 4}
    assert {(bn_threads(n), a) for n, a in BN_CASES if a} == {(nt, a) for nt in (256, 1024) for a in (2, 3, 4)}
    # the _valid pair: threads by B T, row_walk per ITEM over its clamped count
    assert [bn_threads(B * T) for B, T in BNV_SHAPES] == [256, 1024, 1024, 256, 1024]
    kinds = set()
    for B, T in BNV_SHAPES:
        for pat in BNV_PATTERNS:
            v = bnv_valid(pat, B, T)
            assert len(v) == B
            for n in (min(max(a, 0), T) for a in v):
                p, t = bn_walk(n, bn_threads(B * T))
                kinds.add((bn_threads(B * T), p > 0, t > 0))
    assert kinds >= {(nt, p, t) for nt in (256, 1024) for p, t in ((False, False), (False, True), (True, True))}  # an empty item, a tail alone, both loops
    counts = {pat: [sum(min(max(a, 0), T) for a in bnv_valid(pat, B, T)) for B, T in BNV_SHAPES] for pat in BNV_PATTERNS}
    assert set(counts["zero"]) == {0} and set(counts["single"]) == {1}
    assert any(a < 0 for a in bnv_valid("clamped", 3, 24)) and any(a > 24 for a in bnv_valid("clamped", 3, 24))
    # input conditions, on the references alone: ReLU's pre-activations clear their own error bound in both passes
    for n, a in BN_CASES:
        c = bn_case(n, a)
        assert c["fwd"]["relu_clear"] and c["bwd"]["relu_clear"], (n, a)


def bn_run_fwd(dev, c, n_cols, act, momentum=BN_MOM, running=True, valid=None, BT=None):
    y, mean, rstd = guarded(BN_C * n_cols, dev), guarded(BN_C, dev), guarded(BN_C, dev)
    rm, rv = guarded(BN_C, dev), guarded(BN_C, dev)
    rm[:BN_C], rv[:BN_C] = c["rm"].to(dev), c["rv"].to(dev)
    xg, gg, bg = c["x"].to(dev), c["gam"].to(dev), c["bet"].to(dev)
    args = [xg, gg, bg, y, mean, rstd, rm if running else None, rv if running else None, BN_C, n_cols, BN_EPS, momentum, act]
    if valid is None:
        rc = call(lib().evmi_batchnorm_fwd_cbt_f32, *args, stream(dev))
    else:
        rc = call(lib().evmi_batchnorm_fwd_valid_cbt_f32, *args, valid, BT[0], BT[1], stream(dev))
    assert rc == _lib.EVMI_OK
    outs = [t.cpu() for t in (y, mean, rstd, rm, rv)]
    for t, n in zip(outs, (BN_C * n_cols, BN_C, BN_C, BN_C, BN_C)):
        assert guard_ok(t, n), "a BatchNorm forward output was written past its end"
    y, mean, rstd, rm, rv = outs
    return y[: BN_C * n_cols].view(BN_C, n_cols), mean[:BN_C], rstd[:BN_C], rm[:BN_C], rv[:BN_C]


def bn_run_bwd(dev, c, n_cols, act, valid=None, BT=None):
    dx, dg, db = guarded(BN_C * n_cols, dev), guarded(BN_C, dev, 1.0), guarded(BN_C, dev, -2.0)
    ins = [c[k].to(dev) for k in ("x", "gam", "bet", "mean_f", "rstd_f", "dy")]
    if valid is None:
        rc = call(lib().evmi_batchnorm_bwd_cbt_f32, *ins, dx, dg, db, BN_C, n_cols, act, stream(dev))
    else:
        rc = call(lib().evmi_batchnorm_bwd_valid_cbt_f32, *ins, dx, dg, db, BN_C, n_cols, act, valid, BT[0], BT[1], stream(dev))
    assert rc == _lib.EVMI_OK
    dx, dg, db = dx.cpu(), dg.cpu(), db.cpu()
    assert guard_ok(dx, BN_C * n_cols) and guard_ok(dg, BN_C) and guard_ok(db, BN_C), "a BatchNorm backward output was written past its end"
    return dx[: BN_C * n_cols].view(BN_C, n_cols), dg[:BN_C], db[:BN_C]


def bn_check_fwd(got, ref, what, training=True):
    y, mean, rstd, rm, rv = got
    assert_within(y, ref["y"], ref["d_y"], what + " y")
    assert_within(mean, ref["mean"], ref["d_mean"], what + " mean")
    assert_within(rstd, ref["rstd"], ref["d_rstd"], what + " rstd")
    if training:
        assert_within(rm, ref["rm"], ref["d_rm"], what + " running_mean")
        assert_within(rv, ref["rv"], ref["d_rv"], what + " running_var")


def bn_check_bwd(got, ref, what):
    dx, dg, db = got
    assert_within(dx, ref["dx"], ref["d_dx"], what + " dx")
    assert_within(dg, ref["dgamma"], ref["d_dgamma"], what + " dgamma")
    assert_within(db, ref["dbeta"], ref["d_dbeta"], what + " dbeta")


def test_batchnorm_reference_is_batchnorm():
    """The restated forward / backward are torch's BatchNorm1d in float64 (training mode, unbiased running variance) and its autograd: to
    1e-6 of each tensor's scale -- the saved statistics the backward reference takes are the exact ones rounded to fp32, nothing more."""
    for n, a in ((257, 0), (257, 2), (257, 3), (257, 4), (2049, 0)):
        c = bn_case(n, a)
        x = c["x"].double().t()[None].transpose(1, 2).requires_grad_()  # [1, C, n]
        gam, bet = c["gam"].double().requires_grad_(), c["bet"].double().requires_grad_()
        rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
        y = bn_act64(F.batch_norm(x, rm, rv, gam, bet, True, BN_MOM, BN_EPS), a)
        y.backward(c["dy"].double()[None])
        for got, want in ((c["fwd"]["y"], y[0].detach()), (c["fwd"]["rm"], rm), (c["fwd"]["rv"], rv), (c["bwd"]["dx"], x.grad[0]),
                          (c["bwd"]["dgamma"] - 1.0, gam.grad), (c["bwd"]["dbeta"] + 2.0, bet.grad)):
            assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max()), (n, a)


@pytest.mark.parametrize("n_cols,act", BN_CASES)
def test_batchnorm_cbt_forward_backward(cuda_device, n_cols, act):
    """evmi_batchnorm_fwd_cbt_f32 / evmi_batchnorm_bwd_cbt_f32 against bn_fwd_ref / bn_bwd_ref (bounds derived there): y, mean, rstd, both
    running statistics (unbiased variance, divided by 1 at N = 1), dx, dgamma, dbeta (accumulated onto 1 and -2)."""
    c = bn_case(n_cols, act)
    what = f"batchnorm n_cols {n_cols} act {act}"
    bn_check_fwd(bn_run_fwd(cuda_device, c, n_cols, act), c["fwd"], what)
    bn_check_bwd(bn_run_bwd(cuda_device, c, n_cols, act), c["bwd"], what)


@pytest.mark.parametrize("n_cols", [257, 8193])
def test_batchnorm_cbt_constant_channel(cuda_device, n_cols):
    """Channel 1 is 0.75 everywhere: the double sum and its mean are exact, var = 0, rstd = 1 / sqrt(eps) = 316 multiplies whatever the
    deviations are -- the bounds of bn_fwd_ref / bn_bwd_ref hold unchanged."""
    c = bn_case(n_cols, 0, True)
    assert float(c["fwd"]["rstd"][1]) == 1.0 / math.sqrt(BN_EPS)
    bn_check_fwd(bn_run_fwd(cuda_device, c, n_cols, 0), c["fwd"], f"batchnorm constant n_cols {n_cols}")
    bn_check_bwd(bn_run_bwd(cuda_device, c, n_cols, 0), c["bwd"], f"batchnorm constant n_cols {n_cols}")


@pytest.mark.parametrize("n_cols", [257, 8193])
def test_batchnorm_cbt_evaluation_mode_and_no_running_statistics(cuda_device, n_cols):
    """momentum < 0: the running statistics normalise (mean_out is running_mean bit for bit, rstd = 1 / sqrtf(running_var + eps): three
    roundings) and stay untouched bit for bit.  Training mode with running_* = NULL is accepted and gives the bits of the run that
    updates them (the same arithmetic)."""
    dev = cuda_device
    c = bn_case(n_cols, 2)
    ref = bn_fwd_ref(c["x"].double(), c["gam"].double(), c["bet"].double(), c["rm"].double(), c["rv"].double(), 2, training=False)
    got = bn_run_fwd(dev, c, n_cols, 2, momentum=-1.0)
    bn_check_fwd(got, ref, f"batchnorm eval n_cols {n_cols}", training=False)
    assert same_bits(got[1], c["rm"]) and same_bits(got[3], c["rm"]) and same_bits(got[4], c["rv"])
    plain = bn_run_fwd(dev, c, n_cols, 2)
    bare = bn_run_fwd(dev, c, n_cols, 2, running=False)
    assert all(same_bits(a, b) for a, b in zip(bare[:3], plain[:3]))
    assert same_bits(bare[3], c["rm"]) and same_bits(bare[4], c["rv"])  # (the buffers the call did not get)
    # evaluation mode without the statistics, one statistic without the other, an activation that does not exist, no columns
    x, p3, y = c["x"].to(dev), c["gam"].to(dev), guarded(BN_C * n_cols, dev)
    for rm_, rv_, mom, act, n in ((None, None, -1.0, 0, n_cols), (p3, None, BN_MOM, 0, n_cols), (p3, p3, BN_MOM, 1, n_cols), (p3, p3, BN_MOM, 0, 0)):
        assert call(lib().evmi_batchnorm_fwd_cbt_f32, x, p3, p3, y, p3.clone(), p3.clone(), rm_, rv_, BN_C, n, BN_EPS, mom, act, stream(dev)) == INVALID_ARG
    assert torch.isnan(y[: BN_C * n_cols]).all()


@functools.lru_cache(maxsize=None)
def bnv_case(B, T, pattern, act):
    g = torch.Generator().manual_seed(9000 + 7 * B * T + len(pattern) + act)
    n = B * T
    valid = bnv_valid(pattern, B, T)
    cols = torch.cat([b * T + torch.arange(min(max(v, 0), T)) for b, v in enumerate(valid)]).long()
    live = torch.zeros(n, dtype=torch.bool)
    live[cols] = True
    x, dy = torch.randn(BN_C, n, generator=g) * 2 + 0.5, torch.randn(BN_C, n, generator=g)
    gam, bet = torch.rand(BN_C, generator=g) + 0.5, torch.randn(BN_C, generator=g) * 0.3
    rm, rv = torch.randn(BN_C, generator=g), torch.rand(BN_C, generator=g) + 0.5
    fwd = bn_fwd_ref(x[:, cols].double(), gam.double(), bet.double(), rm.double(), rv.double(), act)
    mean_f, rstd_f = fwd["mean"].float(), fwd["rstd"].float()
    bwd = bn_bwd_ref(x[:, cols].double(), gam.double(), bet.double(), mean_f.double(), rstd_f.double(), dy[:, cols].double(), act, 1.0, -2.0)
    x[:, ~live], dy[:, ~live] = NAN, NAN  # never read
    return dict(x=x, dy=dy, gam=gam, bet=bet, rm=rm, rv=rv, fwd=fwd, bwd=bwd, mean_f=mean_f, rstd_f=rstd_f, cols=cols, live=live, valid=valid)


@pytest.mark.parametrize("pattern", BNV_PATTERNS)
@pytest.mark.parametrize("B,T,act", [(B, T, 0) for B, T in BNV_SHAPES] + [(3, 24, 2)])
def test_batchnorm_valid_forward_backward(cuda_device, B, T, act, pattern):
    """The _valid pair: the references of the plain pair over the valid columns alone (count = sum of the clamped valid[b]; count 0
    divides by 1: mean 0, rstd 1 / sqrt(eps), nothing accumulated; count 1: var = 0 and the running variance takes 0 / 1).  x and dy hold
    NaN in every invalid column; y and dx there are exactly 0.  With every column valid the plain pair computes the same sums in another
    (fixed) order: both within the bound, bit equality reported."""
    dev = cuda_device
    c = bnv_case(B, T, pattern, act)
    n, cols, live = B * T, c["cols"], c["live"]
    valid = i32(c["valid"], dev)
    what = f"batchnorm_valid B {B} T {T} {pattern} act {act}"
    y, mean, rstd, rm, rv = bn_run_fwd(dev, c, n, act, valid=valid, BT=(B, T))
    assert (y[:, ~live] == 0).all(), "an invalid column of y is not exactly 0"
    bn_check_fwd((y[:, cols], mean, rstd, rm, rv), c["fwd"], what)
    dx, dg, db = bn_run_bwd(dev, c, n, act, valid=valid, BT=(B, T))
    assert (dx[:, ~live] == 0).all(), "an invalid column of dx is not exactly 0"
    bn_check_bwd((dx[:, cols], dg, db), c["bwd"], what)
    if len(cols) == 0:
        assert float(mean.abs().max()) == 0.0 and same_bits(dg, torch.full((BN_C,), 1.0)) and same_bits(db, torch.full((BN_C,), -2.0))
    if pattern == "full":
        plain = bn_run_fwd(dev, c, n, act) + bn_run_bwd(dev, c, n, act)
        bn_check_fwd(plain[:5], c["fwd"], what + " (plain pair)")
        bn_check_bwd(plain[5:], c["bwd"], what + " (plain pair)")
        names = ("y", "mean", "rstd", "running_mean", "running_var", "dx", "dgamma", "dbeta")
        print(what, "bit-equal to the plain pair:", {k: same_bits(a, b) for k, a, b in zip(names, (y, mean, rstd, rm, rv, dx, dg, db), plain)})


def test_batchnorm_valid_refuses_columns_that_are_not_items(cuda_device):
    dev = cuda_device
    c = bnv_case(3, 24, "full", 0)
    x, p3, v = c["x"].to(dev), c["gam"].to(dev), i32([24, 24, 24], dev)
    y = guarded(BN_C * 72, dev)
    for n, B, T, vv in ((72, 3, 23, v), (72, 0, 24, v), (72, 3, 24, None)):
        assert call(lib().evmi_batchnorm_fwd_valid_cbt_f32, x, p3, p3, y, p3.clone(), p3.clone(), None, None, BN_C, n, BN_EPS, BN_MOM, 0, vv, B, T, stream(dev)) == INVALID_ARG
        assert call(lib().evmi_batchnorm_bwd_valid_cbt_f32, x, p3, p3, p3, p3, x, y, p3.clone(), p3.clone(), BN_C, n, 0, vv, B, T, stream(dev)) == INVALID_ARG
    assert torch.isnan(y[: BN_C * 72]).all()


# =====================================================================================================================
# depthwise convolution backward: evmi_dwconv1d_bwd_cbt_f32
# =====================================================================================================================
DWB_C, DWB_B = 2, 3
# k 1 (no neighbours) / 3 / 4: the 4-tap tier and its edge (4 also: an even width, pad = 1 left and 2 right); 5 / 9 / 12: the 12-tap tier,
# both edges; 13 / 31 / 32: the 32-tap tier, both edges (32 = DW_KMAX).  T 1 / 2 / k - 1 (every tap of every position crosses an end) /
# k / 70 (interior positions, one trip of the 256 threads) / 257 (a second trip of one thread).
DWB_CASES = sorted({(k, T) for k in (1, 3, 4, 5, 9, 12, 13, 31, 32) for T in (1, 2, k - 1, k, 70, 257) if T >= 1})
# the staged form holds T + k - 1 floats in LDS: 40 KiB = 10240 floats
DWB_LONG = [(9, 10232), (9, 10233)]


def dwb_tier(k):
    return 4 if k <= 4 else 12 if k <= 12 else 32 if k <= 32 else None


def dwb_staged(k, T):
    return (T + k - 1) * 4 <= 40 * 1024


def test_dwconv_bwd_rule_restated():
    ks = sorted({k for k, _ in DWB_CASES})
    assert [dwb_tier(k) for k in ks] == [4, 4, 4, 12, 12, 12, 32, 32, 32] and dwb_tier(33) is None
    assert {4, 5, 12, 13, 32} <= set(ks) and 1 in ks  # both sides of both tier edges, the widest and the narrowest filter
    assert all(dwb_staged(k, T) for k, T in DWB_CASES)
    assert dwb_staged(*DWB_LONG[0]) and not dwb_staged(*DWB_LONG[1]) and DWB_LONG[1][1] == DWB_LONG[0][1] + 1
    assert (DWB_LONG[0][1] + 9 - 1) * 4 == 40 * 1024 and dwb_tier(9) == 12
    for k in ks:
        Ts = {T for kk, T in DWB_CASES if kk == k}
        assert {70, 257} <= Ts and (k == 1 or (k - 1 in Ts and k in Ts))
    assert any(T < k for k, T in DWB_CASES) and any(k % 2 == 0 for k in ks)


def dwb_ref(x, w, dy, k):
    """float64 autograd of y[t] = sum_j w[j] x[t + j - pad], pad = (k - 1) // 2 (an even k reaches one further to the right), per item"""
    C, B, T = x.shape
    pad = (k - 1) // 2
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = F.conv1d(F.pad(xr.permute(1, 0, 2), (pad, k - 1 - pad)), wr[:, None, :], None, groups=C).permute(1, 0, 2)
    y.backward(dy)
    return xr.grad, wr.grad, dy.sum((1, 2))


def dwb_run(dev, x, w, dy, k, need_dx=True, need_dw=True, ws_short=0):
    C, B, T = x.shape
    n_ws = lib().evmi_dwconv1d_bwd_cbt_f32_ws_elems(C, B, k)
    assert n_ws == C * B * (k + 1)
    dx, dw, db, ws = guarded(C * B * T, dev), guarded(C * k, dev, 3.0), guarded(C, dev, -5.0), guarded(n_ws, dev)
    rc = call(lib().evmi_dwconv1d_bwd_cbt_f32, x.to(dev), w.to(dev), dy.to(dev), dx if need_dx else None, dw if need_dw else None,
              db if need_dw else None, ws if need_dw else None, n_ws - ws_short, C, B, T, k, (k - 1) // 2, stream(dev))
    dx, dw, db, ws = dx.cpu(), dw.cpu(), db.cpu(), ws.cpu()
    assert guard_ok(dx, C * B * T) and guard_ok(dw, C * k) and guard_ok(db, C) and guard_ok(ws, n_ws), "written past the end of an output"
    return rc, dx[: C * B * T].view(C, B, T), dw[: C * k].view(C, k), db[:C]


@pytest.mark.parametrize("k,T", DWB_CASES + DWB_LONG)
def test_dwconv1d_bwd_cbt(cuda_device, k, T):
    """dx: one FMA chain over the k taps, gamma(k) of sum |w| |dy|.  dw[c][j] and db[c]: every thread chains its ceil(T / 256) positions
    in fp32 (n_t FMAs / additions), the 256 threads and then the items are summed in double (D64) and stored through one rounding each
    (the partial sum per item, the total) before the addition to the start value (3 and -5): gamma(n_t + 2) of sum |x| |dy| (sum |dy|) and
    u of the result.  dx = NULL leaves the buffer untouched and gives the same dw / db bits; dw = NULL leaves dw, db and the workspace
    untouched and gives the same dx bits."""
    dev = cuda_device
    g = torch.Generator().manual_seed(500 * k + T)
    x, dy = torch.randn(DWB_C, DWB_B, T, generator=g), torch.randn(DWB_C, DWB_B, T, generator=g)
    w = torch.randn(DWB_C, k, generator=g)
    want_dx, want_dw, want_db = dwb_ref(x.double(), w.double(), dy.double(), k)
    mag_dx, mag_dw, mag_db = dwb_ref(x.double().abs(), w.double().abs(), dy.double().abs(), k)
    rc, dx, dw, db = dwb_run(dev, x, w, dy, k)
    assert rc == _lib.EVMI_OK
    what = f"dwconv_bwd k {k} T {T}"
    n_t = (T + 255) // 256
    assert_within(dx, want_dx, gamma(k) * mag_dx, what + " dx")
    assert_within(dw, 3.0 + want_dw, (gamma(n_t + 2) + d64(256 * DWB_B)) * mag_dw + U * (3.0 + want_dw).abs(), what + " dw")
    assert_within(db, -5.0 + want_db, (gamma(n_t + 2) + d64(256 * DWB_B)) * mag_db + U * (-5.0 + want_db).abs(), what + " db")
    rc, dx2, dw2, db2 = dwb_run(dev, x, w, dy, k, need_dx=False)
    assert rc == _lib.EVMI_OK and torch.isnan(dx2).all() and same_bits(dw2, dw) and same_bits(db2, db)
    rc, dx3, dw3, db3 = dwb_run(dev, x, w, dy, k, need_dw=False)
    assert rc == _lib.EVMI_OK and same_bits(dx3, dx) and (dw3 == 3.0).all() and (db3 == -5.0).all()


@pytest.mark.parametrize("k,T", DWB_CASES + DWB_LONG)
def test_dwconv1d_bwd_cbt_item_boundary_probe(cuda_device, k, T):
    """dy = one 1.0 at the last frame of item 0 and one 2.0 at frame 0 of item 1, x and the start values small integers: dx holds
    w[c][j] where t = T - 1 + j - pad (item 0) and 2 w[c][j] where t = j - pad (item 1), dw[c][j] = 3 + x[c][0][T - 1 + j - pad] +
    2 x[c][1][j - pad] (terms outside the item missing), db = -5 + 3 -- all exact: products with 1 and 2, sums of small integers -- and
    everything else, item 2 included, is exactly 0.  A tap that crosses an item boundary reads the neighbour's x or dy."""
    dev = cuda_device
    g = torch.Generator().manual_seed(k * 31 + T)
    x = torch.randint(-8, 9, (DWB_C, DWB_B, T), generator=g).float()
    w = torch.randn(DWB_C, k, generator=g)
    pad = (k - 1) // 2
    dy = torch.zeros(DWB_C, DWB_B, T)
    dy[:, 0, T - 1] += 1.0
    dy[:, 1, 0] += 2.0
    want_dx, want_dw = torch.zeros(DWB_C, DWB_B, T), torch.full((DWB_C, k), 3.0)
    for j in range(k):
        t0, t1 = T - 1 + j - pad, j - pad
        if 0 <= t0 < T:
            want_dx[:, 0, t0] = w[:, j]
            want_dw[:, j] += x[:, 0, t0]
        if 0 <= t1 < T:
            want_dx[:, 1, t1] = 2.0 * w[:, j]
            want_dw[:, j] += 2.0 * x[:, 1, t1]
    rc, dx, dw, db = dwb_run(dev, x, w, dy, k)
    assert rc == _lib.EVMI_OK
    assert torch.equal(dx, want_dx), (dx - want_dx).abs().max()
    assert (dx[:, 2] == 0.0).all()
    assert torch.equal(dw, want_dw), (dw - want_dw).abs().max()
    assert torch.equal(db, torch.full((DWB_C,), -2.0))


def test_dwconv1d_bwd_cbt_refusals(cuda_device):
    dev = cuda_device
    x, dy = torch.ones(DWB_C, DWB_B, 8), torch.ones(DWB_C, DWB_B, 8)
    for k in (0, 33):
        dx, dw, db, ws = guarded(48, dev), guarded(66, dev, 3.0), guarded(DWB_C, dev, -5.0), guarded(6 * 34, dev)
        rc = call(lib().evmi_dwconv1d_bwd_cbt_f32, x.to(dev), torch.ones(66, device=dev), dy.to(dev), dx, dw, db, ws, 6 * 34, DWB_C, DWB_B, 8, k, 0, stream(dev))
        assert rc == INVALID_ARG
        assert torch.isnan(dx[:48]).all() and (dw[:66] == 3.0).all() and (db[:DWB_C] == -5.0).all() and torch.isnan(ws[: 6 * 34]).all()
    rc, dx, dw, db = dwb_run(dev, x, torch.ones(DWB_C, 3), dy, 3, need_dx=False, ws_short=1)
    assert rc == INVALID_ARG and (dw == 3.0).all() and (db == -5.0).all()
    w3 = torch.ones(DWB_C, 3, device=dev)
    assert call(lib().evmi_dwconv1d_bwd_cbt_f32, x.to(dev), w3, dy.to(dev), None, guarded(6, dev), guarded(2, dev), None, 24, DWB_C, DWB_B, 8, 3, 1, stream(dev)) == INVALID_ARG
    assert call(lib().evmi_dwconv1d_bwd_cbt_f32, None, w3, dy.to(dev), guarded(48, dev), None, None, None, 0, DWB_C, DWB_B, 8, 3, 1, stream(dev)) == INVALID_ARG


# =====================================================================================================================
# embedding backwards: fs2_table_bwd_kernel (text and bucket tables), per-item table, length regulator
# =====================================================================================================================
TABLE_CHUNK = 4096
# tokens B L: 1; 4095 (one chunk, its last group of four a token short: cnt4 = 4096 walks the staged tail); 4096 (exactly one chunk);
# 4097 (a second chunk of ONE token, cnt4 = 4); 8193 (three chunks).  The LAST item is always full: the token next to every tail is live.
TB_TOKENS = {1: (1, 1), 4095: (3, 1365), 4096: (4, 1024), 4097: (17, 241), 8193: (3, 2731)}
TB_ROWS = (1, 255, 256, 257, 600)  # grid.y = 1 (one row; a thread short of the tile; the tile), 2 (one row into the second), 3
TB_CASES = [(n, rows, D) for n in TB_TOKENS for rows in TB_ROWS for D in (2, 5)]
TB_BINS = (2, 256, 257)
TB_INIT = 7.0


def tb_lens(B, L):
    lens = [(0, 1, L)[b % 3] for b in range(B)]
    lens[-1] = L
    return lens


def test_table_bwd_rule_restated():
    assert {B * L for B, L in TB_TOKENS.values()} == set(TB_TOKENS) == {1, 4095, 4096, 4097, 8193}
    chunks = {n: [min(TABLE_CHUNK, n - b) for b in range(0, n, TABLE_CHUNK)] for n in TB_TOKENS}
    assert chunks[4095] == [4095] and chunks[4096] == [4096] and chunks[4097] == [4096, 1] and chunks[8193] == [4096, 4096, 1]
    cnt4 = lambda c: (c + 3) & ~3  # noqa: E731
    assert {c % 4 for cs in chunks.values() for c in cs} == {0, 1, 3} and cnt4(4095) == 4096 and cnt4(1) == 4
    assert [(r + 255) // 256 for r in TB_ROWS] == [1, 1, 1, 2, 3] and [(b + 255) // 256 for b in TB_BINS] == [1, 1, 2]
    for n, (B, L) in TB_TOKENS.items():
        lens = tb_lens(B, L)
        assert lens[-1] == L and (B < 3 or {0, 1, L} <= set(lens) or L == 1)
    assert {D for _, _, D in TB_CASES} == {2, 5}
    # item embedding: D rows around one workgroup of 256; length regulator: C B L around it
    assert sorted(D * r for D, r in IT_CASES) == [255, 256, 257, 257] and sorted(C * B * L for C, B, L in LR_CASES) == [255, 256, 257, 600]


@functools.lru_cache(maxsize=None)
def tb_tokens(n, rows, D):
    """ids: a third of the tokens on three rows (0, rows / 2 = the skipped id, rows - 1: long collision chains, the table's last row), the
    others anywhere; dx: integers in [-4, 4] (every partial sum is an integer below 2^24: exact in any order)."""
    B, L = TB_TOKENS[n]
    g = torch.Generator().manual_seed(n * 1000 + rows * 7 + D)
    ids = torch.randint(0, rows, (B, L), generator=g)
    hot = torch.tensor([0, rows // 2, rows - 1])[torch.randint(0, 3, (B, L), generator=g)]
    ids = torch.where(torch.rand(B, L, generator=g) < 0.34, hot, ids)
    ids[-1, -1] = rows - 1  # the last token: live, on the last row
    dx = torch.randint(-4, 5, (D, B * L), generator=g).float()
    return B, L, ids.to(torch.int32), dx


@pytest.mark.parametrize("n,rows,D", TB_CASES)
def test_fs2_embed_bwd(cuda_device, n, rows, D):
    """dtable[r][c] = 7 + sum of dx[c][token] over the tokens with id r, l < lens[b] and id != skip_id: integers, so equal to float64
    index_add bit for bit.  The table is allocated three rows longer than `rows` says: those rows (thread r >= rows of the last tile) and
    the guard stay as they were.  rows = 1: the skipped id is 1, outside the table (the padding symbol of a one-row table)."""
    dev = cuda_device
    B, L, ids, dx = tb_tokens(n, rows, D)
    skip = rows // 2 if rows > 1 else 1
    if rows == 1:
        ids = ids.clone()
        ids[:, ::3] = 1
        ids[-1, -1] = 0
    lens = tb_lens(B, L)
    live = (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]) & (ids != skip)
    assert live[-1, -1] and (ids == skip).any() or n == 1
    want = torch.full((rows, D), TB_INIT, dtype=torch.float64)
    want.index_add_(0, ids.long().flatten()[live.flatten()], dx.double().t()[live.flatten()])
    table = guarded((rows + 3) * D, dev, TB_INIT)
    rc = call(lib().evmi_fs2_embed_bwd_f32, dx.to(dev), ids.to(dev), i32(lens, dev), table, rows, B, L, D, skip, stream(dev))
    assert rc == _lib.EVMI_OK
    table = table.cpu()
    assert guard_ok(table, (rows + 3) * D) and (table[rows * D : (rows + 3) * D] == TB_INIT).all(), "a row past `rows` was written"
    got = table[: rows * D].view(rows, D)
    assert torch.equal(got.double(), want), f"{int((got.double() != want).sum())} table entries differ, first at {(got.double() != want).nonzero()[0].tolist()}"


@pytest.mark.parametrize("n_bins", TB_BINS)
@pytest.mark.parametrize("n", list(TB_TOKENS))
def test_fs2_bucket_embed_bwd(cuda_device, n, n_bins):
    """Bucket of a position: the first of the n_bins - 1 boundaries >= value * control, computed as ONE fp32 product and comparisons --
    torch.bucketize(right=False) on the same fp32 product, exactly: values on a boundary (control = 0.5 and the boundaries' doubles: exact),
    between two, below the first and above the last.  Every position counts (no lengths, no skipped id); integer gradients: the table
    equals float64 index_add bit for bit."""
    dev = cuda_device
    B, L = TB_TOKENS[n]
    D, control = 3, 0.5
    g = torch.Generator().manual_seed(n + n_bins)
    bins = torch.arange(n_bins - 1).float() * 0.25 - 3.0
    pick = torch.randint(0, n_bins - 1, (B, L), generator=g)
    kind = torch.randint(0, 4, (B, L), generator=g)
    values = torch.where(kind == 0, 2 * bins[pick], torch.where(kind == 1, 2 * (bins[pick] + 0.125), torch.where(kind == 2, torch.tensor(-100.0), torch.tensor(1000.0))))
    if n >= 4:
        values.view(-1)[-4:] = torch.tensor([2 * float(bins[0]), 2 * float(bins[-1]), -100.0, 1000.0])
    dx = torch.randint(-4, 5, (D, B * L), generator=g).float()
    want_idx = torch.bucketize(values * control, bins, right=False).to(torch.int32)
    assert int(want_idx.max()) <= n_bins - 1 and (n < 4 or {0, n_bins - 2, n_bins - 1} <= set(want_idx.view(-1)[-4:].tolist()))
    want = torch.full((n_bins, D), TB_INIT, dtype=torch.float64)
    want.index_add_(0, want_idx.long().flatten(), dx.double().t())
    table, idx = guarded((n_bins + 3) * D, dev, TB_INIT), torch.full((B * L + GUARD,), -77, dtype=torch.int32, device=dev)
    rc = call(lib().evmi_fs2_bucket_embed_bwd_f32, dx.to(dev), values.to(dev), bins.to(dev), table, idx, n_bins, B, L, D, control, stream(dev))
    assert rc == _lib.EVMI_OK
    table, idx = table.cpu(), idx.cpu()
    assert (idx[B * L :] == -77).all() and torch.equal(idx[: B * L].view(B, L), want_idx)
    assert guard_ok(table, (n_bins + 3) * D) and (table[n_bins * D : (n_bins + 3) * D] == TB_INIT).all()
    assert torch.equal(table[: n_bins * D].view(n_bins, D).double(), want)


def test_table_bwd_refusals(cuda_device):
    dev = cuda_device
    dx, ids, lens, table = torch.ones(2, 4, device=dev), i32([0, 1, 0, 1], dev), i32([4], dev), guarded(4, dev, TB_INIT)
    for args in ((None, ids, lens, table, 2, 1, 4, 2), (dx, ids, None, table, 2, 1, 4, 2), (dx, ids, lens, table, 0, 1, 4, 2), (dx, ids, lens, table, 2, 1, 0, 2)):
        assert call(lib().evmi_fs2_embed_bwd_f32, *args, -1, stream(dev)) == INVALID_ARG
    vals, bins, idx = torch.zeros(4, device=dev), torch.zeros(1, device=dev), i32([0] * 4, dev)
    assert call(lib().evmi_fs2_bucket_embed_bwd_f32, dx, vals, bins, table, idx, 1, 1, 4, 2, 1.0, stream(dev)) == INVALID_ARG  # one bin: no boundary
    assert call(lib().evmi_fs2_bucket_embed_bwd_f32, dx, vals, bins, table, None, 2, 1, 4, 2, 1.0, stream(dev)) == INVALID_ARG
    assert (table[:4] == TB_INIT).all()


IT_CASES = [(5, 51), (4, 64), (1, 257), (257, 1)]  # (D, rows): D rows = 255, 256, 257 (both ways round)


@pytest.mark.parametrize("D,rows", IT_CASES)
def test_fs2_item_embedding_bwd(cuda_device, D, rows):
    """dtable[ids[b]][c] = 7 + sum_{l < min(lens[b], L)} dx[c][b][l]: items 0 and 1 share a row, item 1 is empty (lens 0), item 2 has
    lens > L (clamped) on the last row, item 3 one symbol on row 0; integers: exact."""
    dev = cuda_device
    B, L = 4, 7
    g = torch.Generator().manual_seed(D * rows)
    r0 = rows // 2
    ids, lens = [r0, r0, rows - 1, 0], [L, 0, L + 3, 1]
    dx = torch.randint(-4, 5, (D, B, L), generator=g).float()
    want = torch.full((rows, D), TB_INIT, dtype=torch.float64)
    for b in range(B):
        want[ids[b]] += dx[:, b, : min(lens[b], L)].double().sum(1)
    table = guarded(rows * D, dev, TB_INIT)
    rc = call(lib().evmi_fs2_item_embedding_bwd_f32, dx.to(dev), i32(ids, dev), i32(lens, dev), table, rows, B, L, D, stream(dev))
    assert rc == _lib.EVMI_OK
    table = table.cpu()
    assert guard_ok(table, rows * D) and torch.equal(table[: rows * D].view(rows, D).double(), want)


LR_CASES = [(5, 3, 17), (4, 2, 32), (1, 1, 257), (3, 2, 100)]  # (C, B, L): 255, 256, 257 and 600 outputs


@pytest.mark.parametrize("C,B,L", LR_CASES)
def test_length_regulate_bwd_cbt(cuda_device, C, B, L):
    """dx[c][b][l] = sum of dframes[c][b][t] over cum[l - 1] <= t < min(cum[l], T): durations 0 .. 3 (zeros inside and as the last
    symbol), T two thirds of the longest total, so the tail symbols' cum exceed T (clamped: a symbol cut short, then symbols that own no
    frame and start past T); integer frames: exact.  The buffer starts as NaN: a symbol without frames is written as 0."""
    dev = cuda_device
    g = torch.Generator().manual_seed(C * B * L)
    dur = torch.randint(0, 4, (B, L), generator=g)
    dur[:, -1] = 0
    dur[0, 0] = 0
    cum = dur.cumsum(1)
    T = max(1, int(cum.max()) * 2 // 3)
    assert int(cum[:, -2].max()) > T and (dur == 0).any()
    dfr = torch.randint(-4, 5, (C, B, T), generator=g).float()
    want = torch.zeros(C, B, L)
    for b in range(B):
        for l in range(L):
            t0, t1 = (int(cum[b, l - 1]) if l else 0), min(int(cum[b, l]), T)
            if t1 > t0:
                want[:, b, l] = dfr[:, b, t0:t1].sum(1)
    dx = guarded(C * B * L, dev)
    rc = call(lib().evmi_length_regulate_bwd_cbt_f32, dfr.to(dev), cum.to(torch.int32).to(dev), dx, C, B, L, T, stream(dev))
    assert rc == _lib.EVMI_OK
    dx = dx.cpu()
    assert guard_ok(dx, C * B * L) and torch.equal(dx[: C * B * L].view(C, B, L), want)


# =====================================================================================================================
# elementwise: GLU backward, dropout and dropout fused with its neighbour
# =====================================================================================================================
EW_N = (1, 3, 4, 5, 1023, 1024, 1025)  # dropout_fused: a thread's four elements (a partial vector alone; one short; full; one over) and
#                                        the workgroup's 1024 (a vector short, full, one element into the second workgroup)
EW_P = (0.0, 0.1, 0.999)
SEED_PLAIN, SEED_VALUE, SEED_BASE = 79, 0x300000000000001A, 0x7000000000000123  # their sum has bit 63 set: SeedArg keeps the low 63 bits


def test_elementwise_rule_restated():
    assert [(n + 255) // 256 for n in (1, 255, 256, 257)] == [1, 1, 1, 2]                        # glu_bwd, dropout: one element per thread
    vec = lambda n: ((n + 3) // 4, n % 4 == 0)                                                   # noqa: E731  (threads, last one full)
    assert [vec(n) for n in EW_N] == [(1, False), (1, False), (1, True), (2, False), (256, False), (256, True), (257, False)]
    assert [((n + 3) // 4 + 255) // 256 for n in EW_N] == [1, 1, 1, 1, 1, 1, 2]
    assert dropout_ref.seed_get(SEED_VALUE, SEED_BASE) == (SEED_VALUE + SEED_BASE) - 2 ** 63 != SEED_VALUE
    for p in EW_P:  # what the masks of these tests must show: p = 0 keeps everything, 0.999 one draw in a thousand
        assert dropout_ref.keep_rate(p) == 1.0 - math.ceil(65536.0 * f32(p)) / 65536.0
    for seed in (SEED_PLAIN, dropout_ref.seed_get(SEED_VALUE, SEED_BASE)):  # (seeds chosen so that p = 0.999 keeps something to look at)
        assert dropout_ref.keep_mask(seed, 1025, 0.0).all() and 0 < int(dropout_ref.keep_mask(seed, 1023, 0.999).sum()) < 12
        assert 45 < int((~dropout_ref.keep_mask(seed, 1025, 0.1)).sum()) < 160  # (102.5 expected, six standard deviations of 9.6)


@pytest.mark.parametrize("n_half", [1, 255, 256, 257])
def test_glu_bwd(cuda_device, n_half):
    """p = [a; b], dy -> dp = [dy s; dy a s (1 - s)], s = 1 / (1 + expf(-b)): expf costs E of e = exp(-b), that is E e / (1 + e) <= E of
    s; the sum and the division one rounding each: es = E + 2 u.  da = dy s: es and one rounding.  db = ((dy a) s) (1 - s): 1 - s is off
    by es s + u (1 - s) (absolute: for large b it is all cancellation), three products."""
    dev = cuda_device
    g = torch.Generator().manual_seed(n_half)
    p, dy = torch.randn(2 * n_half, generator=g) * 3, torch.randn(n_half, generator=g)
    a, b, d = p[:n_half].double(), p[n_half:].double(), dy.double()
    s = torch.sigmoid(b)
    es = E + 2 * U
    want = torch.cat([d * s, d * a * s * (1 - s)])
    bound = torch.cat([(es + U) * (d * s).abs(), (d * a).abs() * (es * s * (1 - s) + s * (es * s + U * (1 - s))) + 3 * U * (d * a * s * (1 - s)).abs()])
    dp = guarded(2 * n_half, dev)
    assert call(lib().evmi_glu_bwd_f32, p.to(dev), dy.to(dev), dp, n_half, stream(dev)) == _lib.EVMI_OK
    dp = dp.cpu()
    assert guard_ok(dp, 2 * n_half)
    assert_within(dp[: 2 * n_half], want, bound, f"glu_bwd n_half {n_half}")
    assert call(lib().evmi_glu_bwd_f32, p.to(dev), dy.to(dev), dp.to(dev), 0, stream(dev)) == INVALID_ARG


def ew_inputs(n, seed):
    """a: magnitudes in [0.5, 2.5] (a kept element is never 0), b: N(0, 1) away from the zero of silu'"""
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(n, generator=g) * 2 + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    b = torch.randn(n, generator=g)
    return a, torch.where((b + 1.2785).abs() < 0.05, torch.tensor(0.5), b)  # (silu' crosses 0 at -1.2785: a kept element is never 0 in mode 3)


def seed_args(with_base, dev):
    """(seed_value, seed_base_dev, the seed the kernel uses)"""
    if not with_base:
        return SEED_PLAIN, None, SEED_PLAIN
    return SEED_VALUE, torch.tensor([SEED_BASE], dtype=torch.int64, device=dev), dropout_ref.seed_get(SEED_VALUE, SEED_BASE)


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("p", EW_P)
def test_dropout_kept_set_is_the_restated_generator(cuda_device, p, with_base):
    """evmi_dropout_f32: y = keep ? x / (1 - p) : 0.  The kept set equals dropout_ref.keep_mask(seed, n, p) bit for bit (the seed: the value
    alone, or (value + *base) & (2^63 - 1) with the device-resident base); dropped elements are exactly 0; kept ones: 1 - p in fp32 is one
    rounding, the division one: 2 u."""
    dev = cuda_device
    value, base, seed = seed_args(with_base, dev)
    for n in EW_N:
        x, _ = ew_inputs(n, n)
        y = guarded(n, dev)
        assert call(lib().evmi_dropout_f32, x.to(dev), y, n, p, value, base, stream(dev)) == _lib.EVMI_OK
        y = y.cpu()
        assert guard_ok(y, n)
        keep = torch.from_numpy(dropout_ref.keep_mask(seed, n, p))
        assert torch.equal(y[:n] != 0, keep), f"dropout n {n} p {p}: kept set differs from the restated generator at {(((y[:n] != 0) != keep).nonzero().flatten()[:8]).tolist()}"
        want = torch.where(keep, x.double() / (1.0 - f32(p)), torch.zeros(n, dtype=torch.float64))
        assert_within(y[:n], want, 2 * U * want.abs(), f"dropout n {n} p {p}")
    for bad_n, bad_p in ((0, 0.1), (4, 1.0), (4, -0.1)):
        assert call(lib().evmi_dropout_f32, x.to(dev), guarded(4, dev), bad_n, bad_p, value, base, stream(dev)) == INVALID_ARG


def silu_grad64(z):
    """(silu'(z), its evaluation error as s (1 + z (1 - s)) with s = 1 / (1 + expf(-z)) in uncontracted fp32: s off by es = E + 2 u,
    1 - s by es s + u (1 - s), the product with z, the sum with 1 and the product with s one rounding each)"""
    s = torch.sigmoid(z)
    es = E + 2 * U
    rr = 1 + z * (1 - s)
    g = s * rr
    return g, es * s * rr.abs() + s * (z.abs() * (es * s + 2 * U * (1 - s)) + U * rr.abs()) + U * g.abs()


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("p", EW_P)
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_dropout_fused_kept_set_and_values(cuda_device, mode, p, with_base):
    """evmi_dropout_fused_f32, drop(v) = keep ? v / (1 - p) : 0 on the stream of evmi_dropout_f32 (2 u: the rounding of 1 - p, the division):
    1: b + scale drop(a) -- the product and the sum, contracted or not: u of each;  2: drop(silu(a)), silu = v / (1 + expf(-v)): E + 2 u;
    3: drop(a) silu'(b): silu_grad64's error and the product;  4: scale drop(a): one product.  The kept set -- where the output differs
    from what a dropped element gives (b in mode 1, 0 elsewhere; |a| >= 0.5 and silu'(b) != 0 make every kept element differ) -- equals
    dropout_ref.keep_mask bit for bit."""
    dev = cuda_device
    value, base, seed = seed_args(with_base, dev)
    scale = 0.5 if mode in (1, 4) else 1.0
    for n in EW_N:
        a, b = ew_inputs(n, 100 + n)
        y = guarded(n, dev)
        rc = call(lib().evmi_dropout_fused_f32, mode, a.to(dev), b.to(dev) if mode in (1, 3) else None, y, n, p, value, base, scale, stream(dev))
        assert rc == _lib.EVMI_OK
        y = y.cpu()
        assert guard_ok(y, n)
        keep = torch.from_numpy(dropout_ref.keep_mask(seed, n, p))
        a64, b64, zero = a.double(), b.double(), torch.zeros(n, dtype=torch.float64)
        inv = 1.0 - f32(p)
        if mode == 1:
            d = torch.where(keep, a64 / inv, zero)
            want, bound, dropped = b64 + scale * d, 3 * U * (scale * d).abs() + U * (b64 + scale * d).abs(), b
        elif mode == 2:
            want = torch.where(keep, a64 * torch.sigmoid(a64) / inv, zero)
            bound, dropped = (E + 4 * U) * want.abs(), torch.zeros(n)
        elif mode == 3:
            gz, d_g = silu_grad64(b64)
            assert (gz.abs() > 1e-3).all()
            d = torch.where(keep, a64 / inv, zero)
            want, bound, dropped = d * gz, d.abs() * d_g + 3 * U * (d * gz).abs(), torch.zeros(n)
        else:
            want = torch.where(keep, scale * a64 / inv, zero)
            bound, dropped = 3 * U * want.abs(), torch.zeros(n)
        assert torch.equal(y[:n] != dropped, keep), f"dropout_fused mode {mode} n {n} p {p}: kept set differs from the restated generator"
        assert_within(y[:n], want, bound, f"dropout_fused mode {mode} n {n} p {p}")


def test_dropout_fused_refusals(cuda_device):
    """A pointer that is not 16-byte aligned (any of the three), a mode outside 1 .. 4, modes 1 and 3 without their second operand, p = 1,
    no elements: refused, nothing written."""
    dev = cuda_device
    a, b, y = torch.ones(16, device=dev), torch.ones(16, device=dev), torch.full((16,), NAN, device=dev)
    fn = lib().evmi_dropout_fused_f32
    assert a.data_ptr() % 16 == 0 and a[1:].data_ptr() % 16 == 4
    for args in ((1, a[1:], b, y), (1, a, b[1:], y), (1, a, b, y[1:]), (4, a[1:], None, y), (0, a, b, y), (5, a, b, y), (1, a, None, y), (3, a, None, y), (2, None, None, y), (2, a, None, None)):
        assert call(fn, *args, 8, 0.1, 7, None, 1.0, stream(dev)) == INVALID_ARG, args[0]
    assert call(fn, 2, a, None, y, 8, 1.0, 7, None, 1.0, stream(dev)) == INVALID_ARG
    assert call(fn, 2, a, None, y, 0, 0.1, 7, None, 1.0, stream(dev)) == INVALID_ARG
    assert torch.isnan(y).all()
    assert call(fn, 2, a, None, y, 8, 0.1, 7, None, 1.0, stream(dev)) == _lib.EVMI_OK and not torch.isnan(y[:8]).any() and torch.isnan(y[8:]).all()


# =====================================================================================================================
# attention, training: evmi_mha_{fwd,bwd}_{f32,bf16} at head dimensions 32 / 64 / 128
# =====================================================================================================================
AT_H, AT_B = 2, 3
# query block 128 (four waves of 32 queries), key tile 32: T 1; 31 / 32 / 33 around one key tile (= one wave of queries); 127 / 128 / 129
# around the query block (129: a second workgroup with ONE live query, a fifth key tile with one key); 160: five full key tiles
AT_T = (1, 31, 32, 33, 127, 128, 129, 160)
AT_DH = (32, 64, 128)


def at_lens(T, variant):
    return [T, 1 if variant == "one" else max(1, (T // 2) | 1), 0]


def at_pairs(B, T):
    """attn_drop_pairs: the bf16 kernels hash once per PAIR of mask elements where T is even and the tensor below 2^33 elements"""
    return T % 2 == 0 and B * T * T < 2 ** 33


def test_attention_train_rule_restated():
    tiles = lambda n: (n + 31) // 32   # noqa: E731
    blocks = lambda n: (n + 127) // 128  # noqa: E731
    assert [tiles(T) for T in AT_T] == [1, 1, 1, 2, 4, 4, 5, 5] and [blocks(T) for T in AT_T] == [1, 1, 1, 1, 1, 1, 2, 2]
    assert {T % 32 for T in AT_T} == {1, 31, 0} and {T % 128 for T in AT_T} >= {127, 0, 1}
    for T in AT_T:
        lens = at_lens(T, "odd")
        assert lens[0] == T and lens[1] % 2 == 1 and 1 <= lens[1] <= T and lens[2] == 0 and at_lens(T, "one")[1] == 1
    assert {tiles(at_lens(T, "odd")[1]) for T in AT_T} >= {1, 2, 3}
    from everyvoice_amd.train import ops
    assert set(AT_DH) == set(ops.ATTENTION_SPECIALISED_HEAD_DIMS) and 48 not in AT_DH
    # the mask read-out probes: T even -> one hash per pair (in-thread in the forward / dQ kernels, DPP exchange in the dK / dV kernel),
    # T odd -> one hash per element; an odd length inside the even T; a last query block with clamped queries; a last partial tile
    assert [at_pairs(AT_B, T) for T, _ in PROBE_SHAPES] == [True, False]
    (T0, l0), (T1, l1) = PROBE_SHAPES
    assert T0 % 2 == 0 and l0[1] % 2 == 1 and 1 in l0 and 0 in l1 and T0 % 128 and T1 % 128 and T1 % 32 == 1
    assert at_pairs(1, 2 ** 16) and not at_pairs(1, 2 ** 17)  # (the size switch itself is out of a test's reach: 2^33 mask elements)


def at_entry(kind, dh, operands):
    stem = "evmi_mha" if dh in AT_DH else "evmi_mha_generic"
    return getattr(lib(), f"{stem}_{kind}_{operands}")


def at_fwd(dev, qkv, lens32, dh, operands, p=0.0, seed=0):
    D3, B, T = qkv.shape
    D, H = D3 // 3, D3 // 3 // dh
    out, lse = guarded(D * B * T, dev), guarded(B * H * T, dev)
    rc = call(at_entry("fwd", dh, operands), qkv, lens32, out, lse, B, T, D, H, float(p), seed, None, stream(dev))
    assert rc == _lib.EVMI_OK
    torch.cuda.synchronize()
    assert guard_ok(out, D * B * T) and guard_ok(lse, B * H * T), "attention forward wrote past an output"
    return out[: D * B * T].view(D, B, T), lse[: B * H * T].view(B, H, T)


def at_bwd(dev, qkv, lens32, out, lse, dout, dh, operands, p=0.0, seed=0):
    D3, B, T = qkv.shape
    D, H = D3 // 3, D3 // 3 // dh
    dqkv, dsum = guarded(D3 * B * T, dev), guarded(B * H * T, dev)
    rc = call(at_entry("bwd", dh, operands), qkv, lens32, out.contiguous(), dout, lse.contiguous(), dsum, dqkv, B, T, D, H, float(p), seed, None, stream(dev))
    assert rc == _lib.EVMI_OK
    torch.cuda.synchronize()
    assert guard_ok(dqkv, D3 * B * T) and guard_ok(dsum, B * H * T), "attention backward wrote past an output"
    return dqkv[: D3 * B * T].view(D3, B, T)


def at_ref(qkv, lens, H, dout=None, keep=None, p=0.0):
    """float64 explicit attention on the channel-major layout, qkv [3 D, B, T]: S = q k / sqrt(dh), keys >= lens[b] masked, softmax over
    the keys, dropout on the probabilities (keep [B, H, Tq, Tk], scaled by 1 / (1 - p)), out = Pd V; an item without keys gives zero rows
    and lse = +inf.  Returns out [D, B, T], lse [B, H, T], P, S and, with dout, the gradient [3 D, B, T] by autograd."""
    D3, B, T = qkv.shape
    D = D3 // 3
    dh = D // H
    x = qkv.clone().requires_grad_(dout is not None)
    q, k, v = [t.reshape(H, dh, B, T) for t in x.split(D, dim=0)]
    S = torch.einsum("hdbq,hdbk->bhqk", q, k) * dh ** -0.5
    lens_t = torch.as_tensor(lens)
    dead = (torch.arange(T)[None, :] >= lens_t[:, None])[:, None, None, :] & (lens_t > 0)[:, None, None, None]
    Sm = S.masked_fill(dead, float("-inf"))
    P = torch.softmax(Sm, -1) * (lens_t > 0).double()[:, None, None, None]
    lse = torch.logsumexp(Sm, -1).masked_fill((lens_t == 0)[:, None, None], float("inf"))
    Pd = P if keep is None else P * keep / (1.0 - p)
    out = torch.einsum("bhqk,hdbk->hdbq", Pd, v).reshape(D, B, T)
    grad = None
    if dout is not None:
        out.backward(dout)
        grad = x.grad
    return out.detach(), lse.detach(), P.detach(), S.detach(), grad


@functools.lru_cache(maxsize=None)
def at_case(dh, T, variant):
    D = AT_H * dh
    g = torch.Generator().manual_seed(dh * 1000 + T + (variant == "one"))
    qkv, dout = torch.randn(3 * D, AT_B, T, generator=g), torch.randn(D, AT_B, T, generator=g)
    lens = at_lens(T, variant)
    out, lse, P, S, grad = at_ref(qkv.double(), lens, AT_H, dout.double())
    return dict(qkv=qkv, dout=dout, lens=lens, out=out, lse=lse, P=P, S=S, grad=grad)


def at_f32_bounds(c, dh, T):
    """First-order bounds of the fp32 kernels (exact fp32 products in the matrix cores, fp32 accumulation), from the float64 reference:
    S: scale and the pre-scaled operand one rounding each, dh accumulations: d_S = gamma(dh + 2) scale sum |q| |k|.
    forward: e = expf(S - m) with m a computed score: relative d_e = 2 max_k d_S + 2 u max|S| + E; the running sum over len keys in
      n_t = ceil(len / 32) tiles, each rescaled by expf(m_old - m_new): d_l = d_e + gamma(len) + n_t (E + 3 u); out = acc / l with acc the
      same sums weighted by V: (d_e + d_l + 3 u) sum_k P |V| + u |out|; lse = m + logf(l): max d_S + d_l + E log(len) + 2 u |lse|.
    backward, from the saved (reference, fp32-rounded) out and lse: P = expf(S - lse): relative d_P = d_S + u |lse| + u |S - lse| + E;
      D = sum_d dO O: (gamma(dh) + u) sum |dO| |O|; dPd = dO V: gamma(dh) sum |dO| |V|; dS = P (dPd - D): d_P |dS| + P (d_dP + d_D) +
      2 u P (|dPd| + |D|); dQ = scale sum_k dS K over len keys, dK = scale sum_q dS Q over T queries: the dS errors through |K| (|Q|)
      plus gamma(n + 2) of the magnitudes; dV = sum_q P dO: d_P and gamma(T + 1) of sum_q P |dO|."""
    H, B, D = AT_H, AT_B, AT_H * dh
    scale = dh ** -0.5
    q, k, v = [t.double().reshape(H, dh, B, T) for t in c["qkv"].split(D, dim=0)]
    do = c["dout"].double().reshape(H, dh, B, T)
    lens_t = torch.tensor(c["lens"])
    live = (torch.arange(T)[None, :] < lens_t[:, None])[:, None, None, :].expand(B, H, T, T)
    P, S = c["P"], c["S"]
    d_S = gamma(dh + 2) * scale * torch.einsum("hdbq,hdbk->bhqk", q.abs(), k.abs())
    dSmax = torch.where(live, d_S, torch.zeros(())).amax(-1)
    Smax = torch.where(live, S.abs(), torch.zeros(())).amax(-1)
    ln = lens_t.double()[:, None, None]
    n_t = torch.ceil(ln / 32)
    d_e = 2 * dSmax + 2 * U * Smax + E
    d_l = d_e + ln * U * 1.001 + n_t * (E + 3 * U)
    out = c["out"].reshape(H, dh, B, T)
    b_out = (torch.einsum("bhqk,hdbk->hdbq", P, v.abs()) * (d_e + d_l + 3 * U).permute(1, 0, 2)[:, None] + U * out.abs()).reshape(D, B, T)
    lse0 = c["lse"].masked_fill(lens_t[:, None, None] == 0, 0.0)
    b_lse = dSmax + d_l + E * torch.log(ln.clamp_min(1)) + 2 * U * lse0.abs()
    d_P = d_S + U * lse0.abs()[..., None] + U * (S - lse0[..., None]).abs() + E
    of = out.float().double()
    Dq = torch.einsum("hdbq,hdbq->bhq", do, of)
    d_D = (gamma(dh) + U) * torch.einsum("hdbq,hdbq->bhq", do.abs(), of.abs())
    dP = torch.einsum("hdbq,hdbk->bhqk", do, v)
    d_dP = gamma(dh) * torch.einsum("hdbq,hdbk->bhqk", do.abs(), v.abs())
    dS = P * (dP - Dq[..., None])
    d_dS = d_P * dS.abs() + P * (d_dP + d_D[..., None]) + 2 * U * P * (dP.abs() + Dq.abs()[..., None])
    b_dq = scale * (torch.einsum("bhqk,hdbk->hdbq", d_dS, k.abs()) + gamma(T + 2) * torch.einsum("bhqk,hdbk->hdbq", dS.abs(), k.abs()))
    b_dk = scale * (torch.einsum("bhqk,hdbq->hdbk", d_dS, q.abs()) + gamma(T + 2) * torch.einsum("bhqk,hdbq->hdbk", dS.abs(), q.abs()))
    b_dv = torch.einsum("bhqk,hdbq->hdbk", d_P * P, do.abs()) + gamma(T + 1) * torch.einsum("bhqk,hdbq->hdbk", P, do.abs())
    b_grad = torch.cat([t.reshape(D, B, T) for t in (b_dq, b_dk, b_dv)]) + 2 * U * c["grad"].abs()
    return b_out, b_lse, b_grad


@pytest.mark.parametrize("variant", ["odd", "one"])
@pytest.mark.parametrize("T", AT_T)
@pytest.mark.parametrize("dh", AT_DH)
def test_attention_train_f32_tile_edges(cuda_device, dh, T, variant):
    """evmi_mha_fwd_f32 / evmi_mha_bwd_f32 without dropout, lens = [T, an odd length (or 1), 0]: out, lse and dq / dk / dv against float64
    autograd of the explicit attention within at_f32_bounds; the empty item's out and gradients exactly 0 and its lse +inf; gradients
    at padded keys exactly 0; a second backward bit-equal (one writer per element, fixed order).  The backward takes the reference's out
    and lse rounded to fp32 (its inputs are then the test's own; the empty item's lse is +inf as the forward writes it)."""
    dev = cuda_device
    c = at_case(dh, T, variant)
    D, B = AT_H * dh, AT_B
    b_out, b_lse, b_grad = at_f32_bounds(c, dh, T)
    qkv, lens32 = c["qkv"].to(dev), i32(c["lens"], dev)
    out, lse = at_fwd(dev, qkv, lens32, dh, "f32")
    out, lse = out.cpu(), lse.cpu()
    what = f"mha f32 dh {dh} T {T} lens {c['lens']}"
    assert (out[:, 2] == 0).all() and (lse[2] == float("inf")).all(), "the empty item"
    assert_within(out, c["out"], b_out, what + " out")
    assert_within(lse[:2], c["lse"][:2], b_lse[:2], what + " lse")
    args = (qkv, lens32, c["out"].float().to(dev), c["lse"].float().to(dev), c["dout"].to(dev), dh, "f32")
    dqkv = at_bwd(dev, *args).cpu()
    assert same_bits(at_bwd(dev, *args).cpu(), dqkv), "the backward is not reproducible"
    assert (dqkv[:, 2] == 0).all(), "the empty item's gradients"
    assert (dqkv[D:, 1, c["lens"][1]:] == 0).all(), "gradients at padded keys"
    assert_within(dqkv, c["grad"], b_grad, what + " dqkv")


@pytest.mark.parametrize("variant", ["odd", "one"])
@pytest.mark.parametrize("T", AT_T)
@pytest.mark.parametrize("dh", AT_DH)
def test_attention_train_bf16_tile_edges(cuda_device, dh, T, variant):
    """evmi_mha_fwd_bf16 / evmi_mha_bwd_bf16 at the same edges, by the criteria of test_attention_training_bf16_operands: out within 1e-2 of
    its scale; each gradient block (dq, dk, dv) cosine >= 0.999 and norm within 1 %.  The exact zeros as in fp32.  Where a reference
    block is zero in exact arithmetic -- dq and dk of an item with ONE key: P = 1, D = dO.O = dO.V = dPd, dS = 0 -- the cosine says
    nothing (T = 1: the whole block) and would hide an error on that item otherwise, so that item is held to an absolute floor: dPd from
    bf16-rounded dO and V (2 ub + ub^2 of sum |dO| |V|, fp32 accumulation gamma(dh)) against D from the forward's out (V and the
    probability rounded to bf16: 2 ub, the fp32 dot gamma(dh) + u): |dS| <= (4 ub (1 + ub) + 2 gamma(dh) + u) sum_d |dO| |V|, rounded to
    bf16 and multiplied by the bf16-rounded K (Q) and the scale: (1 + ub)^2 more; dk sums that over the T queries."""
    dev = cuda_device
    c = at_case(dh, T, variant)
    D, B, H = AT_H * dh, AT_B, AT_H
    qkv, lens32 = c["qkv"].to(dev), i32(c["lens"], dev)
    out, lse = at_fwd(dev, qkv, lens32, dh, "bf16")
    what = f"mha bf16 dh {dh} T {T} lens {c['lens']}"
    assert (out[:, 2] == 0).all() and (lse[2] == float("inf")).all(), "the empty item"
    err, scale_o = float((out.cpu() - c["out"]).abs().max()), float(c["out"].abs().max())
    print(what, f"out err / scale {err / scale_o:.2e}")
    assert err <= 1e-2 * scale_o, (what, err, scale_o)
    args = (qkv, lens32, out, lse, c["dout"].to(dev), dh, "bf16")
    dqkv = at_bwd(dev, *args).cpu()
    assert same_bits(at_bwd(dev, *args).cpu(), dqkv), "the backward is not reproducible"
    assert (dqkv[:, 2] == 0).all(), "the empty item's gradients"
    assert (dqkv[D:, 1, c["lens"][1]:] == 0).all(), "gradients at padded keys"
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        a, w = dqkv[sl].double().flatten(), c["grad"][sl].flatten()
        if float(w.norm()) == 0.0:
            continue  # (T = 1: held to the floor below)
        cos, ratio = float(torch.dot(a, w) / (a.norm() * w.norm())), float(a.norm() / w.norm())
        print(what, name, f"cosine {cos:.6f} norm ratio {ratio:.5f}")
        assert cos >= 0.999 and 0.99 <= ratio <= 1.01, (what, name, cos, ratio)
    ones = [b for b in range(2) if c["lens"][b] == 1]
    assert ones or not (variant == "one" or T == 1)
    q, k, v = [t.double().reshape(H, dh, B, T) for t in c["qkv"].split(D, dim=0)]
    do = c["dout"].double().reshape(H, dh, B, T)
    for b in ones:
        assert float(c["grad"][: 2 * D, b].abs().max()) < 1e-12  # zero in exact arithmetic (float64: its own rounding)
        floor_ds = (4 * UB * (1 + UB) + 2 * gamma(dh) + U) * torch.einsum("hdq,hd->hq", do[:, :, b].abs(), v[:, :, b, 0].abs())  # [H, Tq]
        f = dh ** -0.5 * (1 + UB) ** 3
        floor_dq = f * floor_ds[:, None, :] * k[:, :, b, 0].abs()[:, :, None]                    # [H, dh, Tq]
        floor_dk = f * torch.einsum("hq,hdq->hd", floor_ds, q[:, :, b].abs())                    # [H, dh]: key 0
        assert_within(dqkv[:D, b], torch.zeros(D, T, dtype=torch.float64), floor_dq.reshape(D, T), what + f" dq of item {b} (one key)")
        assert_within(dqkv[D : 2 * D, b, 0], torch.zeros(D, dtype=torch.float64), floor_dk.reshape(D), what + f" dk of item {b} (one key)")


def test_attention_train_refusals(cuda_device):
    """A head dimension the specialised entries were not built for is EVMI_ERR_UNSUPPORTED (the generic entries take it); heads that do not
    divide D, p = 1, no positions and a missing buffer are invalid arguments.  out, lse and dqkv stay as they were (the backward's row dot
    D = dO.O runs ahead of the head-dimension switch: dsum is scratch)."""
    dev = cuda_device
    B, T, D, H = 2, 8, 96, 2  # dh = 48
    qkv, lens32 = torch.zeros(3 * D, B, T, device=dev), i32([T, T], dev)
    out, lse, dqkv, dsum = guarded(D * B * T, dev), guarded(B * H * T, dev), guarded(3 * D * B * T, dev), guarded(B * H * T, dev)
    zeros = torch.zeros(D * B * T, device=dev)
    for op in ("f32", "bf16"):
        fwd, bwd = getattr(lib(), f"evmi_mha_fwd_{op}"), getattr(lib(), f"evmi_mha_bwd_{op}")
        assert call(fwd, qkv, lens32, out, lse, B, T, D, H, 0.0, 0, None, stream(dev)) == UNSUPPORTED
        assert call(bwd, qkv, lens32, zeros, zeros, zeros, dsum, dqkv, B, T, D, H, 0.0, 0, None, stream(dev)) == UNSUPPORTED
        for b_, t_, h_, p_, o_ in ((B, T, 5, 0.0, out), (B, T, H, 1.0, out), (B, 0, H, 0.0, out), (0, T, H, 0.0, out), (B, T, H, 0.0, None)):
            assert call(fwd, qkv, lens32, o_, lse, b_, t_, D, h_, p_, 0, None, stream(dev)) == INVALID_ARG
            assert call(bwd, qkv, lens32, zeros, zeros, zeros, dsum, None if o_ is None else dqkv, b_, t_, D, h_, p_, 0, None, stream(dev)) == INVALID_ARG
    torch.cuda.synchronize()
    assert torch.isnan(out[: D * B * T]).all() and torch.isnan(lse[: B * H * T]).all() and torch.isnan(dqkv[: 3 * D * B * T]).all()
    assert guard_ok(dsum, B * H * T)


# ---- mask read-out probes: every kernel's regenerated dropout mask against tests/dropout_ref.py, bit by bit -----------------------------
PROBE_P, PROBE_SEED = 0.3, 2 ** 32 - 2  # (stream seed + 1 = 2^32 - 1, head 1: the low word's last value)
PROBE_SHAPES = [(96, (96, 33, 1)), (97, (97, 64, 0))]
PROBE_CASES = [(op, dh, i) for op in ("f32", "bf16") for dh in (32, 64) for i in range(2)] + [("bf16", 48, 0)]


@functools.lru_cache(maxsize=None)
def probe_keep(T):
    return torch.from_numpy(dropout_ref.attention_keep(PROBE_SEED, AT_B, AT_H, T, PROBE_P))


def probe_check(got, want, lens, unit_of_item, operands, what, shift=None):
    """got / want [rows, B, T'] per item: the mask first -- an element is `on` where it (plus `shift`, the level of a dropped element
    taken from the reference) exceeds half the unit a kept probability adds -- then the values: fp32 within ((2 + log len) E + gamma(len)
    + 16 u) of the unit (expf of a score minus lse = m + logf(l), whose logf costs E log(len); the running sum over len keys; a handful of
    roundings), bf16 within the project's 1e-2 of the item's scale.  A wrong mask bit moves an element by the unit: 100 x either
    criterion."""
    for b, ln in enumerate(lens):
        g, w = got[:, b].double(), want[:, b]
        if ln == 0:
            assert (g == 0).all(), what + f": item {b} is empty"
            continue
        unit = unit_of_item(ln)
        s = 0.0 if shift is None else shift[:, b]
        on_g, on_w = (g + s).abs() > 0.5 * unit, (w + s).abs() > 0.5 * unit
        assert torch.equal(on_g, on_w), what + f": item {b} (len {ln}): {int((on_g != on_w).sum())} mask bits differ from the restated generator, first at {(on_g != on_w).nonzero()[0].tolist()}"
        tol = ((2 + math.log(ln)) * E + gamma(ln) + 16 * U) * unit if operands == "f32" else 1e-2 * float(w.abs().max())
        if operands == "bf16" and float(w.abs().max()) < 1e-9 * unit:
            # a block that is zero in exact arithmetic (dQ of a one-key item: dS = P (mask / (1 - p) - D) with D = that same value) has
            # no scale: D comes from the forward's out, whose ONE probability mask / (1 - p) was rounded to bf16 (ub of it), against the
            # fp32 mask / (1 - p) of the backward (u, and u for the difference); dS is rounded to bf16 on its way to the matrix cores
            tol = (UB + 2 * U) * (1 + UB) * unit
        err = float((g - w).abs().max())
        assert err <= tol, what + f": item {b} (len {ln}): err {err:.3e} > {tol:.3e}"


@pytest.mark.parametrize("operands,dh,shape", PROBE_CASES)
def test_attention_dropout_mask_read_out(cuda_device, operands, dh, shape):
    """With Q = 0 every live key has probability 1 / len, and one-hot operands read single elements of the dropped-out probabilities
    Pd[q][k] = keep(seed + h, (b T + q) T + k) / ((1 - p) len) out of each kernel, a tile of dh keys (queries) per launch:
      forward   V[d][k] = [k = dh j + d]:                              out[d][q] = Pd[q][dh j + d]
      dK / dV   dO[d][q] = [q = dh i + d] (V = 0):                     dV[d][k]  = Pd[dh i + d][k]
      dQ        V[0][k] = 1, dO[0][q] = 1, K[d][k] = [k = dh j + d]:   dQ[d][q]  = scale dS[q][dh j + d], dS = (Pd - P sum_k Pd) -- one
                mask bit moves it by scale / ((1 - p) len)
    against float64 autograd of the explicit attention under dropout_ref's mask.  T = 96 takes the bf16 kernels' pair paths (one hash per
    two keys in-thread; per parity with a lane exchange in the dK / dV kernel), T = 97 and the fp32 kernels the per-element path; the
    lengths put an odd length inside the even T, a partial last tile, clamped queries behind T and a one-key item."""
    dev = cuda_device
    T, lens = PROBE_SHAPES[shape]
    H, B, D = AT_H, AT_B, AT_H * dh
    keep = probe_keep(T).double()
    lens32 = i32(lens, dev)
    kq = 1.0 / (1.0 - PROBE_P)
    scale = dh ** -0.5
    tiles = (T + dh - 1) // dh
    onehot = torch.zeros(tiles, dh, T)  # [tile j][d][t] = [t = dh j + d]
    for j in range(tiles):
        for d in range(min(dh, T - dh * j)):
            onehot[j, d, dh * j + d] = 1.0
    what = f"mask read-out {operands} dh {dh} T {T}"

    def qkv_of(kpart, vpart):  # [dh, T] patterns, the same for every head and item; Q = 0
        x = torch.zeros(3, H, dh, B, T)
        x[1] = kpart[None, :, None, :]
        x[2] = vpart[None, :, None, :]
        return x.reshape(3 * D, B, T)

    def heads(pattern):  # [dh, T] -> [D, B, T]
        return pattern[None, :, None, :].expand(H, dh, B, T).reshape(D, B, T).contiguous()

    zero = torch.zeros(dh, T)
    row0 = torch.zeros(dh, T)
    row0[0] = 1.0
    for j in range(tiles):
        # forward
        x = qkv_of(zero, onehot[j])
        want, _, _, _, _ = at_ref(x.double(), list(lens), H, None, keep, PROBE_P)
        out, _ = at_fwd(dev, x.to(dev), lens32, dh, operands, PROBE_P, PROBE_SEED)
        probe_check(out.cpu(), want, lens, lambda ln: kq / ln, operands, what + f" forward, key tile {j}")
        # dK / dV kernel: V = 0 -> out = 0, dq = dk = 0, dV reads the mask's rows dh j ..
        x = qkv_of(zero, zero)
        do = heads(onehot[j])
        _, _, _, _, grad = at_ref(x.double(), list(lens), H, do.double(), keep, PROBE_P)
        xg = x.to(dev)
        out, lse = at_fwd(dev, xg, lens32, dh, operands, PROBE_P, PROBE_SEED)
        dqkv = at_bwd(dev, xg, lens32, out, lse, do.to(dev), dh, operands, PROBE_P, PROBE_SEED).cpu()
        assert (dqkv[: 2 * D] == 0).all(), what + " dq / dk with V = 0"
        probe_check(dqkv[2 * D :], grad[2 * D :], lens, lambda ln: kq / ln, operands, what + f" dV, query tile {j}")
        # dQ kernel
        x = qkv_of(onehot[j], row0)
        do = heads(row0)
        want_out, _, _, _, grad = at_ref(x.double(), list(lens), H, do.double(), keep, PROBE_P)
        xg = x.to(dev)
        out, lse = at_fwd(dev, xg, lens32, dh, operands, PROBE_P, PROBE_SEED)
        dqkv = at_bwd(dev, xg, lens32, out, lse, do.to(dev), dh, operands, PROBE_P, PROBE_SEED).cpu()
        # dS = P (mask / (1 - p) - D): a kept element holds scale (kq - D) / len, a dropped one -scale D / len, D = sum_k Pd about 1: the
        # two differ by scale kq / len.  Shifted by the reference's dropped level the probe reads as `on` / `off` like the others.
        Dq = want_out.reshape(H, dh, B, T)[:, 0]  # out[0][q] = D [H, B, T]
        shift = torch.zeros(H, dh, B, T, dtype=torch.float64)
        for b, ln in enumerate(lens):
            if ln:
                shift[:, :, b] = (scale / ln) * Dq[:, None, b, :]
        kd = onehot[j].sum(1)  # channels d whose key dh j + d exists
        keyed = torch.zeros(H, dh, B, T, dtype=torch.float64)
        for b, ln in enumerate(lens):
            keyed[:, :, b] = (kd[:, None] * (dh * j + torch.arange(dh)[:, None] < ln)).double()[None]
        shift = (shift * keyed).reshape(D, B, T)
        probe_check(dqkv[:D], grad[:D], lens, lambda ln: scale * kq / ln, operands, what + f" dQ, key tile {j}", shift)
