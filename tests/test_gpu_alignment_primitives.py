"""The alignment-learning kernels (csrc/align_train_ops.hip and the alignment part of csrc/fs2_ops.hip), one entry point at a time,
at the boundaries of the path the launcher picks: the NS = 1 / 2 / 4 instantiations of forward_sum_grad_kernel (512 threads, NS states
of the extended target each), the second and third trip of every 256-stride loop, the LDS limits and the refusals.

Assertions as in tests/test_gpu_primitives.py: (a) position probes bit for bit, (b) float64 references with a bound evaluated from
the operation (gamma_n, MATH_ULP per device math call), (c) torch.equal where the arithmetic is exact.  The log-domain CTC
recurrences have no usable closed bound (fp32 loses digits as the lattice grows).  There the bound is MEASURED AGAINST THE
REFERENCE, on the same input and in the same norm: err32 = error of torch-CPU fp32 ``forward_sum_loss_ref`` (loss / per-item gradient)
against the float64 one, and the kernel must stay within 4 x max(err32, 1e-6 x scale) -- scale = |loss| for a loss and the kernel's own
scale = weight / (B L_b) for a gradient entry (sqrt(T_b L_b) of them in the L2 norm); the factor covers the order of the three-way
log-add and device expf / log1pf at MATH_ULP = 4 ulp against the CPU's <= 1.  A dropped, doubled or misplaced lattice state is an
error of the order of the scale itself; ``test_ctc_calibration`` asserts, without a GPU, that 4 x err32 < 0.05 x scale on every input.

Measured kernel_err / max(err32, 1e-6 scale) on an MI355X (the worst item of each shape; the bound is 4):

    entry point                 T     L   NS   loss   grad max-norm   grad rel-L2
    evmi_forward_sum_grad_f32   272   255   1   0.13       1.12           0.97
                                273   256   2   1.16       1.09           1.08
                                528   511   2   0.29       1.43           1.67
                                529   512   4   0.49       0.98           1.02
                               1040  1023   4   0.67       1.07           1.04
                                947   187   1   0.69       1.40           1.00     (the benchmark's longest utterance)
    evmi_forward_sum_loss_f32   272 .. 1040: the same loss column (the two kernels' losses agree to the digits shown); 317 / 300: 0.22
    align backward, dq | dk     266   256   2   without prior 3.28 | 2.48, with prior 1.14 | 1.15    (worst of both norms and items)
                                267   257   2   without prior 1.65 | 1.14, with prior 1.86 | 1.53
                                710   700   4   without prior 1.36 | 1.07, with prior 0.85 | 0.83

The one-token item's only gradient entry is the residual scale (p - 1), here 0.0041 scale: the kernel's error there is 2.3e-8 scale,
below one ulp of p; measured against the entry itself (5.6e-6 of it) it would exceed torch's fp32 result on that one number (6.7e-8)
eighty-fold -- which is why the floor is stated in the kernel's scale and not in the item's largest entry.
"""

import functools
import math

import pytest
import torch

from everyvoice_amd import _lib
from helpers import E, MATH_ULP, NAN, TINY, U, assert_within, f32, gamma, same_bits  # noqa: F401
from oracle.alignment_ref import alignment_attention_ref, binarization_loss_ref, forward_sum_loss_ref
from oracle.mas_ref import maximum_path_batch_ref

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = 1, _lib.EVMI_ERR_UNSUPPORTED
BLANK = -1.0
FACTOR = 4.0     # kernel error <= FACTOR * max(err32, FLOOR * scale): see the module docstring
FLOOR = 1e-6


def call(fn, *args):
    """fn(...) with tensors passed as their pointers (None as NULL); the tensors stay referenced until the launch has been issued --
    a temporary `t.to(dev)` dropped earlier would hand its block to the next allocation."""
    return fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else 0 if a is None else a for a in args])


def stream(dev):
    return _lib.current_stream_ptr(dev)


def i32(values, dev):
    return torch.tensor(list(values), dtype=torch.int32, device=dev)


# =====================================================================================================================
# CTC forward-sum: selection rule, references, calibration
# =====================================================================================================================
def ns_of(L):
    """evmi_forward_sum_grad_f32: ceil((2 L + 1) / 512) states per thread; the instantiations are 1, 2 and 4 (3 runs as 4)."""
    ns = (2 * L + 1 + 511) // 512
    return ns, (1 if ns == 1 else 2 if ns == 2 else 4)


def test_ns_selection_restated():
    assert [ns_of(L) for L in (255, 256, 511, 512, 767, 768, 1023)] == [(1, 1), (2, 2), (2, 2), (3, 4), (3, 4), (4, 4), (4, 4)]
    assert ns_of(187) == (1, 1) and ns_of(300) == (2, 2)  # the benchmark's lattice; the extra forward-only length
    assert 2 * 1023 + 1 <= 4 * 512 < 2 * 1024 + 1         # L = 1024 has more states than 512 threads x 4


def ragged(L):
    """B = 3: the whole lattice; an exactly feasible item (one frame per token); one token on one frame."""
    T = L + 17
    return (L, T, (L, L // 2 + 1, 1), (T, L // 2 + 1, 1))


# L 255: NS 1 (511 states, one below the stride of 512)      L 256: NS 2 (513 states, the first state of the second trip)
# L 511: NS 2 (1023 states, one below two strides)           L 512: ns = 3 runs the NS 4 instantiation (1025 states)
# L 1023: NS 4, all 2047 of 2048 slots, the largest L        (947, 187): the benchmark's longest utterance, NS 1
GRAD_CASES = [ragged(L) for L in (255, 256, 511, 512, 1023)] + [(187, 947, (187, 140), (947, 733))]
# the forward-only kernel strides 256 over the states: L 300 is 601 states, two full trips and a third (forward_sum_grad: NS 2)
LOSS_CASES = GRAD_CASES[:5] + [ragged(300)]
WEIGHT = f32(0.3)


def case_id(case):
    return f"L{case[0]}-T{case[1]}"


def _ref_run(lp, text_lens, mel_lens, weight):
    """(per-item losses, gradient of weight * mean loss) of oracle.alignment_ref.forward_sum_loss_ref in lp's precision."""
    lp = lp.clone().requires_grad_()
    B = lp.shape[0]
    tl, ml = torch.tensor(text_lens), torch.tensor(mel_lens)
    per_item = [forward_sum_loss_ref(lp[b : b + 1], tl[b : b + 1], ml[b : b + 1], BLANK) for b in range(B)]
    (weight * sum(per_item) / B).backward()
    return torch.stack([p.detach() for p in per_item]), lp.grad


@functools.lru_cache(maxsize=None)
def ctc_reference(case, std=2.0):
    """Input (fixed seed), float64 reference and the fp32-versus-float64 calibration of one case.  Computed once, shared, read only."""
    L, T, text_lens, mel_lens = case
    B = len(text_lens)
    g = torch.Generator().manual_seed(1000 * L + T)
    lp = torch.randn(B, T, L, generator=g) * std
    loss64, grad64 = _ref_run(lp.double(), text_lens, mel_lens, float(WEIGHT))
    loss32, grad32 = _ref_run(lp, text_lens, mel_lens, float(WEIGHT))
    ref = dict(lp=lp, loss64=loss64, grad64=grad64, B=B)
    ref["loss_bound"] = FACTOR * torch.maximum((loss32.double() - loss64).abs(), FLOOR * loss64.abs())
    ref["loss_err32"] = (loss32.double() - loss64).abs()
    e32 = grad_errors(grad32, grad64)
    ref["grad_err32"] = e32
    ref["grad_max64"] = grad64.abs().flatten(1).max(1).values
    # the gradient's scale: grad = scale (p - occupancy) with scale = weight / (B L_b) and p, occupancy in [0, 1], each an fp32 number
    # of that size.  (NOT the item's largest entry: the one-token item's only entry is the residual p - 1, 0.01 scale or less.)
    ref["grad_scale"] = torch.tensor([float(WEIGHT) / (B * n) for n in text_lens], dtype=torch.float64)
    cells = torch.tensor([float(n * m) for n, m in zip(text_lens, mel_lens)], dtype=torch.float64)
    ref["grad_bound_max"] = FACTOR * torch.maximum(e32["max"], FLOOR * ref["grad_scale"])
    ref["grad_bound_l2"] = FACTOR * torch.maximum(e32["l2"], FLOOR * ref["grad_scale"] * cells.sqrt() / grad64.flatten(1).norm(dim=1))
    return ref


def grad_errors(got, want64):
    """Per item: the largest absolute error, and the relative L2 error."""
    d = (got.detach().cpu().double() - want64).flatten(1)
    return dict(max=d.abs().max(1).values, l2=d.norm(dim=1) / want64.flatten(1).norm(dim=1).clamp_min(1e-300))


@pytest.mark.parametrize("case", GRAD_CASES + LOSS_CASES[5:], ids=case_id)
def test_ctc_calibration(case):
    """No GPU: every CTC input has a finite float64 reference with a positive loss per item, and 4 x err32 stays below 0.05 of the
    scale in both norms: an error of the order of the scale (a misplaced state) is >= 20 x outside the bound the kernel gets."""
    ref = ctc_reference(case)
    assert torch.isfinite(ref["loss64"]).all() and (ref["loss64"] > 0).all() and torch.isfinite(ref["grad64"]).all()
    assert (ref["loss_bound"] < 0.05 * ref["loss64"].abs()).all(), (ref["loss_err32"], ref["loss64"])
    assert (ref["grad_bound_max"] < 0.05 * ref["grad_max64"]).all(), (ref["grad_err32"]["max"], ref["grad_max64"])
    assert (ref["grad_bound_l2"] < 0.05).all(), ref["grad_err32"]["l2"]
    print(f"calibration {case_id(case)}: loss err32 / loss {(ref['loss_err32'] / ref['loss64']).tolist()}  "
          f"grad err32 max / largest entry {(ref['grad_err32']['max'] / ref['grad_max64']).tolist()}  rel-L2 {ref['grad_err32']['l2'].tolist()}")


def run_forward_sum_grad(dev, lp, text_lens, mel_lens, weight, ws_short=0, fill=NAN):
    """evmi_forward_sum_grad_f32 -> (rc, loss [B], grad [B, T, L]); both outputs start as `fill`."""
    lib = _lib.load()
    B, T, L = lp.shape
    n = lib.evmi_forward_sum_grad_f32_ws_elems(B, T, L)
    assert n == B * T * (2 * L + 1) + B * T
    ws = torch.empty(n, device=dev)
    loss = torch.full((B,), fill, device=dev)
    grad = torch.full((B, T, L), fill, device=dev)
    lpd, tl, ml = lp.to(dev), i32(text_lens, dev), i32(mel_lens, dev)
    rc = call(lib.evmi_forward_sum_grad_f32, lpd, tl, ml, loss, grad, ws, n - ws_short,
                                       B, T, L, BLANK, weight, stream(dev))
    torch.cuda.synchronize()
    return rc, loss.cpu(), grad.cpu()


def run_forward_sum_loss(dev, lp, text_lens, mel_lens, fill=NAN):
    B, T, L = lp.shape
    loss = torch.full((B,), fill, device=dev)
    lpd, tl, ml = lp.to(dev), i32(text_lens, dev), i32(mel_lens, dev)
    rc = call(_lib.load().evmi_forward_sum_loss_f32, lpd, tl, ml, loss, B, T, L, BLANK, stream(dev))
    torch.cuda.synchronize()
    return rc, loss.cpu()


RATIOS = {}  # test -> measured ratios; every test prints them as well (run with -s to collect the docstring's table)


def check_ctc(ref, loss, grad, what):
    """The assertions of the calibrated bound; every message carries kernel_err / max(err32, floor)."""
    loss_err = (loss.double() - ref["loss64"]).abs()
    loss_ratio = FACTOR * loss_err / ref["loss_bound"]
    msg = f"{what}: loss err / max(err32, 1e-6 scale) per item = {[round(float(r), 3) for r in loss_ratio]}"
    ratios = dict(loss=float(loss_ratio.max()))
    if grad is not None:
        e = grad_errors(grad, ref["grad64"])
        rmax, rl2 = FACTOR * e["max"] / ref["grad_bound_max"], FACTOR * e["l2"] / ref["grad_bound_l2"]
        ratios.update(grad_max=float(rmax.max()), grad_l2=float(rl2.max()))
        msg += f"; gradient max-norm {[round(float(r), 3) for r in rmax]}, rel-L2 {[round(float(r), 3) for r in rl2]}"
    RATIOS[what] = ratios
    print("RATIO", msg)
    assert torch.isfinite(loss).all(), msg
    assert (loss_err <= ref["loss_bound"]).all(), msg
    if grad is not None:
        assert torch.isfinite(grad).all(), msg
        assert (e["max"] <= ref["grad_bound_max"]).all(), msg
        assert (e["l2"] <= ref["grad_bound_l2"]).all(), msg


@pytest.mark.parametrize("case", GRAD_CASES, ids=case_id)
def test_forward_sum_grad_across_ns(cuda_device, case):
    """Loss per item and per call, gradient per item (max norm and relative L2) within the calibrated bound; exact zeros outside the
    item's frames and tokens (the buffer starts as NaN); a second call gives the same bits."""
    L, T, text_lens, mel_lens = case
    ref = ctc_reference(case)
    rc, loss, grad = run_forward_sum_grad(cuda_device, ref["lp"], text_lens, mel_lens, WEIGHT)
    assert rc == _lib.EVMI_OK
    for b in range(ref["B"]):
        assert (grad[b, mel_lens[b] :, :] == 0.0).all() and (grad[b, :, text_lens[b] :] == 0.0).all(), f"item {b}: padding not exactly zero"
    check_ctc(ref, loss, grad, f"forward_sum_grad {case_id(case)} NS {ns_of(L)[1]}")
    call_bound = ref["loss_bound"].mean()  # the loss of the call: weight * mean of the items
    assert abs(float(WEIGHT) * (float(loss.double().mean()) - float(ref["loss64"].mean()))) <= float(WEIGHT) * float(call_bound)
    rc2, loss2, grad2 = run_forward_sum_grad(cuda_device, ref["lp"], text_lens, mel_lens, WEIGHT)
    assert rc2 == _lib.EVMI_OK and same_bits(loss, loss2) and same_bits(grad, grad2)


# ---- closed form: mel_len == text_len leaves one path ----------------------------------------------------------------------------
DIAG = 12.0  # added to logprob[t][t]: the path's normalised log-probabilities stay near 0, so their fp32 SUM (the exponent) stays small


@functools.lru_cache(maxsize=None)
def one_path_reference(L):
    """B = 2 items with mel_len == text_len (L and L // 2 + 1): the extended target has exactly one path, token t on frame t.
    With p = softmax over [blank, tokens < L_b]:  grad[t][l] = scale (p[t][l] - [l == t]),  loss = -sum_t log p[t][t] / L_b.

    Bound, rule (b).  The kernel forms y = raw - lse per state; lse = m + logf(sum of L_b + 1 expf) has
        d_lse = gamma(L_b + 1) + u R + E  (the sum and its terms, R = the row's range)  + E |log s| + u |lse|,   d_y = d_lse + u |y|.
    On the one path every log-add has a -inf partner and returns the other operand exactly, so alpha, beta and the log-likelihood are
    plain fp32 sums of the SAME fp32 y[t][t]; the occupancy exponent (alpha + beta - y) - ll is the difference of two such sums of
    T terms in different orders plus three roundings: |exponent| <= gamma(2 T + 4) sum_t |y[t][t]| =: d, and occ = expf(exponent) is
    within (e^d - 1) + E e^d of 1 on the path and exactly 0 off it.  p = expf(y): relative error d_y + E.  The subtraction, the
    product with scale and scale = weight / (B * L_b) itself add 4 u of the result."""
    T = L
    text_lens = mel_lens = (L, L // 2 + 1)
    B = 2
    g = torch.Generator().manual_seed(77 + L)
    lp = torch.randn(B, T, L, generator=g) * 0.5
    idx = torch.arange(L)
    lp[:, idx, idx] += DIAG
    weight = float(WEIGHT)
    loss64, grad64 = torch.zeros(B, dtype=torch.float64), torch.zeros(B, T, L, dtype=torch.float64)
    loss_bound, grad_bound = torch.zeros(B, dtype=torch.float64), torch.zeros(B, T, L, dtype=torch.float64)
    scales = []
    for b in range(B):
        Lb = text_lens[b]
        raw = torch.cat([torch.full((Lb, 1), BLANK, dtype=torch.float64), lp[b, :Lb, :Lb].double()], 1)  # [T_b, 1 + L_b]
        m = raw.max(1).values
        s = torch.exp(raw - m[:, None]).sum(1)
        lse = m + torch.log(s)
        y = raw - lse[:, None]
        R = (m[:, None] - raw).max(1).values
        d_lse = gamma(Lb + 1) + U * R + E + E * torch.log(s).abs() + U * lse.abs()
        d_y = d_lse[:, None] + U * y.abs()
        p = torch.exp(y)
        scale = weight / (B * Lb)
        scales.append(scale)
        on_path = torch.eye(Lb, dtype=torch.float64)
        y_path = y[idx[:Lb], idx[:Lb] + 1]
        d = gamma(2 * Lb + 4) * (y_path.abs() + d_y[idx[:Lb], idx[:Lb] + 1]).sum()
        d_occ = math.expm1(float(d)) + E * math.exp(float(d))
        want = scale * (p[:, 1:] - on_path)
        grad64[b, :Lb, :Lb] = want
        grad_bound[b, :Lb, :Lb] = scale * (p[:, 1:] * (torch.expm1(d_y[:, 1:]) + E * torch.exp(d_y[:, 1:])) + on_path * d_occ) + 4 * U * want.abs()
        loss64[b] = -y_path.sum() / Lb
        loss_bound[b] = (gamma(Lb) * y_path.abs().sum() + d_y[idx[:Lb], idx[:Lb] + 1].sum()) / Lb + 2 * U * loss64[b].abs()
    return dict(lp=lp, text_lens=text_lens, mel_lens=mel_lens, loss64=loss64, grad64=grad64, loss_bound=loss_bound, grad_bound=grad_bound,
                scales=scales)


# L = T 256: token 255 sits in state 511 (thread 511, j 0) and no token in a second trip's first slot -- state 512 is a blank;
# 512: token 256 is state 513 (thread 1, j 1) and the NS 4 instantiation runs j 2 (state 1024: the last blank);
# 1023: tokens on both sides of the strides at states 511 | 513, 1023 | 1025, 1535 | 1537, the last token in state 2045
ONE_PATH_L = [256, 512, 1023]


@pytest.mark.parametrize("L", ONE_PATH_L)
def test_one_path_bound_is_tight_enough(L):
    """No GPU: the bound of the closed form stays below 0.05 x scale, so a state served by the wrong thread or the wrong j (an error
    of scale at its token) cannot hide; the closed form itself agrees with autograd through the reference in float64."""
    ref = one_path_reference(L)
    for b, scale in enumerate(ref["scales"]):
        assert float(ref["grad_bound"][b].max()) < 0.05 * scale, (b, float(ref["grad_bound"][b].max()), scale)
    loss64, grad64 = _ref_run(ref["lp"].double(), ref["text_lens"], ref["mel_lens"], float(WEIGHT))
    assert torch.allclose(loss64, ref["loss64"], rtol=1e-10, atol=0) and torch.allclose(grad64, ref["grad64"], rtol=1e-9, atol=1e-15)


@pytest.mark.parametrize("L", ONE_PATH_L)
def test_forward_sum_grad_one_path_closed_form(cuda_device, L):
    ref = one_path_reference(L)
    rc, loss, grad = run_forward_sum_grad(cuda_device, ref["lp"], ref["text_lens"], ref["mel_lens"], WEIGHT)
    assert rc == _lib.EVMI_OK
    assert_within(loss, ref["loss64"], ref["loss_bound"], f"one path L {L}: loss")
    assert_within(grad, ref["grad64"], ref["grad_bound"], f"one path L {L}: gradient")
    Lb = ref["text_lens"][1]
    assert (grad[1, Lb:, :] == 0.0).all() and (grad[1, :, Lb:] == 0.0).all()
    rc, loss_fwd = run_forward_sum_loss(cuda_device, ref["lp"], ref["text_lens"], ref["mel_lens"])
    assert rc == _lib.EVMI_OK  # the forward-only kernel walks the same single path: the same bound
    assert_within(loss_fwd, ref["loss64"], ref["loss_bound"], f"one path L {L}: forward-only loss")


# ---- infeasible and empty items ------------------------------------------------------------------------------------------------------
# (T, L) = (40, 9): NS 1;  (310, 300): NS 2, the forward-only kernel's third trip.  The odd item sits in front of and behind its neighbour.
@pytest.mark.parametrize("odd_first", [False, True])
@pytest.mark.parametrize("T,L", [(40, 9), (310, 300)])
@pytest.mark.parametrize("kind", ["one_frame_short", "no_text", "no_frames"])
def test_forward_sum_infeasible_and_empty_items(cuda_device, kind, T, L, odd_first):
    """Loss 0 and an all-zero gradient for the item; its neighbour bit-equal to the same item run alone (weight / 2 with B = 1 is the
    same scale weight / (B * L_b): exact halving)."""
    odd = {"one_frame_short": (L - 2, L - 3), "no_text": (0, T), "no_frames": (L, 0)}[kind]  # (text_len, mel_len)
    good = (L, T)
    g = torch.Generator().manual_seed(T + L)
    lp = torch.randn(2, T, L, generator=g) * 2
    o, n = (0, 1) if odd_first else (1, 0)
    text_lens, mel_lens = [0, 0], [0, 0]
    text_lens[o], mel_lens[o] = odd
    text_lens[n], mel_lens[n] = good
    rc, loss, grad = run_forward_sum_grad(cuda_device, lp, text_lens, mel_lens, 1.0)
    assert rc == _lib.EVMI_OK
    assert same_bits(loss[o : o + 1], torch.zeros(1)) and same_bits(grad[o], torch.zeros(T, L))
    rc, loss1, grad1 = run_forward_sum_grad(cuda_device, lp[n : n + 1], [good[0]], [good[1]], 0.5)
    assert rc == _lib.EVMI_OK and float(loss1) > 0 and float(grad1.abs().max()) > 0
    assert same_bits(loss[n : n + 1], loss1) and same_bits(grad[n : n + 1], grad1)
    rc, fwd = run_forward_sum_loss(cuda_device, lp, text_lens, mel_lens)
    rc1, fwd1 = run_forward_sum_loss(cuda_device, lp[n : n + 1], [good[0]], [good[1]])
    assert rc == rc1 == _lib.EVMI_OK and same_bits(fwd[o : o + 1], torch.zeros(1)) and same_bits(fwd[n : n + 1], fwd1)


# ---- the forward-only kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LOSS_CASES, ids=case_id)
def test_forward_sum_loss_kernel(cuda_device, case):
    """256 threads stride the 2 L + 1 states: two trips from L 128, a third at L 256 and 300, nine at L 1023.  Against float64 and
    against the loss of evmi_forward_sum_grad_f32 (another summation order: the same calibrated bound, not bit equality)."""
    L, T, text_lens, mel_lens = case
    ref = ctc_reference(case)
    rc, loss = run_forward_sum_loss(cuda_device, ref["lp"], text_lens, mel_lens)
    assert rc == _lib.EVMI_OK
    check_ctc(ref, loss, None, f"forward_sum_loss {case_id(case)}")
    rc, loss_g, _ = run_forward_sum_grad(cuda_device, ref["lp"], text_lens, mel_lens, WEIGHT)
    assert rc == _lib.EVMI_OK
    diff = (loss.double() - loss_g.double()).abs()
    assert (diff <= ref["loss_bound"]).all(), f"forward-only vs gradient kernel: |diff| / bound {(diff / ref['loss_bound']).tolist()}"


def test_forward_sum_loss_lds_limit(cuda_device):
    """(L + 1) + 2 (2 L + 1) + 8 = 5 L + 11 floats of LDS: 16381 at L 3274 (65524 bytes, accepted), 16386 at L 3275 (refused)."""
    assert (5 * 3274 + 11) * 4 <= 64 * 1024 < (5 * 3275 + 11) * 4
    g = torch.Generator().manual_seed(3274)
    lp = torch.randn(1, 8, 3274, generator=g) * 2
    rc, loss = run_forward_sum_loss(cuda_device, lp, [5], [8])
    assert rc == _lib.EVMI_OK
    want = forward_sum_loss_ref(lp.double(), torch.tensor([5]), torch.tensor([8]), BLANK)
    want32 = forward_sum_loss_ref(lp, torch.tensor([5]), torch.tensor([8]), BLANK)
    bound = FACTOR * max(abs(float(want32) - float(want)), FLOOR * abs(float(want)))
    assert abs(float(loss) - float(want)) <= bound, (float(loss), float(want), bound)
    rc, loss = run_forward_sum_loss(cuda_device, torch.zeros(1, 8, 3275), [5], [8], fill=-7.0)
    assert rc == UNSUPPORTED and float(loss) == -7.0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_forward_sum_grad_refusals(cuda_device):
    """More than 1023 tokens: EVMI_ERR_UNSUPPORTED; a workspace one element short: EVMI_ERR_INVALID_ARG; nothing is launched --
    the outputs keep their sentinel."""
    rc, loss, grad = run_forward_sum_grad(cuda_device, torch.zeros(1, 2, 1024), [2], [2], 1.0, fill=-7.0)
    assert rc == UNSUPPORTED and (grad == -7.0).all() and (loss == -7.0).all()
    rc, loss, grad = run_forward_sum_grad(cuda_device, torch.zeros(2, 12, 9), [9, 4], [12, 6], 1.0, ws_short=1, fill=-7.0)
    assert rc == INVALID_ARG and (grad == -7.0).all() and (loss == -7.0).all()
    rc, loss, grad = run_forward_sum_grad(cuda_device, torch.zeros(1, 2, 1023), [2], [2], 1.0, fill=-7.0)
    assert rc == _lib.EVMI_OK and torch.isfinite(grad).all()  # the largest accepted L


# =====================================================================================================================
# alignment attention: forward
# =====================================================================================================================
# (A, L): (1, 1) the smallest;  (80, 255) one trip of the 256-stride loops over the tokens, (80, 256) exactly one full trip,
# (80, 257) token 256 is the second trip;  (257, 40): the query load `for c < A` makes a second trip;  (300, 700): both, three trips
ATT_CASES = [(1, 1), (80, 255), (80, 256), (80, 257), (257, 40), (300, 700)]
ATT_T, ATT_B = 5, 2


def attention_inputs(A, L, T, with_prior, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(ATT_B, A, T, generator=g)
    k = torch.randn(ATT_B, A, L, generator=g)
    text_lens = torch.tensor([L, max(1, L // 3)])
    prior = None
    if with_prior:  # zero on the padded tokens, like the beta-binomial prior the trainer passes: log(0 + 1e-8) there
        prior = torch.rand(ATT_B, T, L, generator=g, dtype=torch.float64) * 0.9 + 0.05
        prior = prior.masked_fill(torch.arange(L)[None, None, :] >= text_lens[:, None, None], 0.0)
    temp = f32(2.0 / (A + 20))  # scores of the order of -4 with a spread of a few units at every A
    return q, k, text_lens, prior, temp


def cbt(x):
    return x.permute(1, 0, 2).contiguous()


def run_align_attention(dev, q, k, text_lens, prior, temp):
    from everyvoice_amd.train import ops

    soft, logprob = ops.align_attention_fwd(cbt(q).to(dev), cbt(k).to(dev), None if prior is None else prior.to(dev), text_lens.to(dev, torch.int32), temp)
    torch.cuda.synchronize()
    return soft, logprob


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("A,L", ATT_CASES)
def test_align_attention_forward(cuda_device, A, L, with_prior):
    """logprob everywhere, soft on the valid tokens (rule (b)), soft exactly 0 on the padded ones, every soft row sums to 1 within gamma(L).

    score = -temp sum_c (q - k)^2: the difference, the square (or its FMA) and the product with temp are 4 roundings around a sum of A
    terms: d_sc = (gamma(A) + 4 u) |score|.  With a prior, z = score - lse + logf((float) prior + 1e-8f): lse moves by at most max d_sc
    (it is 1-Lipschitz in the largest change) and its own evaluation costs gamma(L) + u R + E on the sum (R = the row's range),
    E |log s| for logf and u |lse| for the addition; the prior's argument carries 3 u (the cast, the sum, 1e-8f against 1e-8), its logf E;
    two more roundings form z.  soft = expf(z - m) / s over the valid tokens: a softmax moves by a factor e^(2 d) when its inputs move
    by d; expf and the argument cost E + u R each in the numerator and in the sum, the sum gamma(len), the division u."""
    q, k, text_lens, prior, temp = attention_inputs(A, L, ATT_T, with_prior, 100 * A + L)
    soft_g, logprob_g = run_align_attention(cuda_device, q, k, text_lens, prior, temp)
    soft64, logprob64 = alignment_attention_ref(q.double(), k.double(), text_lens, prior, temp)
    score = -temp * ((q.double()[:, :, :, None] - k.double()[:, :, None, :]) ** 2).sum(1)
    d_sc = (gamma(A) + 4 * U) * score.abs()
    if prior is None:
        d_z = d_sc
    else:
        m = score.max(2, keepdim=True).values
        s = torch.exp(score - m).sum(2, keepdim=True)
        lse = m + torch.log(s)
        R = (m - score).max(2, keepdim=True).values
        d_lse = d_sc.max(2, keepdim=True).values + gamma(L) + U * R + E + E * torch.log(s).abs() + U * lse.abs()
        logpr = torch.log(prior + 1e-8)
        d_z = d_sc + d_lse + U * (score - lse).abs() + 3 * U + E * logpr.abs() + U * logprob64.abs()
    assert_within(logprob_g, logprob64, d_z, f"align_attention A {A} L {L} prior {with_prior}: logprob")
    soft_c = soft_g.cpu()
    for b in range(ATT_B):
        n = int(text_lens[b])
        assert (soft_c[b, :, n:] == 0.0).all(), f"item {b}: padded tokens"
        z = logprob64[b, :, :n]
        Rz = (z.max(1, keepdim=True).values - z).max(1, keepdim=True).values
        dz = d_z[b, :, :n].max(1, keepdim=True).values
        rel = torch.expm1(2 * dz) + 2 * (E + U * Rz) + gamma(n) + 2 * U
        assert_within(soft_c[b, :, :n], soft64[b, :, :n], soft64[b, :, :n] * rel, f"align_attention A {A} L {L} prior {with_prior}: soft, item {b}")
        assert ((soft_c[b].double().sum(1) - 1.0).abs() <= gamma(L)).all(), (soft_c[b].double().sum(1) - 1.0).abs().max()


# =====================================================================================================================
# alignment attention: backward
# =====================================================================================================================
# L 256: exactly one trip of `for l < L`; 257 and 700: a second and a third; T = L + 10 so that the CTC lattice is feasible.
# A = 80 (the model's attention width): the float64 reference holds [B, A, T, L] tensors, 0.3 GB at L 700
@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("L", [256, 257, 700])
def test_align_attention_backward(cuda_device, L, with_prior):
    """dq, dk of w_ctc * forward_sum + w_bin * binarisation on the hard path of `maximum_path`, against autograd through the float64
    reference.  The loss holds the CTC recurrence: the bound is calibrated -- err32 = the error of the SAME reference evaluated in
    fp32 on the CPU (same hard path), per item, in the largest entry and in relative L2; the kernels stay within
    4 x max(err32, 1e-6 x scale)."""
    from everyvoice_amd.heavy import maximum_path
    from everyvoice_amd.train import ops

    A, T, dev = 80, L + 10, cuda_device
    q, k, text_lens, prior, temp = attention_inputs(A, L, T, with_prior, 7 * L)
    mel_lens = torch.tensor([T, int(text_lens[1]) + 20])
    w_ctc, w_bin = f32(0.3), f32(0.7)
    tl, ml = text_lens.to(dev, torch.int32), mel_lens.to(dev, torch.int32)
    qd, kd = cbt(q).to(dev), cbt(k).to(dev)
    pd = None if prior is None else prior.to(dev)
    soft_g, logprob_g = ops.align_attention_fwd(qd, kd, pd, tl, temp)
    hard, _ = maximum_path(torch.log(soft_g), ml, tl)
    hard_c = hard.cpu()
    assert int(hard_c.sum()) == int(mel_lens.sum())

    def reference(dtype):
        qr, kr = q.to(dtype).requires_grad_(), k.to(dtype).requires_grad_()
        soft, logprob = alignment_attention_ref(qr, kr, text_lens, prior, temp)
        (w_ctc * forward_sum_loss_ref(logprob, text_lens, mel_lens, BLANK) + w_bin * binarization_loss_ref(hard_c, soft)).backward()
        return qr.grad, kr.grad

    dq64, dk64 = reference(torch.float64)
    dq32, dk32 = reference(torch.float32)
    _, dlogprob = ops.forward_sum_loss_and_grad(logprob_g, tl, ml, w_ctc, BLANK)
    dq, dk = ops.align_attention_bwd(qd, kd, soft_g, logprob_g, pd, hard, dlogprob, tl, temp, w_bin / float(mel_lens.sum()))
    torch.cuda.synchronize()
    for name, got, want, ref32 in (("dq", dq, dq64, dq32), ("dk", dk, dk64, dk32)):
        e, e32 = grad_errors(got.cpu().permute(1, 0, 2), want), grad_errors(ref32, want)
        scale = want.abs().flatten(1).max(1).values
        bmax, bl2 = FACTOR * torch.maximum(e32["max"], FLOOR * scale), FACTOR * torch.clamp(e32["l2"], min=FLOOR)
        msg = (f"align backward L {L} prior {with_prior} {name}: err / max(err32, floor) per item: max-norm "
               f"{[round(float(r), 3) for r in FACTOR * e['max'] / bmax]}, rel-L2 {[round(float(r), 3) for r in FACTOR * e['l2'] / bl2]}")
        print("RATIO", msg)
        assert torch.isfinite(got).all(), msg
        assert (e["max"] <= bmax).all() and (e["l2"] <= bl2).all(), msg


def test_align_colsum_position_probes(cuda_device):
    """da = one 1.0 at (b, t, l), hard = NULL, dlogprob = da, no prior: the row kernel passes it through, rowsum is 1.0 at (b, t) and
    colsum 1.0 at (b, l), bit for bit.  L 700: l 255 | 256 are the two sides of the 256-stride, i = b L + l crosses a workgroup of
    align_colsum_kernel at every multiple of 256."""
    lib = _lib.load()
    dev, B, T, L = cuda_device, ATT_B, ATT_T, 700
    zeros = torch.zeros(B, T, L, device=dev)
    tl = i32([L, L // 3], dev)
    for b in range(B):
        for t in (0, T - 1):
            for l in (0, 255, 256, L - 1):
                dlp = torch.zeros(B, T, L, device=dev)
                dlp[b, t, l] = 1.0
                da = torch.full((B, T, L), NAN, device=dev)
                rs, cs = torch.full((B, T), NAN, device=dev), torch.full((B, L), NAN, device=dev)
                rc = call(lib.evmi_align_attention_bwd_f32, zeros, zeros, 0, 0, dlp, tl, da, rs,
                          cs, B, T, L, 0.0, 0, stream(dev))
                assert rc == _lib.EVMI_OK
                want_rs, want_cs = torch.zeros(B, T), torch.zeros(B, L)
                want_rs[b, t], want_cs[b, l] = 1.0, 1.0
                assert same_bits(da.cpu(), dlp.cpu()) and same_bits(rs.cpu(), want_rs) and same_bits(cs.cpu(), want_cs), (b, t, l)


@pytest.mark.parametrize("A,BN", [(1, 1), (3, 255), (5, 257)])
def test_align_qk_grad(cuda_device, A, BN):
    """m = coef (x * sums[n] - m) in place: the product may be contracted with the subtraction: gamma(2) of both terms + u of the result."""
    g = torch.Generator().manual_seed(A * BN)
    x, m, sums = torch.randn(A, BN, generator=g), torch.randn(A, BN, generator=g), torch.randn(BN, generator=g)
    coef = f32(-0.1)
    md = m.to(cuda_device)
    rc = call(_lib.load().evmi_align_qk_grad_f32, x.to(cuda_device), sums.to(cuda_device), md, A, BN, coef, stream(cuda_device))
    assert rc == _lib.EVMI_OK
    prod = x.double() * sums.double()[None]
    want = coef * (prod - m.double())
    assert_within(md, want, abs(coef) * gamma(2) * (prod.abs() + m.double().abs()) + U * want.abs(), "align_qk_grad")


# =====================================================================================================================
# monotonic alignment search
# =====================================================================================================================
# (B, T, L), text_lens, mel_lens, quantised.  `for x = lo + tid; x < hi; x += 256` makes a second trip when a row's band (up to
# min(t_x, t_y - t_x + 1) cells) is wider than 256: item 1 of the third case (band 290); the zeroing loops `x < L` make one trip at
# L 256, two at 257, three at 600; x itself passes 255 | 256 in item 0 of every case.
MAS_CASES = [
    ((2, 270, 256), (256, 120), (270, 269), False),   # band 15 at the far end of the stride; item 1: band 120
    ((2, 300, 257), (257, 100), (300, 100), True),    # ties (values on a grid of 0.5); item 1: text_len == mel_len, the diagonal only
    ((2, 620, 600), (600, 290), (620, 600), False),   # item 1: band 290, a second trip inside a row
]


@pytest.mark.parametrize("shape,text_lens,mel_lens,quantised", MAS_CASES, ids=lambda v: None)
def test_monotonic_align_past_one_stride(cuda_device, shape, text_lens, mel_lens, quantised):
    from everyvoice_amd.heavy import maximum_path

    B, T, L = shape
    g = torch.Generator().manual_seed(T * L)
    value = torch.randn(B, T, L, generator=g)
    if quantised:
        value = torch.round(value * 2) / 2
    want_path, want_dur = maximum_path_batch_ref(value.numpy(), mel_lens, text_lens)
    path, dur = maximum_path(value.to(cuda_device), torch.tensor(mel_lens), torch.tensor(text_lens))
    assert torch.equal(path.cpu(), torch.from_numpy(want_path)) and torch.equal(dur.cpu(), torch.from_numpy(want_dur))
    assert dur.cpu().sum(1).tolist() == list(mel_lens)


def test_monotonic_align_lds_limit(cuda_device):
    """Two rows of L floats in dynamic LDS: 64 KiB at L 8192 (accepted, exact), refused at 8193."""
    from everyvoice_amd.heavy import maximum_path

    g = torch.Generator().manual_seed(8192)
    value = torch.randn(2, 12, 8192, generator=g)
    text_lens, mel_lens = (8, 3), (12, 7)
    want_path, want_dur = maximum_path_batch_ref(value.numpy(), mel_lens, text_lens)
    path, dur = maximum_path(value.to(cuda_device), torch.tensor(mel_lens), torch.tensor(text_lens))
    assert torch.equal(path.cpu(), torch.from_numpy(want_path)) and torch.equal(dur.cpu(), torch.from_numpy(want_dur))
    dev, B, T, L = cuda_device, 1, 2, 8193
    v = torch.zeros(B, T, L, device=dev)
    p, d = torch.full((B, T, L), -7, dtype=torch.int32, device=dev), torch.full((B, L), -7, dtype=torch.int32, device=dev)
    scratch = torch.zeros(B * T * L, dtype=torch.uint8, device=dev)
    rc = call(_lib.load().evmi_monotonic_align_f32, v, i32([2], dev), i32([2], dev), p, d, scratch,
                                              B, T, L, stream(dev))
    assert rc == UNSUPPORTED and (p == -7).all() and (d == -7).all()


# =====================================================================================================================
# binarisation partial sums
# =====================================================================================================================
# n 1 / 255 / 257: inside and across one workgroup's 256 elements; 2049: more than one trip when n_blocks = 1, nine workgroups' worth;
# 256 * 2048 + 3: with 256 workgroups the grid-stride loop makes 9 trips and the last one is 3 elements wide
@pytest.mark.parametrize("n_blocks", [1, 256])
@pytest.mark.parametrize("n", [1, 255, 257, 2049, 256 * 2048 + 3])
def test_binarization_partials(cuda_device, n, n_blocks):
    """Per workgroup: the count is exact; the sum of logf(max(soft, 1e-12f)) is accumulated in double: MATH_ULP per logf and
    n 2^-53 of the absolute sum.  soft = 0 and 1e-13 on the path take the clamp; cells with hard == 2 are not counted."""
    dev = cuda_device
    g = torch.Generator().manual_seed(n + n_blocks)
    hard = torch.randint(0, 3, (n,), generator=g, dtype=torch.int32)
    soft = torch.rand(n, generator=g) * 0.999 + 0.001
    on = torch.nonzero(hard == 1).flatten()
    if n == 1:
        hard[0], soft[0] = 1, 0.0
    elif len(on) >= 4:
        soft[on[0]], soft[on[1]], soft[on[-1]] = 0.0, 1e-13, 1e-13
    two = torch.nonzero(hard == 2).flatten()
    if len(two):
        soft[two[0]] = 0.5
    part = torch.full((n_blocks, 2), NAN, dtype=torch.float64, device=dev)
    rc = call(_lib.load().evmi_binarization_partials_f64, hard.to(dev), soft.to(dev), part, n_blocks, n, stream(dev))
    assert rc == _lib.EVMI_OK
    part = part.cpu()
    clamp = f32(1e-12)
    logs = torch.where(hard == 1, torch.log(torch.clamp(soft.double(), min=clamp)), torch.zeros(n, dtype=torch.float64))
    block = (torch.arange(n) // 256) % n_blocks  # element i belongs to workgroup (i / 256) mod n_blocks
    want_sum = torch.zeros(n_blocks, dtype=torch.float64).index_add_(0, block, logs)
    want_abs = torch.zeros(n_blocks, dtype=torch.float64).index_add_(0, block, logs.abs())
    want_cnt = torch.zeros(n_blocks, dtype=torch.float64).index_add_(0, block, (hard == 1).double())
    assert torch.equal(part[:, 1], want_cnt) and float(part[:, 1].sum()) == float((hard == 1).sum())
    assert_within(part[:, 0], want_sum, (E + n * 2.0 ** -53) * want_abs, f"binarization n {n} blocks {n_blocks}")
    if n > 1 and len(on) >= 4:
        assert (soft[hard == 1] < clamp).sum() >= 3  # the clamp is on the path
