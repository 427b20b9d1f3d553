"""The reference and the lattice inputs of tests/test_gpu_resblock_fused.py, the plan queries, the weight image and the host-side
refusals of evmi_resblock_pair_bf16 / evmi_resblock_branch_bf16 (csrc/resblock_pair.hip).  No GPU: the plan queries and the relayout
are host code of the library, and a refused call returns before any HIP call."""

import ctypes as C

import pytest
import torch

import resblock_ref as R
from everyvoice_amd import _lib

EVMI_ERR_INVALID_ARG = 1
EVMI_ERR_UNSUPPORTED = 4


def pair_plan(c, ks, dil):
    tt, bn, kc, n = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_longlong(-1)
    ok = _lib.load().evmi_resblock_pair_plan(c, ks, dil, C.byref(tt), C.byref(bn), C.byref(kc), C.byref(n))
    return ok, tt.value, bn.value, kc.value, n.value


def branch_plan(c, ks, dils, np=3):
    tt, bn = C.c_int(-1), C.c_int(-1)
    ok = _lib.load().evmi_resblock_branch_plan(c, ks, np, (C.c_int * 3)(*dils), C.byref(tt), C.byref(bn))
    return ok, tt.value, bn.value


# ---- plan queries ---------------------------------------------------------------------------------------------------------------------------
def test_pair_plan_reports_the_table():
    for c, ks in R.PAIR_ENTRIES:
        for dil in R.pair_dilations(c):
            ok, tt, bn, kc, n = pair_plan(c, ks, dil)
            assert ok == 1 and tt == bn - (ks - 1) and bn in (256, 512) and n == c * c * ks
            assert kc == (64 if c == 128 else c)
    for c, ks, dil in [(64, 5, 1), (64, 3, 6), (128, 7, 1), (48, 3, 1), (64, 3, 0)]:
        assert pair_plan(c, ks, dil) == (0, 0, 0, 0, 0)
    assert _lib.load().evmi_resblock_pair_plan(64, 3, 1, None, None, None, None) == 1  # (outputs are optional)


def test_branch_plan_reports_valid_rows():
    for c, ks in R.BRANCH_ENTRIES:
        h = (ks - 1) // 2
        for dils in R.BRANCH_TRIPLES[(c, ks)]:
            ok, tt, bn = branch_plan(c, ks, dils)
            # rows loaded minus twice the reach of the three pairs (resblock_branch_kernel.h: BN + 2 h1_0 - 2 Mtot)
            assert ok == 1 and tt == bn + 2 * dils[0] * h - 2 * sum(d * h + h for d in dils), (c, ks, dils)
            assert 4 * tt >= 3 * bn
    assert branch_plan(32, 3, (1, 3, 5), np=2) == (0, 0, 0)
    assert branch_plan(32, 11, (1, 3, 5)) == (0, 0, 0)  # no k = 11 entry
    assert branch_plan(64, 3, (9, 9, 9)) == (0, 0, 0)   # 256 + 18 - 60 = 214 valid rows of 256: a halo above 25 %
    assert branch_plan(32, 3, (1, 0, 1)) == (0, 0, 0)


# ---- the reference itself -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [3, 7, 11])
def test_reference_equals_the_oracle_resblock(ks):
    """np = 3, scale = post = 1, no accumulate: ResBlock1Ref of oracle/hifigan_ref.py in float64 on the same parameters."""
    from oracle.hifigan_ref import LRELU_SLOPE, ResBlock1Ref

    c, B, T = 16, 2, 61
    x, ws, bs, _ = R.random_problem(c, ks, B, T, n_pairs=3, seed=ks)
    blk = ResBlock1Ref(c, ks, (1, 3, 5))
    blk.remove_weight_norm()
    blk = blk.double()
    with torch.no_grad():
        for p in range(3):
            blk.convs1[p].weight.copy_(ws[2 * p]); blk.convs1[p].bias.copy_(bs[2 * p])
            blk.convs2[p].weight.copy_(ws[2 * p + 1]); blk.convs2[p].bias.copy_(bs[2 * p + 1])
        want = blk(x.transpose(1, 2)).transpose(1, 2)
    got = R.branch_ref(x, ws, bs, (1, 3, 5), LRELU_SLOPE)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"k={ks}: max|diff| / max|want| = {err:.3e}")
    assert err <= 1e-12


def test_rounded_reference_rounds_only_where_stated():
    x, ws, bs, base = R.random_problem(32, 3, 2, 40)
    a = R.pair_ref(x, ws[0], bs[0], ws[1], bs[1], 3, 0.1, 0.5, 0.5, base, rounded=True)
    b = R.pair_ref(x, ws[0], bs[0], ws[1], bs[1], 3, 0.1, 0.5, 0.5, base, rounded=False)
    assert torch.equal(R.bf16(a), a) and not torch.equal(a, b)
    assert float((a - b).abs().max()) <= 2 ** -7 * float(b.abs().max())


# ---- lattice assertions and sensitivity, on every case of the GPU file ------------------------------------------------------------------
def _pair_cases():
    for c, ks in R.PAIR_ENTRIES:
        for dil in R.pair_dilations(c):
            yield c, ks, dil


@pytest.mark.parametrize("c,ks,dil", list(_pair_cases()))
def test_pair_lattice_is_exact_and_sees_every_wrong_variant(c, ks, dil):
    ok, tt, bn, _, _ = pair_plan(c, ks, dil)
    assert ok
    seen = {v: 0 for v in R.VARIANTS}
    for T, acc, post, scale in R.pair_runs(c, ks, dil, tt):
        x, ws, bs, base = R.lattice(c, ks, R.B_LATTICE, T)
        base = base if acc else None
        want = R.check_lattice(x, ws, bs, (dil,), R.LATTICE_SLOPE, post, scale, base)
        assert want.unique().numel() > (100 if T >= tt - 1 else 4)  # (not a degenerate draw)
        for v in R.VARIANTS:
            # a variant that is the same function at this (T, dil) is not asked for: a seam needs T > tt, a dilated conv2 differs
            # from the dense one only with dil > 1 and a second row
            if (v == "seam_shifted" and T <= tt) or (v == "conv2_dilated" and (dil == 1 or T == 1)):
                continue
            wrong = R.pair_ref(x, ws[0], bs[0], ws[1], bs[1], dil, R.LATTICE_SLOPE, post, scale, base, variant=v, tt=tt)
            n = int((wrong != want).sum())
            assert n > 0, f"{v} is invisible at c={c} k={ks} dil={dil} T={T}"
            seen[v] += 1
    print(f"c={c} k={ks} dil={dil}: runs that saw each wrong variant: {seen}")
    assert seen["t1_not_zeroed"] == 8 and seen["x_replicated"] == 8 and seen["seam_shifted"] >= 2
    assert dil == 1 or seen["conv2_dilated"] >= 6


def _branch_cases():
    for c, ks in R.BRANCH_ENTRIES:
        for k, dils in enumerate(R.BRANCH_TRIPLES[(c, ks)]):
            yield c, ks, k, dils


@pytest.mark.parametrize("c,ks,k,dils", list(_branch_cases()))
def test_branch_lattice_is_exact(c, ks, k, dils):
    ok, tt, bn = branch_plan(c, ks, dils)
    assert ok, "the plan query must take every triple of the GPU file"
    for T, acc, post, scale in R.branch_runs(tt, k):
        x, ws, bs, base = R.lattice(c, ks, R.B_LATTICE, T, n_pairs=3, **R.BRANCH_LATTICE)
        want = R.check_lattice(x, ws, bs, dils, R.LATTICE_SLOPE, post, scale, base if acc else None)
        assert want.unique().numel() > (100 if T >= tt - 1 else 4)
        assert all(bool((w != 0).any(0).any(0).all()) for w in ws)  # every tap of every convolution carries a weight
        # the chain is sensitive to a stage that is not zeroed outside the sequence: pair 1 with the wrong variant, the rest right
        y1 = R.pair_ref(x, ws[0], bs[0], ws[1], bs[1], dils[0], R.LATTICE_SLOPE)
        y2 = R.pair_ref(y1, ws[2], bs[2], ws[3], bs[3], dils[1], R.LATTICE_SLOPE, variant="t1_not_zeroed")
        wrong = R.pair_ref(y2, ws[4], bs[4], ws[5], bs[5], dils[2], R.LATTICE_SLOPE, post, scale, base if acc else None)
        assert not torch.equal(wrong, want), f"pair 1 not zeroing its intermediate is invisible at c={c} k={ks} {dils} T={T}"


def test_tile_walk_lattices_are_exact():
    for c, ks, dil in R.WALK_PAIRS:
        tt = pair_plan(c, ks, dil)[1]
        for B, T, _ in R.walk_problems(tt, ks)[::2]:
            x, ws, bs, base = R.lattice(c, ks, B, T)
            R.check_lattice(x, ws, bs, (dil,), R.LATTICE_SLOPE, 0.5, 0.5, base)
    for c, ks in R.BRANCH_ENTRIES:
        tt = branch_plan(c, ks, (1, 3, 5))[1]
        for B, T, _ in R.walk_problems(tt, ks)[::2]:
            x, ws, bs, base = R.lattice(c, ks, B, T, n_pairs=3, **R.BRANCH_LATTICE)
            R.check_lattice(x, ws, bs, (1, 3, 5), R.LATTICE_SLOPE, 0.5, 0.5, base)


def test_conv_tc_lattice_is_exact():
    x, w, b = R.conv_tc_lattice(128, 3, 2, 300)
    want = R.check_conv_lattice(x, w, b, 1)
    assert want.unique().numel() > 20


# ---- the weight image -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,ks,kc", [(32, 11, 32), (64, 7, 64), (128, 3, 64)])
def test_weight_image_is_chunk_tap_row_kc(c, ks, kc):
    """Three calls, each weight element carrying one of its own coordinates (mo, ci, tap) as an integer below 2**8 (exact in bf16):
    element [chunk][tap][mo][cw] of the image must hold (mo, chunk * kc + cw, tap)."""
    if kc != c or c == 128:
        assert pair_plan(c, ks, 1)[3] == kc  # the chunk the kernel itself asks for
    lib = _lib.load()
    mo, ci, tap = torch.meshgrid(torch.arange(c), torch.arange(c), torch.arange(ks), indexing="ij")
    got = []
    for field in (mo, ci, tap):
        w = field.to(torch.float32).contiguous()
        dst = torch.full((c * c * ks + 8,), -1.0, dtype=torch.bfloat16)
        assert lib.evmi_resblock_pair_relayout_f32(w.data_ptr(), dst.data_ptr(), c, ks, kc) == 0
        assert bool((dst[c * c * ks:] == -1).all())  # exactly C * C * ks elements written
        got.append(dst[:c * c * ks].view(c // kc, ks, c, kc).to(torch.int64))
    chunk, t, m, cw = torch.meshgrid(torch.arange(c // kc), torch.arange(ks), torch.arange(c), torch.arange(kc), indexing="ij")
    assert torch.equal(got[0], m) and torch.equal(got[1], chunk * kc + cw) and torch.equal(got[2], t)


def test_weight_image_rounds_to_nearest_even():
    w = torch.tensor([1.00390625, 1.01171875, -3.0e-40, 0.1], dtype=torch.float32).repeat(64)[:8 * 8 * 3].contiguous()
    dst = torch.zeros(8 * 8 * 3, dtype=torch.bfloat16)
    assert _lib.load().evmi_resblock_pair_relayout_f32(w.data_ptr(), dst.data_ptr(), 8, 3, 8) == 0
    want = w.view(8, 8, 3).permute(2, 0, 1).contiguous().to(torch.bfloat16).view(-1)
    assert torch.equal(dst.view(torch.int16), want.view(torch.int16))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
_BUF = torch.zeros(1 << 16)  # host memory standing in for every device pointer: a refused call never touches it
P = _BUF.data_ptr()
Q = P + (1 << 17)            # a second buffer, far enough from P for the shapes below
SIX = (C.c_void_p * 6)(*([P] * 6))
D135 = (C.c_int * 3)(1, 3, 5)


def _pair_args(x=P, w1=P, b1=P, w2=P, b2=P, out=Q, B=1, T=8, c=64, ks=3, dil=1, n_cu=0):
    return (x, w1, b1, w2, b2, out, B, T, c, ks, dil, 0.1, 1.0, 1.0, 0, n_cu, None)


def _branch_args(x=P, w=SIX, b=SIX, out=Q, B=1, T=8, c=32, ks=3, np=3, dil=D135, n_cu=0):
    return (x, w, b, out, B, T, c, ks, np, dil, 0.1, 1.0, 1.0, 0, n_cu, None)


REFUSALS = {
    "pair_k5": ("evmi_resblock_pair_bf16", _pair_args(ks=5), EVMI_ERR_UNSUPPORTED),
    "pair_dil6": ("evmi_resblock_pair_bf16", _pair_args(dil=6), EVMI_ERR_UNSUPPORTED),
    "pair_c128_k7": ("evmi_resblock_pair_bf16", _pair_args(c=128, ks=7), EVMI_ERR_UNSUPPORTED),
    "pair_dil0": ("evmi_resblock_pair_bf16", _pair_args(dil=0), EVMI_ERR_UNSUPPORTED),
    "pair_null_x": ("evmi_resblock_pair_bf16", _pair_args(x=0), EVMI_ERR_INVALID_ARG),
    "pair_null_w1": ("evmi_resblock_pair_bf16", _pair_args(w1=0), EVMI_ERR_INVALID_ARG),
    "pair_null_b1": ("evmi_resblock_pair_bf16", _pair_args(b1=0), EVMI_ERR_INVALID_ARG),
    "pair_null_w2": ("evmi_resblock_pair_bf16", _pair_args(w2=0), EVMI_ERR_INVALID_ARG),
    "pair_null_b2": ("evmi_resblock_pair_bf16", _pair_args(b2=0), EVMI_ERR_INVALID_ARG),
    "pair_null_out": ("evmi_resblock_pair_bf16", _pair_args(out=0), EVMI_ERR_INVALID_ARG),
    "pair_T0": ("evmi_resblock_pair_bf16", _pair_args(T=0), EVMI_ERR_INVALID_ARG),
    "pair_B0": ("evmi_resblock_pair_bf16", _pair_args(B=0), EVMI_ERR_INVALID_ARG),
    "pair_n_cu_negative": ("evmi_resblock_pair_bf16", _pair_args(n_cu=-8), EVMI_ERR_INVALID_ARG),
    "pair_in_place": ("evmi_resblock_pair_bf16", _pair_args(out=P), EVMI_ERR_INVALID_ARG),
    "pair_overlapping": ("evmi_resblock_pair_bf16", _pair_args(out=P + 64), EVMI_ERR_INVALID_ARG),
    "branch_np2": ("evmi_resblock_branch_bf16", _branch_args(np=2), EVMI_ERR_UNSUPPORTED),
    "branch_halo_above_25_percent": ("evmi_resblock_branch_bf16", _branch_args(c=64, dil=(C.c_int * 3)(9, 9, 9)), EVMI_ERR_UNSUPPORTED),
    "branch_k11": ("evmi_resblock_branch_bf16", _branch_args(ks=11), EVMI_ERR_UNSUPPORTED),
    "branch_c64_k7": ("evmi_resblock_branch_bf16", _branch_args(c=64, ks=7), EVMI_ERR_UNSUPPORTED),
    "branch_null_x": ("evmi_resblock_branch_bf16", _branch_args(x=0), EVMI_ERR_INVALID_ARG),
    "branch_null_out": ("evmi_resblock_branch_bf16", _branch_args(out=0), EVMI_ERR_INVALID_ARG),
    "branch_null_weight_table": ("evmi_resblock_branch_bf16", _branch_args(w=None), EVMI_ERR_INVALID_ARG),
    "branch_null_bias_table": ("evmi_resblock_branch_bf16", _branch_args(b=None), EVMI_ERR_INVALID_ARG),
    "branch_null_dilations": ("evmi_resblock_branch_bf16", _branch_args(dil=None), EVMI_ERR_INVALID_ARG),
    "branch_null_weight_4": ("evmi_resblock_branch_bf16", _branch_args(w=(C.c_void_p * 6)(P, P, P, P, 0, P)), EVMI_ERR_INVALID_ARG),
    "branch_null_bias_5": ("evmi_resblock_branch_bf16", _branch_args(b=(C.c_void_p * 6)(P, P, P, P, P, 0)), EVMI_ERR_INVALID_ARG),
    "branch_T0": ("evmi_resblock_branch_bf16", _branch_args(T=0), EVMI_ERR_INVALID_ARG),
    "branch_B_negative": ("evmi_resblock_branch_bf16", _branch_args(B=-1), EVMI_ERR_INVALID_ARG),
    "branch_in_place": ("evmi_resblock_branch_bf16", _branch_args(out=P), EVMI_ERR_INVALID_ARG),
    "relayout_null": ("evmi_resblock_pair_relayout_f32", (0, P, 64, 3, 64), EVMI_ERR_INVALID_ARG),
    "relayout_kc_not_a_divisor": ("evmi_resblock_pair_relayout_f32", (P, P, 64, 3, 48), EVMI_ERR_INVALID_ARG),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refused_on_the_host_with_the_documented_code(name):
    fn, args, code = REFUSALS[name]
    lib = _lib.load()
    rc = getattr(lib, fn)(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == code, f"{fn}: returned {rc} ({msg!r}), wanted {code}"
    assert fn[len("evmi_"):].rsplit("_bf16", 1)[0].rsplit("_f32", 1)[0] in msg
    assert torch.count_nonzero(_BUF) == 0


def test_the_header_states_the_preconditions():
    from pathlib import Path

    declared = {name for name, _, _ in _lib.declarations()}
    assert {fn for fn, _, _ in REFUSALS.values()} <= declared
    text = " ".join((Path(__file__).resolve().parents[1] / "include" / "evmi.h").read_text().split())  # the comments: the raw text
    for phrase in ("evmi_resblock_pair_bf16", "evmi_resblock_branch_bf16", "x and out overlapping", "EVMI_PAIR_C128=0", "EVMI_BRANCH=0",
                   "0 = the device's compute units"):
        assert phrase in text, phrase
