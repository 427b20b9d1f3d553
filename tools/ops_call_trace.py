"""Which libevmi_hip entry points the convolution operators of everyvoice_amd/train/ops.py (and the tape operators of train/fs2.py built on
them) call, with which arguments -- recorded on the CPU, without the library: ``_lib.load`` is replaced by a recorder that takes
restype / argtypes from ``_lib.SYMBOLS``, ``_lib.current_stream_ptr`` by a constant.  Host-side refactors of those wrappers claim "same
library calls": run this at both commits and compare the two outputs (``--compare a.json b.json``).

    python tools/ops_call_trace.py > trace.json
    python tools/ops_call_trace.py --compare parent.json head.json

Queries (names ending in _ws_elems, _plan, _supported, _rounds, _shares_packed, _frag_elems) are answered from a table per scenario, which
steers every path (packed kernels take the shape / refuse it, matrix-core kernels refuse it, shared packed operands yes / no); every other
entry point returns EVMI_OK and is recorded as (name, canonical arguments): a pointer into one of the case's named tensors becomes
that name (+ byte offset), any other non-null pointer "PTR", NULL stays "NULL"; ctypes structs and arrays are expanded under the same rule.
Every case runs under every combination of the module's switches.  Output: {"traces": {digest: calls}, "queries": {digest: distinct
queries}, "cases": {id: {"trace": digest, "queries": digest, "n_queries": n, "result": ...}}}.
"""

from __future__ import annotations

import ctypes as C
import hashlib
import itertools
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from everyvoice_amd import _lib  # noqa: E402
from everyvoice_amd.train import fs2 as tfs2  # noqa: E402
from everyvoice_amd.train import ops  # noqa: E402
from everyvoice_amd.train.autograd import Tape, Var  # noqa: E402
from everyvoice_amd.train.layers import ParamGroup  # noqa: E402

STREAM = 0x5EED0
_BYREF = type(C.byref(C.c_int()))
QUERY_SUFFIXES = ("_ws_elems", "_plan", "_supported", "_rounds", "_shares_packed", "_frag_elems")

# scenario -> [(substring of the query's name, answer)], first match wins; names no pattern matches answer 64
SCENARIOS = {
    "packed": [],
    "packed_unshared": [("shares_packed", 0)],
    "packed_fwd_only": [("dgrad_cbt_bf16pk", 0), ("wgrad_cbt_bf16pk", 0)],
    "f32_mfma": [("bf16pk", 0), ("shares_packed", 0)],
    "f32_mfma_no_ws": [("bf16pk", 0), ("shares_packed", 0), ("dgrad_cbt_f32_ws", 0), ("wgrad_cbt_f32_ws", 0)],
    "gemm": [("bf16pk", 0), ("shares_packed", 0), ("cbt_f32_supported", 0), ("dgrad_cbt_f32_ws", 0), ("wgrad_cbt_f32_ws", 0)],
}


class Recorder:
    """Stands in for the loaded library: attribute access gives a callable per declared symbol."""

    def __init__(self):
        self.answers, self.named = [], {}
        self.calls, self.queries = [], []

    def begin(self, answers, named):
        self.answers, self.named = answers, named
        self.calls, self.queries = [], []

    def _pointer(self, v):
        if isinstance(v, C.c_void_p):
            v = v.value
        if not v:
            return "NULL"
        if v == STREAM:
            return "STREAM"
        for name, t in self.named.items():
            off = v - t.data_ptr()
            if 0 <= off < max(t.numel() * t.element_size(), 1):
                return name if off == 0 else f"{name}+{off}"
        return "PTR"

    def _canon(self, v, ctype):
        # what the value is decides first: the header types every pointer parameter but those to the mirrored structs as void*
        if isinstance(v, _BYREF):  # byref(x) stands for x
            v = v._obj
            ctype = type(v)
        if isinstance(v, C.Array):  # jobs (structs), pointer tables, small value arrays
            return [self._canon(e, v._type_) for e in v]
        if isinstance(v, C.Structure):
            return {f: self._canon(getattr(v, f), t) for f, t in v._fields_}
        if ctype is C.c_void_p:
            return self._pointer(v)
        if isinstance(v, C._SimpleCData):
            v = v.value
        if v is None:
            return "NULL"
        if ctype in (C.c_float, C.c_double):
            return float(v)
        return v if isinstance(v, (int, float)) else int(v)

    def __getattr__(self, name):
        if name not in _lib.SYMBOLS:
            raise AttributeError(name)
        argtypes = _lib.SYMBOLS[name][1]

        def call(*args):
            if len(args) != len(argtypes):
                raise TypeError(f"{name}: {len(args)} arguments for {len(argtypes)} declared")
            canon = [self._canon(a, t) for a, t in zip(args, argtypes)]
            if name.endswith(QUERY_SUFFIXES):
                self.queries.append([name, canon])
                return next((v for pat, v in self.answers if pat in name), 64)
            self.calls.append([name, canon])
            return _lib.EVMI_OK

        return call


REC = Recorder()


class recording:
    """``with recording():`` _lib.load gives the recorder, _lib.current_stream_ptr the constant; both are put back on the way out."""

    def __enter__(self):
        self.saved = _lib.load, _lib.current_stream_ptr
        _lib.load, _lib.current_stream_ptr = (lambda: REC), (lambda device=None: STREAM)
        return REC

    def __exit__(self, *exc):
        _lib.load, _lib.current_stream_ptr = self.saved
        return False


class Env:
    """The named tensors of one case."""

    def __init__(self):
        self.named = {}

    def t(self, name, *shape, dtype=torch.float32):
        self.named[name] = torch.zeros(*shape, dtype=dtype)
        return self.named[name]

    def layers(self, cin, cmid, cout, k=1):
        """A small ParamGroup: LayerNorm(cin), Dense(cin -> cmid, k), Dense(cmid -> cout)."""
        g = ParamGroup(torch.device("cpu"))
        ln = tfs2.Affine(g, "ln", cin)
        l1 = tfs2.Dense(g, "l1.weight", "l1.bias", cin, cmid, k)
        l2 = tfs2.Dense(g, "l2.weight", "l2.bias", cmid, cout)
        g.finalize()
        self.named["params"], self.named["grads"] = g.flat, g.grad
        return ln, l1, l2


CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def _variants(name, fn, **axes):
    keys = list(axes)
    for combo in itertools.product(*axes.values()):
        kw = dict(zip(keys, combo))
        CASES[name + "[" + ",".join(f"{k}={v}" for k, v in kw.items()) + "]"] = (lambda e, kw=kw: fn(e, **kw))


CIN, COUT, B, T = 16, 24, 2, 20


def _conv1d_fwd(e, act, slope, geo):
    k, stride, pad, dil, groups = geo
    x, w, b = e.t("x", CIN, B, T), e.t("w", COUT, CIN // groups, k), e.t("bias", COUT)
    ops.conv1d_fwd(x, w, b, stride, pad, dil, groups, lrelu_slope=slope, act=act, keep={})


GEOS = [(1, 1, 0, 1, 1), (3, 1, 1, 1, 1), (4, 2, 1, 1, 1), (3, 1, 2, 2, 4)]
_variants("conv1d_fwd", _conv1d_fwd, act=[ops.ACT_NONE, ops.ACT_SILU, ops.ACT_RELU, ops.ACT_TANH], slope=[None], geo=GEOS)
_variants("conv1d_fwd", _conv1d_fwd, act=[ops.ACT_NONE], slope=[0.1], geo=GEOS)


def _conv1d_bwd(e, need_dx, need_dw, packed, x_standin, geo, sinks):
    k, stride, pad, dil, groups = geo
    t_out = ops.conv_out_len(T, k, stride, pad, dil)
    x, w, dy = e.t("x", CIN, B, T), e.t("w", COUT, CIN // groups, k), e.t("dy", COUT, B, t_out)
    dw, db = (e.t("dw", COUT, CIN // groups, k), e.t("db", COUT)) if sinks else (None, None)
    pk = {"x_packed": e.t("x_packed", 64)} if packed == "x" else ({} if packed == "empty" else None)
    ops.conv1d_bwd(x, w, dy, stride, pad, dil, groups, need_dx=need_dx, dw_out=dw, db_out=db, accumulate=sinks, need_dw=need_dw, packed=pk,
                   x_standin=x_standin)


_variants("conv1d_bwd", _conv1d_bwd, need_dx=[True, False], need_dw=[True, False], packed=[None, "empty", "x"], x_standin=[False, True],
          geo=GEOS[:3], sinks=[True])
_variants("conv1d_bwd", _conv1d_bwd, need_dx=[True, False], need_dw=[True, False], packed=[None, "empty", "x"], x_standin=[False, True],
          geo=GEOS[:1], sinks=[False])


def _fused_fwd(e, act, pre_slope, residual, geo):
    k, stride, pad, dil, groups = geo
    x, w, b = e.t("x", CIN, B, T), e.t("w", COUT, CIN // groups, k), e.t("bias", COUT)
    r = e.t("res", COUT, B, ops.conv_out_len(T, k, stride, pad, dil)) if residual else None
    ops.conv1d_fused_fwd(x, w, b, stride, pad, dil, groups, act=act, act_param=0.1, pre_slope=pre_slope, residual=r)


_variants("conv1d_fused_fwd", _fused_fwd, act=[ops.ACT_NONE, ops.ACT_LRELU, ops.ACT_TANH], pre_slope=[1.0, 0.1], residual=[False, True], geo=GEOS[1:3])


def _fused_dgrad(e, masks, residual, fallback_x, geo):
    k, stride, pad, dil, groups = geo
    t_in = 40 if k < stride else T
    t_out = ops.conv_out_len(t_in, k, stride, pad, dil)
    dy, w = e.t("dy", COUT, B, t_out), e.t("w", COUT, CIN // groups, k)
    m1, m2 = (e.t("dy_mask", COUT, B, t_out), e.t("dx_mask", CIN, B, t_in)) if masks else (None, None)
    r = e.t("res", CIN, B, t_in) if residual else None
    ops.conv1d_fused_dgrad(dy, w, t_in, stride, pad, dil, groups, dy_mask=m1, dy_mask_slope=0.1, dx_mask=m2, dx_mask_slope=0.2, residual=r,
                           x_for_fallback=e.t("x", CIN, B, t_in) if fallback_x else None)


_variants("conv1d_fused_dgrad", _fused_dgrad, masks=[False, True], residual=[False, True], fallback_x=[False, True], geo=GEOS[1:3] + [(2, 4, 0, 1, 1)])


def _fused_wgrad(e, slope, accumulate, geo):
    k, stride, pad, dil, groups = geo
    x, dy, dw = e.t("x", CIN, B, T), e.t("dy", COUT, B, ops.conv_out_len(T, k, stride, pad, dil)), e.t("dw", COUT, CIN // groups, k)
    ops.conv1d_fused_wgrad(x, dw.shape, dy, dw, stride, pad, dil, groups, x_pre_slope=slope, accumulate=accumulate)


_variants("conv1d_fused_wgrad", _fused_wgrad, slope=[1.0, 0.1], accumulate=[True, False], geo=GEOS[1:3])


def _bwd_data(e, geo, keep):
    k, stride, pad, dil, groups = geo
    t_in = 40
    dy, w = e.t("dy", COUT, B, ops.conv_out_len(t_in, k, stride, pad, dil)), e.t("w", COUT, CIN // groups, k)
    ops.conv1d_bwd_data_mfma(dy, w, t_in, stride, pad, dil, groups, keep={} if keep else None)


_variants("conv1d_bwd_data_mfma", _bwd_data, geo=GEOS + [(2, 4, 0, 1, 1), (7, 3, 2, 1, 1)], keep=[False, True])


def _ptw(e, cin=CIN, cout=COUT, t=T):
    """The tensors of a pointwise layer on one item of B * t columns."""
    n = B * t
    return e.t("x", cin, 1, n), e.t("w", cout, cin, 1), e.t("bias", cout), n


@case
def layernorm_dense_fwd(e):
    x, w, b, _ = _ptw(e)
    ops.layernorm_dense_fwd(x, e.t("gamma", CIN), e.t("beta", CIN), w, b, {}, act=ops.ACT_RELU)


@case
def conv1d_fwd_silu_dropout(e):
    x, w, b, _ = _ptw(e)
    ops.conv1d_fwd_silu_dropout(x, w, b, 0.2, 7, {})


def _bwd_silu_dropout_dy(e, xp, db):
    x, w, _, n = _ptw(e)
    ops.conv1d_bwd_silu_dropout_dy(x, w, e.t("ds", COUT, 1, n), e.t("pre", COUT, 1, n), 0.2, 7, e.t("dw", COUT, CIN, 1), e.t("db", COUT) if db else None,
                                   {"x_packed": e.t("x_packed", 64)} if xp else {})


_variants("conv1d_bwd_silu_dropout_dy", _bwd_silu_dropout_dy, xp=[True, False], db=[True, False])


def _fwd_resdrop(e, in_p):
    x, w, b, n = _ptw(e)
    ops.conv1d_fwd_resdrop(x, w, b, e.t("res", COUT, 1, n), 0.2, 7, 0.5, {}, in_p=in_p, in_seed=9)


_variants("conv1d_fwd_resdrop", _fwd_resdrop, in_p=[None, 0.3])


def _bwd_dropout_dy(e, xp, db, x_standin):
    x, w, _, n = _ptw(e)
    ops.conv1d_bwd_dropout_dy(x, w, e.t("dy", COUT, 1, n), 0.2, 7, 0.5, e.t("dw", COUT, CIN, 1), e.t("db", COUT) if db else None,
                              {"x_packed": e.t("x_packed", 64)} if xp else {}, x_standin=x_standin)


_variants("conv1d_bwd_dropout_dy", _bwd_dropout_dy, xp=[True, False], db=[True, False], x_standin=[False, True])

CMID = 32


def _ffn_tensors(e, n):
    return (e.t("x", CIN, 1, n), e.t("gamma", CIN), e.t("beta", CIN), e.t("w1", CMID, CIN, 1), e.t("b1", CMID), e.t("w2", COUT, CMID, 1), e.t("b2", COUT),
            e.t("res", COUT, 1, n))


def _ffn_packed_fwd(e, n):
    ops.ffn_packed_fwd(*_ffn_tensors(e, n), 0.2, 7, 9, 0.5, {})


def _ffn_packed_infer(e, n):
    ops.ffn_packed_infer(*_ffn_tensors(e, n))


def _ffn_packed_bwd(e, n, db):
    x, _, _, w1, _, w2, _, _ = _ffn_tensors(e, n)
    keep = {"x_packed": e.t("x_packed", 64), "s_packed": e.t("s_packed", 64), "a_pk": e.t("a_pk", CMID // 8 * ops.pk_pitch(1, n) * 4)}
    ops.ffn_packed_bwd(x, w1, w2, e.t("dy", COUT, 1, n), 0.2, 7, 9, 0.5, e.t("dw1", CMID, CIN, 1), e.t("db1", CMID) if db else None,
                       e.t("dw2", COUT, CMID, 1), e.t("db2", COUT) if db else None, keep)


_variants("ffn_packed_fwd", _ffn_packed_fwd, n=[64, 77])
_variants("ffn_packed_infer", _ffn_packed_infer, n=[64, 77])
_variants("ffn_packed_bwd", _ffn_packed_bwd, n=[64, 77], db=[True, False])


def _convt_fwd(e, bias, k, stride, pad):
    ops.conv_transpose1d_fwd(e.t("x", CIN, B, T), e.t("w", CIN, COUT, k), e.t("bias", COUT) if bias else None, stride, pad)


def _convt_bwd(e, need_dx, need_dw, sinks, k, stride, pad):
    x, w = e.t("x", CIN, B, T), e.t("w", CIN, COUT, k)
    dy = e.t("dy", COUT, B, (T - 1) * stride - 2 * pad + k)
    dw, db = (e.t("dw", CIN, COUT, k), e.t("db", COUT)) if sinks else (None, None)
    ops.conv_transpose1d_bwd(x, w, dy, stride, pad, need_dx=need_dx, dw_out=dw, db_out=db, accumulate=sinks, need_dw=need_dw)


for _k, _stride, _pad in ((4, 2, 1), (16, 8, 4), (2, 4, 0)):
    _variants("conv_transpose1d_fwd", _convt_fwd, bias=[True, False], k=[_k], stride=[_stride], pad=[_pad])
    _variants("conv_transpose1d_bwd", _convt_bwd, need_dx=[True, False], need_dw=[True, False], sinks=[True, False], k=[_k], stride=[_stride], pad=[_pad])


def _predicates(e, b, t, c_in, c_mid, c_out):
    return [ops.shares_packed(b, t, 1, 1, 0, 1, 1), ops.ffn_fused_supported(b, t, c_mid, c_out), ops.ln_dense_fused_supported(b, t, c_in, c_mid),
            ops.resdrop_fused_supported(b, t, c_mid, c_out), ops.ffn_packed_supported(b, t, c_in, c_mid, c_out),
            bool(ops.wgrad_takes_bf16(b, c_in, t, c_out, t, 1, 1, 0, 1, 1)), ops.dgrad_mfma_supported(b, c_in, t, c_out, t, 3, 2, 1, 1)]


_variants("predicates", _predicates, b=[1, 2], t=[64], c_in=[256, 16], c_mid=[1024, 12], c_out=[256])


# ---- the tape operators of train/fs2.py: forward, then backward from a given output gradient ------------------------------------------
def _run_tape(e, build):
    tape = Tape()
    y = build(tape)
    y.grad = e.t("dy", *y.data.shape)
    tape.backward()


def _dense(e, k, act, needs_grad):
    _, l1, _ = e.layers(CIN, CMID, COUT, k)
    x = Var(e.t("x", CIN, B, T), needs_grad=needs_grad)
    _run_tape(e, lambda tape: tfs2.dense(tape, x, l1, act))


_variants("tape_dense", _dense, k=[1, 3], act=[ops.ACT_NONE, ops.ACT_RELU, ops.ACT_TANH], needs_grad=[True, False])


def _dense_residual_dropout(e, p, k, t):
    _, l1, _ = e.layers(CIN, CMID, COUT, k)
    h, a = Var(e.t("x", CIN, B, t)), Var(e.t("res", CMID, B, t))
    _run_tape(e, lambda tape: tfs2.dense_residual_dropout(tape, a, h, l1, p, 7, 0.5))


_variants("tape_dense_residual_dropout", _dense_residual_dropout, p=[0.2, 0.0], k=[1], t=[T, 32])
_variants("tape_dense_residual_dropout", _dense_residual_dropout, p=[0.2], k=[3], t=[T])


def _ln_dense(e, cin, k):
    ln, l1, _ = e.layers(cin, CMID, COUT, k)
    x = Var(e.t("x", cin, B, T))
    _run_tape(e, lambda tape: tfs2.ln_dense(tape, x, ln, l1))


_variants("tape_ln_dense", _ln_dense, cin=[128, CIN], k=[1, 3])


def _ffn_core(e, res, p, cin, cmid):
    ln, l1, l2 = e.layers(cin, cmid, cin)
    x = Var(e.t("x", cin, B, 32))
    _run_tape(e, lambda tape: tfs2.ffn_core(tape, x, ln, l1, l2, p, 7, res=x if res else None, seed_out=9, sb=0.5))


_variants("tape_ffn_core", _ffn_core, res=[True, False], p=[0.2, 0.0], cin=[128, CIN], cmid=[CMID, 12])


# ---- the switch matrix ---------------------------------------------------------------------------------------------------------------
SWITCHES = [dict(zip(("operands", "packed", "wgrad", "dgrad", "fwd", "ffn_packed", "resdrop"), c))
            for c in itertools.product(("f32", "bf16"), (True, False), ("mfma", "auto", "gemm"), ("mfma", "gemm"), ("mfma", "gemm"), (True, False), (True, False))]


def _digest(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()[:16]


def run_case(fn, switches, scenario):
    """One case under one switch setting and one query scenario -> (calls, queries, result or error)."""
    saved = dict(ops.CONV_BACKEND), ops.FFN_PACKED[0], ops.RESDROP_FUSION[0], ops.SEED_BASE[0]
    env = Env()
    ops.CONV_BACKEND.update({k: switches[k] for k in ("operands", "packed", "wgrad", "dgrad", "fwd")})
    ops.FFN_PACKED[0], ops.RESDROP_FUSION[0] = switches["ffn_packed"], switches["resdrop"]
    ops.SEED_BASE[0] = env.t("seed_base", 1, dtype=torch.int64)
    REC.begin(SCENARIOS[scenario], env.named)
    try:
        with recording():
            result = fn(env)
        result = result if isinstance(result, list) else None
    except (RuntimeError, AssertionError) as ex:  # a precondition the operator states (e.g. a missing packed input): part of the behaviour
        result = "raised " + type(ex).__name__
    finally:
        ops.CONV_BACKEND.update(saved[0])
        ops.FFN_PACKED[0], ops.RESDROP_FUSION[0], ops.SEED_BASE[0] = saved[1:]
    return REC.calls, REC.queries, result


def trace_all(cases=None, switches=None, scenarios=None):
    traces, queries, out = {}, {}, {}
    for name, fn in CASES.items():
        if cases and not any(name.startswith(c) for c in cases):
            continue
        for sw in switches or SWITCHES:
            for sc in scenarios or SCENARIOS:
                calls, qs, result = run_case(fn, sw, sc)
                distinct = sorted({json.dumps(q) for q in qs})
                dc, dq = _digest(calls), _digest(distinct)
                traces.setdefault(dc, calls)
                queries.setdefault(dq, [json.loads(q) for q in distinct])
                cid = name + "|" + ",".join(f"{k}={v}" for k, v in sw.items()) + "|" + sc
                out[cid] = {"trace": dc, "queries": dq, "n_queries": len(qs), "result": result}
    return {"traces": traces, "queries": queries, "cases": out}


def compare(parent, head):
    """Problems (strings) that keep ``head`` from issuing ``parent``'s library calls: another call sequence or result in a case, more
    queries, a query with arguments the parent never asked with."""
    bad = []
    if set(parent["cases"]) != set(head["cases"]):
        bad.append(f"case sets differ: {sorted(set(parent['cases']) ^ set(head['cases']))[:5]} ...")
    for cid, p in parent["cases"].items():
        h = head["cases"].get(cid)
        if h is None:
            continue
        if parent["traces"][p["trace"]] != head["traces"][h["trace"]]:
            bad.append(f"{cid}: the call sequence differs")
        if p["result"] != h["result"]:
            bad.append(f"{cid}: result {p['result']} -> {h['result']}")
        if h["n_queries"] > p["n_queries"]:
            bad.append(f"{cid}: {p['n_queries']} -> {h['n_queries']} queries")
        asked = {json.dumps(q) for q in parent["queries"][p["queries"]]}
        new = [q for q in head["queries"][h["queries"]] if json.dumps(q) not in asked]
        if new:
            bad.append(f"{cid}: queries the parent did not make: {new[:2]}")
    return bad


def main(argv):
    if argv[:1] == ["--compare"]:
        parent, head = (json.loads(Path(p).read_text()) for p in argv[1:3])
        bad = compare(parent, head)
        n = len(parent["cases"])
        fewer = sum(head["cases"][c]["n_queries"] < p["n_queries"] for c, p in parent["cases"].items() if c in head["cases"])
        print(f"{n} cases, {len(parent['traces'])} distinct call sequences: {'identical' if not bad else f'{len(bad)} differences'}; "
              f"fewer queries in {fewer} cases")
        for b in bad[:40]:
            print("  " + b)
        return 1 if bad else 0
    json.dump(trace_all(cases=argv or None), sys.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
