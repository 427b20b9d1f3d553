"""The pieces of the FastSpeech2 training step that stand alone (everyvoice_amd/train/step.py: SideBranch; train/fs2.py: the tape operators
of the embeddings, the length regulator and the positional term), without a GPU: a SideBranch that is not enabled runs inline, and the
operators are read off the library calls they issue (tools/ops_call_trace.py: the recorder stands in for the library)."""

import importlib.util
from pathlib import Path

import pytest
import torch

from everyvoice_amd.train import fs2 as tfs2
from everyvoice_amd.train import ops
from everyvoice_amd.train.autograd import Tape, Var, activation_elements, alias
from everyvoice_amd.train.layers import ParamGroup
from everyvoice_amd.train.step import SideBranch

_spec = importlib.util.spec_from_file_location("ops_call_trace", Path(__file__).resolve().parent.parent / "tools" / "ops_call_trace.py")
trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(trace)

CPU = torch.device("cpu")


# ---- SideBranch, not enabled --------------------------------------------------------------------------------------------------------
def test_a_branch_that_is_not_enabled_adds_its_aliases_gradients_in_the_documented_order_once_each(monkeypatch):
    """Two aliases of one tensor on a branch, one reader on the main tape: x.grad = main's, then the second alias's, then the first
    alias's (the joins run in reverse order of the aliases' creation) -- each exactly once, whatever the branch's backward did before."""
    added = []
    monkeypatch.setattr(ops, "axpby", lambda a, x, b, y, out=None: (added.append(float(y[0])), out.copy_(a * x + b * y))[1])
    br = SideBranch(CPU, enabled=False)
    assert br.stream is None and not br.enabled
    tape = Tape()
    x = Var(torch.zeros(3))
    a1, a2 = tfs2.joined_alias(tape, br, x), tfs2.joined_alias(tape, br, x)
    assert a1.data is x.data and a2.data is x.data
    tape.record(lambda: x.accumulate(torch.full((3,), 1.0)))                       # the main chain's own reader of x
    assert br.fork(lambda a, b: (a, b), 7, 8) == (7, 8) and br.fork(lambda: 5, done=False) == 5  # inline, arguments handed on
    br.tape.record(lambda: a1.accumulate(torch.full((3,), 10.0)))
    br.tape.record(lambda: a2.accumulate(torch.full((3,), 100.0)))
    br.kept.append(torch.zeros(1))
    br.backward()
    assert x.grad is None and float(a1.grad[0]) == 10.0 and float(a2.grad[0]) == 100.0 and not br.tape._ops
    br.backward()  # (an empty tape: nothing)
    br.join()
    br.join()      # (a second join: nothing)
    tape.backward()
    assert added == [100.0, 10.0] and torch.equal(x.grad, torch.full((3,), 111.0))
    br.close()
    assert br.kept == []
    br.hand_over(x.data)  # (not enabled: nothing to hand over)


def test_begin_opens_a_new_use_and_a_branch_without_a_stream_stays_inline():
    br = SideBranch(CPU, enabled=False)
    old = br.tape
    br.tape.record(lambda: None)
    br.kept.append(torch.zeros(1))
    assert br.begin(True) is br and not br.enabled  # (constructed without a stream: it cannot be switched on)
    assert br.tape is not old and not br.tape._ops and br.kept == []


def test_alias_shares_the_data_and_is_not_counted():
    activation_elements(reset=True)
    x = Var(torch.zeros(4, 5))
    a = alias(x)
    assert a.data is x.data and a.grad is None and a.needs_grad and activation_elements() == 20


# ---- the tape operators under the call recorder -------------------------------------------------------------------------------------
D, B, L, T, ROWS = 6, 2, 5, 9, 4
REC = trace.REC


class _Case:
    """Named tensors, a small parameter group (a table of ROWS rows, the bias-free Linear of the phonological features) and the calls of
    one operator: ``run(build)`` -> (forward calls, backward calls, output Var, activation elements the forward counted)."""

    def __init__(self):
        self.env = e = trace.Env()
        g = ParamGroup(CPU)
        self.table = tfs2.Table(g, "table.weight", ROWS, D)
        self.linear = tfs2.Dense(g, "text_input_layer.weight", None, 43, D, linear=True)
        g.finalize()
        e.named["params"], e.named["grads"] = g.flat, g.grad
        self.lens = e.t("lens", B, dtype=torch.int32)
        self.inv_freq = e.t("inv_freq", D // 2)

    def run(self, build, grad=True):
        REC.begin([], self.env.named)
        with trace.recording():
            tape = Tape()
            activation_elements(reset=True)
            y = build(tape)
            counted = activation_elements()
            fwd = list(REC.calls)
            if grad:
                y.grad = self.env.t("dy", *y.data.shape)
            tape.backward()
        return fwd, REC.calls[len(fwd):], y, counted


def _names(calls):
    return [c[0] for c in calls]


@pytest.mark.parametrize("position", [False, True])
def test_text_embedding_of_symbol_ids(position):
    c = _Case()
    ids = c.env.t("ids", B, L, dtype=torch.int32)
    fwd, bwd, y, counted = c.run(lambda tape: tfs2.embed_text(tape, ids, c.lens, c.table, c.inv_freq if position else None))
    assert fwd == [["evmi_fs2_embed_f32", ["ids", "lens", "params", "inv_freq" if position else "NULL", "PTR", B, L, D, "STREAM"]]]
    assert bwd == [["evmi_fs2_embed_bwd_f32", ["dy", "ids", "lens", "grads", ROWS, B, L, D, 0, "STREAM"]]]
    assert tuple(y.data.shape) == (D, B, L) and counted == D * B * L
    assert c.run(lambda tape: tfs2.embed_text(tape, ids, c.lens, c.table), grad=False)[1] == []


@pytest.mark.parametrize("position", [False, True])
def test_text_embedding_of_phonological_features(position):
    """The Linear (tfs2.dense's calls, whatever kernels serve it), then a masked copy, or a copy with the positional term whose backward
    is the mask of a copy of the gradient; the Linear's backward follows on the masked gradient."""
    c = _Case()
    feats = c.env.t("pfs", 43, B, L)
    only_dense = c.run(lambda tape: tfs2.dense(tape, Var(feats, needs_grad=False), c.linear))
    fwd, bwd, y, counted = c.run(lambda tape: tfs2.embed_text(tape, feats, c.lens, c.linear, c.inv_freq if position else None))
    assert fwd[:-1] == only_dense[0] and _names(bwd[1:]) == _names(only_dense[1])
    if position:
        assert fwd[-1] == ["evmi_fs2_add_posemb_f32", ["PTR", "lens", "inv_freq", B, L, D, "STREAM"]]
    else:
        assert fwd[-1] == ["evmi_mask_cols_f32", ["PTR", "lens", D, B, L, "STREAM"]]
    assert bwd[0] == ["evmi_mask_cols_f32", ["PTR", "lens", D, B, L, "STREAM"]]  # (a copy of the gradient: "dy" itself stays as it was)
    assert counted == 43 * B * L + 2 * D * B * L
    assert c.run(lambda tape: tfs2.embed_text(tape, feats, c.lens, c.linear, c.inv_freq if position else None), grad=False)[1] == []


def test_item_embedding_for_a_table_and_for_the_style_matrix_differ_in_table_rows_and_sink_only():
    c = _Case()
    x, item_ids = c.env.t("x", D, B, L), c.env.t("item_ids", B, dtype=torch.int32)
    style = Var(c.env.t("style", B, D))
    xv, xs = Var(x), Var(x)
    t_fwd, t_bwd, y, counted = c.run(lambda tape: tfs2.add_item_embedding(tape, xv, item_ids, c.lens, c.table.data(), c.table.grad()))
    assert t_fwd == [["evmi_fs2_add_item_embedding_f32", ["PTR", "item_ids", "lens", "params", B, L, D, "STREAM"]]]
    assert t_bwd == [["evmi_fs2_item_embedding_bwd_f32", ["dy", "item_ids", "lens", "grads", ROWS, B, L, D, "STREAM"]]]
    assert xv.grad is y.grad and y.data is not x and counted == D * B * L
    s_fwd, s_bwd, y, counted = c.run(lambda tape: tfs2.add_item_embedding(tape, xs, item_ids, c.lens, style.data, style))
    assert s_fwd == [[t_fwd[0][0], t_fwd[0][1][:3] + ["style"] + t_fwd[0][1][4:]]]
    assert s_bwd == [[t_bwd[0][0], t_bwd[0][1][:3] + ["PTR", B] + t_bwd[0][1][5:]]]
    assert xs.grad is y.grad and tuple(style.grad.shape) == (B, D) and not style.grad.any() and counted == D * B * L
    assert c.run(lambda tape: tfs2.add_item_embedding(tape, Var(x), item_ids, c.lens, style.data, style), grad=False)[1] == []


def test_bucket_embedding():
    c = _Case()
    x, values, bins = Var(c.env.t("x", D, B, L)), c.env.t("values", B, L), c.env.t("bins", ROWS - 1)
    fwd, bwd, y, counted = c.run(lambda tape: tfs2.add_bucket_embedding(tape, x, values, bins, c.table))
    assert fwd == [["evmi_fs2_bucket_embed_add_f32", ["PTR", "values", "bins", "params", ROWS, B, L, D, 1.0, "STREAM"]]]
    assert bwd == [["evmi_fs2_bucket_embed_bwd_f32", ["dy", "values", "bins", "grads", "PTR", ROWS, B, L, D, 1.0, "STREAM"]]]
    assert x.grad is y.grad and counted == D * B * L
    assert c.run(lambda tape: tfs2.add_bucket_embedding(tape, Var(x.data), values, bins, c.table), grad=False)[1] == []


@pytest.mark.parametrize("position", [False, True])
def test_length_regulator_masks_the_gradient_first(position):
    c = _Case()
    x, cum, mel_lens = Var(c.env.t("x", D, B, L)), c.env.t("cum", B, L, dtype=torch.int32), c.env.t("mel_lens", B, dtype=torch.int32)
    fwd, bwd, y, counted = c.run(lambda tape: tfs2.length_regulate(tape, x, cum, mel_lens, T, c.inv_freq if position else None))
    assert fwd[0] == ["evmi_length_regulate_cbt_f32", ["x", "cum", "PTR", D, B, L, T, "STREAM"]]
    assert fwd[1:] == ([["evmi_fs2_add_posemb_f32", ["PTR", "mel_lens", "inv_freq", B, T, D, "STREAM"]]] if position else [])
    assert bwd == [["evmi_mask_cols_f32", ["dy", "mel_lens", D, B, T, "STREAM"]],
                   ["evmi_length_regulate_bwd_cbt_f32", ["dy", "cum", "PTR", D, B, L, T, "STREAM"]]]
    assert tuple(y.data.shape) == (D, B, T) and tuple(x.grad.shape) == (D, B, L) and counted == D * B * T
    assert c.run(lambda tape: tfs2.length_regulate(tape, Var(x.data), cum, mel_lens, T), grad=False)[1] == []


def test_the_positional_term_in_place_gives_an_alias_and_its_backward_is_the_mask():
    c = _Case()
    h, mel_lens = Var(c.env.t("h", D, B, T)), c.env.t("mel_lens", B, dtype=torch.int32)
    fwd, bwd, y, counted = c.run(lambda tape: tfs2.add_position_(tape, h, mel_lens, c.inv_freq))
    assert fwd == [["evmi_fs2_add_posemb_f32", ["h", "mel_lens", "inv_freq", B, T, D, "STREAM"]]]
    assert bwd == [["evmi_mask_cols_f32", ["dy", "mel_lens", D, B, T, "STREAM"]]]
    assert y.data is h.data and h.grad is y.grad and counted == 0
    assert c.run(lambda tape: tfs2.add_position_(tape, Var(h.data), mel_lens, c.inv_freq), grad=False)[1] == []
