#!/usr/bin/env python3
"""Alignment scores: the fused call (evmi_align_scores_f32, csrc/align_scores.hip) beside the chain that was the only way to the same
numbers before it -- ops.align_attention_fwd (soft attention and log-probabilities as [B, T, L] tensors) -> evmi_forward_sum_loss_f32 ->
a gather along the path and a sum per symbol in torch on the device --, alternated in one process: every round times each once, so drift
of the clocks or of a shared machine lands on both alike.  Shape: the batch of tools/align_infer_bench.py -- B 32, ragged, about 100
symbols and 585 frames an utterance, planted alignments under the beta-binomial prior at the model's temperature; the rows scored are
what evmi_align_durations_f32 finds on it.  Prints both times (median, min, max over the rounds), both memory footprints (the bytes each
way allocates beside its inputs, from the shapes, and the peak the allocator saw during one call) and how far the two ways' numbers lie
apart.  (They may differ beyond rounding in a ragged batch: with a prior the chain's log-softmax runs over the padded keys too, as the
trainer's does; the fused call reads each item's own symbols alone.)

usage: python tools/align_scores_bench.py [out.json] [rounds]"""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import torch  # noqa: E402

BLANK = -1.0


def main():
    from align_infer_bench import A, B, TEMPERATURE, batch

    from everyvoice_amd import _lib
    from everyvoice_amd.train import ops

    out_path = sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "align_scores_bench.json")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    q, k, prior, tl, ml, L, T = batch(dev)
    dur = ops.align_durations(q, k, prior, tl, ml, TEMPERATURE)
    lib = _lib.load()
    frames = torch.arange(T, device=dev)[None, :].expand(B, T).contiguous()

    def fused():
        return ops.align_scores(q, k, prior, tl, ml, dur, TEMPERATURE, BLANK)

    def chain():
        soft, logprob = ops.align_attention_fwd(q, k, prior, tl, TEMPERATURE)
        ctc = torch.empty(B, device=dev, dtype=torch.float32)
        _lib.check(lib.evmi_forward_sum_loss_f32(logprob.data_ptr(), tl.data_ptr(), ml.data_ptr(), ctc.data_ptr(), B, T, L, BLANK, _lib.current_stream_ptr(dev)),
                   "evmi_forward_sum_loss_f32")
        symbol_of = torch.searchsorted(dur.cumsum(1), frames, right=True).clamp_(max=L - 1)  # [B, T]: the symbol that holds each frame
        on_path = torch.log(torch.clamp(soft.gather(2, symbol_of[:, :, None])[:, :, 0], min=1e-12)) * (frames < ml[:, None])
        path = -on_path.sum(1) / ml
        symbol = torch.zeros(B, L, device=dev).scatter_add_(1, symbol_of, on_path) / dur
        return ctc, path, torch.where(torch.arange(L, device=dev)[None, :] < tl[:, None], symbol, torch.zeros_like(symbol))

    jobs = {"fused": fused, "chain": chain}
    peak, results = {}, {}
    for name, run in jobs.items():  # first calls: code objects loaded, LDS attributes set -- and the allocator's peak
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        results[name] = [t.double().cpu() for t in run()]
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated(dev) - before
        run()
    torch.cuda.synchronize()
    times = {name: [] for name in jobs}
    for _ in range(rounds):
        for name, run in jobs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3)
    cells = B * T * L
    apart = {what: float((a - b).abs().max()) for what, a, b in zip(("ctc", "path", "symbol"), results["fused"], results["chain"])}
    result = {"B": B, "L": L, "T": T, "A": A, "mean_text_len": float(tl.float().mean()), "mean_mel_len": float(ml.float().mean()),
              "temperature": TEMPERATURE, "rounds": rounds, "device": torch.cuda.get_device_name(0),
              "us_per_call": {name: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for name, v in times.items()},
              "bytes_from_shapes": {"prior (both)": 8 * cells, "fused: ctc, path, symbol": 4 * (2 * B + B * L),
                                    "chain: soft, logprob (4 B a cell each) + frame-to-symbol map and path terms (8 + 4 B a frame) + the results":
                                        8 * cells + 12 * B * T + 4 * (2 * B + B * L)},
              "allocator_peak_bytes_first_call": peak,
              "all_finite": {name: bool(all(torch.isfinite(t).all() for t in r)) for name, r in results.items()},
              "mean_scores_fused": {what: float(t[t != 0].mean()) for what, t in zip(("ctc", "path", "symbol"), results["fused"])},
              "fused_minus_chain_max_abs": apart}
    text = json.dumps(result, indent=1)
    print(text)
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(text + "\n")


if __name__ == "__main__":
    main()
