#!/usr/bin/env python3
"""The aligner at inference: the fused call (evmi_align_durations_f32, csrc/align_infer.hip) beside the chain that was the only way to
the same durations before it (ops.align_attention_fwd -> log -> heavy.maximum_path), alternated in one process: every round times
each once, so drift of the clocks or of a shared machine lands on both alike.  Shape: the LJSpeech-shaped batch of the benchmark --
B 32, about 100 symbols and 566 frames an utterance, ragged -- with planted alignments (tests/align_ref.py) under the beta-binomial prior
at the model's temperature.  Prints both times (median, min, max over the rounds) and both memory footprints: the bytes each way
allocates beside its inputs, from the shapes, and the peak the allocator saw during one call.

usage: python tools/align_infer_bench.py [out.json] [rounds]"""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, A, TEMPERATURE = 32, 80, 0.0005


def batch(dev):
    from align_ref import planted_case

    from everyvoice_amd.heavy import BetaBinomialInterpolator

    rng = np.random.default_rng(0)
    text_lens = rng.integers(60, 141, B)
    mel_lens = np.maximum(text_lens, np.round(text_lens * rng.uniform(5.0, 6.3, B)).astype(np.int64))
    L, T = int(text_lens.max()), int(mel_lens.max())
    q, k = torch.zeros(A, B, T), torch.zeros(A, B, L)
    prior = torch.zeros(B, T, L, dtype=torch.float64, device=dev)
    interp = BetaBinomialInterpolator(device=dev)
    for b in range(B):
        qb, kb, _ = planted_case(int(text_lens[b]), int(mel_lens[b]), seed=b)
        q[:, b, : mel_lens[b]], k[:, b, : text_lens[b]] = torch.from_numpy(qb), torch.from_numpy(kb)
        prior[b, : mel_lens[b], : text_lens[b]] = interp(int(mel_lens[b]), int(text_lens[b]))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    return q.to(dev), k.to(dev), prior, i32(text_lens), i32(mel_lens), L, T


def main():
    from everyvoice_amd.heavy import maximum_path
    from everyvoice_amd.train import ops

    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    q, k, prior, tl, ml, L, T = batch(dev)

    def fused():
        return ops.align_durations(q, k, prior, tl, ml, TEMPERATURE)

    def chain():
        soft, _ = ops.align_attention_fwd(q, k, prior, tl, TEMPERATURE)
        return maximum_path(ops.elementwise(16, soft), ml, tl)[1]

    jobs = {"fused": fused, "chain": chain}
    peak, results = {}, {}
    for name, run in jobs.items():  # first calls: code objects loaded, LDS attributes set, workspaces grown -- and the allocator's peak
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        results[name] = run().to(torch.int64).cpu()
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
    sums_ok = {name: bool((r.sum(1) == ml.cpu()).all()) for name, r in results.items()}
    result = {"B": B, "L": L, "T": T, "A": A, "mean_text_len": float(tl.float().mean()), "mean_mel_len": float(ml.float().mean()),
              "temperature": TEMPERATURE, "rounds": rounds, "device": torch.cuda.get_device_name(0),
              "us_per_call": {name: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for name, v in times.items()},
              "bytes_from_shapes": {"prior (both)": 8 * cells, "fused: 1 decision byte a cell (rows padded to 16) + durations": ops.align_durations_ws_bytes(B, T, L) + 4 * B * L,
                                    "chain: soft, logprob, log(soft), path (4 B each) + 1 scratch byte a cell + durations": 17 * cells + 12 * B * L},
              "allocator_peak_bytes_first_call": peak,
              "rows_sum_to_mel_lens": sums_ok, "rows_equal": int((results["fused"] == results["chain"]).all(1).sum())}
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(text + "\n")


if __name__ == "__main__":
    main()
