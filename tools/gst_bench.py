#!/usr/bin/env python3
"""Global Style Token module: what it costs.  One JSON line with
  * the FastSpeech2 training step (the batch bench.py times: 32 items, default model, learned alignment, captured into a HIP graph)
    with the module off and on -- same script, same batch, interleaved rounds, median of the rounds;
  * the same step with the module length-masked (model.gst_mask_padding), and the module on unmasked / masked
    with and without graph_buckets: eager without buckets is what a style-token user was told to run before the flag, a replayed
    graph under buckets is what the flag allows;
  * the latency of ONE style embedding from a 947-frame reference (fs2.StyleTokens.forward, default size), alone and as the shortest of
    a padded batch with lengths.
usage: gst_bench.py [steps per round = 20] [rounds = 3] [precision = bf16] [only = "" | "on" | "off" | "masked"]
only: ONE trainer (module on / off / on and masked), four warm-up steps and `steps` timed ones, nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats`: the difference of the two runs' kernel calls, divided by 4 + steps, is what the module adds to a step."""
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import torch  # noqa: E402

from fs2_train_bench import training_batch  # noqa: E402

BUCKETS = (16, 64)  # (symbols, frames): the multiples the documented example pads to


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    from everyvoice_amd.fs2 import FastSpeech2, FastSpeech2ModelConfig
    from everyvoice_amd.train.fs2 import FastSpeech2Trainer

    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    precision = sys.argv[3] if len(sys.argv) > 3 else "bf16"
    only = sys.argv[4] if len(sys.argv) > 4 else ""
    dev = torch.device("cuda:0")
    batch, _ = training_batch(32, learn_alignment=True, device=dev)
    # name -> (module, masked, graph, graph_buckets); the first two are the pair this tool has always printed
    variants = {"off": (False, False, True, None), "on": (True, False, True, None), "masked": (True, True, True, None),
                "on_eager": (True, False, False, None), "masked_eager": (True, True, False, None),
                "on_buckets_graph": (True, False, True, BUCKETS), "masked_buckets_graph": (True, True, True, BUCKETS)}
    trainers = {}
    for name, (flag, masked, graph, buckets) in variants.items():
        if only and name != only:
            continue
        cfg = FastSpeech2ModelConfig(learn_alignment=True, use_global_style_token_module=flag, gst_mask_padding=masked)
        tr = FastSpeech2Trainer(cfg, device=dev, precision=precision, use_graph=graph, graph_buckets=buckets)
        tr.batch_ready = True
        for _ in range(4):  # two eager steps, the capture, one replay
            tr.training_step(batch)
        torch.cuda.synchronize()
        trainers[name] = tr
    if only:
        print(json.dumps({"only": only, "precision": precision, "steps": steps, "ms_per_step": timed(lambda: trainers[only].training_step(batch), steps)}))
        return
    ms = {name: [] for name in trainers}
    for _ in range(rounds):
        for name, tr in trainers.items():
            ms[name].append(timed(lambda: tr.training_step(batch), steps))
    med = {name: statistics.median(v) for name, v in ms.items()}
    out = {"precision": precision, "steps_per_round": steps,
           "fs2_train_ms_per_step_module_off": med["off"], "fs2_train_ms_per_step_module_on": med["on"],
           "fs2_train_ms_per_step_module_masked": med["masked"],
           "fs2_train_ms_per_step": {k: round(v, 3) for k, v in med.items()},
           "masked_over_unmasked_graph": med["masked"] / med["on"],
           "masked_buckets_graph_over_unmasked_eager": med["masked_buckets_graph"] / med["on_eager"],
           "graph_buckets": list(BUCKETS), "padded_frames": {k: int(t._prepare(batch)[1]["T"]) for k, t in trainers.items() if k in ("on", "masked_buckets_graph")},
           "rounds_off": [round(v, 3) for v in ms["off"]], "rounds_on": [round(v, 3) for v in ms["on"]],
           "rounds": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "graph": {k: bool(t.last_step_was_graph) for k, t in trainers.items()},
           "parameters": {k: t.params.numel() for k, t in trainers.items()}}
    model = FastSpeech2(FastSpeech2ModelConfig(use_global_style_token_module=True), device=dev).init_random(1)
    mel = torch.randn(1, 947, 80, device=dev)
    for _ in range(5):
        model.gst.forward(mel)
    out["style_embedding_ms_947_frames"] = timed(lambda: model.gst.forward(mel), 50)
    mel32 = torch.randn(32, 947, 80, device=dev)
    for _ in range(3):
        model.gst.forward(mel32)
    out["style_embedding_ms_947_frames_batch_32"] = timed(lambda: model.gst.forward(mel32), 20)
    lens32 = torch.full((32,), 947, dtype=torch.int32, device=dev)
    lens32[0] = 240  # the shortest of a padded batch: its rows beyond 240 frames cost stores, not FMAs
    for _ in range(3):
        model.gst.forward(mel32, lens32)
    out["style_embedding_ms_947_frames_batch_32_with_lengths"] = timed(lambda: model.gst.forward(mel32, lens32), 20)
    one = torch.full((1,), 947, dtype=torch.int32, device=dev)
    out["style_embedding_ms_947_frames_with_lengths"] = timed(lambda: model.gst.forward(mel, one), 50)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
