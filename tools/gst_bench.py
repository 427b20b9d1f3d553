#!/usr/bin/env python3
"""Global Style Token module: what it costs.  One JSON line with
  * the FastSpeech2 training step (the batch bench.py times: 32 items, default model, learned alignment, captured into a HIP graph)
    with the module off and on -- same script, same batch, interleaved rounds, median of the rounds;
  * the latency of ONE style embedding from a 947-frame reference (fs2.StyleTokens.forward, default size).
usage: gst_bench.py [steps per round = 20] [rounds = 3] [precision = bf16] [only = "" | "on" | "off"]
only: ONE trainer (module on / off), four warm-up steps and `steps` timed ones, nothing else -- the run to put under
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
    trainers = {}
    for name, flag in (("off", False), ("on", True)):
        if only and name != only:
            continue
        tr = FastSpeech2Trainer(FastSpeech2ModelConfig(learn_alignment=True, use_global_style_token_module=flag), device=dev, precision=precision,
                                use_graph=True)
        tr.batch_ready = True
        for _ in range(4):  # two eager steps, the capture, one replay
            tr.training_step(batch)
        torch.cuda.synchronize()
        trainers[name] = tr
    if only:
        print(json.dumps({"only": only, "precision": precision, "steps": steps, "ms_per_step": timed(lambda: trainers[only].training_step(batch), steps)}))
        return
    ms = {"off": [], "on": []}
    for _ in range(rounds):
        for name, tr in trainers.items():
            ms[name].append(timed(lambda: tr.training_step(batch), steps))
    out = {"precision": precision, "steps_per_round": steps,
           "fs2_train_ms_per_step_module_off": statistics.median(ms["off"]), "fs2_train_ms_per_step_module_on": statistics.median(ms["on"]),
           "rounds_off": [round(v, 3) for v in ms["off"]], "rounds_on": [round(v, 3) for v in ms["on"]],
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
