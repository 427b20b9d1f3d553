#!/usr/bin/env python3
"""One bf16 GAN training step (captured graph, as bench.py runs it) at B = 16 x 8192 output samples for three configurations:
  a  the default configuration (22.05 kHz in and out, spec_type "mel-librosa");
  b  22.05 -> 44.1 kHz: upsample_rates [8, 8, 4, 2], kernels [16, 16, 8, 4]; the reconstruction loss at 2048 / 2048 / 512;
  c  spec_type "mel" (torchaudio mel: power spectrum, HTK scale) at the default rates.
Device events around ``--steps`` steps, the cases alternating in one process after a warm-up of every shape (which captures each
trainer's graph).  Prints one JSON line: per case ms per step (median, min, max over the repetitions).  Nothing is targeted for b and c:
their times are recorded.  ``--cases a`` times the default step alone (what a parent / HEAD comparison alternates between processes).
Usage: python tools/vocoder_rates_bench.py [--reps 7] [--steps 5] [--cases abc] [--out profiles/vocoder_rates_bench.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from everyvoice_amd.config import HiFiGANConfig  # noqa: E402
from everyvoice_amd.train.hifigan import HiFiGANTrainer  # noqa: E402

CASES = {
    "a": (dict(), dict(), 256),
    "b": (dict(upsample_rates=[8, 8, 4, 2], upsample_kernel_sizes=[16, 16, 8, 4]), dict(output_sampling_rate=44100), 512),
    "c": (dict(), dict(spec_type="mel"), 256),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=8192)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234)
    y = (0.3 * torch.tanh(torch.randn(a.batch, 1, a.samples, generator=g))).to(dev)
    jobs = {}
    for name in a.cases:
        model, audio, hop = CASES[name]
        tr = HiFiGANTrainer(HiFiGANConfig(model=model, preprocessing=dict(audio=audio)), device=dev, precision="bf16", use_graph=True)
        mel = (torch.randn(a.batch, 80, a.samples // hop, generator=g) * 2.0 - 5.0).clamp(-11.5129, 2.0).to(dev)
        jobs[name] = (tr, mel)
    losses = {}
    for name, (tr, mel) in jobs.items():  # warm-up: two eager steps, the capture, one replay
        for _ in range(4):
            losses[name] = tr.training_step(mel, y)
        assert tr._graph_failed is None and len(tr._graphs) == 1, (name, tr._graph_failed)
    torch.cuda.synchronize()
    ms = {name: [] for name in jobs}
    for _ in range(a.reps):
        for name, (tr, mel) in jobs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                tr.training_step(mel, y, sync=False)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    result = {"label": a.label, "batch": a.batch, "samples": a.samples, "precision": "bf16", "graph": True, "reps": a.reps, "steps_per_rep": a.steps,
              "cases": {name: {"ms_per_step_median": statistics.median(v), "ms_per_step_min": min(v), "ms_per_step_max": max(v),
                               "ms_per_step": [round(x, 4) for x in v], "g_mel_after_warmup": losses[name]["g_mel"]} for name, v in ms.items()}}
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
