"""Device time of a dataset's SoX effect chain on one preprocessing batch ("SoX effect chains").

    python tools/sox_effects_bench.py [--items 32] [--seconds 10] [--rate 22050] [--iters 20]

The batch is synthetic, on the 16-bit grid: tone bursts of 0.2-1.5 s between noise-floor gaps of 0.1-0.8 s, so every rule of the
wizard's chains has work to do.  Times the wizard's full chain (channels 1, norm -3, start-and-end trim, gap removal) and each part,
with torch.cuda events around `iters` calls after two warm-up calls, and prints one JSON line."""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from everyvoice_amd.sox import apply_sox_effects, parse_sox_effects  # noqa: E402

CHAINS = {
    "full": [["channels", "1"], ["norm", "-3.0"], ["silence", "1", "0.1", "0.1%"], ["reverse"], ["silence", "1", "0.1", "0.1%"], ["reverse"],
             ["silence", "1", "0.1", "1.0%", "-1", "0.4", "1%"]],
    "norm": [["norm", "-3.0"]],
    "trim_ends": [["silence", "1", "0.1", "0.1%"], ["reverse"], ["silence", "1", "0.1", "0.1%"], ["reverse"]],
    "remove_gaps": [["silence", "1", "0.1", "1.0%", "-1", "0.4", "1%"]],
}


def batch(items: int, seconds: float, rate: int, seed: int = 0) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    n = int(seconds * rate)
    out = np.zeros((items, n), dtype=np.float32)
    for i in range(items):
        pos, loud = 0, False
        while pos < n:
            k = int(rng.uniform(0.2, 1.5) * rate) if loud else int(rng.uniform(0.1, 0.8) * rate)
            k = min(k, n - pos)
            if loud:
                f = rng.uniform(100, 300)
                seg = rng.uniform(0.2, 0.6) * np.sin(2 * np.pi * f * np.arange(k) / rate)
            else:
                seg = rng.uniform(-1e-3, 1e-3, k)
            out[i, pos : pos + k] = seg
            pos, loud = pos + k, not loud
    return torch.from_numpy(np.round(out * 32767) / 32768)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x = batch(a.items, a.seconds, a.rate).to(dev)
    lens = torch.full((a.items,), x.shape[1], dtype=torch.int32, device=dev)
    result = {"items": a.items, "seconds": a.seconds, "rate": a.rate, "iters": a.iters}
    for name, chain in CHAINS.items():
        effects = parse_sox_effects(chain)
        for _ in range(2):
            y, out_lens = apply_sox_effects(x, lens, a.rate, effects)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            y, out_lens = apply_sox_effects(x, lens, a.rate, effects)
        t1.record()
        torch.cuda.synchronize()
        result[f"{name}_ms"] = round(t0.elapsed_time(t1) / a.iters, 4)
        result[f"{name}_kept_fraction"] = round(float(out_lens.sum()) / (a.items * x.shape[1]), 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
