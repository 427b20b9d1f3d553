#!/usr/bin/env python3
"""What a ragged vocoder batch costs: HiFiGAN-V1 in bf16, B = 32, T = 768, three forms of the same work timed with device events,
alternating in one process:

  padded   Generator(mel)                 the rectangle, padding frames computed and thrown away
  ragged   Generator(mel, lens=lens)      every kernel bounded by the item's length, tiles beyond it not computed
  solo     32 x Generator(mel[i, :, :n])  one forward per item: the form whose bits the ragged one reproduces

on two seeded sets of lengths: all equal to T, and spread uniformly over [96, 768].  Prints ONE JSON line; per set the three median
times and fill = sum(lens) / (B * T), the share of the rectangle that is real work (ragged_over_padded is to be read against it).

  python tools/vocoder_ragged_bench.py [--rounds 9] [--warmup 2]
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

B, T, LOW = 32, 768, 96


def main(argv=None):
    import torch

    from everyvoice_amd.config import HiFiGANConfig
    from everyvoice_amd.vocoder import Generator

    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--warmup", type=int, default=2)
    args = p.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    gen = Generator(HiFiGANConfig(), precision="bf16").to(dev).eval()
    g = torch.Generator().manual_seed(1234)
    mel = torch.clamp(torch.randn(B, 80, T, generator=g) * 2.0 - 5.0, -11.5129, 2.0).to(dev)
    sets = {"uniform": torch.full((B,), T, dtype=torch.int32), "spread": torch.randint(LOW, T + 1, (B,), generator=g, dtype=torch.int32)}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    out = {"tool": "vocoder_ragged_bench", "model": "hifigan_v1", "dtype": "bf16", "B": B, "T": T, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    for name, lens in sets.items():
        dev_lens = lens.to(dev)
        items = [mel[i : i + 1, :, : int(n)].contiguous() for i, n in enumerate(lens.tolist())]
        forms = {
            "padded": lambda: gen(mel),
            "ragged": lambda: gen(mel, lens=dev_lens),
            "solo": lambda: [gen(x) for x in items],
        }
        ms = {k: [] for k in forms}
        for r in range(args.warmup + args.rounds):
            for k, fn in forms.items():  # alternating: the three forms share clocks and thermal state
                t = timed(fn)
                if r >= args.warmup:
                    ms[k].append(t)
        med = {k: statistics.median(v) for k, v in ms.items()}
        fill = float(lens.sum()) / (B * T)
        out[name] = {
            "fill": round(fill, 4), "lens_min": int(lens.min()), "lens_max": int(lens.max()),
            "padded_ms": round(med["padded"], 3), "ragged_ms": round(med["ragged"], 3), "solo_loop_ms": round(med["solo"], 3),
            "ragged_over_padded": round(med["ragged"] / med["padded"], 4),
            "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
