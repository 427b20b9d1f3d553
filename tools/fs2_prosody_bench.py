"""What prosody steering costs, at the FastSpeech2 inference shape ``bench.py --full`` times: B = 32 LJSpeech-shaped
texts, default model sizes, random parameters (``tools/fs2_bench.synthetic_batch``).

  python tools/fs2_prosody_bench.py [--parent DIR] [--rounds 7] [--steps 30] [--warmup 5] [--precision bf16] [--out FILE.json]

Two questions, one job:
  * default forward, parent against this tree: ``--parent DIR`` names a built checkout of the parent commit.  The two trees are timed in
    processes of their own (each imports its own package and library), ALTERNATING, ``--rounds`` times each; the medians over the rounds
    are compared.  The launches are the same, so no difference is expected; what is seen is reported.
  * steered forwards against the default forward of this tree, in the same process, with ``target_frames`` = the frame counts the default
    forward's given durations sum to, so that the decoder works on the same lengths.  ``controls``: a control per symbol for the durations,
    the pitch and the energy, nothing forced -- every predictor runs as in the default forward, so the difference is the three new kernels
    in place of the two they generalise.  ``steered``: the same with forced energy values in place of the energy control (that predictor
    is not run).

Every figure is milliseconds per forward = a host clock around ``--steps`` forwards that end in a device synchronise, after ``--warmup``
forwards of the same call.  The last line printed is the JSON that ``--out`` also writes.  Needs a GPU: there is no CPU path.
"""

from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def worker(tree: Path, steps: int, warmup: int, precision: str) -> dict:
    """One round in the tree ``tree``: ms per forward of the default call and, where the tree has it, of the steered one."""
    sys.path[:0] = [str(tree), str(tree / "tools")]
    import torch

    from everyvoice_amd import fs2
    from fs2_bench import synthetic_batch

    assert Path(fs2.__file__).resolve().parent.parent == tree.resolve(), f"imported {fs2.__file__}, not the package of {tree}"
    dev = torch.device("cuda:0")
    model = fs2.FastSpeech2(device=dev, precision=precision).init_random(1234)
    ids, lens, durs, t_i = synthetic_batch(32, 1234)
    ids, lens, durs = ids.to(dev), lens.to(dev), durs.to(dev)
    B, L = ids.shape

    def timed(call):
        for _ in range(warmup):
            call()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            call()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / steps * 1e3

    out = {"default_ms": timed(lambda: model(ids, lens, durations=durs)), "frames": int(t_i.sum()), "symbols": int(lens.sum())}
    if hasattr(fs2, "check_prosody_arguments"):
        g = torch.Generator().manual_seed(7)
        steer = dict(duration_control=(torch.rand(B, L, generator=g) + 0.5).to(dev), pitch_control=(torch.rand(B, L, generator=g) + 0.5).to(dev),
                     energy=torch.randn(B, L, generator=g).to(dev), target_frames=t_i.to(dev))
        # the same without anything forced: every predictor runs, as in the default forward -- what the three new kernels cost in place
        # of the two they generalise
        controls = dict(steer, energy_control=(torch.rand(B, L, generator=g) + 0.5).to(dev))
        del controls["energy"]
        for kw in (steer, controls):
            got = model(ids, lens, **kw)
            assert got[5].cpu().tolist() == t_i.tolist(), "the steered forward did not come out at the target lengths"
        out["controls_ms"] = timed(lambda: model(ids, lens, **controls))
        out["steered_ms"] = timed(lambda: model(ids, lens, **steer))
        out["default_again_ms"] = timed(lambda: model(ids, lens, durations=durs))  # (the default call on both sides of the steered one)
    return out


def spread(values: list) -> dict:
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4), "rounds": [round(v, 4) for v in values]}


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--parent", type=Path, default=None, help="a built checkout of the parent commit (its default forward is timed alternately with this tree's)")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--precision", default="bf16", choices=("bf16", "f32"))
    p.add_argument("--out", type=Path, default=None)
    p.add_argument("--worker", type=Path, default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker is not None:
        print(json.dumps(worker(args.worker, args.steps, args.warmup, args.precision)))
        return 0
    trees = {"this": ROOT}
    if args.parent is not None:
        trees["parent"] = args.parent.resolve()
    rounds = {name: [] for name in trees}
    for _ in range(args.rounds):
        for name, tree in trees.items():  # alternating: parent, this, parent, this, ...
            cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", str(tree), "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--precision", args.precision]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if done.returncode != 0:
                sys.stderr.write(done.stdout + done.stderr)
                return done.returncode or 1
            rounds[name].append(json.loads(done.stdout.strip().splitlines()[-1]))
    mine = rounds["this"]
    result = {"what": "FastSpeech2 inference forward, ms per forward (host clock around steps forwards ending in a synchronise)",
              "shape": {"B": 32, "symbols": mine[0]["symbols"], "frames": mine[0]["frames"], "precision": args.precision},
              "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
              "default_ms": spread([r["default_ms"] for r in mine]),
              "default_again_ms": spread([r["default_again_ms"] for r in mine]),
              "controls_ms": spread([r["controls_ms"] for r in mine]),
              "steered_ms": spread([r["steered_ms"] for r in mine])}
    result["controls_over_default"] = round(result["controls_ms"]["median"] / result["default_ms"]["median"], 4)
    result["steered_over_default"] = round(result["steered_ms"]["median"] / result["default_ms"]["median"], 4)
    if "parent" in rounds:
        result["parent_default_ms"] = spread([r["default_ms"] for r in rounds["parent"]])
        result["this_over_parent"] = round(result["default_ms"]["median"] / result["parent_default_ms"]["median"], 4)
    text = json.dumps(result)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(json.dumps(result, indent=1) + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
