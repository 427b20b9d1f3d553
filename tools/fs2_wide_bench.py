#!/usr/bin/env python3
"""FastSpeech2 at Conformer widths above 256 channels: what the LayerNorm backward costs per launch and what the packed
feed-forward chain is worth per training step.

  launches   evmi_layernorm_bwd_cbt_f32 at C 256 (the yardstick: the forms that existed), 384, 512 (<32, 16>) and 1024 (the form that
             reads dy twice), n_cols 4512 / 18112 (the benchmark batch's encoder and decoder), with and without accumulation into dx;
             every candidate once per round in ONE process, medians.  Bytes are the least traffic: x and dy read once, dx written
             once, one more read when accumulating -- not what a form that re-reads actually moves.
  step       one fresh child process per timing (EVMI_FS2_FFN_PACKED is read at import): the benchmark batch at precision="bf16",
             input_dim W with 2 heads and feedforward_dim 4 W, the switch 1 / 0 alternating (with EVMI_FS2_FFN_PACKED_WIDE beside it:
             above 256 channels the chain is not dispatched unless asked for).

usage: python tools/fs2_wide_bench.py [out.json] [rounds] [launches per timing] [step repeats]
       python tools/fs2_wide_bench.py --launches ROUNDS LAUNCHES | --step WIDTH STEPS      (the child processes)"""
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

WIDTHS_LAUNCH = (256, 384, 512, 1024)
N_COLS = (4512, 18112)
WIDTHS_STEP = (384, 512)


def launches(rounds, per_timing):
    import torch

    from everyvoice_amd import _lib

    dev = torch.device("cuda:0")
    lib = _lib.load()
    s = _lib.current_stream_ptr(dev)
    g = torch.Generator().manual_seed(0)
    jobs = []
    for n in N_COLS:
        for C in WIDTHS_LAUNCH:
            x, dy = (torch.randn(C, 1, n, generator=g) * 1.7 + 0.3).to(dev), torch.randn(C, 1, n, generator=g).to(dev)
            gamma, dx = (torch.rand(C, generator=g) + 0.5).to(dev), torch.zeros(C, 1, n, device=dev)
            n_ws = lib.evmi_layernorm_bwd_cbt_f32_ws_elems(C, n)
            ws = torch.empty(n_ws, device=dev)
            for acc in (0, 1):
                run = lambda x=x, dy=dy, gamma=gamma, dx=dx, ws=ws, n_ws=n_ws, C=C, n=n, acc=acc: _lib.check(  # noqa: E731
                    lib.evmi_layernorm_bwd_cbt_f32(x.data_ptr(), gamma.data_ptr(), dy.data_ptr(), dx.data_ptr(), None, None,
                                                   ws.data_ptr(), n_ws, C, n, 1e-5, acc, s), "layernorm_bwd")
                jobs.append(((C, n, acc), run))
    for _, run in jobs:
        run()
        run()
    torch.cuda.synchronize()
    times = {key: [] for key, _ in jobs}
    for _ in range(rounds):
        for key, run in jobs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(per_timing):
                run()
            t1.record()
            t1.synchronize()
            times[key].append(t0.elapsed_time(t1) * 1e3 / per_timing)  # us per call (the partial sums stay in ws, as in a training step: the dx kernel alone)
    rows = []
    for (C, n, acc), v in times.items():
        us = statistics.median(v)
        gbs = C * n * 4 * (3 + acc) / us * 1e-3
        rows.append({"C": C, "n_cols": n, "accumulate": acc, "us_median": round(us, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                     "min_traffic_GBps": round(gbs, 1)})
    base = {(r["n_cols"], r["accumulate"]): r["min_traffic_GBps"] for r in rows if r["C"] == 256}
    for r in rows:
        r["rate_over_C256"] = round(r["min_traffic_GBps"] / base[(r["n_cols"], r["accumulate"])], 3)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": rounds, "launches_per_timing": per_timing, "rows": rows}))


def step(width, steps):
    import torch

    from everyvoice_amd.fs2 import FastSpeech2ModelConfig
    from everyvoice_amd.train import ops
    from everyvoice_amd.train.fs2 import FastSpeech2Trainer
    from fs2_train_bench import training_batch

    dev = torch.device("cuda:0")
    c = FastSpeech2ModelConfig()
    for part in (c.encoder, c.decoder):
        part.input_dim, part.heads, part.feedforward_dim = width, 2, 4 * width
    for v in (c.variance_predictors.duration, c.variance_predictors.pitch, c.variance_predictors.energy):
        v.input_dim = width
    tr = FastSpeech2Trainer(c, device=dev, precision="bf16", use_graph=True)
    batch, _ = training_batch(32, device=dev)
    tr.batch_ready = True
    for _ in range(4):  # two eager steps, the capture, one replay
        losses = tr.training_step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        losses = tr.training_step(batch)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    print(json.dumps({"width": width, "ffn_packed": bool(ops.FFN_PACKED[0]), "ms_per_step": round(ms, 3), "graph": bool(tr.last_step_was_graph),
                      "total_loss": round(float(losses["total"]), 5)}))


def _child(args, env=None, limit=300):
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), *map(str, args)], capture_output=True, text=True, timeout=limit,
                       env=dict(os.environ, **(env or {})))
    if r.returncode != 0:  # (nothing more is started on the device behind a child that failed)
        raise SystemExit(f"child {args} ended with {r.returncode}:\n{r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--launches":
        return launches(int(sys.argv[2]), int(sys.argv[3]))
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        return step(int(sys.argv[2]), int(sys.argv[3]))
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    per_timing = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    result = {"layernorm_bwd": _child(["--launches", rounds, per_timing]), "training_step": []}
    for width in WIDTHS_STEP:
        runs = {"1": [], "0": []}
        for _ in range(repeats):
            for switch in ("1", "0"):
                runs[switch].append(_child(["--step", width, 20], env={"EVMI_FS2_FFN_PACKED": switch, "EVMI_FS2_FFN_PACKED_WIDE": switch}))
        result["training_step"].append({
            "width": width, "heads": 2, "feedforward_dim": 4 * width, "batch": 32, "precision": "bf16", "steps_per_timing": 20,
            "ms_per_step_ffn_packed": [r["ms_per_step"] for r in runs["1"]], "ms_per_step_separate": [r["ms_per_step"] for r in runs["0"]],
            "median_ffn_packed": statistics.median(r["ms_per_step"] for r in runs["1"]),
            "median_separate": statistics.median(r["ms_per_step"] for r in runs["0"]),
            "graph": all(r["graph"] for r in runs["1"] + runs["0"]),
            "total_loss_ffn_packed": runs["1"][0]["total_loss"], "total_loss_separate": runs["0"][0]["total_loss"]})
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(text + "\n")


if __name__ == "__main__":
    main()
