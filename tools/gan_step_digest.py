#!/usr/bin/env python3
"""SHA-256 digests of what a few HiFiGAN GAN training steps do and leave behind, for a host-side refactor of the step that claims "same
library calls, same bits": run it at both commits and compare.

    python tools/gan_step_digest.py --all --out head.json [--root <another checkout>]           # bits, on a GPU: each configuration in a fresh child
    python tools/gan_step_digest.py --calls --all --out head_calls.json [--root <checkout>]    # library call sequences, on the CPU, in this process
    python tools/gan_step_digest.py [--calls] --config bf16_graph                               # one configuration, in this process -> one JSON line
    python tools/gan_step_digest.py --compare parent.json head.json                            # exit status 1 if any digest differs

Bits: a configuration builds a trainer from a fixed seed, runs STEPS steps on one fixed batch (B = 2, S = 2048: the smallest shape the GAN
tests use) and digests ``g_params.flat``, ``d_params.flat``, both optimisers' ``m`` / ``v`` and every step's loss vector.  ``--all`` stops at
the first child that fails (non-zero exit, or its time limit) and starts nothing after it.

Calls (``--calls``): two steps on ``device="cpu"`` under the recorder of ``tools/ops_call_trace.py`` (no library, no GPU): the digest of the
whole call list, with pointers into the two flat parameter / gradient buffers named.  The packed discriminator chains and the time-major
generator stages need a GPU tensor, so this mode sees the two-call routing of the generator step only.  Under ``process_group`` two
recording reducers write ``launch(lo, hi)`` / ``finish()`` into the same list.  ``--root``: the checkout whose ``everyvoice_amd`` is imported
(default: this file's)."""

import argparse
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

STEPS, B, S = 3, 2, 2048
CHILD_SECONDS = 240

# bits: name -> (trainer settings, extras: env = environment of the child, istft = an iSTFT generator, dist = a one-rank "nccl" world)
CONFIGS = {f"{prec}_{'graph' if graph else 'eager'}": (dict(precision=prec, use_graph=graph), {}) for prec in ("f32", "bf16") for graph in (False, True)}
CONFIGS.update({
    "bf16_one_stream": (dict(precision="bf16", parallel_streams=False), {}),
    "bf16_graph_warmup1": (dict(precision="bf16", use_graph=True, generator_warmup_steps=1), {}),
    "bf16_two_call": (dict(precision="bf16"), dict(env={"EVMI_DISC_CHAIN": "0"})),
    "wgan_rms": (dict(precision="bf16", use_graph=True, gan_type="wgan", optimizer="rms"), {}),
    "mel_mrstft": (dict(precision="bf16", use_graph=True, reconstruction_loss="mel+mrstft"), {}),
    "istft": (dict(precision="bf16", use_graph=True), dict(istft=True)),
    "data_parallel_world_of_one_eager": (dict(precision="bf16", process_group=True), dict(dist=True)),
    "data_parallel_world_of_one_graph": (dict(precision="bf16", process_group=True, use_graph=True), dict(dist=True)),
})

# calls: name -> trainer settings (two steps each)
CALL_CONFIGS = {
    "f32": dict(precision="f32"),
    "bf16": dict(precision="bf16"),
    "f32_warmup1": dict(precision="f32", generator_warmup_steps=1),
    "bf16_warmup1": dict(precision="bf16", generator_warmup_steps=1),
    "wgan_rms": dict(precision="f32", gan_type="wgan", optimizer="rms"),
    "mel_mrstft": dict(precision="f32", reconstruction_loss="mel+mrstft"),
    "one_stream": dict(precision="f32", parallel_streams=False),
    "data_parallel": dict(precision="bf16", process_group=True),
    "data_parallel_warmup1": dict(precision="bf16", process_group=True, generator_warmup_steps=1),
}


def _sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def _batch(device):
    import torch

    g = torch.Generator().manual_seed(8)
    y = (0.3 * torch.tanh(torch.randn(B, 1, S, generator=g))).to(device)
    return torch.randn(B, 80, S // 256, generator=g).to(device), y


def _model_config(istft=False):
    from everyvoice_amd.config import HiFiGANConfig

    return HiFiGANConfig(model=dict(istft_layer=True, upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16])) if istft else HiFiGANConfig()


def run_config(name: str) -> dict:
    settings, extra = CONFIGS[name]
    os.environ.update(extra.get("env", {}))  # (read when train/hifigan.py is imported: this is a fresh process)
    import torch

    from everyvoice_amd.train.hifigan import HiFiGANTrainer

    dev = torch.device("cuda:0")
    dist = None
    if extra.get("dist"):
        import socket

        import torch.distributed as dist

        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        tr = HiFiGANTrainer(_model_config(extra.get("istft", False)), device=dev, seed=5, **settings)
        mel, y = _batch(dev)
        out = {"losses": [_sha(tr.training_step(mel, y, sync=False)) for _ in range(STEPS)]}
        torch.cuda.synchronize(dev)
        if tr._graph_failed is not None:
            raise RuntimeError(f"capture failed: {tr._graph_failed}")
        out.update(g_params=_sha(tr.g_params.flat), d_params=_sha(tr.d_params.flat), g_m=_sha(tr.g_params.m), g_v=_sha(tr.g_params.v),
                   d_m=_sha(tr.d_params.m), d_v=_sha(tr.d_params.v), stretches=[len(e["graphs"]) for e in tr._graphs.values()])
    finally:
        if dist is not None:
            dist.destroy_process_group()
    return out


class _RecordingReducer:
    """Stands in for a BucketReducer: its collectives go into the recorder's call list, between the library calls around them."""

    def __init__(self, name, rec):
        self.name, self.rec = name, rec

    def launch(self, lo, hi):
        self.rec.calls.append([self.name + ".launch", [lo, hi]])

    def finish(self):
        self.rec.calls.append([self.name + ".finish", []])


def trace_config(name, steps: int = 2) -> list:
    """The library calls (and, data parallel, the collectives) of `steps` steps on the CPU, one list per step.  ``name``: a key of
    CALL_CONFIGS, or trainer settings."""
    import everyvoice_amd  # noqa: F401  (from --root, before tools/ops_call_trace.py puts its own checkout in front)

    sys.path.insert(0, str(Path(__file__).resolve().parent))
    import ops_call_trace as oct

    from everyvoice_amd.train.hifigan import HiFiGANTrainer

    mel, y = _batch("cpu")
    out = []
    with oct.recording():
        oct.REC.begin([], {})
        tr = HiFiGANTrainer(device="cpu", seed=5, **(CALL_CONFIGS[name] if isinstance(name, str) else name))
        named = {"g_params.flat": tr.g_params.flat, "g_params.grad": tr.g_params.grad, "d_params.flat": tr.d_params.flat, "d_params.grad": tr.d_params.grad}
        if tr.pg is not None:
            tr._dp_reducers = (_RecordingReducer("d", oct.REC), _RecordingReducer("g", oct.REC))
        for _ in range(steps):
            oct.REC.begin([], named)
            tr.training_step(mel, y, sync=False)
            out.append(oct.REC.calls)
    return out


def calls_config(name: str) -> dict:
    steps = trace_config(name)
    return {"calls": hashlib.sha256(json.dumps(steps, sort_keys=True).encode()).hexdigest()[:16], "n_calls": [len(s) for s in steps]}


def run_all(root: Path, out_path: Path, names) -> int:
    table = {}
    for name in names:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--config", name, "--root", str(root)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_SECONDS)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {CHILD_SECONDS} s -- stopping here", flush=True)
            return 124
        if p.returncode != 0:
            print(f"{name}: exit status {p.returncode} -- stopping here\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            return p.returncode
        table[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(f"{name}: g {table[name]['g_params']} d {table[name]['d_params']} stretches {table[name]['stretches']}", flush=True)
        out_path.parent.mkdir(parents=True, exist_ok=True)
        out_path.write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
    return 0


def compare(a: dict, b: dict) -> list:
    """One line per configuration: "identical", or the keys whose digests differ."""
    lines = [(f"configurations differ: {sorted(set(a) ^ set(b))}", False)] if set(a) != set(b) else []
    for name in sorted(set(a) & set(b)):
        bad = [f"{k}: {a[name].get(k)} != {b[name].get(k)}" for k in sorted(set(a[name]) | set(b[name])) if a[name].get(k) != b[name].get(k)]
        lines.append((f"{name}: " + ("identical" if not bad else "; ".join(bad)), not bad))
    return lines


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", type=Path, default=Path(__file__).resolve().parent.parent)
    ap.add_argument("--calls", action="store_true", help="library call sequences on the CPU instead of bits on the GPU")
    ap.add_argument("--config", choices=sorted({*CONFIGS, *CALL_CONFIGS}))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--only", nargs="*", help="with --all: these configurations only")
    ap.add_argument("--out", type=Path, default=Path("gan_step_digest.json"))
    ap.add_argument("--compare", nargs=2, type=Path)
    args = ap.parse_args()
    if args.compare:
        lines = compare(*(json.loads(p.read_text()) for p in args.compare))
        for line, _ in lines:
            print(line)
        return 0 if lines and all(ok for _, ok in lines) else 1
    sys.path.insert(0, str(args.root.resolve()))
    if args.calls:
        table = {name: calls_config(name) for name in (args.only or list(CALL_CONFIGS) if args.all else [args.config])}
        if args.all:
            args.out.parent.mkdir(parents=True, exist_ok=True)
            args.out.write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
        for name, rec in table.items():
            print(f"{name}: {json.dumps(rec, sort_keys=True)}", flush=True)
        return 0
    if args.all:
        return run_all(args.root.resolve(), args.out, args.only or list(CONFIGS))
    print(json.dumps(run_config(args.config), sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
