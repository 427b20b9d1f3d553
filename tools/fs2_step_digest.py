#!/usr/bin/env python3
"""SHA-256 digests of what a few FastSpeech2 training steps leave behind, for a host-side refactor of the step that claims "same bits":
run it at both commits and compare.

    python tools/fs2_step_digest.py --all --out head.json [--root <another checkout>]   # every configuration, each in a fresh child process
    python tools/fs2_step_digest.py --config learn1_bf16_graph1                          # one configuration, in this process -> one JSON line
    python tools/fs2_step_digest.py --compare parent.json head.json                      # exit status 1 if any digest differs

A configuration builds a trainer from a fixed seed and runs STEPS steps on one fixed small batch (B = 4, L = 24, T ~ 96; dropout on) and
digests: ``params.flat`` / ``m`` / ``v``, the state dict, every step's losses, ``evaluate()``'s losses and ``activation_elements()`` of one
training step and of one evaluation.  ``--all`` stops at the first child that fails (non-zero exit, or its time limit) and starts nothing
after it.  ``--root``: the checkout whose ``everyvoice_amd`` is imported (default: this file's)."""

import argparse
import hashlib
import json
import subprocess
import sys
from pathlib import Path

STEPS, B, L = 5, 4, 24
CHILD_SECONDS = 240

# name -> (model settings, trainer settings); levels = (pitch, energy)
CONFIGS = {f"learn{learn}_{prec}_graph{graph}": (dict(learn=bool(learn)), dict(precision=prec, use_graph=bool(graph)))
           for learn in (0, 1) for prec in ("f32", "bf16") for graph in (0, 1)}
_BF16_GRAPH = dict(precision="bf16", use_graph=True)
CONFIGS.update({
    "frame_frame": (dict(learn=True, levels=("frame", "frame")), _BF16_GRAPH),
    "phone_frame": (dict(learn=True, levels=("phone", "frame")), _BF16_GRAPH),
    "speakers_languages_style": (dict(learn=True, speakers=3, languages=2, style=True), _BF16_GRAPH),
    "mae": (dict(learn=True, mae=True), _BF16_GRAPH),
    "phonological_features": (dict(learn=True, pfs=True), _BF16_GRAPH),
    "data_parallel_world_of_one": (dict(learn=True), dict(_BF16_GRAPH, process_group=True)),
})


def _sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def _loss_digest(losses: dict) -> str:
    return _sha(*[losses[k].reshape(1).float() for k in sorted(losses)]) + ":" + ",".join(sorted(losses))


def model_config(learn, levels=("phone", "phone"), speakers=0, languages=0, style=False, mae=False, pfs=False):
    from everyvoice_amd.fs2 import FastSpeech2ModelConfig

    c = FastSpeech2ModelConfig(learn_alignment=learn)
    c.variance_predictors.pitch.level, c.variance_predictors.energy.level = levels
    if mae:
        c.mel_loss = "mae"
        for name in ("duration", "pitch", "energy"):
            getattr(c.variance_predictors, name).loss = "mae"
    if speakers:
        c.multispeaker, c.n_speakers = True, speakers
    if languages:
        c.multilingual, c.n_languages = True, languages
    c.use_global_style_token_module = style
    if pfs:
        c.target_text_representation_level = "phonological_features"
    return c


def make_batch(c, dev, seed=7):
    """One batch with everything any configuration reads: durations and phone-level targets only where the aligner does not give them."""
    import torch

    from everyvoice_amd.fs2 import N_PHONOLOGICAL_FEATURES

    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(L // 2, L + 1, (B,), generator=g)
    lens[0], lens[-1] = L, L // 2
    pad = torch.arange(L)[None] >= lens[:, None]
    durs = torch.randint(1, 8, (B, L), generator=g).masked_fill(pad, 0)
    mel_lens = durs.sum(1)
    T = int(mel_lens.max())
    fpad = torch.arange(T)[None] >= mel_lens[:, None]
    batch = dict(lens=lens, mel=torch.randn(B, T, c.n_mels, generator=g).masked_fill(fpad[..., None], 0.0),
                 pitch_frames=torch.randn(B, T, generator=g).masked_fill(fpad, 0.0), energy_frames=torch.randn(B, T, generator=g).masked_fill(fpad, 0.0))
    if c.target_text_representation_level == "phonological_features":
        batch["pfs"] = torch.randint(0, 2, (B, L, N_PHONOLOGICAL_FEATURES), generator=g).float().masked_fill(pad[..., None], 0.0)
    else:
        batch["ids"] = torch.randint(1, c.n_symbols, (B, L), generator=g).masked_fill(pad, 0)
    if c.learn_alignment:
        from everyvoice_amd.heavy import BetaBinomialInterpolator

        interp = BetaBinomialInterpolator(device=dev)
        prior = torch.zeros(B, T, L, dtype=torch.float64)
        for b in range(B):
            prior[b, : mel_lens[b], : lens[b]] = interp(int(mel_lens[b]), int(lens[b])).cpu()
        batch.update(mel_lens=mel_lens, attn_prior=prior)
    else:
        batch["durations"] = durs
        for key in ("pitch", "energy"):
            if getattr(c.variance_predictors, key).level == "phone":
                batch[key] = torch.randn(B, L, generator=g).masked_fill(pad, 0.0)
    if c.multispeaker:
        batch["speakers"] = torch.randint(0, c.n_speakers, (B,), generator=g)
    if c.multilingual:
        batch["languages"] = torch.randint(0, c.n_languages, (B,), generator=g)
    return {k: (v if k in ("lens", "mel_lens") else v.to(dev)) for k, v in batch.items()}


def run_config(name: str) -> dict:
    import torch

    from everyvoice_amd.train import ops
    from everyvoice_amd.train.autograd import activation_elements
    from everyvoice_amd.train.fs2 import FastSpeech2Trainer

    model, trainer = CONFIGS[name]
    dev = torch.device("cuda:0")
    dist = None
    if trainer.get("process_group"):
        import os
        import socket

        import torch.distributed as dist

        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        c = model_config(**model)
        tr = FastSpeech2Trainer(c, device=dev, seed=11, **trainer)
        tr.current_epoch = 50  # (half way up the binarisation loss's warm-up: the term is on)
        batch = make_batch(c, dev)
        out = {"losses": [], "was_graph": []}
        for _ in range(STEPS):
            out["losses"].append(_loss_digest(tr.training_step(batch)))
            out["was_graph"].append(bool(tr.last_step_was_graph))
        torch.cuda.synchronize(dev)
        if tr._graph_failed is not None:
            raise RuntimeError(f"capture failed: {tr._graph_failed}")
        sd = tr.state_dict()
        out.update(params=_sha(tr.params.flat), m=_sha(tr.params.m), v=_sha(tr.params.v), state_dict=_sha(*[sd[k] for k in sorted(sd)]),
                   branch_on_stream=bool(tr.last_step_branch_on_stream), stretches=[len(e["graphs"]) for e in tr._graphs.values()])
        activation_elements(reset=True)
        out["evaluate"] = _loss_digest(tr.evaluate(batch))
        out["activation_elements_evaluate"] = activation_elements(reset=True)
        with ops.mode(operands=tr.precision):
            tr.forward_backward(batch)
        out["activation_elements_step"] = activation_elements(reset=True)
        torch.cuda.synchronize(dev)
    finally:
        if dist is not None:
            dist.destroy_process_group()
    return out


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
        print(f"{name}: {table[name]['params']} graph steps {sum(table[name]['was_graph'])}", flush=True)
        out_path.parent.mkdir(parents=True, exist_ok=True)
        out_path.write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
    return 0


def compare(a: dict, b: dict) -> list:
    bad = [f"configurations differ: {sorted(set(a) ^ set(b))}"] if set(a) != set(b) else []
    for name in sorted(set(a) & set(b)):
        bad += [f"{name}.{k}: {a[name].get(k)} != {b[name].get(k)}" for k in sorted(set(a[name]) | set(b[name])) if a[name].get(k) != b[name].get(k)]
    return bad


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", type=Path, default=Path(__file__).resolve().parent.parent)
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--only", nargs="*", help="with --all: these configurations only")
    ap.add_argument("--out", type=Path, default=Path("fs2_step_digest.json"))
    ap.add_argument("--compare", nargs=2, type=Path)
    args = ap.parse_args()
    if args.compare:
        a, b = (json.loads(p.read_text()) for p in args.compare)
        bad = compare(a, b)
        print(f"{len(a)} configurations: " + ("every digest equal" if not bad else f"{len(bad)} differences"))
        for line in bad:
            print("  " + line)
        return 1 if bad else 0
    sys.path.insert(0, str(args.root.resolve()))
    if args.all:
        return run_all(args.root.resolve(), args.out, args.only or list(CONFIGS))
    print(json.dumps(run_config(args.config), sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
