#!/usr/bin/env python3
"""model.mask_padding: what it costs.  One JSON line with
  * the FastSpeech2 inference forward and the training step (default model, bf16 operands, 32 items, durations given / learned
    alignment, the step captured into a HIP graph) with the flag off and on: one process, the variants alternating inside every
    round, device events around each variant's calls, median over the rounds;
  * the `postnet_layers - 1` column-mask launches of the inference postnet alone;
  * the depthwise convolution with lengths and its backward against the kernels they stand beside, at the Conformer's shape
    (C = 256, k = 9) on the frame axis of the same batch, with the batch's lengths and with every length = T.
The batch is ragged on purpose: text lengths uniform over [L / 4, L] (seeded), 3 to 8 frames per symbol.
usage: fs2_padding_bench.py [rounds = 9] [calls per round = 10] [L = 187] [precision = bf16] [only = "" | "kernels" | "kernels:batch" | "kernels:full"]
only = kernels: the last block alone (":batch" / ":full": the kernels with lengths on the batch's lengths / on full lengths only, so that
a profiler's per-name averages are of one case) -- the run to put under `rocprofv3 --kernel-trace --stats`, whose per-kernel durations are the kernel
times (the event timings of this block include the launch path of the Python wrappers: at 33 MB per tensor a launch is about as long
as the kernel)."""
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

B = 32


def ragged_batch(L, seed=1234, n_mels=80):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(L // 4, L + 1, (B,), generator=g)
    lens[0] = L
    pad = torch.arange(L)[None] >= lens[:, None]
    ids = torch.randint(2, 80, (B, L), generator=g).masked_fill(pad, 0)
    durs = torch.randint(3, 9, (B, L), generator=g).masked_fill(pad, 0)
    T_i = durs.sum(1)
    T = int(T_i.max())
    mel = torch.randn(B, T, n_mels, generator=g).masked_fill((torch.arange(T)[None] >= T_i[:, None])[..., None], 0.0)
    return ids, lens, durs, T_i, mel, g


def training_batch(ids, lens, T_i, mel, g, dev):
    """The learned-alignment batch of tools/fs2_train_bench.py on these lengths, resident on the device."""
    from everyvoice_amd.heavy import BetaBinomialInterpolator

    interp = BetaBinomialInterpolator(device=dev)
    T, L = mel.shape[1], ids.shape[1]
    prior = torch.zeros(B, T, L, dtype=torch.float64)
    for b in range(B):
        prior[b, : T_i[b], : lens[b]] = interp(int(T_i[b]), int(lens[b])).cpu()
    batch = dict(ids=ids, lens=lens, mel=mel, mel_lens=T_i, attn_prior=prior, pitch_frames=torch.randn(B, T, generator=g),
                 energy_frames=torch.randn(B, T, generator=g))
    return {k: (v if k in ("lens", "mel_lens") else v.to(dev)) for k, v in batch.items()}


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def alternate(variants: dict, rounds: int, n: int) -> dict:
    """name -> callable; every round times each variant in turn -> {name: {"median_ms", "rounds_ms"}}"""
    for fn in variants.values():  # every shape warm
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            ms[name].append(event_ms(fn, n))
    return {name: {"median_ms": round(statistics.median(v), 4), "rounds_ms": [round(x, 4) for x in v]} for name, v in ms.items()}


def main():
    from everyvoice_amd import _lib

    rounds = max(9, int(sys.argv[1])) if len(sys.argv) > 1 else 9
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    L = int(sys.argv[3]) if len(sys.argv) > 3 else 187
    precision = sys.argv[4] if len(sys.argv) > 4 else "bf16"
    only = sys.argv[5] if len(sys.argv) > 5 else ""
    dev = torch.device("cuda:0")
    _lib.load()
    ids, lens, durs, T_i, mel, g = ragged_batch(L)
    T = int(T_i.max())
    out = {"precision": precision, "batch": B, "max_tokens": L, "max_frames": T, "tokens": int(lens.sum()), "frames": int(T_i.sum()),
           "valid_share_of_padded_frames": round(float(T_i.sum()) / (B * T), 3), "rounds": rounds, "calls_per_round": n}

    mel_lens32 = T_i.to(dev, torch.int32)
    if not only.startswith("kernels"):
        model_timings(out, ids, lens, durs, T_i, mel, g, dev, precision, rounds, n)
    kernel_timings(out, mel_lens32, T, dev, rounds, n, only.partition(":")[2])
    print(json.dumps(out))


def model_timings(out, ids, lens, durs, T_i, mel, g, dev, precision, rounds, n):
    from everyvoice_amd.fs2 import FastSpeech2, FastSpeech2ModelConfig, _mask_cols_
    from everyvoice_amd.train.fs2 import FastSpeech2Trainer

    T = int(T_i.max())
    # -- inference forward
    models = {}
    for name, flag in (("off", False), ("on", True)):
        models[name] = FastSpeech2(FastSpeech2ModelConfig(mask_padding=flag), device=dev, precision=precision).init_random(1234)
    d_ids, d_lens, d_durs = ids.to(dev), lens.to(dev), durs.to(dev)
    res = alternate({name: (lambda m=m: m(d_ids, d_lens, durations=d_durs)) for name, m in models.items()}, rounds, n)
    out["infer_ms_per_batch"] = res
    out["infer_on_over_off"] = round(res["on"]["median_ms"] / res["off"]["median_ms"], 4)
    c = models["on"].config
    h = torch.randn(c.postnet_channels, B, T, device=dev)
    mel_lens32 = T_i.to(dev, torch.int32)
    res = alternate({"postnet_masks": lambda: [_mask_cols_(h, mel_lens32) for _ in range(c.postnet_layers - 1)]}, rounds, n)
    out["postnet_mask_launches"] = {"launches": c.postnet_layers - 1, "shape": [c.postnet_channels, B, T], **res["postnet_masks"]}
    del models

    # -- training step (captured)
    batch = training_batch(ids, lens, T_i, mel, g, dev)
    trainers = {}
    for name, flag in (("off", False), ("on", True)):
        tr = FastSpeech2Trainer(FastSpeech2ModelConfig(learn_alignment=True, mask_padding=flag), device=dev, precision=precision, use_graph=True)
        tr.batch_ready = True
        for _ in range(4):  # two eager steps, the capture, one replay
            tr.training_step(batch)
        trainers[name] = tr
    res = alternate({name: (lambda t=t: t.training_step(batch)) for name, t in trainers.items()}, rounds, n)
    out["train_ms_per_step"] = res
    out["train_on_over_off"] = round(res["on"]["median_ms"] / res["off"]["median_ms"], 4)
    out["train_graph"] = {name: bool(t.last_step_was_graph) for name, t in trainers.items()}


def kernel_timings(out, mel_lens32, T, dev, rounds, n, case=""):
    """The kernels alone: C = 256, k = 9 on [C, B, T]."""
    from everyvoice_amd.fs2 import _dwconv
    from everyvoice_amd.train import ops

    C, k = 256, 9
    x, dy = torch.randn(C, B, T, device=dev), torch.randn(C, B, T, device=dev)
    w, bias = torch.randn(C, k, device=dev), torch.randn(C, device=dev)
    full = torch.full((B,), T, dtype=torch.int32, device=dev)
    dw, db = torch.zeros(C, 1, k, device=dev), torch.zeros(C, device=dev)
    w3 = w.view(C, 1, k)
    kernels = {
        "fwd_existing": lambda: _dwconv(x, w, bias, k, 1),
        "fwd_lens_batch_lengths": lambda: _dwconv(x, w, bias, k, 1, mel_lens32),
        "fwd_lens_all_full": lambda: _dwconv(x, w, bias, k, 1, full),
        "bwd_existing": lambda: ops.dwconv_bwd(x, w3, dy, dw, db, k),
        "bwd_lens_batch_lengths": lambda: ops.dwconv_bwd(x, w3, dy, dw, db, k, lens=mel_lens32),
        "bwd_lens_all_full": lambda: ops.dwconv_bwd(x, w3, dy, dw, db, k, lens=full),
    }
    kernels = {name: fn for name, fn in kernels.items() if not case or "lens" not in name or {"batch": "batch_lengths", "full": "all_full"}[case] in name}
    out["dwconv_kernels_ms"] = {"shape": [C, B, T], "k": k, "tensor_bytes": 4 * C * B * T, **alternate(kernels, rounds, 4 * n)}


if __name__ == "__main__":
    main()
