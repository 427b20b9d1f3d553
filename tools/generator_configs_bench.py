#!/usr/bin/env python3
"""Generator forward of configurations outside HiFi-GAN V1 (V2, V3, and one whose every shape misses the specialised kernel tables)
at B = 32, T = 768: bf16 (generic-shape MFMA convolution where the tables hold nothing) against precision="f32" (the exact fp32
path), device events, both precisions alternating in one process after a warm-up of every shape.  Prints one JSON line:
per configuration samples/s (median, min, max over the repetitions) per precision, the bf16 / f32 ratio, and the share of the bf16
forward spent in the generic kernel.  `--v1` adds V1 (with EVMI_CONV_GENERIC=1 in the environment: the generic kernel at the shapes
the specialised kernels cover); `--configs a,b` runs those configurations only.  The iSTFTNet configurations also report the share of
the bf16 forward spent in the head.  Usage: python tools/generator_configs_bench.py [--reps 7] [--v1] [--configs NAMES] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from everyvoice_amd.config import HiFiGANConfig  # noqa: E402
from everyvoice_amd.vocoder import HiFiGANGenerator  # noqa: E402

V3 = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=256,
          resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]])
ODD1 = dict(n_mels=100, upsample_initial_channel=192, upsample_rates=[5, 4, 3], upsample_kernel_sizes=[11, 8, 7],
            resblock_kernel_sizes=[5, 9], resblock_dilation_sizes=[[1, 2, 4], [1, 7]])
# iSTFTNet heads other than 16 / 4 on 32 / 64 / 128 channels (the generic head, csrc/istft_head_generic.hip): every one hop 256
C8C8C2I_8_2 = dict(istft_layer=True, upsample_rates=[8, 8, 2], upsample_kernel_sizes=[16, 16, 4], upsample_initial_channel=128,
                   gen_istft_n_fft=8, gen_istft_hop_size=2)
C8I_128_32 = dict(istft_layer=True, upsample_rates=[8], upsample_kernel_sizes=[16], upsample_initial_channel=48,
                  gen_istft_n_fft=128, gen_istft_hop_size=32)
C8C2I_64_16 = dict(istft_layer=True, upsample_rates=[8, 2], upsample_kernel_sizes=[16, 4], upsample_initial_channel=256,
                   gen_istft_n_fft=64, gen_istft_hop_size=16)
CONFIGS = {"v2": dict(upsample_initial_channel=128), "v3": V3, "odd1": ODD1, "c8c8c2i_8_2": C8C8C2I_8_2, "c8i_128_32": C8I_128_32,
           "c8c2i_64_16": C8C2I_64_16}
HBM_BYTES_PER_S = 8.0e12  # MI355X peak
TOP_LEVEL = ("n_mels", "gen_istft_n_fft", "gen_istft_hop_size")  # keys of a spec that are not fields of `model`


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=768)
    ap.add_argument("--v1", action="store_true")
    ap.add_argument("--configs", help="comma-separated names out of " + ", ".join(CONFIGS))
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    configs = dict(CONFIGS if not a.configs else {n: CONFIGS[n] for n in a.configs.split(",")}, **({"v1": {}} if a.v1 else {}))
    jobs = {}
    for name, spec in configs.items():
        n_mels = spec.get("n_mels", 80)
        cfg = HiFiGANConfig(model={k: v for k, v in spec.items() if k not in TOP_LEVEL}, preprocessing=dict(audio=dict(n_mels=n_mels)),
                            **{k: v for k, v in spec.items() if k.startswith("gen_istft")})
        torch.manual_seed(1234)
        bf16 = HiFiGANGenerator(cfg, precision="bf16")
        f32 = HiFiGANGenerator(cfg, precision="f32")
        f32.load_state_dict(bf16.state_dict())
        g = torch.Generator().manual_seed(7)
        mel = (torch.randn(a.batch, n_mels, a.frames, generator=g) * 2.0 - 5.0).clamp(-11.5129, 2.0).to(dev)
        jobs[name] = (bf16.to(dev).eval(), f32.to(dev).eval(), mel)
    for bf16, f32, mel in jobs.values():  # warm-up of every shape in both precisions
        for _ in range(2):
            bf16(mel)
            f32(mel)
    torch.cuda.synchronize()
    result = {"batch": a.batch, "frames": a.frames, "reps": a.reps, "EVMI_CONV_GENERIC": os.environ.get("EVMI_CONV_GENERIC", ""), "configs": {}}
    for name, (bf16, f32, mel) in jobs.items():
        samples = a.batch * a.frames * bf16.generator.hop
        ms = {"bf16": [], "f32": []}
        for _ in range(a.reps):
            for prec, model in (("bf16", bf16), ("f32", f32)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                model(mel)
                e1.record()
                e1.synchronize()
                ms[prec].append(e0.elapsed_time(e1))
        _, records = bf16.generator.forward_profiled(mel)
        total = sum(r["ms"] for r in records)
        generic = sum(r["ms"] for r in records if r["kernel"].startswith("conv_tc_generic"))
        entry = {}
        for prec, v in ms.items():
            entry[prec] = {"samples_per_s_median": samples / (statistics.median(v) * 1e-3), "samples_per_s_min": samples / (max(v) * 1e-3),
                           "samples_per_s_max": samples / (min(v) * 1e-3), "ms_median": statistics.median(v)}
        entry["bf16_over_f32"] = statistics.median(ms["f32"]) / statistics.median(ms["bf16"])
        entry["generic_kernel_share_of_bf16_ms"] = generic / total if total else 0.0
        entry["generic_launches"] = sum(1 for r in records if r["kernel"].startswith("conv_tc_generic"))
        entry["launches"] = len(records)
        head = [r for r in records if r["layer"] == "conv_post+istft"]
        if head:
            entry["istft_head_kernel"] = head[0]["kernel"]
            entry["istft_head_ms"] = head[0]["ms"]
            entry["istft_head_share_of_bf16_ms"] = head[0]["ms"] / total if total else 0.0
            entry["istft_head_share_of_hbm_bound"] = head[0]["bytes"] / HBM_BYTES_PER_S / (head[0]["ms"] * 1e-3)
        result["configs"][name] = entry
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
