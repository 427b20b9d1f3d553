#!/usr/bin/env python3
"""The iSTFT output head alone through evmi_istft_head_bf16: variant 0 (the kernel the generator picks: the specialised one at
n_fft 16 / hop 4 on 32 / 64 / 128 channels) against variant 1 (the generic one, csrc/istft_head_generic.hip), alternating in one
process after a warm-up, device events around `--launches` launches each, `--rounds` rounds.  The weight relayout the entry point
performs per call (a few hundred KB at most) is inside the timed window of both variants.  Prints one JSON line: per case ms per
launch (median, min, max over the rounds) per variant, the HBM bound bytes / 8 TB/s with bytes = B L C 2 + B hop L 4, and each
variant's share of it.  Cases (C, n_fft, hop, L) at B = 32: the bench shape of C8C8I, the 8 / 2 head of C8C8C2I at V2 width, the
128 / 32 head of C8I on 24 channels.  Usage: python tools/istft_head_bench.py [--launches 200] [--rounds 5] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from everyvoice_amd import _lib  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak
CASES = {"c8c8i_16_4_c128": (128, 16, 4, 64 * 768), "c8c8c2i_8_2_c16": (16, 8, 2, 128 * 768), "c8i_128_32_c24": (24, 128, 32, 8 * 768)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = _lib.current_stream_ptr(dev)
    result = {"batch": a.batch, "launches": a.launches, "rounds": a.rounds, "cases": {}}
    for name, (C, n_fft, hop, L) in CASES.items():
        g = torch.Generator(device=dev).manual_seed(C + n_fft + hop)
        x = torch.randn(a.batch, L, C, generator=g, device=dev).to(torch.bfloat16)
        w = torch.randn(n_fft + 2, C, 7, generator=g, device=dev) * (7 * C) ** -0.5
        b = torch.randn(n_fft + 2, generator=g, device=dev) * 0.1
        laid = torch.empty(lib.evmi_istft_head_weight_elems(C, n_fft), dtype=torch.bfloat16, device=dev)
        wav = [torch.empty(a.batch, hop * L, device=dev) for _ in range(2)]

        def launch(variant):
            _lib.check(lib.evmi_istft_head_bf16(x.data_ptr(), w.data_ptr(), b.data_ptr(), laid.data_ptr(), wav[variant].data_ptr(), a.batch, L,
                                                C, n_fft, hop, variant, stream), "evmi_istft_head_bf16")

        for variant in (0, 1, 0, 1):
            launch(variant)
        torch.cuda.synchronize()
        diff = float((wav[0] - wav[1]).abs().max())
        ms = {0: [], 1: []}
        for _ in range(a.rounds):
            for variant in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    launch(variant)
                e1.record()
                e1.synchronize()
                ms[variant].append(e0.elapsed_time(e1) / a.launches)
        nbytes = a.batch * L * C * 2 + a.batch * hop * L * 4
        bound_ms = nbytes / HBM_BYTES_PER_S * 1e3
        entry = {"C": C, "n_fft": n_fft, "hop": hop, "L": L, "bytes": nbytes, "hbm_bound_ms": bound_ms, "max_abs_diff_between_variants": diff,
                 "frame_tile": lib.evmi_istft_head_frame_tile(n_fft, hop)}
        for variant, v in ms.items():
            med = statistics.median(v)
            entry[f"variant{variant}"] = {"ms_median": med, "ms_min": min(v), "ms_max": max(v), "share_of_hbm_bound": bound_ms / med}
        result["cases"][name] = entry
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
