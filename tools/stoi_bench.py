#!/usr/bin/env python3
"""STOI of a batch of syntheses against their recordings: the fused call (evmi_stoi_f32, csrc/stoi.hip) beside a torch chain of the
same definition on the same device -- frames by unfold, the energies and the 40 dB mask, the kept frames moved to the front by one
stable argsort and one gather, overlap-add by fold, frames again, rfft, the band matrix, the 30-frame segments by unfold, the clipped
and normalised correlation, the masked mean.  The two are alternated in one process: every round times each once, so drift of the
clocks or of a shared machine lands on both alike.  Shape: 32 items of 6 s at 10 kHz (467 frames each): noise under a slow envelope
with a silent stretch per item (tests/stoi_ref.py: noise_pair), the synthesis that plus noise.  Also: one item in numpy on the host
(the float32 restatement).

usage: python tools/stoi_bench.py [out.json] [rounds]"""
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

B, S = 32, 60000


def batch(dev):
    import stoi_ref as R

    pairs = [R.noise_pair(100 + i, S, g=0.2 + 0.05 * (i % 8), gap=(9000 + 1000 * i, 9000 + 1000 * i + 300 * (i % 11))) for i in range(B)]
    ref = torch.from_numpy(np.stack([np.asarray(a, np.float32) for a, _ in pairs]))
    deg = torch.from_numpy(np.stack([np.asarray(b, np.float32) for _, b in pairs]))
    return ref.to(dev), deg.to(dev)


def make_chain(ref, deg):
    """The torch chain on equal-length rows ref, deg [B, S] -> a call returning (stoi [B], kept frames [B])."""
    import stoi_ref as R

    from everyvoice_amd.pipeline import third_octave_bands

    dev, S = ref.device, ref.shape[1]
    F = -(-(S - 256) // 128)
    # the chain's constants (not timed)
    w = torch.from_numpy(R.window(np.float32)).to(dev)
    obm = torch.zeros(15, 257, device=dev)
    for b, (lo, hi) in enumerate(third_octave_bands()):
        obm[b, lo:hi] = 1.0
    eps, clip = R.EPS, 1.0 + 10.0 ** (15.0 / 20.0)
    frame_ix, seg_ix = torch.arange(F, device=dev), torch.arange(F - 30, device=dev)
    L = (F - 1) * 128 + 256

    def chain():
        xf, yf = ref.unfold(1, 256, 128)[:, :F] * w, deg.unfold(1, 256, 128)[:, :F] * w
        e = 20.0 * torch.log10(xf.norm(dim=2) + eps)
        keep = (e.max(dim=1, keepdim=True).values - 40.0 - e) < 0
        K = keep.sum(dim=1)
        order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)[:, :, None].expand(-1, -1, 256)
        valid = (frame_ix[None, :] < K[:, None])[:, :, None]
        bands = []
        for frames in (xf, yf):
            kept = (frames.gather(1, order) * valid).transpose(1, 2)
            sig = torch.nn.functional.fold(kept, (1, L), (1, 256), stride=(1, 128))[:, 0, 0]
            again = sig.unfold(1, 256, 128)[:, : F - 1] * w
            power = torch.fft.rfft(again, n=512, dim=2).abs().square()
            bands.append(torch.sqrt(power @ obm.T).unfold(1, 30, 1))  # [B, F - 30, 15, 30]
        x, y = bands
        c = x.norm(dim=3, keepdim=True) / (y.norm(dim=3, keepdim=True) + eps)
        y = torch.minimum(c * y, x * clip)
        x, y = x - x.mean(dim=3, keepdim=True), y - y.mean(dim=3, keepdim=True)
        rho = ((x / (x.norm(dim=3, keepdim=True) + eps)) * (y / (y.norm(dim=3, keepdim=True) + eps))).sum(dim=3)
        J = (K - 30).clamp(min=0)
        rho = rho * (seg_ix[None, :] < J[:, None])[:, :, None]
        return rho.sum(dim=(1, 2)) / (15 * J), K

    return chain


def main():
    import stoi_ref as R

    from everyvoice_amd.train import ops

    out_path = sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "stoi_bench.json")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    ref, deg = batch(dev)
    lens = torch.full((B,), S, dtype=torch.int32, device=dev)
    F = -(-(S - 256) // 128)

    def fused():
        return ops.stoi(ref, lens, deg, lens)

    chain = make_chain(ref, deg)
    jobs = {"fused": fused, "chain": chain}
    peak, results = {}, {}
    for name, run in jobs.items():  # first calls: code objects loaded, LDS attributes set, transform plans made -- and the allocator's peak
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        results[name] = run()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated(dev) - before
        run()
    torch.cuda.synchronize()
    times = {name: [] for name in jobs}
    for _ in range(rounds):
        for name, run in jobs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            run()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3)
    value, counts = results["fused"][0].double().cpu(), results["fused"][1].cpu()
    chain_value, chain_K = results["chain"][0].double().cpu(), results["chain"][1].cpu()
    x, y = ref[0].cpu().numpy(), deg[0].cpu().numpy()
    t0 = time.perf_counter()
    host = R.stoi(x, y, np.float32)
    host_s = time.perf_counter() - t0
    result = {"B": B, "samples": S, "frames": F, "mean_active_frames": float(counts[:, 1].float().mean()), "rounds": rounds,
              "device": torch.cuda.get_device_name(0),
              "us_per_call": {name: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for name, v in times.items()},
              "allocator_peak_bytes_first_call": peak,
              "all_finite": {"fused": bool(torch.isfinite(value).all()), "chain": bool(torch.isfinite(chain_value).all())},
              "mean_stoi_fused": float(value.mean()), "same_active_frames": bool(torch.equal(counts[:, 1].long(), chain_K.long())),
              "stoi_fused_minus_chain_max_abs": float((value - chain_value).abs().max()),
              "numpy_one_item": {"seconds": round(host_s, 3), "stoi": float(host["stoi"]), "fused_stoi_of_that_item": float(value[0]),
                                 "same_counts": bool(tuple(counts[0].tolist()) == (host["F"], host["K"], host["J"]))}}
    print(json.dumps(result))
    text = json.dumps(result, indent=1)
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(text + "\n")


if __name__ == "__main__":
    main()
