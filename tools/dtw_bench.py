#!/usr/bin/env python3
"""Mel-cepstral distortion along the warping path: the fused call (evmi_dtw_cepstral_f32, csrc/dtw_cepstral.hip) beside a torch chain on
the device -- the cepstra as two matrix products, ONE cdist into a [B, Ta, Tb] cost tensor, its anti-diagonals made contiguous by one
gather, then one update per anti-diagonal (slices of three rotating rows: min, min, add) into a [B, Ta + Tb - 1, Tb] tensor of
accumulated costs, the item's end cell gathered at the end.  The chain stops there: it finds the accumulated cost only, not the path
(the fused call also walks it and writes steps, lo, hi and the per-frame values).  The two are alternated in one process: every round
times each once, so drift of the clocks or of a shared machine lands on both alike.  Shape: the batch of tools/align_infer_bench.py
-- B 32, ragged, a mean of about 585 recorded frames --, a synthesized side of 0.8 .. 1.3 times that, 80 mel bins, 13 cepstra; mel-like
inputs (tests/dtw_ref.py: real_case).  Also: one item of that batch in numpy on the host (the float32 restatement).

usage: python tools/dtw_bench.py [out.json] [rounds]"""
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

B, M, K = 32, 80, 13


def batch(dev):
    import dtw_ref as D

    rng = np.random.default_rng(0)
    text_lens = rng.integers(60, 141, B)  # (the draws of tools/align_infer_bench.py: the same recorded lengths)
    ref_lens = np.maximum(text_lens, np.round(text_lens * rng.uniform(5.0, 6.3, B)).astype(np.int64))
    syn_lens = np.round(ref_lens * np.random.default_rng(1).uniform(0.8, 1.3, B)).astype(np.int64)
    Ta, Tb = int(syn_lens.max()), int(ref_lens.max())
    a, b = torch.zeros(B, Ta, M), torch.zeros(B, Tb, M)
    for i in range(B):
        r = D.real_case(int(syn_lens[i]), int(ref_lens[i]))
        a[i, : syn_lens[i]], b[i, : ref_lens[i]] = torch.from_numpy(r["a"]), torch.from_numpy(r["b"])
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    return a.to(dev), b.to(dev), i32(syn_lens), i32(ref_lens), torch.from_numpy(D.dct_basis(M, K)).to(dev), Ta, Tb


def main():
    import dtw_ref as D

    from everyvoice_amd.train import ops

    out_path = sys.argv[1] if len(sys.argv) > 1 else str(ROOT / "profiles" / "dtw_bench.json")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    a, b, la, lb, basis, Ta, Tb = batch(dev)
    S = Ta + Tb - 1
    ws = torch.empty(ops.dtw_ws_bytes(B, Ta, Tb), dtype=torch.uint8, device=dev)
    # the chain's constants (not timed): cell (s - j, j) of every anti-diagonal, and whether it exists
    rows = torch.arange(S, device=dev)[:, None] - torch.arange(Tb, device=dev)[None, :]
    inside = (rows >= 0) & (rows < Ta)
    flat = (rows.clamp(0, Ta - 1) * Tb + torch.arange(Tb, device=dev)[None, :]).reshape(-1)
    end = ((la + lb - 2).long() * Tb + (lb - 1).long())[:, None]
    inf = torch.tensor(float("inf"), device=dev)

    def fused():
        return ops.dtw_cepstral(a, la, b, lb, basis, D.MCD_SCALE, ws=ws)

    def chain():
        c = torch.cdist(a @ basis.T, b @ basis.T)  # [B, Ta, Tb]
        skew = torch.where(inside, c.reshape(B, Ta * Tb)[:, flat].view(B, S, Tb), inf)  # [B, S, Tb]: anti-diagonal s, column j
        acc = torch.empty(B, S, Tb, device=dev)
        buf = [torch.full((B, Tb + 1), float("inf"), device=dev) for _ in range(3)]  # (slot 0: the column left of column 0)
        buf[0][:, 1] = skew[:, 0, 0]
        acc[:, 0] = buf[0][:, 1:]
        for s in range(1, S):
            cur, p1, p2 = buf[s % 3], buf[(s - 1) % 3], buf[(s - 2) % 3]
            torch.add(skew[:, s], torch.minimum(torch.minimum(p2[:, :-1], p1[:, 1:]), p1[:, :-1]), out=cur[:, 1:])
            acc[:, s] = cur[:, 1:]
        return acc.view(B, S * Tb).gather(1, end)[:, 0]

    jobs = {"fused": fused, "chain": chain}
    peak, results = {}, {}
    for name, run in jobs.items():  # first calls: code objects loaded, LDS attributes set -- and the allocator's peak
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
    dist, steps = results["fused"][0].double().cpu(), results["fused"][1].double().cpu()
    total_fused = dist * steps / D.MCD_SCALE  # the accumulated cost D[Na - 1][Nb - 1] the distortion was made from
    total_chain = results["chain"].double().cpu()
    item = int(torch.argsort(lb.cpu())[B // 2])  # the item of median recorded length, in numpy on the host
    na, nb = int(la[item]), int(lb[item])
    xa, xb, xbasis = a[item, :na].cpu().numpy(), b[item, :nb].cpu().numpy(), basis.cpu().numpy()
    t0 = time.perf_counter()
    host = D.dtw(xa, xb, xbasis, np.float32(D.MCD_SCALE), np.float32)
    host_s = time.perf_counter() - t0
    cells = B * Ta * Tb
    result = {"B": B, "Ta": Ta, "Tb": Tb, "M": M, "K": K, "mean_recorded_frames": float(lb.float().mean()), "mean_synthesized_frames": float(la.float().mean()),
              "rounds": rounds, "device": torch.cuda.get_device_name(0),
              "us_per_call": {name: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for name, v in times.items()},
              "bytes_from_shapes": {"fused: one decision byte a cell of the padded diagonals (the workspace, passed in) + the five results":
                                        ops.dtw_ws_bytes(B, Ta, Tb) + 4 * (2 * B + 3 * B * Tb),
                                    "chain: costs [B, Ta, Tb], their anti-diagonals and the accumulated costs [B, Ta + Tb - 1, Tb] (4 B a cell each)":
                                        4 * cells + 8 * B * S * Tb},
              "allocator_peak_bytes_first_call": peak,
              "all_finite": {"fused": bool(torch.isfinite(dist).all()), "chain": bool(torch.isfinite(total_chain).all())},
              "mean_mcd_db_fused": float(dist.mean()), "mean_path_steps_fused": float(steps.mean()),
              "accumulated_cost_fused_minus_chain_max_rel": float(((total_fused - total_chain).abs() / total_chain).max()),
              "numpy_one_item": {"frames": [na, nb], "seconds": round(host_s, 3), "mcd_db": float(host["dist"]),
                                 "fused_mcd_db_of_that_item": float(dist[item]), "same_steps": bool(int(steps[item]) == host["steps"])}}
    text = json.dumps(result, indent=1)
    print(text)
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(text + "\n")


if __name__ == "__main__":
    main()
