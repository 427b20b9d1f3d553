#!/usr/bin/env python3
"""Per-launch times of the attention kernels for any head dimension (csrc/attention_generic.hip) beside the specialised ones
(csrc/attention_train.hip), interleaved in one process: every round times every candidate once, so drift of the clocks or of a
shared machine lands on all of them alike.  Shapes: B 32, T 566 (the mean frame count of the benchmark batch), D = H * dh.

usage: python tools/attention_generic_bench.py [out.json] [rounds] [launches per timing]"""
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from everyvoice_amd import _lib  # noqa: E402

B, T = 32, 566
# (label, entry-point family, D, heads)
CASES = [("specialised dh 128", "mha", 256, 2), ("generic dh 128", "mha_generic", 256, 2), ("generic dh 96", "mha_generic", 192, 2),
         ("generic dh 192", "mha_generic", 384, 2), ("generic dh 256", "mha_generic", 512, 2)]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    launches = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    dev = torch.device("cuda:0")
    lib = _lib.load()
    s = _lib.current_stream_ptr(dev)
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(T // 2, T + 1, (B,), generator=g).to(dev, torch.int32)
    jobs = []
    for label, family, D, H in CASES:
        x, dout = torch.randn(3 * D, B, T, generator=g).to(dev), torch.randn(D, B, T, generator=g).to(dev)
        out, lse, dsum, dqkv = torch.empty(D, B, T, device=dev), torch.empty(B, H, T, device=dev), torch.empty(B, H, T, device=dev), torch.empty_like(x)
        for operands in ("f32", "bf16"):
            fwd, bwd = getattr(lib, f"evmi_{family}_fwd_{operands}"), getattr(lib, f"evmi_{family}_bwd_{operands}")
            run_f = lambda fwd=fwd, x=x, out=out, lse=lse, D=D, H=H: _lib.check(  # noqa: E731
                fwd(x.data_ptr(), lens.data_ptr(), out.data_ptr(), lse.data_ptr(), B, T, D, H, 0.1, 7, None, s), "fwd")
            run_b = lambda bwd=bwd, x=x, out=out, dout=dout, lse=lse, dsum=dsum, dqkv=dqkv, D=D, H=H: _lib.check(  # noqa: E731
                bwd(x.data_ptr(), lens.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dsum.data_ptr(), dqkv.data_ptr(), B, T, D, H, 0.1, 7,
                    None, s), "bwd")
            jobs.append((f"{label} {operands} forward", run_f))
            jobs.append((f"{label} {operands} backward", run_b))
    for _, run in jobs:  # warm-up: code objects loaded, LDS attributes set
        run()
        run()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in jobs}
    for _ in range(rounds):
        for name, run in jobs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(launches):
                run()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3 / launches)
    result = {"B": B, "T": T, "p_drop": 0.1, "rounds": rounds, "launches_per_timing": launches, "device": torch.cuda.get_device_name(0),
              "us_per_launch": {name: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for name, v in times.items()}}
    text = json.dumps(result, indent=1)
    print(text)
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(text + "\n")


if __name__ == "__main__":
    main()
