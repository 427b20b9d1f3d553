#!/usr/bin/env python3
"""The fused mel front end (csrc/mel_frontend.hip) under device events, two questions per run:

  ab       this build against another build of the library (`--other-lib PATH`, e.g. the parent commit's libevmi_hip.so) at the
           preprocessing shape [32, 176400] (32 utterances of 8 s, n_fft 1024 / win 1024 / hop 256) through the entry point both
           export (evmi_mel_spectrogram_f32), the two alternating round by round in one process.  Per round and library the median
           of `--reps` launches; reported: every round's median, the median of those, and the spread (max - min) of the other
           library's round medians -- the yardstick for a difference between the two.
  support  n_fft 2048 / win 1200 / hop 300 at [32, 192000]: the loop over the window's support (win_length = 1200 declared) against
           the loop over all n_fft rows of the same basis (win_length = 2048 declared), alternating the same way.

`--dump DIR` also writes mel, energy and magnitude of seeded inputs at three of today's configurations from both libraries
(DIR/this/*.bin, DIR/other/*.bin) for a byte comparison (cmp), and reports torch.equal for each.  One JSON line per question.
Usage: python tools/mel_frontend_bench.py [--other-lib PATH] [--rounds 7] [--reps 200] [--dump DIR] [--out FILE]"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from everyvoice_amd import _lib  # noqa: E402
from everyvoice_amd.spectral import MelSpectrogram  # noqa: E402


def bind(path):
    """Another build of the library: the one entry point every build exports, with the table's argument types."""
    lib = C.CDLL(str(path))
    for name in ("evmi_mel_spectrogram_f32", "evmi_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SYMBOLS[name]
    return lib


class Case:
    def __init__(self, tr, B, S, seed, dev):
        self.tr, self.B, self.S = tr, B, S
        self.x = (0.3 * torch.tanh(torch.randn(B, S, generator=torch.Generator().manual_seed(seed)))).to(dev)
        self.basis, self.melb = tr._consts(dev)
        frames = 1 + S // tr.hop
        self.mel = torch.empty(B, tr.n_mels, frames, device=dev)
        self.energy = torch.empty(B, frames, device=dev)
        self.mag = torch.empty(B, tr.n_fft // 2 + 1, frames, device=dev)

    def full(self, lib, mag=True):
        """evmi_mel_spectrogram_f32 of `lib` (win_length == n_fft)."""
        tr = self.tr
        rc = lib.evmi_mel_spectrogram_f32(self.x.data_ptr(), self.basis.data_ptr(), self.melb.data_ptr(), self.mel.data_ptr(), self.energy.data_ptr(),
                                          self.mag.data_ptr() if mag else 0, self.B, self.S, tr.n_fft, tr.hop, tr.nb_pad, tr.n_mels, 1,
                                          _lib.current_stream_ptr(self.x.device))
        if rc:
            raise RuntimeError(f"evmi_mel_spectrogram_f32: {rc}: {lib.evmi_last_error()}")

    def win(self, declared_win, mag=True):
        """evmi_mel_spectrogram_win_f32 of this build, declaring `declared_win`."""
        tr = self.tr
        _lib.check(_lib.load().evmi_mel_spectrogram_win_f32(self.x.data_ptr(), 0, self.basis.data_ptr(), self.melb.data_ptr(), self.mel.data_ptr(),
                                                            self.energy.data_ptr(), self.mag.data_ptr() if mag else 0, self.B, self.S, tr.n_fft,
                                                            declared_win, tr.hop, tr.nb_pad, tr.n_mels, 1, _lib.current_stream_ptr(self.x.device)),
                   "evmi_mel_spectrogram_win_f32")

    def outputs(self):
        torch.cuda.synchronize()
        return {"mel": self.mel.cpu(), "energy": self.energy.cpu(), "mag": self.mag.cpu()}


def alternate(runs: dict, rounds: int, reps: int):
    """{name: callable} -> {name: [median ms of `reps` launches, per round]}, the names taking turns inside every round."""
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in runs}
    for r in range(rounds):
        order = list(runs) if r % 2 == 0 else list(runs)[::-1]
        for name in order:
            events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for e0, e1 in events:
                e0.record()
                runs[name]()
                e1.record()
            torch.cuda.synchronize()
            out[name].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in events))
    return out


def summary(per_round: dict):
    return {name: {"round_medians_ms": [round(v, 5) for v in vals], "median_ms": round(statistics.median(vals), 5),
                   "spread_ms": round(max(vals) - min(vals), 5)} for name, vals in per_round.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--dump")
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    this = _lib.load()
    other = bind(a.other_lib) if a.other_lib else None
    lines = []

    if a.dump and other is not None:
        cases = {"1024_1024_256_b32_s176400": Case(MelSpectrogram(), 32, 176400, 1, dev), "1024_1024_256_b16_s8192": Case(MelSpectrogram(), 16, 8192, 2, dev),
                 "2048_2048_512_b16_s8192": Case(MelSpectrogram(2048, 2048, 512, 44100, 80, 0, 8000), 16, 8192, 3, dev)}
        equal = {}
        for name, case in cases.items():
            got = {}
            for side, run in (("other", lambda c=case: c.full(other)), ("this", lambda c=case: c.win(c.tr.n_fft)), ("this_full_entry", lambda c=case: c.full(this))):
                for t in (case.mel, case.energy, case.mag):
                    t.fill_(float("nan"))
                run()
                got[side] = case.outputs()
                if side != "this_full_entry":
                    for kind, t in got[side].items():
                        path = Path(a.dump) / side / f"{name}_{kind}.bin"
                        path.parent.mkdir(parents=True, exist_ok=True)
                        path.write_bytes(t.numpy().tobytes())
            equal[name] = {kind: bool(torch.equal(got["other"][kind], got["this"][kind]) and torch.equal(got["other"][kind], got["this_full_entry"][kind])
                                      and torch.isfinite(got["this"][kind]).all()) for kind in ("mel", "energy", "mag")}
        lines.append({"question": "bits", "other_lib": str(a.other_lib), "equal": equal})

    if other is not None:
        case = Case(MelSpectrogram(), 32, 176400, 1, dev)
        per_round = alternate({"other": lambda: case.full(other, mag=False), "this": lambda: case.full(this, mag=False)}, a.rounds, a.reps)
        s = summary(per_round)
        lines.append({"question": "ab", "shape": [32, 176400], "n_fft_win_hop": [1024, 1024, 256], "rounds": a.rounds, "reps": a.reps, "other_lib": str(a.other_lib),
                      **s, "this_minus_other_ms": round(s["this"]["median_ms"] - s["other"]["median_ms"], 5),
                      "within_other_spread": bool(s["this"]["median_ms"] - s["other"]["median_ms"] <= s["other"]["spread_ms"])})

    tr = MelSpectrogram(2048, 1200, 300, 24000, 100, 0, 12000)
    case = Case(tr, 32, 192000, 4, dev)
    reps = max(20, a.reps // 4)
    per_round = alternate({"support": lambda: case.win(1200, mag=False), "full": lambda: case.win(2048, mag=False)}, a.rounds, reps)
    s = summary(per_round)
    lines.append({"question": "support", "shape": [32, 192000], "n_fft_win_hop": [2048, 1200, 300], "rounds": a.rounds, "reps": reps, "plan": tr.plan,
                  "mfma_steps_support_over_full": (tr.plan["k1"] - tr.plan["k0"]) / 2048, **s,
                  "support_over_full_time": round(s["support"]["median_ms"] / s["full"]["median_ms"], 4)})

    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
