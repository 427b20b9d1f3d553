#!/usr/bin/env python3
"""Copy the reference's SoX ``silence`` test input as DATA (build container only).

Run:  python tests/golden/make_sox_golden.py      (needs /root/reference mounted)

Captured (reference file):
  440tone-with-leading-trailing-silence.wav   everyvoice/tests/data/  -> tone440_silence.npz (``pcm`` int16, ``sr``)
The reference's ``test_remove_silence`` (everyvoice/tests/test_preprocessing.py:62-108) trims this file with the chain
``channels 1, silence 1 0.1 0.1%, reverse, silence 1 0.1 0.1%, reverse`` and expects round(seconds, 2) == 2.5, at the file's
44.1 kHz and after resampling to 22.05 kHz; tests/test_sox_effects.py and tests/test_gpu_sox_effects.py check that expectation.
"""

from __future__ import annotations

import wave
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent


def main():
    src = REF / "everyvoice" / "tests" / "data" / "440tone-with-leading-trailing-silence.wav"
    with wave.open(str(src), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2, "expected mono 16-bit PCM"
        sr = w.getframerate()
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16)
    np.savez_compressed(OUT / "tone440_silence.npz", pcm=pcm, sr=np.int64(sr))
    print(f"tone440_silence.npz: {pcm.size} samples at {sr} Hz")


if __name__ == "__main__":
    main()
