"""The two bf16 MFMA shapes of the wide inference convolutions (conv_tc_dma_kernel.h) against the oracle and against each other.

``EVMI_CONV_MFMA`` is read once per process, so each shape runs in a child process of its own: same weights, same mel, at
  * a tile-ragged length (2 x 301 frames),
  * a length shorter than one tile's halo (3 x 8 frames),
  * one utterance, whose stages take the 128-row tiles (1 x 130 frames),
  * the GAN step's generator shape (16 x 32 frames).
Both shapes must sit within the bf16 bounds of the fp32 oracle (tests/test_gpu_generator.py), and within SHAPE_REL_L2 of each other.

SHAPE_REL_L2: one 16x16x32 instruction sums 32 channels where 32x32x16 sums 16, so the fp32 partial sums -- and with them the bf16
rounding of every layer's output -- differ between the shapes, as they do between two kernel variants that order the sum differently.
The yardstick is therefore the largest rel-L2 between any two of the existing variants of
``test_kernel_variants_behind_switches_match_the_oracle`` (default, EVMI_CONV_DMA=0, EVMI_PAIR_C128=0, EVMI_BRANCH=0, all on the
32x32x16 shape) on these same inputs, MEASURED_VARIANT_REL_L2 below; twice that is allowed.

Measured on MI355X: the two shapes gave IDENTICAL waveforms in all four cases (rel-L2 0.0; both 4.69e-3 .. 4.78e-3 from the oracle) --
the 32-deep instruction evidently rounds like two 16-deep ones in the same channel order.  That is an observation about the
hardware, not a contract, so the test holds the shapes to the bound above and not to equal bits.
"""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from helpers import make_ref_generator, rel_l2, synthetic_mel

pytestmark = pytest.mark.gpu

BF16_REL_L2 = 1e-2  # tests/test_gpu_generator.py
BF16_ATOL = 5e-2
CASES = ((2, 301), (3, 8), (1, 130), (16, 32))
# measured on MI355X with this file's child at EVMI_CONV_MFMA=32 and each of the four variants, all pairs, all CASES: the largest is
# default vs EVMI_CONV_DMA=0 at 3 x 8 frames, 4.354e-3 (4.29e-3 .. 4.35e-3 for that pair over the cases; EVMI_PAIR_C128=0 vs default
# 1.29e-3 .. 1.44e-3; EVMI_BRANCH=0 vs default 0: identical by design)
MEASURED_VARIANT_REL_L2 = 4.354e-3
SHAPE_REL_L2 = 2 * MEASURED_VARIANT_REL_L2

CHILD = """
import os, sys, torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
from everyvoice_amd import _lib
_lib.load()  # a child without the native library fails here
from helpers import make_ref_generator, synthetic_mel
from test_gpu_generator import _product_from_ref
model = _product_from_ref(make_ref_generator(seed=1234), torch.device("cuda:0"), "bf16")
for B, T in {cases!r}:
    wav = model(synthetic_mel(B, T, seed=99 + T).to("cuda:0"))
    torch.save(wav.cpu(), {out!r} + f"/wav_{{B}}_{{T}}.pt")
print("EVMI_CHILD_DONE", os.environ.get("EVMI_CONV_MFMA"))
"""


def run_child(out_dir: Path, env: dict) -> dict:
    """One process with `env` on top of the caller's: {(B, T): waveform}."""
    root = str(Path(__file__).resolve().parents[1])
    out_dir.mkdir(parents=True, exist_ok=True)
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=root, out=str(out_dir), cases=CASES)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "EVMI_CHILD_DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = {(B, T): torch.load(out_dir / f"wav_{B}_{T}.pt") for B, T in CASES}
    assert len(got) == len(CASES)
    return got


def test_both_mfma_shapes_match_the_oracle_and_each_other(tmp_path, cuda_device):
    outs = {shape: run_child(tmp_path / f"mfma{shape}", {"EVMI_CONV_MFMA": shape}) for shape in ("16", "32")}
    torch.set_num_threads(8)
    ref = make_ref_generator(seed=1234)
    for B, T in CASES:
        with torch.no_grad():
            want = ref(synthetic_mel(B, T, seed=99 + T))
        for shape in ("16", "32"):
            got = outs[shape][(B, T)]
            err, amax = rel_l2(got, want), float((got - want).abs().max())
            print(f"mfma {shape} B={B} T={T}: rel_l2 vs oracle {err:.3e} max_abs {amax:.3e}")
            assert got.shape == want.shape and torch.isfinite(got).all()
            assert err <= BF16_REL_L2 and amax <= BF16_ATOL, (shape, B, T, err, amax)
        between = rel_l2(outs["16"][(B, T)], outs["32"][(B, T)])
        print(f"mfma 16 vs 32 B={B} T={T}: rel_l2 {between:.3e} (allowed {SHAPE_REL_L2})")
        assert between <= SHAPE_REL_L2, (B, T, between)
