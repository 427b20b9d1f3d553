#!/usr/bin/env python3
"""Pins copied as DATA from the upstream EveryVoice tree, so that the tests that check against them need nothing outside this
repository.

Run:  python tests/golden/make_reference_pins.py <path to an EveryVoice checkout>

Captured (upstream file) -> tests/golden/:
  everyvoice/.schema/everyvoice-spec-to-wav-0.5.json   spec_to_wav_schema_defaults.json   the `default` of every property of
                                                                                           HiFiGANModelConfig and AudioConfig
  everyvoice/tests/data/test.ckpt                      position_inv_freq.npy              state_dict["position_embedding.inv_freq"]
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

OUT = Path(__file__).resolve().parent
CONFIGS = ("HiFiGANModelConfig", "AudioConfig")


def main(upstream: Path) -> None:
    schema = json.loads((upstream / "everyvoice/.schema/everyvoice-spec-to-wav-0.5.json").read_text())
    defaults = {name: {field: spec["default"] for field, spec in schema["$defs"][name]["properties"].items() if "default" in spec}
                for name in CONFIGS}
    (OUT / "spec_to_wav_schema_defaults.json").write_text(json.dumps(defaults, indent=1) + "\n")
    ck = torch.load(upstream / "everyvoice/tests/data/test.ckpt", map_location="cpu", weights_only=False)
    inv = ck["state_dict"]["position_embedding.inv_freq"].numpy()
    assert inv.dtype == np.float32 and inv.shape == (128,)
    np.save(OUT / "position_inv_freq.npy", inv)
    print({k: len(v) for k, v in defaults.items()}, "inv_freq", inv.shape)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(Path(sys.argv[1]))
