"""FastSpeech2 at Conformer widths above 256 channels, whole model against oracle/fs2_ref.py: the three tests of
tests/test_gpu_fs2_head_dims.py (their bodies, helpers and tolerances: called, not copied) at input_dim 320 with 2 heads, 384 with 4 and
512 with 2 -- head dimensions 160, 96 and 256.  Every LayerNorm of the model, and the variance predictors, run at C = input_dim: the
training step is the test that needs the LayerNorm backward above 256 channels.  At precision="bf16" the step at 384 and 512 must also
take the LayerNorm -> packed-input fusion (evmi_layernorm_pack_bf16pk_w), read off the library calls it issues."""

import pytest

from tests import test_gpu_fs2_head_dims as head_dims

pytestmark = pytest.mark.gpu

WIDTHS = [(320, 2, 640), (384, 4, 768), (512, 2, 1024)]  # (input_dim, heads, feedforward_dim)


class _Recording:
    """Stands in FRONT of the loaded library: every entry point called through it is noted by name, then runs."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn):
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)

        return call


@pytest.mark.parametrize("input_dim,heads,feedforward_dim", WIDTHS)
def test_fs2_inference_f32(cuda_device, input_dim, heads, feedforward_dim):
    head_dims.test_fs2_inference_f32(cuda_device, input_dim, heads, feedforward_dim)


@pytest.mark.parametrize("input_dim,heads,feedforward_dim", WIDTHS)
def test_fs2_inference_bf16_operands(cuda_device, input_dim, heads, feedforward_dim):
    head_dims.test_fs2_inference_bf16_operands(cuda_device, input_dim, heads, feedforward_dim)


@pytest.mark.parametrize("input_dim,heads,feedforward_dim", WIDTHS)
def test_fs2_training_step(cuda_device, input_dim, heads, feedforward_dim, monkeypatch):
    from everyvoice_amd import _lib

    rec = _Recording(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    head_dims.test_fs2_training_step(cuda_device, input_dim, heads, feedforward_dim)
    assert "evmi_layernorm_bwd_cbt_f32" in rec.names  # (the calls did go through the recorder)
    if input_dim in (384, 512):
        assert "evmi_layernorm_pack_bf16pk_w" in rec.names
