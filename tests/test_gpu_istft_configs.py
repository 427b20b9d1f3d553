"""Whole iSTFTNet generators with heads other than n_fft 16 / hop 4 on 32 / 64 / 128 channels, through HiFiGANGenerator, against the
CPU oracle (oracle/hifigan_ref.py).

Tolerances: those of tests/test_gpu_generator.py for its iSTFT configurations -- the exact-fp32 paths within 2e-4 x max(1, max|want|),
bf16 within rel_l2 2.5e-2.  The bf16 comparison catches plumbing (weight image, pad row, dispatch: an error there is of order one);
sharp accuracy of the head is tests/test_gpu_istft_head.py's job.
"""

import pytest
import torch
from helpers import make_ref_generator, rel_l2, synthetic_mel

pytestmark = pytest.mark.gpu

F32_RTOL = 2e-4
BF16_REL_L2_ISTFT = 2.5e-2

CONFIGS = {
    "c8c8c2i_8_2": dict(istft_layer=True, upsample_rates=[8, 8, 2], upsample_kernel_sizes=[16, 16, 4], upsample_initial_channel=128,
                        gen_istft_n_fft=8, gen_istft_hop_size=2),
    "c8i_128_32": dict(istft_layer=True, upsample_rates=[8], upsample_kernel_sizes=[16], upsample_initial_channel=48,
                       gen_istft_n_fft=128, gen_istft_hop_size=32),
    "c8c2i_64_16": dict(istft_layer=True, upsample_rates=[8, 2], upsample_kernel_sizes=[16, 4], upsample_initial_channel=256,
                        gen_istft_n_fft=64, gen_istft_hop_size=16),
    "odd_12_5": dict(istft_layer=True, upsample_rates=[5, 4], upsample_kernel_sizes=[11, 8], upsample_initial_channel=96,
                     gen_istft_n_fft=12, gen_istft_hop_size=5),
}
# heads of 16 / 4 off the specialised kernel's channel counts, and the V2-width C8C8I that stays on it
MUST_RUN = {
    "v2_width_c8c8i_32ch": dict(istft_layer=True, upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16], upsample_initial_channel=128),
    "head_16_4_on_16ch": dict(istft_layer=True, upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16], upsample_initial_channel=64),
}


def _product_from_ref(ref, device, precision):
    from everyvoice_amd.config import HiFiGANConfig
    from everyvoice_amd.vocoder import HiFiGANGenerator

    c = ref.cfg
    cfg = HiFiGANConfig(model=dict(resblock=c.resblock, upsample_rates=c.upsample_rates, upsample_kernel_sizes=c.upsample_kernel_sizes,
                                   upsample_initial_channel=c.upsample_initial_channel, resblock_kernel_sizes=c.resblock_kernel_sizes,
                                   resblock_dilation_sizes=c.resblock_dilation_sizes, istft_layer=c.istft_layer),
                        gen_istft_n_fft=c.gen_istft_n_fft, gen_istft_hop_size=c.gen_istft_hop_size)
    model = HiFiGANGenerator(cfg, precision=precision)
    model.load_state_dict({"generator." + k: v for k, v in ref.state_dict().items()})
    return model.to(device).eval()


_REFS: dict = {}


def _ref(name):
    from oracle.hifigan_ref import HiFiGANModelConfigRef

    if name not in _REFS:
        torch.set_num_threads(8)
        _REFS[name] = make_ref_generator(HiFiGANModelConfigRef(**{**CONFIGS, **MUST_RUN}[name]), seed=4321)
    return _REFS[name]


def _head_kernels(model, mel):
    _, recs = model.generator.forward_profiled(mel)
    return [r["kernel"] for r in recs if r["layer"] == "conv_post+istft"]


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("B,T", [(1, 1), (2, 9)])
def test_istft_configuration_vs_oracle(cuda_device, name, B, T):
    ref = _ref(name)
    mel = synthetic_mel(B, T, seed=7 + T)
    with torch.no_grad():
        want = ref(mel)
    scale = float(want.abs().max())
    assert torch.isfinite(want).all() and want.shape == (B, 1, T * ref.hop)
    for prec in ("f32", "f32-direct"):
        got32 = _product_from_ref(ref, cuda_device, prec)(mel.to(cuda_device)).cpu()
        err32 = float((got32 - want).abs().max())
        print(f"istft {name} B={B} T={T}: {prec} max|diff| = {err32:.3e} (bound {F32_RTOL * max(1.0, scale):.3e}, |wav| max {scale:.2f})")
        assert got32.shape == want.shape
        assert err32 <= F32_RTOL * max(1.0, scale), prec
    model = _product_from_ref(ref, cuda_device, "bf16")
    got16 = model(mel.to(cuda_device)).cpu()
    err = rel_l2(got16, want)
    print(f"istft {name} B={B} T={T}: bf16 rel_l2 = {err:.3e} (|wav| max {scale:.2f})")
    assert got16.shape == want.shape
    assert torch.isfinite(got16).all() and err <= BF16_REL_L2_ISTFT


@pytest.mark.parametrize("name", list(MUST_RUN))
def test_heads_of_16_4_at_other_widths_run(cuda_device, name):
    ref = _ref(name)
    mel = synthetic_mel(2, 9, seed=16)
    with torch.no_grad():
        want = ref(mel)
    got16 = _product_from_ref(ref, cuda_device, "bf16")(mel.to(cuda_device)).cpu()
    err = rel_l2(got16, want)
    print(f"istft {name}: bf16 rel_l2 = {err:.3e} (|wav| max {float(want.abs().max()):.2f})")
    assert got16.shape == want.shape
    assert torch.isfinite(got16).all() and err <= BF16_REL_L2_ISTFT


def test_profile_names_the_specialised_head_exactly_at_its_shapes(cuda_device):
    from oracle.hifigan_ref import HiFiGANModelConfigRef

    mel = synthetic_mel(1, 3, seed=5).to(cuda_device)
    for ch0, cl in ((128, 32), (256, 64), (512, 128)):  # C8C8I: two stages
        ref = make_ref_generator(HiFiGANModelConfigRef(istft_layer=True, upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16],
                                                       upsample_initial_channel=ch0), seed=1)
        assert _head_kernels(_product_from_ref(ref, cuda_device, "bf16"), mel) == ["istft_head"], cl
    want = {"head_16_4_on_16ch": "istft_head_generic<c16,n16,h4>", "c8c8c2i_8_2": "istft_head_generic<c16,n8,h2>",
            "c8i_128_32": "istft_head_generic<c24,n128,h32>", "c8c2i_64_16": "istft_head_generic<c64,n64,h16>",
            "odd_12_5": "istft_head_generic<c24,n12,h5>"}
    for name, kernel in want.items():
        assert _head_kernels(_product_from_ref(_ref(name), cuda_device, "bf16"), mel) == [kernel], name
