"""Host-side checks of the generator configurations (no GPU): what precision="bf16" refuses is refused at construction with a
ValueError that names the configuration field, and macs_per_sample() is right for configurations outside V1."""

import pytest

from everyvoice_amd.config import HiFiGANConfig
from everyvoice_amd.vocoder import Generator
from oracle.hifigan_ref import GeneratorRef, HiFiGANModelConfigRef

V3 = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=256,
          resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]])
ODD1 = dict(n_mels=100, upsample_initial_channel=192, upsample_rates=[5, 4, 3], upsample_kernel_sizes=[11, 8, 7],
            resblock_kernel_sizes=[5, 9], resblock_dilation_sizes=[[1, 2, 4], [1, 7]])
CONFIGS = {"v2": dict(upsample_initial_channel=128), "v3": V3, "odd1": ODD1}


def _config(spec):
    model = {k: v for k, v in spec.items() if k != "n_mels"}
    return HiFiGANConfig(model=model, preprocessing=dict(audio=dict(n_mels=spec.get("n_mels", 80))))


REFUSED = {
    # stages of 96 / 48 / 24 / 12 channels
    "channel_count_12": (dict(upsample_initial_channel=96, upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8]), "upsample_initial_channel"),
    "even_resblock_kernel": (dict(resblock_kernel_sizes=[3, 4, 11]), "resblock_kernel_sizes"),
    "upsampler_4_7": (dict(upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 7]), "upsample_kernel_sizes"),
    # (11 - 1) * 27 = 270 rows > 256
    "halo_beyond_limit": (dict(resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 27]]), "resblock_dilation_sizes"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_bf16_refuses_at_construction_and_names_the_field(name):
    spec, field = REFUSED[name]
    with pytest.raises(ValueError, match=field) as e:
        Generator(_config(spec))  # precision="bf16" is the default
    assert 'precision="f32"' in str(e.value)
    assert Generator(_config(spec), precision="f32").precision == "f32"


def test_halo_limit_itself_is_taken():
    Generator(_config(dict(resblock_kernel_sizes=[3, 7, 9], resblock_dilation_sizes=[[1, 3, 128], [1, 3, 5], [1, 3, 32]])))


def _macs_from_layer_shapes(spec):
    """Multiply-accumulates per output sample from the oracle's layer shapes: a Conv1d costs out * in * k per output position, a
    ConvTranspose1d in * out * k per INPUT position; positions per mel frame follow the upsampling rates."""
    ref = GeneratorRef(HiFiGANModelConfigRef(**spec))
    per_frame = ref.conv_pre.weight_v.numel()
    rate = 1
    nk = ref.num_kernels
    for i, up in enumerate(ref.ups):
        per_frame += rate * up.weight_v.numel()
        rate *= ref.cfg.upsample_rates[i]
        for rb in ref.resblocks[i * nk:(i + 1) * nk]:
            convs = list(rb.convs1) + list(rb.convs2) if hasattr(rb, "convs1") else list(rb.convs)
            per_frame += rate * sum(c.weight_v.numel() for c in convs)
    per_frame += rate * ref.conv_post.weight_v.numel()
    assert rate == ref.hop
    return per_frame / ref.hop


@pytest.mark.parametrize("name", list(CONFIGS))
def test_macs_per_sample_of_other_configurations(name):
    got = Generator(_config(CONFIGS[name])).macs_per_sample()
    assert got == pytest.approx(_macs_from_layer_shapes(CONFIGS[name]), rel=1e-12)


def test_v1_and_c8c8i_still_construct_and_report_their_counts():
    assert Generator(HiFiGANConfig()).macs_per_sample() == pytest.approx(1_199_424)
    c8c8i = HiFiGANConfig(model=dict(istft_layer=True, upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16]))
    assert Generator(c8c8i).macs_per_sample() == pytest.approx(803_872)
