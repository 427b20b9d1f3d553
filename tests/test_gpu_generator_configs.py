"""Whole generators outside the V1 / iSTFT shapes through HiFiGANGenerator: HiFi-GAN V2 and V3 and two configurations whose every
hyper-parameter misses the specialised kernel tables (n_mels 100, channels 192 / 96 / 48 / 24, upsamplers (5, 11) (4, 8) (3, 7),
resblock kernels 5 / 9, dilations up to 7) -- the shapes the generic-shape convolution (csrc/conv_tc_generic.hip) exists for.

fp32: max |diff| <= 2e-4 against the CPU oracle, as for V1.

bf16: no fixed tolerance.  The yardstick is computed here on the CPU from the oracle alone: the same oracle with its weights
rounded to bf16 and every convolution's input and output (conv_post's output excepted) rounded to bf16 through forward hooks.  That
emulation rounds at a superset of the storage points of the product's unfused path; the product must stay within
    rel_l2(product, oracle) <= 1.5 x rel_l2(emulated, oracle)   and   max|diff| <= 2 x the emulated max|diff|
(the product applies the activation after the rounding and adds residuals in fp32, so the two are not identical; a wrong tap, a
dropped channel or a misplaced phase gives errors of order 0.1 to 1; the single-sample metric gets the wider margin because it is
the noisier one).
"""

import copy
from pathlib import Path

import pytest
import torch
from torch import nn

from helpers import make_ref_generator, rel_l2, synthetic_mel

pytestmark = pytest.mark.gpu

F32_ATOL = 2e-4
GENERIC = "conv_tc_generic"  # the generic kernel's name in a profile starts with this

V3 = dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8], upsample_initial_channel=256,
          resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]])
ODD1 = dict(n_mels=100, upsample_initial_channel=192, upsample_rates=[5, 4, 3], upsample_kernel_sizes=[11, 8, 7],
            resblock_kernel_sizes=[5, 9], resblock_dilation_sizes=[[1, 2, 4], [1, 7]])
CONFIGS = {
    "v2": dict(upsample_initial_channel=128),
    "v3": V3,
    "odd1": ODD1,
    "odd2": dict(ODD1, resblock="2"),
    # n_mels 76 pads to 80 channels, where the specialised table holds a conv_pre: the padded image is the generic kernel's
    "v2_mels76": dict(n_mels=76, upsample_initial_channel=128),
}
SIZES = [(1, 1), (2, 9), (1, 70)]


def _product_config(name):
    from everyvoice_amd.config import HiFiGANConfig

    model = {k: v for k, v in CONFIGS[name].items() if k != "n_mels"}
    return HiFiGANConfig(model=model, preprocessing=dict(audio=dict(n_mels=CONFIGS[name].get("n_mels", 80))))


_REFS: dict = {}
_CASES: dict = {}


def _ref(name):
    from oracle.hifigan_ref import HiFiGANModelConfigRef

    if name not in _REFS:
        _REFS[name] = make_ref_generator(HiFiGANModelConfigRef(**CONFIGS[name]), seed=4321)
    return _REFS[name]


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _emulated(ref):
    """The oracle with bf16 weights and bf16 storage around every convolution (conv_post's output stays fp32)."""
    emu = copy.deepcopy(ref)
    with torch.no_grad():
        for n, p in emu.named_parameters():
            if n.endswith("weight"):
                p.copy_(_bf(p))
    for n, m in emu.named_modules():
        if isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)):
            m.register_forward_pre_hook(lambda mod, args: (_bf(args[0]),))
            if n != "conv_post":
                m.register_forward_hook(lambda mod, args, out: _bf(out))
    return emu


def _case(name, B, T):
    """(mel, oracle output, emulated rel-L2, emulated max-abs), computed once per case and shared."""
    key = (name, B, T)
    if key not in _CASES:
        ref = _ref(name)
        mel = synthetic_mel(B, T, CONFIGS[name].get("n_mels", 80), seed=7 + T)
        with torch.no_grad():
            want = ref(mel)
            emu = _emulated(ref)(mel)
        assert want.shape == (B, 1, T * ref.hop)
        _CASES[key] = (mel, want, rel_l2(emu, want), float((emu - want).abs().max()))
    return _CASES[key]


def _product(name, device, precision):
    from everyvoice_amd.vocoder import HiFiGANGenerator

    model = HiFiGANGenerator(_product_config(name), precision=precision)
    model.load_state_dict({"generator." + k: v for k, v in _ref(name).state_dict().items()})
    return model.to(device).eval()


def _assert_bf16_bound(got, want, emu_l2, emu_max, what):
    err, mx = rel_l2(got, want), float((got - want).abs().max())
    print(f"{what}: bf16 rel_l2={err:.3e} (emulated {emu_l2:.3e}) max_abs={mx:.3e} (emulated {emu_max:.3e})")
    assert torch.isfinite(got).all()
    assert err <= 1.5 * emu_l2
    assert mx <= 2.0 * emu_max


@pytest.mark.parametrize("B,T", SIZES)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_generator_config_f32_vs_oracle(cuda_device, name, B, T):
    mel, want, _, _ = _case(name, B, T)
    got = _product(name, cuda_device, "f32")(mel.to(cuda_device)).cpu()
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    print(f"{name} B={B} T={T}: f32 max_abs={err:.3e}")
    assert err <= F32_ATOL


@pytest.mark.parametrize("B,T", SIZES)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_generator_config_bf16_vs_oracle(cuda_device, name, B, T):
    mel, want, emu_l2, emu_max = _case(name, B, T)
    model = _product(name, cuda_device, "bf16")
    got, records = model.generator.forward_profiled(mel.to(cuda_device))
    got = got.cpu()
    assert got.shape == want.shape and torch.isfinite(got).all()
    generic = [r for r in records if r["kernel"].startswith(GENERIC)]
    assert generic, sorted({r["kernel"] for r in records})
    assert sum(r["flops"] for r in generic) > 0
    assert torch.equal(model(mel.to(cuda_device)).cpu(), got)  # the plain forward runs the same launches
    _assert_bf16_bound(got, want, emu_l2, emu_max, f"{name} B={B} T={T}")


def test_v3_item_alone_equals_item_in_batch(cuda_device):
    model = _product("v3", cuda_device, "bf16")
    mel = synthetic_mel(4, 300, seed=307).to(cuda_device)
    wav = model(mel)
    assert wav.shape == (4, 1, 300 * 256) and torch.isfinite(wav).all()
    alone = model(mel[2:3].contiguous())
    assert torch.equal(alone[0], wav[2])


def test_v3_weight_norm_checkpoint_loads_with_the_default_precision(cuda_device):
    """load_hifigan_from_checkpoint(ckpt, device): the default precision, bf16, on a configuration the specialised tables miss."""
    from everyvoice_amd.vocoder import load_hifigan_from_checkpoint

    mel, want, emu_l2, emu_max = _case("v3", 2, 9)
    state = {}
    for k, w in _ref("v3").state_dict().items():
        if k.endswith(".weight"):  # weight = g * v / ||v|| (norm over all dimensions but the first)
            state["generator." + k + "_v"] = 2.0 * w
            state["generator." + k + "_g"] = w.pow(2).sum(dim=tuple(range(1, w.dim())), keepdim=True).sqrt()
        else:
            state["generator." + k] = w
    ckpt = {"state_dict": state, "hyper_parameters": {"config": _product_config("v3").model_dump(mode="json")},
            "model_info": {"name": "HiFiGANGenerator", "version": "1.0"}}
    model, _ = load_hifigan_from_checkpoint(ckpt, cuda_device)
    assert model.generator.precision == "bf16"
    got = model(mel.to(cuda_device)).cpu()
    assert got.shape == want.shape
    _assert_bf16_bound(got, want, emu_l2, emu_max, "v3 checkpoint")


def test_bf16_refused_configuration_still_runs_and_profiles_in_f32(cuda_device):
    """Stages of 96 / 48 / 24 / 12 channels: bf16 refuses at construction; the fp32 precisions keep the native object (finalize reports
    the bf16 refusal and leaves it usable)."""
    from everyvoice_amd.config import HiFiGANConfig
    from everyvoice_amd.vocoder import HiFiGANGenerator

    spec = dict(upsample_initial_channel=96, upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8])
    with pytest.raises(ValueError, match="upsample_initial_channel"):
        HiFiGANGenerator(HiFiGANConfig(model=spec))
    mel = synthetic_mel(1, 3, seed=5).to(cuda_device)
    torch.manual_seed(3)
    f32 = HiFiGANGenerator(HiFiGANConfig(model=spec), precision="f32").to(cuda_device).eval()
    direct = HiFiGANGenerator(HiFiGANConfig(model=spec), precision="f32-direct").to(cuda_device).eval()
    direct.load_state_dict(f32.state_dict())
    want = f32(mel)
    got, records = f32.generator.forward_profiled(mel)
    assert records and torch.isfinite(got).all()
    assert float((got - want).abs().max()) <= F32_ATOL and float((direct(mel) - want).abs().max()) <= F32_ATOL


def test_generic_kernel_at_v1_shapes_meets_v1_bounds():
    """EVMI_CONV_GENERIC=1 (read once per process: a child): every single convolution of V1 on the generic kernel, no fused pair or
    branch launches, against V1's own bf16 bounds in tests/test_gpu_generator.py."""
    from helpers import child_pytest_results

    target = str(Path(__file__).resolve().parent / "test_gpu_generator.py")
    jobs = {"generic": ([target, "-q", "-x", "-k", "bf16_vs_oracle or committed_fixture"], {"EVMI_CONV_GENERIC": "1"})}
    rc, out = child_pytest_results("generator_generic_v1", jobs, parallel=1, timeout=600)["generic"]
    assert rc == 0, out
