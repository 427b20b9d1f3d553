"""Host side of the iSTFT head for any gen_istft_n_fft / gen_istft_hop_size (csrc/istft_head_generic.hip); no GPU needed.

What precision="bf16" takes and refuses at construction, what no precision takes, macs_per_sample() and hop of such configurations,
the argument refusals of evmi_istft_head_bf16 (host pointers, never dereferenced: a refusal behind a launch would end in EVMI_ERR_HIP
on a machine without a device), the fp32 workspace of a wide head behind a narrow stage, and the compiler's resource remarks of the
new kernels."""

import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest
import torch

from everyvoice_amd import _lib
from everyvoice_amd.config import HiFiGANConfig
from everyvoice_amd.vocoder import Generator, _model_cfg_to_c
from oracle.hifigan_ref import GeneratorRef, HiFiGANModelConfigRef

ROOT = Path(__file__).resolve().parents[1]
INVALID_ARG, UNSUPPORTED = 1, _lib.EVMI_ERR_UNSUPPORTED

C8C8I = dict(istft_layer=True, upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16])
CONFIGS = {
    "c8c8c2i_8_2": (dict(istft_layer=True, upsample_rates=[8, 8, 2], upsample_kernel_sizes=[16, 16, 4], upsample_initial_channel=128), 8, 2),
    "c8i_128_32": (dict(istft_layer=True, upsample_rates=[8], upsample_kernel_sizes=[16], upsample_initial_channel=48), 128, 32),
    "c8c2i_64_16": (dict(istft_layer=True, upsample_rates=[8, 2], upsample_kernel_sizes=[16, 4], upsample_initial_channel=256), 64, 16),
    "odd_12_5": (dict(istft_layer=True, upsample_rates=[5, 4], upsample_kernel_sizes=[11, 8], upsample_initial_channel=96), 12, 5),
    "head_16_4_on_8ch": (dict(C8C8I, upsample_initial_channel=32), 16, 4),
    "head_16_4_on_16ch": (dict(C8C8I, upsample_initial_channel=64), 16, 4),
}
HOPS = {"c8c8c2i_8_2": 256, "c8i_128_32": 256, "c8c2i_64_16": 256, "odd_12_5": 100, "head_16_4_on_8ch": 256, "head_16_4_on_16ch": 256}


def _config(model, n_fft=16, hop=4):
    return HiFiGANConfig(model=model, gen_istft_n_fft=n_fft, gen_istft_hop_size=hop)


def _macs_from_layer_shapes(model, n_fft, hop):
    """Multiply-accumulates per output sample from the oracle's layer shapes (the method of tests/test_generator_configs_host.py): a
    Conv1d costs out * in * k per output position, a ConvTranspose1d in * out * k per INPUT position; positions per mel frame follow
    the upsampling rates, samples per frame are those positions times the head's hop."""
    ref = GeneratorRef(HiFiGANModelConfigRef(**model, gen_istft_n_fft=n_fft, gen_istft_hop_size=hop))
    per_frame = ref.conv_pre.weight_v.numel()
    rate = 1
    nk = ref.num_kernels
    for i, up in enumerate(ref.ups):
        per_frame += rate * up.weight_v.numel()
        rate *= ref.cfg.upsample_rates[i]
        for rb in ref.resblocks[i * nk:(i + 1) * nk]:
            convs = list(rb.convs1) + list(rb.convs2) if hasattr(rb, "convs1") else list(rb.convs)
            per_frame += rate * sum(c.weight_v.numel() for c in convs)
    assert ref.conv_post.weight_v.shape[0] == n_fft + 2
    per_frame += rate * ref.conv_post.weight_v.numel()
    assert rate * hop == ref.hop
    return per_frame / ref.hop


@pytest.mark.parametrize("name", list(CONFIGS))
def test_bf16_constructs_and_counts(name):
    model, n_fft, hop = CONFIGS[name]
    g = Generator(_config(model, n_fft, hop))  # precision="bf16" is the default
    assert g.precision == "bf16"
    assert g.hop == HOPS[name]
    assert g.conv_post.weight.shape == (n_fft + 2, model["upsample_initial_channel"] >> len(model["upsample_rates"]), 7)
    assert g.macs_per_sample() == pytest.approx(_macs_from_layer_shapes(model, n_fft, hop), rel=1e-12)


BF16_REFUSED = {
    "n_fft_130": (C8C8I, 130, 4, "gen_istft_n_fft"),
    "hop_above_half": (C8C8I, 16, 9, "gen_istft_hop_size"),
    "last_stage_520_channels": (dict(istft_layer=True, upsample_rates=[8], upsample_kernel_sizes=[16], upsample_initial_channel=1040,
                                     resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1]]), 16, 4, "upsample_initial_channel"),
}


@pytest.mark.parametrize("name", list(BF16_REFUSED))
def test_bf16_refuses_outside_the_domain_and_names_the_field(name):
    model, n_fft, hop, field = BF16_REFUSED[name]
    with pytest.raises(ValueError, match=field) as e:
        Generator(_config(model, n_fft, hop))
    assert 'precision="f32"' in str(e.value)
    assert Generator(_config(model, n_fft, hop), precision="f32").precision == "f32"
    assert _lib.load().evmi_generator_bf16_check(C.byref(_model_cfg_to_c(_config(model, n_fft, hop)))) == UNSUPPORTED


NO_PRECISION = {"odd_n_fft": (15, 4, "gen_istft_n_fft"), "hop_0": (16, 0, "gen_istft_hop_size"), "hop_equals_n_fft": (16, 16, "gen_istft_hop_size")}


@pytest.mark.parametrize("precision", ["bf16", "f32", "f32-direct"])
@pytest.mark.parametrize("name", list(NO_PRECISION))
def test_every_precision_refuses_what_no_kernel_runs(name, precision):
    n_fft, hop, field = NO_PRECISION[name]
    with pytest.raises(ValueError, match=field) as e:
        Generator(_config(C8C8I, n_fft, hop), precision=precision)
    assert 'precision="f32" takes it' not in str(e.value)


@pytest.mark.parametrize("name", list(NO_PRECISION))
def test_generator_create_returns_invalid_arg(name):
    n_fft, hop, field = NO_PRECISION[name]
    lib = _lib.load()
    cfg = _model_cfg_to_c(_config(C8C8I))
    cfg.istft_n_fft, cfg.istft_hop = n_fft, hop
    h = C.c_void_p()
    assert lib.evmi_generator_create(C.byref(cfg), 0, C.byref(h)) == INVALID_ARG
    assert field in lib.evmi_last_error().decode() and not h.value
    assert lib.evmi_generator_bf16_check(C.byref(cfg)) == INVALID_ARG
    cfg.istft_layer = 0  # without the head the fields are not read
    assert lib.evmi_generator_create(C.byref(cfg), 0, C.byref(h)) == _lib.EVMI_OK
    lib.evmi_generator_destroy(h)


_BUF = torch.zeros(64)  # host memory standing in for every device pointer
P = _BUF.data_ptr()


def _head_args(null=None, B=2, L=5, Cc=24, n_fft=8, hop=2, variant=0):
    ptrs = [0 if i == null else P for i in range(5)]
    return (*ptrs, B, L, Cc, n_fft, hop, variant, None)


def _refused(args, code):
    lib = _lib.load()
    rc = lib.evmi_istft_head_bf16(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == code, f"evmi_istft_head_bf16{args}: returned {rc} ({msg!r}), wanted {code}"
    assert "istft_head_bf16" in msg, msg
    return msg


def test_head_entry_refuses_before_any_launch():
    for i in range(5):
        _refused(_head_args(null=i), INVALID_ARG)
    for kw in (dict(B=0), dict(B=-1), dict(L=0), dict(L=-2), dict(variant=2), dict(variant=-1), dict(B=65536)):
        _refused(_head_args(**kw), INVALID_ARG)
    for kw in (dict(Cc=12), dict(Cc=0), dict(Cc=-8), dict(Cc=520)):
        assert "C " in _refused(_head_args(**kw), UNSUPPORTED)
    for kw in (dict(n_fft=2, hop=1), dict(n_fft=130), dict(n_fft=9), dict(n_fft=0)):
        assert "n_fft" in _refused(_head_args(**kw), UNSUPPORTED)
    for kw in (dict(hop=0), dict(hop=5), dict(hop=8), dict(hop=-1)):
        assert "hop" in _refused(_head_args(**kw), UNSUPPORTED)
    for variant in (0, 1):  # the specialised shape has the same domain in both variants
        _refused(_head_args(null=3, Cc=32, n_fft=16, hop=4, variant=variant), INVALID_ARG)


def test_head_weight_elems_and_frame_tile():
    lib = _lib.load()
    for Cc, n_fft in ((8, 4), (24, 128), (32, 16), (128, 16), (512, 128)):
        n = lib.evmi_istft_head_weight_elems(Cc, n_fft)
        assert n >= (n_fft + 2) * Cc * 7 and n % 8 == 0
    assert lib.evmi_istft_head_weight_elems(12, 16) == 0 and lib.evmi_istft_head_weight_elems(32, 130) == 0
    assert lib.evmi_istft_head_weight_elems(520, 16) == 0 and lib.evmi_istft_head_weight_elems(32, 15) == 0
    # every (n_fft, hop) of the domain: a tile of 64 / 128 / 192 frames that yields at least one hop of samples
    for n_fft in range(4, 129, 2):
        for hop in range(1, n_fft // 2 + 1):
            tile = lib.evmi_istft_head_frame_tile(n_fft, hop)
            assert tile in (64, 128, 192) and tile - 2 * ((n_fft // 2 - 1) // hop) - 1 >= 1, (n_fft, hop, tile)
    assert lib.evmi_istft_head_frame_tile(128, 32) == 64
    assert lib.evmi_istft_head_frame_tile(16, 9) == 0 and lib.evmi_istft_head_frame_tile(130, 4) == 0


def test_f32_workspace_covers_the_logits_of_a_wide_head():
    """c8i_128_32: Z [B][n_fft + 2][L + 1] is five times the widest stage ([B][L + 1][24]); every one of the five buffers holds it."""
    lib = _lib.load()
    model, n_fft, hop = CONFIGS["c8i_128_32"]
    cfg = _model_cfg_to_c(_config(model, n_fft, hop))
    h = C.c_void_p()
    _lib.check(lib.evmi_generator_create(C.byref(cfg), 0, C.byref(h)), "evmi_generator_create")
    try:
        for B, T in ((1, 1), (2, 9), (3, 100)):
            L = 8 * T
            total = lib.evmi_generator_workspace_bytes(h, B, T, _lib.EVMI_PREC_F32)
            assert total // 5 >= 4 * B * (n_fft + 2) * (L + 1), (B, T, total)
            # the bf16 path keeps its logits in LDS: its workspace does not grow with the head
            assert lib.evmi_generator_workspace_bytes(h, B, T, _lib.EVMI_PREC_BF16) < total
    finally:
        lib.evmi_generator_destroy(h)


def test_declarations_match_the_ctypes_table():
    header = {n: (ret, params) for n, ret, params in _lib.declarations()}
    for name in ("evmi_istft_head_bf16", "evmi_istft_head_weight_elems", "evmi_istft_head_frame_tile"):
        assert name in header, f"{name} is not declared in include/evmi.h"
        ret, params = header[name]
        assert all("*" in t or t == "int" for t, _ in params), (name, params)
        declared = [C.c_void_p if "*" in t else C.c_int for t, _ in params]
        fn = getattr(_lib.load(), name)
        assert list(fn.argtypes) == declared, (name, fn.argtypes, declared)
        assert fn.restype is {"int": C.c_int, "long long": C.c_longlong}[ret]


# ---- static rule on the compiled kernels ------------------------------------------------------------------------------------
def test_no_head_kernel_uses_scratch_memory(tmp_path):
    """Every kernel of istft_head_generic.hip: ScratchSize 0 bytes per lane and no spilled register in the compiler's resource remarks."""
    hipcc = Path("/opt/rocm/bin/hipcc")
    if not hipcc.exists():
        pytest.skip("hipcc not found")
    r = subprocess.run([str(hipcc), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT / 'include'}", f"-I{ROOT / 'everyvoice_amd' / 'csrc'}",
                        "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", "-o", str(tmp_path / "istft_head_generic.s"),
                        str(ROOT / "everyvoice_amd" / "csrc" / "istft_head_generic.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"remark: Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vspill = [int(v) for v in re.findall(r"remark:\s+VGPRs Spill: (\d+)", r.stderr)]
    sspill = [int(v) for v in re.findall(r"remark:\s+SGPRs Spill: (\d+)", r.stderr)]
    heads = [n for n in names if "istft_head_generic_kernel" in n]
    assert len(heads) == 3 and len(names) == len(scratch) == len(vspill) == len(sspill) == 5, (names, scratch)  # 3 frame tiles + 2 relayouts
    bad = [(n, s, v, q) for n, s, v, q in zip(names, scratch, vspill, sspill) if s or v or q]
    assert not bad, bad
