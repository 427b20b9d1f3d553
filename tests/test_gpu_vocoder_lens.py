"""Ragged vocoder batches: ``Generator.forward(mel, lens)`` gives every item the waveform it gets alone at its own length, bit for bit.

The criterion everywhere: ``out[i, 0, :lens[i] * hop]`` is ``torch.equal`` to ``Generator(mel[i:i+1, :, :lens[i]])`` and the rest of
the row is zero.  No tolerance: the kernels bound their loads, stores and zero padding by the item's length, and the bits of an output
element do not depend on the tile it was computed in.

Inputs are chosen to expose a miss: the mel's padding frames are not zero, and before each ragged call a uniform forward on
large-magnitude input leaves the reused workspace buffers dirty.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

STD = 0.01  # the upstream init: conv_post stays far from tanh's saturation, so a wrong tail row is not rounded away (test 1 asserts it)
V1_LENS = [40, 23, 1, 16]


def _config(spec):
    from everyvoice_amd.config import HiFiGANConfig

    spec = dict(spec)
    audio = dict(n_mels=spec.pop("n_mels", 80))
    top = {k: spec.pop(k) for k in ("gen_istft_n_fft", "gen_istft_hop_size") if k in spec}
    return HiFiGANConfig(model=spec, preprocessing=dict(audio=audio), **top)


_GENS: dict = {}
_SOLO: dict = {}


def _gen(name, spec, device, precision="bf16"):
    """One seeded generator per (configuration, precision), shared by the tests."""
    from everyvoice_amd.vocoder import Generator

    key = (name, precision)
    if key not in _GENS:
        torch.manual_seed(77)
        g = Generator(_config(spec), precision=precision)
        g.reset_parameters(std=STD)
        _GENS[key] = g.to(device).eval()
    return _GENS[key]


def _mel(gen, B, T, device, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (1.5 * torch.randn(B, gen.config.preprocessing.audio.n_mels, T, generator=g)).to(device)  # padding frames included


def _dirty(gen, B, T, device):
    gen(50.0 * _mel(gen, B, T, device, seed=99))


def _solo(key, gen, mel, i, n):
    """Item i alone at n frames; computed once per (generator, mel, item, length) and left unchanged."""
    k = (key, tuple(mel.shape), i, n)
    if k not in _SOLO:
        _SOLO[k] = gen(mel[i : i + 1, :, :n].contiguous())[0, 0].clone()
    return _SOLO[k]


def _where(gen, mel, lens, i, t):
    """Where sample t of item i falls: its frame, and its row in every stage's sequence with the kernels that ran on that stage."""
    hop = gen.hop
    _, recs = gen.forward_profiled(mel, lens=lens)
    m = gen.config.model
    nk = len(m.resblock_kernel_sizes)
    lines, per = [f"sample {t} = frame {t // hop} + {t % hop} of item {i}"], 1
    for s, u in enumerate(m.upsample_rates):
        per *= u
        layers = [f"ups.{s}"] + [f"resblocks.{n}." for n in range(s * nk, (s + 1) * nk)]
        kernels = sorted({r["kernel"] for r in recs if any(r["layer"].startswith(p) for p in layers)})
        lines.append(f"stage {s}: row {t * per // hop} ({per} rows per frame), kernels {kernels}")
    lines.append(f"output: {[r['kernel'] for r in recs if r['layer'].startswith('conv_post')]}")
    return "; ".join(lines)


def _assert_ragged_equals_solo(key, gen, mel, lens, device, out=None):
    B, _, T = mel.shape
    hop = gen.hop
    if out is None:
        _dirty(gen, B, T, device)
        out = gen(mel, lens=torch.tensor(lens))
    assert out.shape == (B, 1, T * hop)
    for i, n in enumerate(lens):
        got = out[i, 0, : n * hop]
        if n:
            want = _solo(key, gen, mel, i, n)
            if not torch.equal(got, want):
                t = int((got != want).nonzero()[0])
                pytest.fail(f"item {i} (length {n} of {T}) differs from the item alone, first at {_where(gen, mel, torch.tensor(lens), i, t)}: "
                            f"{float(got[t])!r} != {float(want[t])!r}; {int((got != want).sum())} samples differ")
        tail = out[i, 0, n * hop :]
        assert not tail.any(), f"item {i}: {int((tail != 0).sum())} non-zero samples beyond its length"
    return out


# ---- 1. solo equality on V1, every kernel family of the flagship -----------------------------------------------------------------
def test_v1_items_equal_their_solo_runs_to_the_bit(cuda_device):
    gen = _gen("v1", {}, cuda_device)
    mel = _mel(gen, 4, 40, cuda_device)
    _assert_ragged_equals_solo("v1", gen, mel, V1_LENS, cuda_device)
    # the kernels this is about ran: LDS-DMA convolutions, the 128-channel chunked pair, the 64 / 32-channel pairs and branches
    _, recs = gen.forward_profiled(mel, lens=torch.tensor(V1_LENS))
    kernels = {r["kernel"] for r in recs}
    for prefix in ("conv_tc_dma<", "conv_tc_mfma<", "resblock_pair_mfma<c128", "resblock_pair_mfma<c64", "resblock_pair_mfma<c32",
                   "resblock_branch_mfma<", "conv_post_tanh"):
        assert any(k.startswith(prefix) for k in kernels), (prefix, sorted(kernels))
    # the inputs exercise the gap: run as a rectangle, item 1 ends on what the layers made of the padding frames
    hop, n = gen.hop, V1_LENS[1]
    rect = gen(mel)
    assert not torch.equal(rect[1, 0, (n - 1) * hop : n * hop], _solo("v1", gen, mel, 1, n)[(n - 1) * hop :])


# ---- 2. item ends around the tile seams -----------------------------------------------------------------------------------------
def test_item_ends_one_row_before_on_and_after_the_tile_seams(cuda_device):
    # first stage: u = 8, so 15 / 16 / 17 frames end at rows 120 / 128 / 136 and 31 / 32 / 33 at 248 / 256 / 264: around the 128-row
    # and 256-row tile boundaries, and the corresponding seams of the later stages
    gen = _gen("v1", {}, cuda_device)
    mel = _mel(gen, 6, 33, cuda_device, seed=6)
    _assert_ragged_equals_solo("v1", gen, mel, [15, 16, 17, 31, 32, 33], cuda_device)


# ---- 3. every kernel family -----------------------------------------------------------------------------------------------------
def _family_cases():
    from test_gpu_generator_configs import CONFIGS as GEN
    from test_gpu_istft_configs import CONFIGS as ISTFT
    from test_gpu_istft_configs import MUST_RUN

    def pairs_only(r):
        # a branch needs three dilations: with two, every ResBlock1 of V1 runs as pairs -- also the c64-k3, c32-k3 and c32-k7 blocks,
        # whose ragged pair instantiations the branch kernels otherwise keep any generator test from reaching
        names = {x["kernel"] for x in r}
        return not any(k.startswith("resblock_branch_mfma<") for k in names) and all(
            any(k.startswith(p) for k in names) for p in ("resblock_pair_mfma<c64,k3", "resblock_pair_mfma<c32,k3", "resblock_pair_mfma<c32,k7"))

    return {
        "pairs_only": (dict(resblock_dilation_sizes=[[1, 3], [1, 3], [1, 3]]), pairs_only),
        "v2_generic_conv": (GEN["v2"], lambda r: any(x["kernel"].startswith("conv_tc_generic") for x in r)),
        "resblock2": (GEN["v3"], lambda r: not any(x["kernel"].startswith("resblock_") for x in r) and any(x["layer"].startswith("resblocks.") for x in r)),
        "upsampler_k_not_2u": (GEN["odd1"], lambda r: all(x["kernel"].startswith("conv_tc_generic") for x in r if x["layer"].startswith("ups."))),
        "istft_16_4_specialised": (MUST_RUN["v2_width_c8c8i_32ch"], lambda r: [x["kernel"] for x in r if x["layer"] == "conv_post+istft"] == ["istft_head"]),
        "istft_8_2_generic": (ISTFT["c8c8c2i_8_2"], lambda r: [x["kernel"][:18] for x in r if x["layer"] == "conv_post+istft"] == ["istft_head_generic"]),
        "istft_12_5_generic": (ISTFT["odd_12_5"], lambda r: [x["kernel"][:18] for x in r if x["layer"] == "conv_post+istft"] == ["istft_head_generic"]),
    }


@pytest.mark.parametrize("name", ["pairs_only", "v2_generic_conv", "resblock2", "upsampler_k_not_2u", "istft_16_4_specialised", "istft_8_2_generic",
                                  "istft_12_5_generic"])
def test_every_kernel_family(cuda_device, name):
    spec, intended_kernel_ran = _family_cases()[name]
    gen = _gen(name, spec, cuda_device)
    lens = [24, 9, 2]
    mel = _mel(gen, 3, 24, cuda_device, seed=8)
    _assert_ragged_equals_solo(name, gen, mel, lens, cuda_device)
    _, recs = gen.forward_profiled(mel, lens=torch.tensor(lens))
    assert intended_kernel_ran(recs), sorted({(r["layer"], r["kernel"]) for r in recs})


# ---- 4. full lengths ------------------------------------------------------------------------------------------------------------
def test_full_lengths_equal_the_forward_without_lens(cuda_device):
    gen = _gen("v1", {}, cuda_device)
    mel = _mel(gen, 4, 40, cuda_device)
    _dirty(gen, 4, 40, cuda_device)
    assert torch.equal(gen(mel, lens=torch.tensor([40] * 4)), gen(mel))


# ---- 5. graph replay ------------------------------------------------------------------------------------------------------------
def test_a_captured_forward_follows_the_lengths_in_device_memory(cuda_device):
    gen = _gen("v1", {}, cuda_device)
    mel = _mel(gen, 4, 40, cuda_device)
    dev_lens = torch.tensor(V1_LENS, dtype=torch.int32, device=cuda_device)
    gen(mel, lens=dev_lens)  # workspace and kernel attributes exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one capture stream: no parallel branches
        out = gen(mel, lens=dev_lens)
    for lens in (V1_LENS, [16, 40, 23, 1], [7, 7, 39, 40]):
        dev_lens.copy_(torch.tensor(lens, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        _assert_ragged_equals_solo("v1", gen, mel, lens, cuda_device, out=out)


# ---- 6. zero length, lengths out of range ---------------------------------------------------------------------------------------
def test_a_zero_length_gives_a_zero_row_and_leaves_the_others(cuda_device):
    gen = _gen("v1", {}, cuda_device)
    mel = _mel(gen, 4, 40, cuda_device)
    _dirty(gen, 4, 40, cuda_device)
    out = gen(mel, lens=torch.tensor([40, 0, 1, 16], dtype=torch.int32, device=cuda_device))
    _assert_ragged_equals_solo("v1", gen, mel, [40, 0, 1, 16], cuda_device, out=out)
    # the clamp is the kernel's: a negative length is a zero row, one beyond T is T
    out = gen(mel, lens=torch.tensor([1000, -3, 1, 16], dtype=torch.int32, device=cuda_device))
    _assert_ragged_equals_solo("v1", gen, mel, [40, 0, 1, 16], cuda_device, out=out)


# ---- 7. the fp32 precisions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f32-direct"])
def test_fp32_precisions_equal_the_solo_runs(cuda_device, precision):
    gen = _gen("v1", {}, cuda_device, precision=precision)
    mel = _mel(gen, 3, 24, cuda_device, seed=8)
    _assert_ragged_equals_solo("v1-" + precision, gen, mel, [24, 9, 2], cuda_device)


# ---- 8. synthesis ---------------------------------------------------------------------------------------------------------------
def test_synthesis_with_masked_vocoder_padding_equals_from_spec(cuda_device, tmp_path):
    from everyvoice_amd.config import HiFiGANConfig
    from everyvoice_amd.fs2 import FastSpeech2, FastSpeech2ModelConfig
    from everyvoice_amd.pipeline import synthesize_from_spec, synthesize_helper
    from everyvoice_amd.vocoder import HiFiGANGenerator

    model = FastSpeech2(FastSpeech2ModelConfig(), device=cuda_device).init_random(3)
    model.duration_predictor.b_lin.fill_(1.0)  # a few frames per token instead of the zeros a random duration predictor gives
    torch.manual_seed(78)
    voc = HiFiGANGenerator(HiFiGANConfig())
    voc.generator.reset_parameters(std=STD)
    voc = voc.to(cuda_device).eval()
    texts = [[3, 4, 5, 6, 7, 8, 9, 10, 11], [9, 10, 11]]

    def run(out, **kw):
        _, _, preds, _ = synthesize_helper(model, texts, None, None, 1.0, 0, ["wav", "spec"], output_dir=tmp_path / out, vocoder_model=voc, **kw)
        assert len(preds) == 2 and preds[0]["frames"] != preds[1]["frames"]
        return preds

    masked = run("masked", mask_vocoder_padding=True)
    for j, p in enumerate(masked):
        solo = synthesize_from_spec(torch.load(p["spec"]), voc, tmp_path / "from_spec", f"item{j}")
        with open(p["wav"], "rb") as a, open(solo, "rb") as b:
            assert a.read() == b.read(), f"item {j} ({p['frames']} frames)"
    plain, off = run("plain"), run("off", mask_vocoder_padding=False)
    for p, q in zip(plain, off):
        with open(p["wav"], "rb") as a, open(q["wav"], "rb") as b:
            assert a.read() == b.read()
        assert torch.equal(torch.load(p["spec"]), torch.load(q["spec"]))
