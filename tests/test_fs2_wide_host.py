"""Host side of FastSpeech2 at Conformer widths above 256 channels; no GPU needed.

The bound on ``input_dim`` where the configuration is read (1024: the widest column the LayerNorm kernels normalise), the argument
refusals of the LayerNorm backward and of LayerNorm written as a packed input (host pointers, never dereferenced: a refusal behind a
launch would end in EVMI_ERR_HIP on a machine without a device), the backward's workspace formula, and a private segment of zero
bytes in every LayerNorm backward / pack instantiation, checked as tests/test_attention_generic_host.py checks its file."""

import re
import subprocess
from pathlib import Path

import pytest
import torch

from everyvoice_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
INVALID_ARG, UNSUPPORTED = 1, _lib.EVMI_ERR_UNSUPPORTED

_BUF = torch.zeros(64)  # 64-byte aligned host memory standing in for every device pointer
P = _BUF.data_ptr()
assert P % 16 == 0


def _config(d, heads):
    from everyvoice_amd.fs2 import FastSpeech2ModelConfig

    c = FastSpeech2ModelConfig()
    for part in (c.encoder, c.decoder):
        part.input_dim, part.heads = d, heads
    return c


@pytest.mark.parametrize("d,heads", [(2048, 8), (1026, 6)])
def test_a_width_above_the_layernorm_kernels_is_refused_where_the_configuration_is_read(d, heads):
    """Head dimensions 256 and 171: every other rule of check_conformer_widths holds, only the width itself is too large."""
    from everyvoice_amd.fs2 import FastSpeech2ModelConfig, check_conformer_widths

    with pytest.raises(ValueError, match=re.escape("model.encoder.input_dim")):
        check_conformer_widths(_config(d, heads))
    c = FastSpeech2ModelConfig()
    c.decoder.input_dim, c.decoder.heads = d, heads
    with pytest.raises(ValueError, match=re.escape("model.decoder.input_dim")):
        check_conformer_widths(c)


@pytest.mark.parametrize("d,heads", [(1024, 4), (768, 3)])
def test_the_widest_widths_pass_the_check(d, heads):
    from everyvoice_amd.fs2 import check_conformer_widths

    check_conformer_widths(_config(d, heads))


def _refused(name, args, code, says):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == code, f"{name}{args}: returned {rc} ({msg!r}), wanted {code}"
    assert says in msg, f"{name}: evmi_last_error() = {msg!r} does not name the entry point ({says!r})"


@pytest.mark.parametrize("C", [1025, 0])
def test_layernorm_backward_refuses_a_width_outside_1_to_1024_before_any_launch(C):
    n = 1 << 20  # (a workspace size that is large enough for either width: the refusal is the width's)
    _refused("evmi_layernorm_bwd_cbt_f32", (P, P, P, P, P, P, P, n, C, 65, 1e-5, 0, None), INVALID_ARG, "layernorm_bwd")
    jobs = (_lib.LnPartials * 1)()
    jobs[0].ws, jobs[0].dgamma, jobs[0].dbeta, jobs[0].C, jobs[0].n_cols = P, P, P, C, 65
    _refused("evmi_layernorm_bwd_partials_reduce", (1, jobs, None), INVALID_ARG, "layernorm_bwd_partials_reduce")


@pytest.mark.parametrize("c_in", [272, 1056])
def test_layernorm_pack_refuses_a_width_that_is_no_multiple_of_32_or_above_1024(c_in):
    _refused("evmi_layernorm_pack_bf16pk", (P, P, P, P, 1 << 24, 1, c_in, 64, 2 * c_in, 1e-5, None), UNSUPPORTED, "layernorm_pack_bf16pk")


def test_layernorm_backward_workspace_is_two_rows_of_c_per_64_columns():
    lib = _lib.load()
    assert lib.evmi_layernorm_bwd_cbt_f32_ws_elems(1024, 65) == 2 * 2 * 1024
    assert lib.evmi_layernorm_bwd_cbt_f32_ws_elems(384, 64) == 2 * 384
    assert lib.evmi_layernorm_bwd_cbt_f32_ws_elems(256, 130) == 3 * 2 * 256  # (the formula did not change)


# ---- static rule on the compiled kernels --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    """The compiler's resource remarks of csrc/fs2_train_ops.hip and csrc/conv_cbt_bf16_pk.hip for gfx950 (compiled side by side)."""
    hipcc = Path("/opt/rocm/bin/hipcc")
    if not hipcc.exists():
        pytest.skip("hipcc not found")
    tmp = tmp_path_factory.mktemp("layernorm_wide")
    procs = []
    for stem in ("fs2_train_ops", "conv_cbt_bf16_pk"):
        cmd = [str(hipcc), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT / 'include'}", f"-I{ROOT / 'everyvoice_amd' / 'csrc'}",
               "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", "-o", str(tmp / f"{stem}.s"),
               str(ROOT / "everyvoice_amd" / "csrc" / f"{stem}.hip")]
        procs.append(subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
    out = []
    for p in procs:
        _, err = p.communicate(timeout=1800)
        assert p.returncode == 0, err[-2000:]
        out.append(err)
    return "\n".join(out)


def test_no_layernorm_backward_or_pack_kernel_uses_scratch_memory(remarks):
    """Every instantiation, the ones for 256 < C <= 1024 among them: ScratchSize 0 bytes per lane and no spilled vector register."""
    names = re.findall(r"remark: Function Name: (\S+)", remarks)
    scratch = [int(v) for v in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    spills = [int(v) for v in re.findall(r"remark:\s+VGPRs Spill: (\d+)", remarks)]
    assert len(names) == len(scratch) == len(spills)
    found = {n: (s, v) for n, s, v in zip(names, scratch, spills) if "layernorm_bwd_cbt" in n or "layernorm_pack" in n}
    # the three narrow backward forms + <32, 16> + the re-reading form; the two narrow pack forms + the two wide ones
    assert sum("layernorm_bwd_cbt_kernel" in n for n in found) == 4 and sum("layernorm_bwd_cbt_wide_kernel" in n for n in found) == 1, sorted(found)
    assert sum("layernorm_pack_kernel" in n for n in found) == 2 and sum("layernorm_pack_wide_kernel" in n for n in found) == 2, sorted(found)
    bad = {n: sv for n, sv in found.items() if sv != (0, 0)}
    assert not bad, bad
