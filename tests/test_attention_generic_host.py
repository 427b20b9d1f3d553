"""Host side of the attention kernels for any head dimension up to 256 (csrc/attention_generic.hip); no GPU needed.

Argument refusals of the six entry points (host pointers, never dereferenced: a refusal behind a launch would end in EVMI_ERR_HIP on a
machine without a device), their declarations, the choice between the specialised and the generic entry points, the refusal of a
Conformer width where the configuration is read, and two static rules on the compiled kernels: the LDS-direct hand-over of
DESIGN.md 11.9 and a private segment of zero bytes in every instantiation."""

import ctypes
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from everyvoice_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

INVALID_ARG, UNSUPPORTED = 1, _lib.EVMI_ERR_UNSUPPORTED

_BUF = torch.zeros(64)  # host memory standing in for every device pointer
P = _BUF.data_ptr()

INFER = ("evmi_attention_generic_f32", "evmi_attention_generic_bf16")
FWD = ("evmi_mha_generic_fwd_f32", "evmi_mha_generic_fwd_bf16")
BWD = ("evmi_mha_generic_bwd_f32", "evmi_mha_generic_bwd_bf16")
COUNTERPART = {"evmi_attention_generic_f32": "evmi_attention_cbt_f32", "evmi_attention_generic_bf16": "evmi_attention_cbt_bf16",
               "evmi_mha_generic_fwd_f32": "evmi_mha_fwd_f32", "evmi_mha_generic_fwd_bf16": "evmi_mha_fwd_bf16",
               "evmi_mha_generic_bwd_f32": "evmi_mha_bwd_f32", "evmi_mha_generic_bwd_bf16": "evmi_mha_bwd_bf16"}


def _args(name, B=2, T=8, D=96, heads=2, p=0.0, null=None):
    """A valid argument list of `name` with host pointers; `null`: index of the pointer to pass as NULL."""
    n_ptr = 3 if name in INFER else 4 if name in FWD else 7
    ptrs = [0 if i == null else P for i in range(n_ptr)]
    tail = [None] if name in INFER else [p, 0, None, None]
    return (*ptrs, B, T, D, heads, *tail)


def _refused(name, args, code):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    msg = (lib.evmi_last_error() or b"").decode()
    assert rc == code, f"{name}{args}: returned {rc} ({msg!r}), wanted {code}"
    assert name[len("evmi_"):] in msg, f"{name}: evmi_last_error() = {msg!r} does not name the entry point"
    return msg


@pytest.mark.parametrize("name", INFER + FWD + BWD)
def test_generic_entry_points_refuse_before_any_launch(name):
    n_ptr = 3 if name in INFER else 4 if name in FWD else 7
    for i in range(n_ptr):
        _refused(name, _args(name, null=i), INVALID_ARG)
    for kw in (dict(B=0), dict(T=0), dict(D=0), dict(heads=0), dict(B=-1), dict(T=-3), dict(D=100, heads=3), dict(D=96, heads=5)):
        _refused(name, _args(name, **kw), INVALID_ARG)
    if name not in INFER:
        for p in (-0.1, 1.0, 1.5):
            _refused(name, _args(name, p=p), INVALID_ARG)
    assert "256" in _refused(name, _args(name, D=514, heads=2), UNSUPPORTED)   # head dimension 257
    assert "256" in _refused(name, _args(name, D=257, heads=1), UNSUPPORTED)
    assert "65535" in _refused(name, _args(name, B=65536), UNSUPPORTED)
    assert "65535" in _refused(name, _args(name, D=2 * 65536, heads=65536), UNSUPPORTED)


def test_generic_entry_points_are_declared_with_their_counterparts_arguments():
    """include/evmi.h declares the six symbols; parameter by parameter they match _lib.py's ctypes table, which gives each the argument
    list of the specialised entry point it generalises."""
    header = {n: (ret, params) for n, ret, params in _lib.declarations()}
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "unsigned long long": ctypes.c_ulonglong}
    for name, other in COUNTERPART.items():
        assert name in header, f"{name} is not declared in include/evmi.h"
        ret, params = header[name]
        assert ret == "int"
        declared = [ctypes.c_void_p if "*" in t else ctype[t] for t, _ in params]
        restype, argtypes = _signature(name)
        assert restype is ctypes.c_int and list(argtypes) == declared, (name, argtypes, declared)
        assert list(_signature(other)[1]) == list(argtypes), (name, other)
        assert hasattr(_lib.load(), name)


def _signature(name):
    fn = getattr(_lib.load(), name)
    return fn.restype, fn.argtypes


def test_dispatch_picks_the_specialised_entry_points_exactly_at_32_64_128():
    from everyvoice_amd.train import ops

    stems = {"infer": ("evmi_attention_cbt", "evmi_attention_generic"), "fwd": ("evmi_mha_fwd", "evmi_mha_generic_fwd"),
             "bwd": ("evmi_mha_bwd", "evmi_mha_generic_bwd")}
    for kind, (specialised, generic) in stems.items():
        for operands in ("f32", "bf16"):
            for dh in range(1, 257):
                want = (specialised if dh in (32, 64, 128) else generic) + "_" + operands
                assert ops.attention_entry(kind, dh, operands) == want
                assert hasattr(_lib.load(), want)
    with ops.mode(operands="bf16"):  # the default follows the operand mode, as the call sites did
        assert ops.attention_entry("fwd", 48) == "evmi_mha_generic_fwd_bf16" and ops.attention_entry("fwd", 64) == "evmi_mha_fwd_bf16"
    assert ops.attention_entry("infer", 192) == "evmi_attention_generic_f32"


def _config(**changes):
    from everyvoice_amd.fs2 import FastSpeech2ModelConfig

    c = FastSpeech2ModelConfig()
    for key, value in changes.items():
        part, field = key.split("__")
        setattr(getattr(c, part), field, value)
    return c


BAD_WIDTHS = [
    (dict(encoder__input_dim=255), "model.encoder.input_dim"),                       # odd
    (dict(decoder__input_dim=101, decoder__heads=1), "model.decoder.input_dim"),
    (dict(encoder__input_dim=100, encoder__heads=3), "model.encoder.heads"),         # 100 % 3
    (dict(decoder__input_dim=100, decoder__heads=3), "model.decoder.heads"),
    (dict(encoder__input_dim=1024, encoder__heads=2), "model.encoder.heads"),        # head dimension 512
    (dict(decoder__input_dim=1024, decoder__heads=2), "model.decoder.heads"),
]


@pytest.mark.parametrize("changes,field", BAD_WIDTHS)
def test_a_width_the_kernels_do_not_run_is_refused_at_construction(changes, field):
    """ValueError naming the field from the model, the trainer and lightning.FastSpeech2Config -- in front of the device check, so a CPU
    device gets this far -- and from the check function itself."""
    from everyvoice_amd.fs2 import FastSpeech2, check_conformer_widths
    from everyvoice_amd.lightning import FastSpeech2Config
    from everyvoice_amd.train.fs2 import FastSpeech2Trainer

    with pytest.raises(ValueError, match=re.escape(field)):
        check_conformer_widths(_config(**changes))
    with pytest.raises(ValueError, match=re.escape(field)):
        FastSpeech2(_config(**changes), device="cpu")
    with pytest.raises(ValueError, match=re.escape(field)):
        FastSpeech2Trainer(_config(**changes), device="cpu")
    with pytest.raises(ValueError, match=re.escape(field)):
        FastSpeech2Config(model=_config(**changes))


def test_the_widths_people_choose_pass_the_check():
    from everyvoice_amd.fs2 import check_conformer_widths

    for d, heads in ((384, 2), (384, 4), (512, 2), (192, 4), (256, 1), (256, 2), (64, 2), (96, 2), (192, 1), (200, 2)):
        check_conformer_widths(_config(encoder__input_dim=d, encoder__heads=heads, decoder__input_dim=d, decoder__heads=heads))


# ---- static rules on the compiled kernels -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """(path of the gfx950 assembly of attention_generic.hip, the compiler's resource remarks)"""
    hipcc = Path("/opt/rocm/bin/hipcc")
    if not hipcc.exists():
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("attention_generic") / "attention_generic.s"
    r = subprocess.run([str(hipcc), "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT / 'include'}", f"-I{ROOT / 'everyvoice_amd' / 'csrc'}",
                        "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", "-o", str(out),
                        str(ROOT / "everyvoice_amd" / "csrc" / "attention_generic.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return out, r.stderr


def test_generic_lds_direct_tiles_are_handed_over_behind_a_vmcnt_wait(compiled):
    """The rule of tests/test_isa_rules.py on the new file: a loop header that runs into an s_barrier waits vmcnt(0) first."""
    from isa_scan import lds_dma_handover_findings

    path, _ = compiled
    assert "global_load_lds" in path.read_text()  # (the rule looks at something)
    bad = lds_dma_handover_findings(path)
    assert not bad, bad[:3]


def test_no_generic_kernel_uses_scratch_memory(compiled):
    """Every instantiation: ScratchSize 0 bytes per lane and no spilled register in the compiler's resource remarks.  (Their LDS is
    dynamic and does not show here: the launches of the 256-wide kernels in tests/test_gpu_attention_generic.py ask for the largest sizes.)"""
    _, remarks = compiled
    names = re.findall(r"remark: Function Name: (\S+)", remarks)
    scratch = [int(v) for v in re.findall(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    spills = [int(v) for v in re.findall(r"remark:\s+VGPRs Spill: (\d+)", remarks)]
    kernels = [n for n in names if "attention_generic" in n]
    # 6 padded head dimensions x (3 fp32 kernels + 3 bf16 kernels x 3 dropout forms)
    assert len(kernels) == 6 * (3 + 3 * 3) and len(names) == len(scratch) == len(spills), (len(kernels), len(names), len(scratch))
    bad = [(n, s, v) for n, s, v in zip(names, scratch, spills) if s or v]
    assert not bad, bad
