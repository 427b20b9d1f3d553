"""ctypes binding of libevmi_hip.so, derived from include/evmi.h: the header is the one description of the C ABI.

Importing this module reads the header once: its constants become module attributes (EVMI_OK, EVMI_ERR_*, EVMI_PREC_*, EVMI_MAX_*,
EVMI_ABI_VERSION) and every function it declares gets its restype / argtypes in SYMBOLS.  Only the six structs that Python fills or
reads field by field are mirrored by hand (tests/test_header_binding.py holds them to the header).

There is NO fallback: if the header or the shared library is missing or a symbol is absent, importing the compute modules fails
loudly -- the product never silently runs a CPU or eager-PyTorch path, and never binds from a table of its own.
"""

from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path
from typing import NamedTuple

_HERE = Path(__file__).resolve().parent
LIB_NAME = "libevmi_hip.so"
HEADER = _HERE.parent / "include" / "evmi.h"


class EvmiError(RuntimeError):
    """A libevmi_hip call returned a non-zero status."""


# ---- the header ----------------------------------------------------------------------------------------------------------------------
class Header(NamedTuple):
    constants: dict     # name -> int: the members of the enums and the integer #defines
    structs: dict       # name -> [(C type, member, [extents])] of every struct defined with a body
    declarations: list  # [(name, return C type, [(parameter C type, parameter name)])] in the header's order


_FUNCTION = re.compile(r"([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_DECLARATOR = re.compile(r"(\w+)((?:\s*\[\s*\w+\s*\])*)")


def _c_type(text: str) -> str:
    """'const  float *const *' -> 'const float* const*'."""
    return re.sub(r"\s+\*", "*", " ".join(text.replace("*", "* ").split()))


def _typed_name(text: str, where: str):
    """'const float* x_dev' -> ('const float*', 'x_dev', ''); a struct member may carry extents: 'char kernel[48]'."""
    m = re.fullmatch(r"(.*[\s*])" + _DECLARATOR.pattern, text.strip(), flags=re.S)
    if not m:
        raise ValueError(f"{where}: cannot read {' '.join(text.split())!r} as a type and a name")
    return _c_type(m.group(1)), m.group(2), m.group(3)


def parse_header(text: str) -> Header:
    """Reads the subset of C that include/evmi.h is written in.  Anything else raises: the parser never guesses and never skips."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {name: int(value) for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)

    def enum(m):
        for item in filter(None, (" ".join(i.split()) for i in m.group(1).split(","))):
            im = re.fullmatch(r"(\w+) = (-?\d+)", item)
            if not im:
                raise ValueError(f"enum member {item!r}: only `NAME = integer` is read")
            constants[im.group(1)] = int(im.group(2))
        return " "

    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)

    def extent(e, where):
        if not (e.isdigit() or e in constants):
            raise ValueError(f"{where}: unknown array extent {e!r}")
        return int(e) if e.isdigit() else constants[e]

    structs = {}

    def struct(m):
        members, name = [], m.group(2)
        for line in filter(None, (s.strip() for s in m.group(1).split(";"))):
            ctype = None
            for d in line.split(","):  # `int c_in, c_out;`: the later declarators repeat the first one's type
                if ctype and "*" in ctype:
                    raise ValueError(f"struct {name}: {line!r}: one pointer member per declaration")
                ctype, member, extents = _typed_name(f"{ctype} {d}" if ctype else d, f"struct {name}")
                members.append((ctype, member, [extent(e, f"{name}.{member}") for e in re.findall(r"\w+", extents)]))
        structs[name] = members
        return " "

    text = _STRUCT.sub(struct, text)
    text = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", " ", text)  # opaque handles
    declarations = []

    def function(m):
        name = m.group(2)
        params = [] if m.group(3).strip() in ("", "void") else [_typed_name(p, name) for p in m.group(3).split(",")]
        if any(extents for _, _, extents in params):
            raise ValueError(f"{name}: array parameters are not read")
        declarations.append((name, _c_type(m.group(1)), [p[:2] for p in params]))
        return " "

    rest = re.sub(r'extern\s+"C"\s*\{', " ", _FUNCTION.sub(function, text)).split()
    if rest not in ([], ["}"]):
        raise ValueError(f"not read as a declaration: {' '.join(rest)[:200]!r}")
    return Header(constants, structs, declarations)


def _read_header() -> Header:
    if not HEADER.exists():
        raise ImportError(f"{HEADER} not found: the ctypes binding is derived from it and there is no built-in table.")
    return parse_header(HEADER.read_text())


_HEADER = _read_header()  # once per process
_K = _HEADER.constants
globals().update(_K)  # EVMI_OK, EVMI_ERR_*, EVMI_PREC_*, EVMI_MAX_*, EVMI_ABI_VERSION as module attributes


def declarations() -> list:
    """Every function include/evmi.h declares: [(name, return C type, [(parameter C type, parameter name)])]."""
    return _HEADER.declarations


def struct_members() -> dict:
    """Every struct include/evmi.h defines: name -> [(C type, member, [array extents])]."""
    return _HEADER.structs


# ---- the structs Python fills or reads by field -----------------------------------------------------------------------------------
class GeneratorConfig(C.Structure):
    _fields_ = [
        ("n_mels", C.c_int),
        ("upsample_initial_channel", C.c_int),
        ("num_upsamples", C.c_int),
        ("upsample_rates", C.c_int * _K["EVMI_MAX_UPSAMPLES"]),
        ("upsample_kernel_sizes", C.c_int * _K["EVMI_MAX_UPSAMPLES"]),
        ("resblock_type", C.c_int),
        ("num_kernels", C.c_int),
        ("resblock_kernel_sizes", C.c_int * _K["EVMI_MAX_RESBLOCK_KERNELS"]),
        ("num_dilations", C.c_int * _K["EVMI_MAX_RESBLOCK_KERNELS"]),
        ("resblock_dilations", (C.c_int * _K["EVMI_MAX_DILATIONS"]) * _K["EVMI_MAX_RESBLOCK_KERNELS"]),
        ("lrelu_slope", C.c_float),
        ("post_lrelu_slope", C.c_float),
        ("istft_layer", C.c_int),
        ("istft_n_fft", C.c_int),
        ("istft_hop", C.c_int),
    ]


class LaunchRecord(C.Structure):
    _fields_ = [
        ("kernel", C.c_char * 48),
        ("layer", C.c_char * 48),
        ("ms", C.c_float),
        ("flops", C.c_double),
        ("bytes", C.c_double),
    ]


class PkFlatJob(C.Structure):  # evmi_pkflat_job
    _fields_ = [("mode", C.c_int), ("c_in", C.c_int), ("c_out", C.c_int), ("k", C.c_int), ("stride", C.c_int), ("groups", C.c_int),
                ("w", C.c_void_p), ("wf", C.c_void_p), ("wf_elems", C.c_longlong)]


class PkFlatPair(C.Structure):  # evmi_pkflat_pair
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("units", C.c_longlong), ("plane", C.c_longlong), ("rows", C.c_int), ("scale", C.c_float)]


class PkFlatRows(C.Structure):  # evmi_pkflat_rows
    _fields_ = [("dy", C.c_void_p), ("plane", C.c_longlong), ("units", C.c_longlong), ("C", C.c_int), ("db", C.c_void_p)]


class LnPartials(C.Structure):  # evmi_ln_partials
    _fields_ = [("ws", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("C", C.c_int), ("n_cols", C.c_longlong)]


MIRRORS = {"evmi_generator_config": GeneratorConfig, "evmi_launch_record": LaunchRecord, "evmi_pkflat_job": PkFlatJob,
           "evmi_pkflat_pair": PkFlatPair, "evmi_pkflat_rows": PkFlatRows, "evmi_ln_partials": LnPartials}

# ---- C types -> ctypes ------------------------------------------------------------------------------------------------------------
# A single pointer to a mirrored struct is POINTER(mirror); every other pointer is c_void_p, pointers to pointers and the opaque
# evmi_generator* included: the header cannot say whether an int* is a host out-parameter or a device buffer, so none is typed
# (c_void_p takes an address, None, byref(...) and a ctypes array alike).
C_TYPES = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
           "int64_t": C.c_int64, "char*": C.c_char_p}


def _ctypes_of(c_type: str, where: str, returned: bool = False):
    bare = " ".join(w for w in c_type.replace("*", " * ").split() if w != "const").replace(" *", "*")
    if bare in C_TYPES:
        return C_TYPES[bare]
    if bare == "void" and returned:
        return None
    if bare.endswith("*"):
        return C.POINTER(MIRRORS[bare[:-1]]) if bare[:-1] in MIRRORS else C.c_void_p
    raise TypeError(f"{where}: no ctypes type is given for the C type {c_type!r}")


def bind_types(decls) -> dict:
    """name -> (restype, argtypes) of the given declarations; a C type outside the table above raises, naming symbol and parameter."""
    return {name: (_ctypes_of(ret, f"{name}: return type", returned=True), [_ctypes_of(t, f"{name}: parameter {p}") for t, p in params])
            for name, ret, params in decls}


SYMBOLS = bind_types(declarations())  # name -> (restype, argtypes); every symbol include/evmi.h declares

_lib = None


def lib_path() -> Path:
    override = os.environ.get("EVMI_LIB")
    return Path(override) if override else _HERE / LIB_NAME


def load() -> C.CDLL:
    """Load the library once and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not path.exists():
        raise ImportError(
            f"{path} not found: build it with `make` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "everyvoice_amd has no CPU fallback."
        )
    lib = C.CDLL(str(path))
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.evmi_abi_version() != _K["EVMI_ABI_VERSION"]:
        raise ImportError(f"{path}: ABI version {lib.evmi_abi_version()} != {_K['EVMI_ABI_VERSION']} of {HEADER}")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != _K["EVMI_OK"]:
        msg = load().evmi_last_error()
        raise EvmiError(f"{what or 'libevmi_hip'} failed (code {rc}): {msg.decode() if msg else '?'}")


def ptr(t) -> int:
    """Device/host pointer of a torch tensor (None -> NULL)."""
    return 0 if t is None else t.data_ptr()


_raw_stream = None


def current_stream_ptr(device=None) -> int:
    """hipStream_t of torch's current stream on `device` (a torch.device, an index or None = the current device).  Every
    operator wrapper calls this once per launch: torch's raw accessor (no Stream object) costs a fraction of a microsecond
    where ``torch.cuda.current_stream(device).cuda_stream`` costs two to three."""
    global _raw_stream
    import torch

    if _raw_stream is None:
        _raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", False)
    if not _raw_stream:
        return torch.cuda.current_stream(device).cuda_stream
    idx = device if isinstance(device, int) else (None if device is None else device.index)
    if idx is None:
        idx = torch.cuda.current_device()
    return _raw_stream(idx)
