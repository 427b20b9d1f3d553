"""The ctypes binding is derived from include/evmi.h (everyvoice_amd/_lib.py): the parser on small headers written here, the table it
gives for the real header, and the six hand-written struct mirrors against the header's struct definitions.  Host only."""

import ctypes as C

import pytest

from everyvoice_amd import _lib

SMALL = """
/* a comment with ( and ) and ; inside: int evmi_not_a_function(int x); */
#ifndef X_H
#define X_H
#define EVMI_N 3   // trailing (comment);
enum { EVMI_A = 0, EVMI_B = 7 /* seven; */ };
typedef struct evmi_generator evmi_generator; /* opaque */
typedef struct evmi_launch_record {
  char kernel[48]; /* name (kernel) */
  int  grid[EVMI_N][2];
  long long a, b;
  const float* w;
} evmi_launch_record;
int evmi_none(void);
const char* evmi_text(void);
void evmi_free(evmi_generator* g);
// int evmi_commented_out(int a);
long long evmi_spread(const float* x_dev,
                      int   B,   /* batch (items); */
                      unsigned long long seed,
                      void* stream);
int evmi_tables(const float* const* bias_dev, const void *const *w_laid, evmi_generator** out, const evmi_launch_record* recs,
                char* name, int64_t* numel, double scale);
#endif
"""


def test_parser_reads_the_shapes_the_header_uses():
    h = _lib.parse_header(SMALL)
    assert h.constants == {"EVMI_N": 3, "EVMI_A": 0, "EVMI_B": 7}
    assert h.structs == {"evmi_launch_record": [("char", "kernel", [48]), ("int", "grid", [3, 2]), ("long long", "a", []), ("long long", "b", []),
                                                ("const float*", "w", [])]}
    assert h.declarations == [
        ("evmi_none", "int", []),
        ("evmi_text", "const char*", []),
        ("evmi_free", "void", [("evmi_generator*", "g")]),
        ("evmi_spread", "long long", [("const float*", "x_dev"), ("int", "B"), ("unsigned long long", "seed"), ("void*", "stream")]),
        ("evmi_tables", "int", [("const float* const*", "bias_dev"), ("const void* const*", "w_laid"), ("evmi_generator**", "out"),
                                ("const evmi_launch_record*", "recs"), ("char*", "name"), ("int64_t*", "numel"), ("double", "scale")]),
    ]
    assert _lib.bind_types(h.declarations) == {
        "evmi_none": (C.c_int, []),
        "evmi_text": (C.c_char_p, []),
        "evmi_free": (None, [C.c_void_p]),
        "evmi_spread": (C.c_longlong, [C.c_void_p, C.c_int, C.c_ulonglong, C.c_void_p]),
        "evmi_tables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_lib.LaunchRecord), C.c_char_p, C.c_void_p, C.c_double]),
    }


@pytest.mark.parametrize("decl, names", [
    ("int evmi_short(const float* x_dev, short n);", ("evmi_short", "n", "short")),      # a scalar the table does not hold
    ("size_t evmi_sized(int n);", ("evmi_sized", "return", "size_t")),
    ("int evmi_by_value(evmi_launch_record rec);", ("evmi_by_value", "rec", "evmi_launch_record")),
    ("int evmi_void_param(void x);", ("evmi_void_param", "x", "void")),
])
def test_an_unknown_type_raises_and_names_symbol_and_parameter(decl, names):
    with pytest.raises(TypeError) as e:
        _lib.bind_types(_lib.parse_header(decl).declarations)
    assert all(n in str(e.value) for n in names), str(e.value)


@pytest.mark.parametrize("text, says", [
    ("int evmi_unnamed(int, float x);", "evmi_unnamed"),                  # a parameter without a name
    ("int evmi_array(int dil[3]);", "evmi_array"),
    ("int evmi_callback(void (*fn)(int), int n);", "not read"),           # nothing is skipped: what is left over is an error
    ("static const int evmi_table_size = 4;", "not read"),
    ("enum { EVMI_IMPLICIT, EVMI_NEXT };", "EVMI_IMPLICIT"),
    ("typedef struct { int n[EVMI_UNKNOWN]; } evmi_s;", "EVMI_UNKNOWN"),
    ("typedef struct { float *a, *b; } evmi_s;", "evmi_s"),
])
def test_what_the_parser_does_not_read_is_an_error(text, says):
    with pytest.raises(ValueError, match=says):
        _lib.parse_header(text)


# ---- the real header ----------------------------------------------------------------------------------------------------------------
def test_the_header_gives_the_whole_table():
    decls = _lib.declarations()
    names = [name for name, _, _ in decls]
    assert len(decls) >= 212 and len(set(names)) == len(names) and all(n.startswith("evmi_") for n in names)
    assert _lib.SYMBOLS == _lib.bind_types(decls) and list(_lib.SYMBOLS) == names
    scalars = {C.c_int, C.c_float, C.c_double, C.c_longlong, C.c_ulonglong, C.c_int64}
    pointers = {C.c_void_p, C.c_char_p} | {C.POINTER(m) for m in _lib.MIRRORS.values()}
    for name, (restype, argtypes) in _lib.SYMBOLS.items():
        assert restype in scalars | {None, C.c_char_p}, name
        assert all(t in scalars | pointers for t in argtypes), name
    for name, _, params in decls:  # a parameter called `stream` is the void* of the header's conventions
        assert [t for t, p in params if p == "stream"] in ([], ["void*"]), name


def test_spot_pins():
    S = _lib.SYMBOLS
    assert S["evmi_abi_version"] == (C.c_int, []) and S["evmi_last_error"] == (C.c_char_p, [])
    assert S["evmi_generator_destroy"] == (None, [C.c_void_p])
    assert S["evmi_generator_workspace_bytes"] == (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int])
    assert S["evmi_generator_macs_per_sample"] == (C.c_double, [C.c_void_p])
    assert S["evmi_generator_create"] == (C.c_int, [C.POINTER(_lib.GeneratorConfig), C.c_int, C.c_void_p])
    assert S["evmi_generator_set_weight"] == (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64])
    assert S["evmi_conv1d_cbt_f32"] == (C.c_int, [C.c_void_p] * 5 + [C.c_longlong] + [C.c_int] * 15 + [C.c_float, C.c_void_p])
    assert S["evmi_store_u64"] == (C.c_int, [C.c_void_p, C.c_ulonglong, C.c_void_p])
    assert S["evmi_pkflat_rowsum_ws_elems"] == (C.c_longlong, [C.c_int, C.POINTER(_lib.PkFlatRows)])
    assert S["evmi_layernorm_bwd_partials_reduce"] == (C.c_int, [C.c_int, C.POINTER(_lib.LnPartials), C.c_void_p])
    assert S["evmi_resblock_branch_bf16"] == (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p] + [C.c_float] * 3 + [C.c_int, C.c_int, C.c_void_p])


def test_constants_are_the_headers():
    assert (_lib.EVMI_OK, _lib.EVMI_ERR_INVALID_ARG, _lib.EVMI_ERR_HIP, _lib.EVMI_ERR_NOT_READY, _lib.EVMI_ERR_UNSUPPORTED,
            _lib.EVMI_ERR_OOM) == (0, 1, 2, 3, 4, 5)
    assert (_lib.EVMI_PREC_BF16, _lib.EVMI_PREC_F32) == (0, 1)
    assert _lib.EVMI_MAX_UPSAMPLES == _lib.EVMI_MAX_RESBLOCK_KERNELS == _lib.EVMI_MAX_DILATIONS == 8
    assert _lib.EVMI_ABI_VERSION == 2


# C type of a struct member -> ctypes, as the mirrors spell it: data pointers inside a struct are plain addresses
MEMBER_TYPES = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong, "char": C.c_char}


@pytest.mark.parametrize("c_name", sorted(_lib.MIRRORS))
def test_struct_mirror_matches_the_header(c_name):
    """Name, order, C type and array extents of every member."""
    want = []
    for c_type, member, extents in _lib.struct_members()[c_name]:
        t = C.c_void_p if c_type.endswith("*") else MEMBER_TYPES[c_type]
        for n in reversed(extents):  # int a[2][3] is (c_int * 3) * 2
            t = t * n
        want.append((member, t))
    assert _lib.MIRRORS[c_name]._fields_ == want


def test_every_struct_of_the_header_is_mirrored():
    assert set(_lib.struct_members()) == set(_lib.MIRRORS)
