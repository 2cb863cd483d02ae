"""The Python binding is read from include/mi355r.h (torch_renderer_amd/_abi.py): the reader's rules one by one on
small synthetic headers, what it refuses, and the real header against the loaded library. No GPU."""
import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint8, c_void_p

import pytest

from torch_renderer_amd import _abi, _lib

SNIPPET = """
/* a comment that looks like a call: mr_x(+_backward), and mr_y(int32_t a); too */
#ifndef H
#define H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
enum { MR_A = 0, MR_B = 3,
       /* a comment between two values, with MR_NOT = 9 inside */
       MR_C = 16,
       MR_D = 1024 };
typedef struct mr_view { float R[9]; float ax, bx; } mr_view_t;
typedef struct mr_some_thing {
  int32_t kind;          /* padding follows */
  int64_t count;
  float a[3], b[3];
  float ax, bx;
  const float* data;     /* a pointer member */
  uint8_t* bytes;
  double d;
  size_t n;
  uint8_t flag;
} mr_some_thing_t;
const char* mr_name(void);
int32_t mr_split(const float* x,
                 int64_t n,   // a line comment
                 void* stream);
size_t mr_mixed(float f, double d, int32_t i, int64_t l, size_t s);
int64_t mr_pointers(int32_t* out, const void* ws, uint64_t* visited, const uint8_t* mask, const double* m);
int32_t mr_structs(const mr_some_thing_t* s, mr_some_thing_t* t, const mr_view_t* views, mr_view_t* views_out);
#ifdef __cplusplus
}
#endif
#endif
"""


@pytest.fixture(scope="module")
def abi():
    return _abi.read_header(SNIPPET)


@pytest.fixture(scope="module")
def protos(abi):
    return {name: (res, args) for name, res, args in abi.prototypes}


def test_reader_imports_neither_torch_nor_the_library():
    src = open(_abi.__file__).read()
    assert set(re.findall(r"^(?:from|import)\s+(\w+)", src, flags=re.M)) == {"__future__", "ctypes", "re", "typing"}


def test_prototypes_in_header_order_and_none_from_comments(abi):
    assert [p[0] for p in abi.prototypes] == ["mr_name", "mr_split", "mr_mixed", "mr_pointers", "mr_structs"]


def test_void_and_const_char_return(protos):
    assert protos["mr_name"] == (c_char_p, [])


def test_prototype_over_three_lines(protos):
    assert protos["mr_split"] == (c_int32, [c_void_p, c_int64, c_void_p])


def test_scalars_double_beside_float(protos):
    assert protos["mr_mixed"] == (c_size_t, [c_float, c_double, c_int32, c_int64, c_size_t])


def test_scalar_and_void_pointers_are_void_p(protos):
    assert protos["mr_pointers"] == (c_int64, [c_void_p] * 5)


def test_struct_pointers(abi, protos):
    S = abi.structs["MrSomeThing"]
    assert protos["mr_structs"] == (c_int32, [POINTER(S), POINTER(S), c_void_p, c_void_p])  # mr_view_t*: device array


def test_enum_over_lines_with_comments(abi):
    assert abi.constants == {"MR_A": 0, "MR_B": 3, "MR_C": 16, "MR_D": 1024}


def test_struct_members(abi):
    assert sorted(abi.structs) == ["MrSomeThing", "MrView"]
    S = abi.structs["MrSomeThing"]
    assert issubclass(S, ctypes.Structure) and S.__name__ == "MrSomeThing"
    assert [n for n, _ in S._fields_] == ["kind", "count", "a", "b", "ax", "bx", "data", "bytes", "d", "n", "flag"]
    types = dict(S._fields_)
    assert types["a"] is types["b"] is c_float * 3 and types["ax"] is types["bx"] is c_float
    assert types["data"] is types["bytes"] is c_void_p  # kernels._mesh_struct assigns data_ptr() integers
    assert (types["kind"], types["count"], types["d"], types["n"], types["flag"]) == (c_int32, c_int64, c_double,
                                                                                     c_size_t, c_uint8)
    s = S()
    s.data = 0x1234
    assert s.data == 0x1234
    V = abi.structs["MrView"]
    assert dict(V._fields_)["R"] is c_float * 9 and ctypes.sizeof(V) == 44


def test_struct_padding(abi):
    S = abi.structs["MrSomeThing"]
    assert (S.kind.offset, S.count.offset, S.a.offset, S.b.offset, S.ax.offset, S.bx.offset) == (0, 8, 16, 28, 40, 44)
    assert (S.data.offset, S.bytes.offset, S.d.offset, S.n.offset, S.flag.offset) == (48, 56, 64, 72, 80)
    assert ctypes.sizeof(S) == 88


@pytest.mark.parametrize("text, named", [
    ("int32_t mr_bad_param(int64_t n, unsigned int flags);", "mr_bad_param"),
    ("int32_t mr_bad_param(int x);", "mr_bad_param"),
    ("int32_t mr_bad_param(uint8_t by_value);", "mr_bad_param"),
    ("int32_t mr_bad_pointer(char** names);", "mr_bad_pointer"),
    ("typedef struct mr_s { float a; } mr_s_t; int32_t mr_by_value(mr_s_t s);", "mr_by_value"),
    ("typedef struct mr_bad { int32_t a; long b; } mr_bad_t;", "mr_bad_t"),
    ("typedef struct mr_bad { char* name; } mr_bad_t;", "mr_bad_t"),
    ("void mr_bad_return(int32_t a);", "mr_bad_return"),
    ("float mr_bad_return(void);", "mr_bad_return"),
    ("int32_t* mr_bad_return(void);", "mr_bad_return"),
    ("enum { MR_BAD };", "MR_BAD"),
    ("extern int32_t mr_global;", "mr_global"),
])
def test_what_the_reader_does_not_understand_raises(text, named):
    with pytest.raises(_abi.AbiError, match=named):
        _abi.read_header(text)


# ---- the real header ----

def header_text():
    return re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)


def header_param_counts():
    """name -> parameter count, by a regex of this file's own (not the reader's)."""
    return {name: 0 if params.strip() == "void" else params.count(",") + 1
            for name, params in re.findall(r"\b(mr_[a-z0-9_]+)\s*\(([^)]*)\)", header_text())}


def test_every_prototype_of_the_header_is_read():
    names = sorted(set(re.findall(r"\b(mr_[a-z0-9_]+)\s*\(", header_text())))  # test_capi.header_symbols' count
    assert len(_lib.EXPORTED_SYMBOLS) == len(set(_lib.EXPORTED_SYMBOLS)) == len(names) >= 117
    assert sorted(_lib.EXPORTED_SYMBOLS) == names


def test_signatures_where_a_wrong_type_changes_the_call():
    sig = {name: (res, args) for name, res, args in _lib.ABI.prototypes}
    assert sig["mr_points_alignment"][1][7] is c_double
    a = sig["mr_icp_plane_iterate_grid"][1]
    assert (a[9], a[10], a[11]) == (c_size_t, c_float, c_float)
    assert sig["mr_pixel_range"][1][:2] == [c_float, c_float]
    assert sig["mr_binning_background_pixels"][0] is c_int64
    assert sig["mr_last_error"][0] is c_char_p and sig["mr_timing_kernel_name"][0] is c_char_p
    assert sig["mr_render_forward_opencv"][1][:3] == [POINTER(_lib.MrMesh), POINTER(_lib.MrOpencvPoses), c_void_p]
    assert sig["mr_render_workspace"] == (c_size_t, [c_int64, c_int64, c_int32, c_int32, c_int32])


def test_constants_and_structs_are_the_headers():
    vals = dict(re.findall(r"\b(MR_[A-Z_0-9]+)\s*=\s*(\d+)", header_text()))
    assert len(vals) >= 29 and {"MR_OK", "MR_EWORKSPACE", "MR_CHAMFER_ALL", "MR_ICP_ALL"} <= set(vals)
    for name, v in vals.items():
        assert getattr(_lib, name) == int(v), name
    assert (_lib.MR_OK, _lib.MR_EINVAL, _lib.MR_ELAUNCH, _lib.MR_EUNSUPPORTED, _lib.MR_EWORKSPACE) == (0, 1, 2, 3, 4)
    sizes = {"MrView": 64, "MrRasterSettings": 40, "MrShadeParams": 132, "MrMesh": 160, "MrPoses": 48,
             "MrOpencvPoses": 48}
    assert {n: ctypes.sizeof(getattr(_lib, n)) for n in sizes} == sizes
    assert _lib.MrMesh.max_view_faces.offset == 152 and _lib.MrMesh.tex_kind.offset == 56
    assert _lib.MrMesh.vcolors.offset == 64  # (padded after the int32 tex_kind)


def test_missing_header_raises(tmp_path):
    path = str(tmp_path / "include" / "mi355r.h")
    with pytest.raises(RuntimeError, match=re.escape(path)):
        _lib.read_header(path)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from torch_renderer_amd import _build

        _build.build()
    return _lib.load()


def test_loaded_library_has_the_headers_parameter_counts(lib):
    counts = header_param_counts()
    assert sorted(counts) == sorted(_lib.EXPORTED_SYMBOLS)
    for name in _lib.EXPORTED_SYMBOLS:
        assert len(getattr(lib, name).argtypes) == counts[name], name


def test_struct_sizes_are_the_librarys(lib):
    for which, cls in enumerate((_lib.MrView, _lib.MrRasterSettings, _lib.MrShadeParams, _lib.MrMesh)):
        assert ctypes.sizeof(cls) == lib.mr_struct_size(which), cls.__name__


def test_torch_ext_names_its_entry_points():
    mod = _lib.torch_ext()
    assert len(mod.abi_functions) == len(set(mod.abi_functions)) == 15
    assert set(mod.abi_functions) <= set(_lib.EXPORTED_SYMBOLS)
