"""CPU: what _backend derives from the text of include/gsplat_hip.h besides the prototypes -- a ctypes.Structure per host struct and
an int per ``#define GS_*`` -- on small synthetic headers (one per declarator form the real header uses, one per construct the parser
must refuse instead of guessing) and on the real header."""
import ctypes
import itertools

import pytest

from gscodec_studio_amd import _backend as B

_N = itertools.count()


def _struct(tmp_path, text: str, name: str = "gs_t"):
    h = tmp_path / f"h{next(_N)}.h"
    h.write_text(text)
    return B.struct(name, str(h))


def _layout(cls):
    """[(name, ctype, offset, size)] in field order"""
    return [(n, t, getattr(cls, n).offset, getattr(cls, n).size) for n, t in cls._fields_]


def test_several_declarators_per_line(tmp_path):
    cls = _struct(tmp_path, "typedef struct gs_t {\n    uint32_t C, N;\n    uint64_t n;\n    int32_t a,b ,c;\n} gs_t;\n")
    assert _layout(cls) == [("C", ctypes.c_uint32, 0, 4), ("N", ctypes.c_uint32, 4, 4), ("n", ctypes.c_uint64, 8, 8),
                            ("a", ctypes.c_int32, 16, 4), ("b", ctypes.c_int32, 20, 4), ("c", ctypes.c_int32, 24, 4)]
    assert ctypes.sizeof(cls) == 32  # (tail padding to the 8-byte alignment of n)


def test_const_and_pointers_of_any_pointee_are_void_pointers(tmp_path):
    cls = _struct(tmp_path, "typedef struct gs_t {\n    uint32_t n;\n    const float *means, *covars;\n    int64_t *ids;\n    void *work;\n"
                            "    const uint8_t* vis;\n    const gs_unknown_t **pp;\n    float const *q;\n} gs_t;\n")
    names = ["means", "covars", "ids", "work", "vis", "pp", "q"]
    assert _layout(cls) == [("n", ctypes.c_uint32, 0, 4)] + [(f, ctypes.c_void_p, 8 + 8 * i, 8) for i, f in enumerate(names)]


def test_fixed_arrays_and_uint8(tmp_path):
    cls = _struct(tmp_path, "typedef struct gs_t {\n    uint8_t flag;\n    uint8_t tag[3];\n    float lo[4], hi [ 4 ];\n    float x;\n"
                            "    float *rows[2];\n} gs_t;\n")
    lay = _layout(cls)
    assert [(n, o, s) for n, _, o, s in lay] == [("flag", 0, 1), ("tag", 1, 3), ("lo", 4, 16), ("hi", 20, 16), ("x", 36, 4), ("rows", 40, 16)]
    types = dict(cls._fields_)
    assert types["flag"] is ctypes.c_uint8 and types["x"] is ctypes.c_float
    for f, elem, length in (("tag", ctypes.c_uint8, 3), ("lo", ctypes.c_float, 4), ("hi", ctypes.c_float, 4), ("rows", ctypes.c_void_p, 2)):
        assert types[f]._type_ is elem and types[f]._length_ == length, f


def test_struct_by_value_and_comments(tmp_path):
    text = ("/* typedef struct gs_ghost { int32_t x; } gs_ghost; */\n"
            "typedef struct gs_inner { uint32_t a; uint64_t b; } gs_inner;\n"
            "typedef struct gs_t {\n    uint32_t n; /* a comment; with a semicolon, and { braces } */\n    gs_inner plan; // and: this\n"
            "    const gs_inner *p;\n    size_t bytes;\n    gs_stream_t stream;\n} gs_t;\n")
    cls = _struct(tmp_path, text)
    inner = _struct(tmp_path, text, "gs_inner")
    assert _layout(inner) == [("a", ctypes.c_uint32, 0, 4), ("b", ctypes.c_uint64, 8, 8)]
    lay = _layout(cls)
    assert [(n, o, s) for n, _, o, s in lay] == [("n", 0, 4), ("plan", 8, 16), ("p", 24, 8), ("bytes", 32, 8), ("stream", 40, 8)]
    assert issubclass(lay[1][1], ctypes.Structure) and [f[0] for f in lay[1][1]._fields_] == ["a", "b"]
    assert lay[2][1] is ctypes.c_void_p and lay[3][1] is ctypes.c_size_t and lay[4][1] is ctypes.c_void_p
    with pytest.raises(ImportError, match="does not define struct gs_ghost"):
        _struct(tmp_path, text, "gs_ghost")


@pytest.mark.parametrize("what, body, names", [
    ("unknown type", "uint32_t n;\n    double x;", ("double",)),
    ("unknown type, two words", "uint32_t n;\n    unsigned int x;", ("unsigned",)),
    ("struct used before its definition", "uint32_t n;\n    gs_later later;", ("gs_later",)),
    ("bit-field", "uint32_t n;\n    uint32_t flag : 1;", ("bit-field", "flag")),
    ("union", "uint32_t n;\n    union { float f; uint32_t u; } v;", ("union",)),
    ("anonymous union", "uint32_t n;\n    union { float f; uint32_t u; };", ("union",)),
    ("nested anonymous struct", "uint32_t n;\n    struct { float f; uint32_t u; } v;", ("nested struct",)),
    ("function pointer", "uint32_t n;\n    int32_t (*fn)(void *);", ("function pointer", "fn")),
    ("preprocessor line", "uint32_t n;\n#ifdef GS_WIDE\n    uint64_t wide;\n#endif\n    float x;", ("preprocessor",)),
    ("two-dimensional array", "uint32_t n;\n    float m[4][4];", ("m[4][4]",)),
    ("array with a symbolic length", "uint32_t n;\n    float m[GS_ROW_FLOATS];", ("GS_ROW_FLOATS",)),
])
def test_constructs_the_parser_does_not_know_are_refused(tmp_path, what, body, names):
    text = "typedef struct gs_t {\n    " + body + "\n} gs_t;\ntypedef struct gs_later { uint32_t a; } gs_later;\n"
    with pytest.raises(ImportError) as e:
        _struct(tmp_path, text)
    msg = str(e.value)
    assert "gs_t" in msg, (what, msg)  # names the struct ...
    for n in names:  # ... and the declaration
        assert n in msg, (what, msg)


def test_constants_of_synthetic_defines(tmp_path):
    h = tmp_path / "c.h"
    h.write_text("#define GS_A 3\n  #  define GS_B 4u /* four */\n#define GS_C 0x10\n#define GS_D (1 << 2)\n#define GS_E 1.5\n"
                 "#define GS_F\n#define OTHER 7\n/* #define GS_G 9 */\n#define GS_H 12U // twelve\n")
    assert {n: B.const(n, str(h)) for n in ("GS_A", "GS_B", "GS_H")} == {"GS_A": 3, "GS_B": 4, "GS_H": 12}
    for n in ("GS_C", "GS_D", "GS_E", "GS_F", "OTHER", "GS_G"):  # not decimal integer literals, not GS_*, or commented out
        with pytest.raises(ImportError, match=f"c.h does not define {n}"):
            B.const(n, str(h))


def test_constants_of_the_real_header():
    assert B.const("GS_ROW_FLOATS") == 16
    assert B.const("GS_ROW_COLOR") == 6
    assert B.const("GS_CAMERA_FISHEYE") == 2
    assert B.const("GS_ADAM_MULTI_MAX") == int(B.query("gs_adam_multi_max"))
    assert B.const("GS_QUANT_MULTI_MAX") == 8
    assert B.const("GS_ABI_VERSION") == B.header_abi_version()
    assert len(B._header().consts) == 26


def test_python_side_names_are_the_header_values():
    from gscodec_studio_amd import _wrapper as W
    from gscodec_studio_amd import dynamic
    from gscodec_studio_amd.compression_simulation import ops

    assert W.ROW == B.const("GS_ROW_FLOATS") == 16
    assert W.ROW_COLOR == B.const("GS_ROW_COLOR") == 6
    assert (W.ROW_MEAN2D, W.ROW_CONIC, W.ROW_OPACITY, W.ROW_DEPTH, W.ROW_RADIUS, W.ROW_COMP) == tuple(
        B.const("GS_ROW_" + c) for c in ("MEAN2D", "CONIC", "OPACITY", "DEPTH", "RADIUS", "COMPENSATION"))
    assert W._CAMERA_MODELS["fisheye"] == B.const("GS_CAMERA_FISHEYE") == 2
    assert W._CAMERA_MODELS == {"pinhole": B.const("GS_CAMERA_PINHOLE"), "ortho": B.const("GS_CAMERA_ORTHO"), "fisheye": 2}
    assert W.SSIM_PADDING["valid"] == B.const("GS_SSIM_VALID") == 1 and W.SSIM_PADDING["same"] == B.const("GS_SSIM_SAME")
    assert ops._ACTS["sigmoid"] == B.const("GS_ACT_SIGMOID") == 2
    assert ops._ACTS[None] == B.const("GS_ACT_NONE") and ops._ACTS["exp"] == B.const("GS_ACT_EXP")
    assert (W.ADAM_DENSE, W.ADAM_SELECTIVE) == (B.const("GS_ADAM_DENSE"), B.const("GS_ADAM_SELECTIVE"))
    assert ops.QUANT_MULTI_MAX == B.const("GS_QUANT_MULTI_MAX")
    assert dynamic._RAW_BITS == {"scales": B.const("GS_DYN_RAW_SCALES"), "opacities": B.const("GS_DYN_RAW_OPACITIES"),
                                 "trbf_scale": B.const("GS_DYN_RAW_TRBF_SCALE")}


def test_real_header_structs():
    """All four host structs of the real header, with the sizes their C definitions have; the plan made through the operator path
    is an instance of the derived class."""
    from gscodec_studio_amd import _wrapper as W

    sizes = {n: ctypes.sizeof(B.struct(n)) for n in ("gs_raster_plan", "gs_quant_desc", "gs_adam_desc", "gs_step")}
    assert sizes == {"gs_raster_plan": 64, "gs_quant_desc": 64, "gs_adam_desc": 96, "gs_step": 608}
    step = B.struct("gs_step")
    assert len(step._fields_) == 78 and dict(step._fields_)["plan"] is B.struct("gs_raster_plan")
    plan, scratch_bytes = W._raster_plan(64, 1000, 3)
    assert isinstance(plan, B.struct("gs_raster_plan")) and plan.scratch_bytes == scratch_bytes and plan.channels == 3


def test_anonymous_or_mistagged_typedef_struct_is_refused(tmp_path):
    for text in ("typedef struct { uint32_t n; } gs_t;\n", "typedef struct gs_tag { uint32_t n; } gs_t;\n"):
        with pytest.raises(ImportError, match="gs_t"):
            _struct(tmp_path, text)


_COUNT_READS = """
import builtins, os
opened, real_open = [], builtins.open
def counting_open(file, *a, **k):
    if isinstance(file, (str, os.PathLike)):
        opened.append(os.path.abspath(os.fspath(file)))
    return real_open(file, *a, **k)
builtins.open = counting_open
import gscodec_studio_amd
from gscodec_studio_amd import _backend as B, _step, _wrapper, dynamic
from gscodec_studio_amd.compression_simulation import ops
L = B.lib()
B.prototypes(), B.parse_header(), B.header_abi_version(), B.header_hash(), B.struct("gs_step"), B.const("GS_ROW_FLOATS"), B.check_layouts()
_wrapper._raster_plan(64, 1000, 3)
assert B._header() is B._header(B.HEADER_PATH)
print("READS", opened.count(os.path.abspath(B.HEADER_PATH)))
"""


def test_the_header_is_read_once():
    """In a fresh process, along the path production takes (the package's import, lib(), every accessor with its default path):
    prototypes, version, hash, structs and constants all come from ONE read of the header."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _COUNT_READS], env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]
    assert "READS 1\n" in r.stdout, r.stdout[-200:]


def test_missing_header_keeps_its_message(tmp_path):
    with pytest.raises(ImportError, match="ABI header gsplat_hip.h not found"):
        B.parse_header(str(tmp_path / "nowhere.h"))
