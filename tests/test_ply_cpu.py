"""The host side of the .ply reader and writer (gscodec_studio_amd.ply): the header parser on hand-built byte strings, every
refusal, the writer's header text, the column table against one derived from numpy's own field offsets, the two trainer helpers
beside it, and what the native entry points and the device functions answer without a GPU."""
import ctypes
import random

import numpy as np
import pytest
import torch

import ply_cases as C

from gscodec_studio_amd import ply as P


def parse(n, props, **kw):
    data = C.header_bytes(n, props, **kw)
    return P.parse_ply_header(data + b"\0" * 16, "case"), data


def check_layout(h, data, n, props):
    dt = C.dtype_of(props)
    assert (h.format, h.count, h.stride, h.payload_offset) == ("binary_little_endian", n, dt.itemsize, len(data))
    assert [(p.name, p.offset) for p in h.properties] == [(name, dt.fields[name][1]) for _, name in props]
    assert [np.dtype(C.NUMPY_OF[p.type]) for p in h.properties] == [dt.fields[name][0] for _, name in props]


def test_header_of_the_62_and_59_float_layouts():
    for normals, floats in ((True, 62), (False, 59)):
        props = [("float", name) for name in C.standard_names(15, normals)]
        h, data = parse(1000, props)
        check_layout(h, data, 1000, props)
        assert h.stride == 4 * floats and h.elements_after == ()
        cols = P.column_table(h)
        assert (cols.S0, cols.SN, cols.S, cols.Q, cols.route) == (3, 45, 3, 4, "words") and cols.widths == (3, 3, 45, 1, 3, 4)


def test_header_shuffled_comments_crlf_double_uchar_and_trailing_face():
    props = C.layout("shuffled", 3)
    h, data = parse(7, props)
    check_layout(h, data, 7, props)
    assert P.column_table(h).route == "words"

    props = C.layout("standard", 0)
    h, data = parse(3, props, comments=("comment written by hand", "obj_info anything at all", "comment element vertex 99"))
    check_layout(h, data, 3, props)
    assert P.column_table(h).widths == (3, 3, 0, 1, 3, 4)

    h, data = parse(5, props, newline="\r\n")
    check_layout(h, data, 5, props)
    assert data.endswith(b"end_header\r\n")

    props = C.layout("double", 3)
    h, data = parse(5, props)
    check_layout(h, data, 5, props)
    cols = P.column_table(h)
    at = {p.name: p.offset for p in h.properties}
    assert h.stride == 4 * 26 + 4 * 4 and cols.entries[3 + 3 + 9] == at["opacity"] | 1 << 16 and cols.route == "words"
    assert [e >> 16 for e in cols.entries] == [0] * 15 + [1] * 4 + [0] * 4

    props = C.layout("uchar_front", 3)
    h, data = parse(5, props)
    check_layout(h, data, 5, props)
    cols = P.column_table(h)
    assert [p.offset for p in h.properties[:4]] == [0, 1, 2, 3] and cols.entries[:3] == (3, 7, 11) and cols.route == "unaligned"

    props = C.layout("standard", 3)
    h, data = parse(4, props, after="element face 2\nproperty list uchar int vertex_indices\nproperty uchar flag\nelement edge 0")
    check_layout(h, data, 4, props)
    assert h.elements_after == (("face", 2), ("edge", 0))


F = [("float", name) for name in C.standard_names(3)]


def without(*names):
    return [p for p in F if p[1] not in names]


@pytest.mark.parametrize("what,data,fragment", [
    ("ascii", C.header_bytes(1, F).replace(b"binary_little_endian", b"ascii"), "ascii is not supported"),
    ("big endian", C.header_bytes(1, F).replace(b"little", b"big"), "binary_big_endian is not supported"),
    ("magic", b"plx\n" + C.header_bytes(1, F), "no `ply` magic"),
    ("list in vertex", C.header_bytes(1, F + [("list uchar", "int idx")]), "list property inside vertex"),
    ("element first", C.header_bytes(1, F).replace(b"element vertex 1", b"element face 0\nelement vertex 1"), "before vertex"),
    ("missing x", C.header_bytes(1, without("x")), "missing property x"),
    ("missing z", C.header_bytes(1, without("z")), "missing property z"),
    ("missing opacity", C.header_bytes(1, without("opacity")), "missing property opacity"),
    ("gap", C.header_bytes(1, without("f_rest_1")), "gap in the numbered group f_rest_"),
    ("S0 % 3", C.header_bytes(1, without("f_dc_2")), "f_dc_* properties: not divisible by 3"),
    ("SN % 3", C.header_bytes(1, without("f_rest_8")), "f_rest_* properties: not divisible by 3"),
    ("integer", C.header_bytes(1, [("int", n) if n == "scale_1" else (t, n) for t, n in F]), "scale_1 has the integer type int"),
    ("stride", C.header_bytes(1, F + [("double", f"pad_{i}") for i in range(116)]), "row stride 1032 bytes above the limit of 1024"),
    ("2^31", C.header_bytes(1 << 31, F), "fewer than 2^31"),
    ("no end", C.header_bytes(1, F).replace(b"end_header", b"end_of_it"), "no `end_header`"),
])
def test_refused_headers(what, data, fragment):
    with pytest.raises(ValueError) as e:
        P.column_table(P.parse_ply_header(data + b"\0" * 64, "case"), name="case")
    assert fragment in str(e.value), (what, str(e.value))


def test_refused_truncated_payload_and_missing_gpu(tmp_path, monkeypatch):
    """The file is judged before the device: a short payload is a ValueError with or without a GPU; a sound file then needs one."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    rows = C.payload(10, F)
    path = tmp_path / "short.ply"
    path.write_bytes(C.header_bytes(10, F) + rows.tobytes()[:-1])
    for fn in (P.load_ply, P.load_ply_to_rasterizer_inputs):
        with pytest.raises(ValueError, match="payload shorter than 10 rows of 104 bytes"):
            fn(path)
    path.write_bytes(C.header_bytes(10, F) + rows.tobytes())
    assert P.read_ply_header(path).count == 10
    for fn in (P.load_ply, P.load_ply_to_rasterizer_inputs, lambda p: P.load_ply(p, device="cpu")):
        with pytest.raises(RuntimeError, match="no GPU"):
            fn(path)


def test_save_ply_refusals_without_a_gpu(tmp_path):
    n = 5
    good = {"means": torch.zeros(n, 3), "sh0": torch.zeros(n, 1, 3), "shN": torch.zeros(n, 3, 3), "opacities": torch.zeros(n),
            "scales": torch.zeros(n, 3), "quats": torch.zeros(n, 4)}
    path = tmp_path / "out.ply"
    for bad, fragment in (({k: v for k, v in good.items() if k != "shN"}, "key 'shN' missing"),
                          ({**good, "scales": torch.zeros(n + 1, 3)}, "mismatched N"),
                          ({**good, "quats": torch.zeros(n, 4, dtype=torch.float64)}, "quats must be float32"),
                          ({**good, "sh0": torch.zeros(n, 3)}, "sh0 has shape")):
        with pytest.raises(ValueError, match=fragment):
            P.save_ply(bad, path)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.save_ply(good, path)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.save_ply(torch.nn.ParameterDict({k: torch.nn.Parameter(v) for k, v in good.items()}), path)
    assert list(tmp_path.iterdir()) == []  # neither the file nor its .tmp


@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("kn", [0, 3, 15])
def test_writer_header_text(normals, kn):
    text = P.ply_header_text(12345, 3, 3 * kn, 3, 4, normals)
    names = C.standard_names(kn, normals)
    want = "ply\nformat binary_little_endian 1.0\nelement vertex 12345\n" + "".join(f"property float {p}\n" for p in names) + "end_header\n"
    assert text == want.encode("ascii")
    h = P.parse_ply_header(text)  # and the reader takes what the writer writes
    assert (h.count, h.stride, h.payload_offset) == (12345, 4 * len(names), len(text)) and [p.name for p in h.properties] == names


def test_column_table_of_the_golden_layout_against_numpy_field_offsets():
    z = np.load(C.GOLDEN)
    for tag, kn in (("deg3", 15), ("deg1", 3)):
        names = [str(s) for s in z[f"{tag}_names"]]
        assert names == C.standard_names(kn)
        fields = np.dtype([(s, "<f4") for s in names]).fields
        want = [fields[s][1] for s in ("x", "y", "z")]
        want += [fields[f"f_dc_{c + k}"][1] for k in range(1) for c in range(3)]
        want += [fields[f"f_rest_{c * kn + k}"][1] for k in range(kn) for c in range(3)]
        want += [fields[s][1] for s in ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]]
        h = P.parse_ply_header(P.ply_header_text(300, 3, 3 * kn))
        cols = P.column_table(h)
        assert list(cols.entries) == want and cols.widths == (3, 3, 3 * kn, 1, 3, 4)
        fused = P.column_table(h, fused=True)
        assert fused.entries == cols.entries and fused.widths == (3, 3 + 3 * kn, 0, 1, 3, 4)
        # the table applied by numpy to the recorded payload gives the recorded arrays
        words = z[f"{tag}_payload"].view(np.uint32).reshape(300, -1)
        flat = words[:, np.array(cols.entries) // 4]
        for key, lo in zip(C.KEYS, np.cumsum((0,) + cols.widths[:-1])):
            got = flat[:, lo:lo + cols.widths[C.KEYS.index(key)]]
            assert np.array_equal(got.reshape(-1), C.bits(z[f"{tag}_loaded_{key}"]).reshape(-1)), (tag, key)


def test_rgb_to_sh_and_set_random_seed():
    import gscodec_studio_amd.utils as U

    rgb = torch.tensor([[0.0, 0.5, 1.0], [0.25, 0.75, 0.1]])
    assert torch.equal(U.rgb_to_sh(rgb), (rgb - 0.5) / 0.28209479177387814)
    assert U.rgb_to_sh(torch.tensor(0.5)).item() == 0.0 and abs(U.rgb_to_sh(torch.tensor(1.0)).item() - 1.7724538509055159) < 1e-6
    U.set_random_seed(42)
    first = (random.random(), float(np.random.rand()), float(torch.rand(())))
    random.seed(42), np.random.seed(42), torch.manual_seed(42)
    assert first == (random.random(), float(np.random.rand()), float(torch.rand(())))
    U.set_random_seed(42)
    assert first == (random.random(), float(np.random.rand()), float(torch.rand(())))


def test_utils_reexports_the_ply_names():
    import gscodec_studio_amd.utils as U

    assert U.load_ply is P.load_ply and U.save_ply is P.save_ply and U.load_ply_to_rasterizer_inputs is P.load_ply_to_rasterizer_inputs
    assert U.read_ply_header is P.read_ply_header
    assert {"knn", "rgb_to_sh", "set_random_seed", "load_ply", "save_ply", "load_ply_to_rasterizer_inputs", "read_ply_header"} <= set(U.__all__)


def test_entry_points_are_declared_exported_and_refuse_before_launching():
    from gscodec_studio_amd import _backend as B

    protos = B.prototypes()  # (loads the library: every declared name is exported)
    assert sorted(n for n in protos if n.startswith("gs_ply_")) == ["gs_ply_block_rows", "gs_ply_max_columns", "gs_ply_max_stride",
                                                                   "gs_ply_pack", "gs_ply_unpack"]
    assert protos["gs_ply_unpack"][2] == ["n", "stride", "rows", "cols", "widths6", "outs6", "activate", "normalize_quats", "force_bytes",
                                          "stream"]
    assert protos["gs_ply_pack"][2] == ["n", "stride", "cols", "widths6", "ins6", "rows", "stream"]
    assert (B.query("gs_ply_max_stride"), B.query("gs_ply_max_columns")) == (1024, 128)
    assert [B.query("gs_ply_block_rows", s) for s in (0, 1, 236, 248, 256, 257, 356, 512, 513, 1024, 1025)] == \
        [0, 256, 256, 256, 256, 128, 128, 128, 64, 64, 0]

    cols = (ctypes.c_uint32 * 4)(0, 4, 8, 12)
    widths = (ctypes.c_uint32 * 6)(3, 0, 0, 1, 0, 0)
    fake = 4096  # an aligned non-null address that is never dereferenced: every call below is refused on the host
    ptrs = (ctypes.c_void_p * 6)(fake, None, None, fake, None, None)
    A = ctypes.addressof

    def unpack(n=10, stride=16, rows=fake, c=A(cols), w=A(widths), p=A(ptrs)):
        return lambda: B.call("gs_ply_unpack", n, stride, rows, c, w, p, 0, 0, 0, None)

    def pack(n=10, stride=16, rows=fake, c=A(cols), w=A(widths), p=A(ptrs)):
        return lambda: B.call("gs_ply_pack", n, stride, c, w, p, rows, None)

    beyond = (ctypes.c_uint32 * 4)(0, 4, 8, 16)
    double_at_end = (ctypes.c_uint32 * 4)(0, 4, 8, 12 | 1 << 16)
    odd = (ctypes.c_uint32 * 4)(0, 4, 8, 13)
    flag = (ctypes.c_uint32 * 4)(0, 4, 8, 12 | 1 << 17)
    null_out = (ctypes.c_void_p * 6)(fake, None, None, None, None, None)
    too_wide = (ctypes.c_uint32 * 6)(3, 100, 100, 1, 0, 0)
    all_set = (ctypes.c_void_p * 6)(*[fake] * 6)
    for make in (unpack, pack):
        for fn, fragment in ((make(rows=None), "null pointer"), (make(c=None), "null pointer"), (make(w=None), "null pointer"),
                             (make(p=None), "null pointer"), (make(p=A(null_out)), "null pointer"), (make(stride=0), "stride"),
                             (make(stride=1028), "stride"), (make(n=0), "1 <= n"), (make(c=A(beyond)), "beyond the stride"),
                             (make(rows=fake + 4), "16-byte aligned"), (make(c=A(flag)), "unknown type flag"),
                             (make(w=A(too_wide), p=A(all_set)), "more than 128 columns")):
            with pytest.raises(RuntimeError, match=fragment):
                fn()
    with pytest.raises(RuntimeError, match="beyond the stride"):
        unpack(c=A(double_at_end))()
    with pytest.raises(RuntimeError, match="unknown type flag"):  # the writer has float columns only
        pack(c=A(double_at_end), stride=24)()
    with pytest.raises(RuntimeError, match="multiples of 4"):
        pack(c=A(odd), stride=20)()
