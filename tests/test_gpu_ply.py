"""The .ply kernels (csrc/ply.hip behind gscodec_studio_amd.ply) on the GPU: the reference's own payload bytes and loaded arrays
(tests/golden/ply.npz), every layout and row-block size against numpy's reading of the same bytes, chunking, round trips bit for
bit, the fused decode against float64 numpy and in a render, the command-line tool, and the refusals that need a device."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import grid_sort_cases as G
import ply_cases as C
from util import N

from gscodec_studio_amd import ply as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def same_bits(t, a):
    """A float32 tensor equals a numpy array bit for bit (NaN payloads included) and in shape."""
    return tuple(t.shape) == a.shape and t.dtype == torch.float32 and torch.equal(t.detach().view(torch.int32).cpu(), torch.from_numpy(C.bits(a).view(np.int32)))


def assert_splats_equal(got, want, what):
    assert list(got.keys()) == list(C.KEYS), (what, list(got.keys()))
    for k in C.KEYS:
        assert same_bits(got[k], want[k]), (what, k, tuple(got[k].shape), want[k].shape)


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(C.GOLDEN)


@pytest.mark.parametrize("tag,kn", [("deg3", 15), ("deg1", 3)])
def test_golden_payload_loads_and_saves_as_the_reference_does(tag, kn, tmp_path):
    z = golden()
    payload = z[f"{tag}_payload"].tobytes()
    path = tmp_path / "golden.ply"
    path.write_bytes(P.ply_header_text(300, 3, 3 * kn) + payload)
    loaded = P.load_ply(path)
    assert isinstance(loaded, torch.nn.ParameterDict) and all(isinstance(v, torch.nn.Parameter) and v.is_cuda for v in loaded.values())
    assert_splats_equal(loaded, {k: z[f"{tag}_loaded_{k}"] for k in C.KEYS}, tag)
    out = tmp_path / "saved.ply"
    P.save_ply({k: torch.from_numpy(z[f"{tag}_in_{k}"]).to(DEV) for k in C.KEYS}, out)
    data = out.read_bytes()
    header = P.ply_header_text(300, 3, 3 * kn)
    assert data[:len(header)] == header and data[len(header):] == payload
    assert not os.path.exists(str(out) + ".tmp")


@pytest.mark.parametrize("kn", C.SHN_COEFFS)
@pytest.mark.parametrize("kind", C.LAYOUTS)
def test_every_layout_and_block_size_against_numpy(kind, kn, tmp_path):
    props = C.layout(kind, kn)
    stride = C.dtype_of(props).itemsize
    rows_per_block = {True: 256, False: 128 if 128 * stride <= 65536 else 64}[256 * stride <= 65536]
    from gscodec_studio_amd import _backend as B

    assert B.query("gs_ply_block_rows", stride) == rows_per_block
    for n in C.SIZES:
        data = C.header_bytes(n, props) + C.payload(n, props, seed=n + kn).tobytes()
        path = tmp_path / f"{n}.ply"
        path.write_bytes(data)
        header = P.read_ply_header(path)
        assert P.column_table(header).route == ("unaligned" if kind == "uchar_front" else "words")
        want = C.oracle(data, header)
        assert_splats_equal(P.load_ply(path), want, (kind, kn, n))
        raw = P.load_ply_to_rasterizer_inputs(path, activate=False, normalize_quats=False)
        assert all(same_bits(raw[k], want[k]) for k in C.KEYS), (kind, kn, n)
        if kind == "standard":  # the byte route on a file the word route takes gives the same
            forced = P.load_ply_to_rasterizer_inputs(path, activate=False, normalize_quats=False, _force_bytes=True)
            assert all(torch.equal(forced[k].view(torch.int32), raw[k].view(torch.int32)) for k in raw), (kn, n)


def test_trailing_elements_crlf_and_an_empty_file(tmp_path):
    props = C.layout("standard", 3)
    rows = C.payload(40, props, seed=3)
    data = C.header_bytes(40, props, newline="\r\n", comments=("comment x", "obj_info y"),
                          after="element face 1\nproperty list uchar int vertex_indices") + rows.tobytes() + b"\x03\1\0\0\0\2\0\0\0\3\0\0\0"
    path = tmp_path / "faces.ply"
    path.write_bytes(data)
    assert_splats_equal(P.load_ply(path), C.reference_columns(rows), "faces")
    host = P.load_ply(path, device="cpu")
    assert all(not v.is_cuda for v in host.values())
    assert_splats_equal(host, C.reference_columns(rows), "host")

    path = tmp_path / "empty.ply"
    path.write_bytes(C.header_bytes(0, props))
    empty = P.load_ply(path)
    assert [tuple(v.shape) for v in empty.values()] == [(0, 3), (0, 1, 3), (0, 3, 3), (0,), (0, 3), (0, 4)]
    path.write_bytes(C.header_bytes(0, C.layout("standard", 0)))
    assert tuple(P.load_ply(path)["shN"].shape) == (0, 0, 3)
    P.save_ply(dict(empty.items()), tmp_path / "empty_out.ply")
    assert (tmp_path / "empty_out.ply").read_bytes() == P.ply_header_text(0, 3, 9)


def test_chunked_load_and_save_equal_one_chunk(tmp_path):
    props = C.layout("standard", 15)
    rows = C.payload(1000, props, seed=9)
    for name in ("nx", "ny", "nz"):
        rows[name] = 0.0  # what save_ply writes there
    data = C.header_bytes(1000, props) + rows.tobytes()
    path = tmp_path / "a.ply"
    path.write_bytes(data)
    one = P.load_ply(path)
    four = P.load_ply(path, _chunk_rows=256)  # 256 + 256 + 256 + 232
    assert all(torch.equal(one[k].view(torch.int32), four[k].view(torch.int32)) for k in C.KEYS)
    fused = P.load_ply_to_rasterizer_inputs(path, _chunk_rows=256)
    assert all(torch.equal(fused[k], v) for k, v in P.load_ply_to_rasterizer_inputs(path).items())
    P.save_ply(four, tmp_path / "b.ply", _chunk_rows=256)
    assert (tmp_path / "b.ply").read_bytes() == data


def special_splats(n=700, kn=15):
    rs = np.random.RandomState(77)
    s = {"means": rs.randn(n, 3), "sh0": rs.randn(n, 1, 3), "shN": rs.randn(n, kn, 3), "opacities": rs.randn(n), "scales": rs.randn(n, 3),
         "quats": rs.randn(n, 4)}
    s = {k: v.astype(np.float32) for k, v in s.items()}
    odd = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7FA00000], np.uint32).view(np.float32)
    for k, v in s.items():  # NaNs with payloads (one signalling), the infinities, -0, the smallest and the largest denormal
        flat = v.reshape(-1)
        flat[rs.permutation(flat.size)[:len(odd)]] = odd
    return s


@pytest.mark.parametrize("normals", [True, False])
def test_round_trip_bit_for_bit_on_a_side_stream(normals, tmp_path):
    s = special_splats()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        dev = {k: torch.from_numpy(v).to(DEV) for k, v in s.items()}
        P.save_ply(dev, tmp_path / "s.ply", normals=normals)
        back = P.load_ply(tmp_path / "s.ply", _chunk_rows=512)
        side.synchronize()
    assert_splats_equal(back, s, normals)
    header = P.read_ply_header(tmp_path / "s.ply")
    assert header.stride == (62 if normals else 59) * 4 and header.count == 700
    if normals:  # zeros where the reference writes np.zeros_like(means)
        rows = np.frombuffer((tmp_path / "s.ply").read_bytes(), header.numpy_dtype(), offset=header.payload_offset)
        assert not rows["nx"].view(np.uint32).any() and not rows["ny"].view(np.uint32).any() and not rows["nz"].view(np.uint32).any()


def test_round_trip_from_views_that_are_not_dense(tmp_path):
    """Slices and transposes are accepted: save_ply copies a view to a dense tensor before it packs."""
    s = special_splats(n=300)
    sh = torch.from_numpy(np.concatenate([s["sh0"], s["shN"]], axis=1)).to(DEV)  # [N, 16, 3]
    wide = torch.from_numpy(np.concatenate([s["means"], s["scales"], s["quats"]], axis=1)).to(DEV)  # [N, 10]
    views = {"means": wide[:, :3], "sh0": sh[:, :1], "shN": sh[:, 1:], "opacities": torch.from_numpy(np.stack([s["opacities"]] * 2, 1)).to(DEV)[:, 1],
             "scales": wide[:, 3:6], "quats": torch.from_numpy(np.ascontiguousarray(s["quats"].T)).to(DEV).t()}
    assert not any(v.is_contiguous() for v in views.values())
    P.save_ply(views, tmp_path / "v.ply")
    assert_splats_equal(P.load_ply(tmp_path / "v.ply"), s, "views")


def test_fused_decode_activations_against_float64(tmp_path):
    s = {k: v for k, v in G.asset_splats().items()}
    s["quats"][5] = 0.0  # the clamp of the normalisation
    s["quats"][6] = 1e-20
    P.save_ply({k: torch.from_numpy(v).to(DEV) for k, v in s.items()}, tmp_path / "g.ply")
    raw = P.load_ply(tmp_path / "g.ply")
    plain = P.load_ply_to_rasterizer_inputs(tmp_path / "g.ply", activate=False, normalize_quats=False)
    assert all(torch.equal(plain[k].view(torch.int32), raw[k].view(torch.int32)) for k in C.KEYS)
    act = P.load_ply_to_rasterizer_inputs(tmp_path / "g.ply")
    assert set(act) == {"means", "quats", "scales", "opacities", "sh0", "shN", "colors"}
    assert act["colors"].shape == (4096, 4, 3) and act["colors"].is_contiguous()
    assert act["sh0"].data_ptr() == act["colors"].data_ptr() and act["shN"].data_ptr() == act["colors"][:, 1:].data_ptr()  # views
    assert torch.equal(act["sh0"], raw["sh0"]) and torch.equal(act["shN"], raw["shN"]) and torch.equal(act["means"], raw["means"])
    assert np.allclose(N(act["scales"]), np.exp(s["scales"].astype(np.float64)), rtol=2e-6, atol=0)
    assert np.allclose(N(act["opacities"]), 1 / (1 + np.exp(-s["opacities"].astype(np.float64))), rtol=2e-6, atol=1e-9)
    q = s["quats"].astype(np.float64)
    want = q / np.maximum(np.linalg.norm(q, axis=-1, keepdims=True), 1e-12)
    print("quats: worst |fused - float64| =", float(np.abs(N(act["quats"]) - want).max()))
    assert np.allclose(N(act["quats"]), want, rtol=2e-6, atol=1e-7)
    assert np.array_equal(N(act["quats"])[5], np.zeros(4, np.float32))
    only_q = P.load_ply_to_rasterizer_inputs(tmp_path / "g.ply", activate=False)
    assert torch.equal(only_q["quats"], act["quats"]) and torch.equal(only_q["scales"], raw["scales"])


def test_render_from_both_routes_is_identical(tmp_path):
    """``ply_loader_renderer.py --ply_path`` both ways at 64 x 64: ``load_ply`` followed by the activations in torch, and the
    fused load.  Twice: as the reference's renderer feeds the rasterizer (its lines 680-682: ``torch.exp``, ``torch.sigmoid``, the
    quaternions as they are) against ``normalize_quats=False``; and with the quaternions normalised, the sum of squares written
    out left to right as ``gs_decode_splats`` and ``gs_ply_unpack`` add it, against the defaults.  The kernel's exp and sigmoid
    give torch's bits (0 of 16,384 values differ on an MI355X), so both pairs of images are equal bit for bit.
    ``F.normalize`` is not in that pair on purpose: torch adds the four squares pairwise, (a + b) + (c + d), which moves 1,990 of
    the 16,384 quaternion components by up to 2 ulp and the image by 1.8e-7."""
    from gscodec_studio_amd import rasterization

    s = G.asset_splats()
    P.save_ply({k: torch.from_numpy(v).to(DEV) for k, v in s.items()}, tmp_path / "g.ply")
    z = np.load(G.ASSET)
    vm = torch.from_numpy(z["viewmats"][:1]).to(DEV)
    K = z["Ks"][:1].copy()
    K[:, 0] *= 64.0 / float(z["width"])
    K[:, 1] *= 64.0 / float(z["height"])
    K = torch.from_numpy(K).to(DEV)

    def render(quats, scales, opacities, colors):
        return rasterization(raw["means"], quats, scales, opacities, colors, vm, K, 64, 64, sh_degree=1, packed=False)[:2]

    with torch.no_grad():
        raw = P.load_ply(tmp_path / "g.ply")
        q = raw["quats"]
        colors = torch.cat([raw["sh0"], raw["shN"]], 1)
        sumsq = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        routes = ((q, dict(normalize_quats=False)), (q / torch.sqrt(sumsq).clamp_min(1e-12)[:, None], dict()))
        for quats, flags in routes:
            a_img, a_alpha = render(quats, torch.exp(raw["scales"]), torch.sigmoid(raw["opacities"]), colors)
            f = P.load_ply_to_rasterizer_inputs(tmp_path / "g.ply", **flags)
            assert torch.equal(f["means"], raw["means"])
            b_img, b_alpha = render(f["quats"], f["scales"], f["opacities"], f["colors"])
            print(f"render {flags}: max |a - b| =", float((a_img - b_img).abs().max()), "coverage", float(a_alpha.mean()))
            assert float(a_alpha.max()) > 0.05  # something was drawn
            assert torch.equal(a_img, b_img) and torch.equal(a_alpha, b_alpha), flags


def test_tool_compress_then_decompress_in_a_child_process(tmp_path):
    from gscodec_studio_amd.compression import PngCompression

    s = G.asset_splats()
    P.save_ply({k: torch.from_numpy(v).to(DEV) for k, v in s.items()}, tmp_path / "in.ply")
    tool = os.path.join(C.ROOT, "tools", "ply_codec.py")
    for args in (["compress", str(tmp_path / "in.ply"), str(tmp_path / "dir"), "--sort", "morton"],
                 ["decompress", str(tmp_path / "dir"), str(tmp_path / "out.ply")]):
        r = subprocess.run([sys.executable, tool] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    want = PngCompression(verbose=False).decompress(str(tmp_path / "dir"))
    got = P.load_ply(tmp_path / "out.ply")
    assert got["means"].shape == (4096, 3)
    for k in C.KEYS:
        assert got[k].shape == want[k].shape and torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k


def test_refusals_on_the_device(tmp_path):
    s = special_splats(n=10, kn=3)
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in s.items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.save_ply({**dev, "scales": dev["scales"].cpu()}, tmp_path / "x.ply")
    with pytest.raises(ValueError, match="mismatched N"):
        P.save_ply({**dev, "scales": dev["scales"][:9]}, tmp_path / "x.ply")
    assert list(tmp_path.iterdir()) == []
    props = C.layout("standard", 3)
    (tmp_path / "short.ply").write_bytes(C.header_bytes(100000, props) + C.payload(99999, props).tobytes())
    torch.cuda.synchronize()
    before = (torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"])
    with pytest.raises(ValueError, match="payload shorter than 100000 rows"):
        P.load_ply(tmp_path / "short.ply")
    with pytest.raises(ValueError, match="payload shorter than 100000 rows"):
        P.load_ply_to_rasterizer_inputs(tmp_path / "short.ply")
    assert (torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]) == before  # nothing was allocated
