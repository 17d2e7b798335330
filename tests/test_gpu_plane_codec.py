"""The transform-coded planes on the GPU (csrc/plane_codec.hip behind gscodec_studio_amd.compression.plane_codec) and
HevcCompression: levels, planes and file bytes equal to the numpy module that defines the format
(gscodec_studio_amd/compression/plane_codec_reference.py), element for element, and the directory level.  Only valid streams are
decoded here; what a damaged file does to the kernel is argued from its bounded reads (ans_range / ans_byte, the clamped levels)."""
import json
import os

import numpy as np
import pytest
import torch

from plane_codec_cases import (CASE_IDS, CASES, ODD_STREAM_LEN, QPS, STREAM_LENS, case_plane, garden_splats, plane, reference_blob,
                               reference_plane)
from util import N, T

pytestmark = pytest.mark.gpu

from gscodec_studio_amd.compression import plane_codec_reference as R  # noqa: E402


def test_forward_transform_matches_the_module():
    from gscodec_studio_amd.compression.plane_codec import transform_levels

    for case in CASES:
        p = case_plane(case)
        for qp in QPS:
            got = transform_levels(T(p), qp)
            assert got.dtype == torch.int16 and np.array_equal(N(got), R.forward_levels(p, qp)), (case[0], qp)
    two_d = plane("smooth", 24, 24, 1)[:, :, 0]
    assert np.array_equal(N(transform_levels(T(two_d), 4)), R.forward_levels(two_d, 4))


def test_inverse_transform_matches_the_module():
    """On the levels the forward transform gives, and on int16 levels drawn over the full range, -32768 included: the clamp."""
    from gscodec_studio_amd.compression.plane_codec import inverse_transform

    rng = np.random.default_rng(5)
    for case in CASES:
        p = case_plane(case)
        h, w, ch = p.shape
        for qp in QPS:
            lv = R.forward_levels(p, qp)
            assert np.array_equal(N(inverse_transform(T(lv), qp, h, w)), reference_plane(case[0], qp)), (case[0], qp)
        wild = rng.integers(-32768, 32768, (ch, R.n_blocks(h, w), 64)).astype(np.int16)
        wild[0, 0, :4] = [-32768, 32767, -32767, 0]
        for qp in (0, 29, 51):
            assert np.array_equal(N(inverse_transform(T(wild), qp, h, w)), R.inverse_levels(wild, qp, h, w)), (case[0], qp)


@pytest.mark.parametrize("name", CASE_IDS)
def test_files_and_planes_match_the_module(name):
    """plane_encode writes the module's bytes; plane_decode reads the module's file into the module's plane."""
    from gscodec_studio_amd.compression import plane_decode, plane_encode

    p = T(case_plane(CASES[CASE_IDS.index(name)]))
    for qp in (0, 22, 51):
        for s_len in STREAM_LENS:
            want = reference_blob(name, qp, s_len)
            got = plane_encode(p, qp, stream_len=s_len)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (name, qp, s_len)
            out = plane_decode(want, device="cuda")
            assert out.dtype == torch.uint8 and out.is_cuda and np.array_equal(N(out), reference_plane(name, qp)), (name, qp, s_len)


def test_cross_reading_side_stream_and_odd_stream_lengths():
    """The numpy module reads what plane_encode wrote; streams that end inside a block and other resolutions; a side stream."""
    from gscodec_studio_amd.compression import plane_decode, plane_encode

    for content, ch, bits in (("smooth", 3, 14), ("checker", 4, 11), ("noise", 1, 8)):
        p = plane(content, 100, 100, ch)
        blob = plane_encode(T(p), 22, stream_len=ODD_STREAM_LEN, bits=bits)
        assert np.array_equal(blob, R.encode(p, 22, stream_len=ODD_STREAM_LEN, bits=bits))
        assert np.array_equal(R.decode(blob), R.reconstruct(p, 22))
        assert np.array_equal(N(plane_decode(blob.tobytes())), R.reconstruct(p, 22))  # bytes or an array
    name = "smooth-100x100x3"
    p = T(case_plane(CASES[CASE_IDS.index(name)]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        blob = plane_encode(p, 22, stream_len=64)
        out = plane_decode(reference_blob(name, 22, 64))
    side.synchronize()
    assert np.array_equal(blob, reference_blob(name, 22, 64)) and np.array_equal(N(out), reference_plane(name, 22))


def _splats():
    return {k: torch.from_numpy(np.array(v)).cuda() for k, v in garden_splats().items()}


PLANE_ATTRIBUTES = ("scales", "quats", "opacities", "sh0")


@pytest.mark.parametrize("use_sort", [False, "morton"])
@pytest.mark.parametrize("qp", [4, 34])
def test_directory_round_trip(qp, use_sort, tmp_path):
    from gscodec_studio_amd.compression import HevcCompression, PngCompression, dequantize_grid, quantize_grid
    from gscodec_studio_amd.compression._container import prepare_splats

    splats = _splats()
    before = {k: v.clone() for k, v in splats.items()}
    d = str(tmp_path / "hevc")
    codec = HevcCompression(use_sort=use_sort, verbose=False, n_clusters=256, qp=qp, kmeans_method="fixed")
    codec.compress(d, splats)
    assert all(torch.equal(splats[k], before[k]) for k in before)  # the caller's dictionary is left alone
    assert sorted(os.listdir(d)) == sorted("means_l.png means_u.png scales.bin quats.bin opacities.bin sh0.bin shN.npz mask.bin meta.json".split())
    with open(os.path.join(d, "meta.json")) as f:
        meta = json.load(f)
    assert list(meta) == ["means", "scales", "quats", "opacities", "sh0", "shN"]
    assert set(meta["means"]) == {"shape", "dtype", "mins", "maxs"}
    for k in PLANE_ATTRIBUTES:
        assert set(meta[k]) == {"shape", "dtype", "mins", "maxs", "quantization"} and meta[k]["quantization"] == 8, k
    out = HevcCompression(verbose=False).decompress(d)  # decoding needs none of the encoder's settings: qp is in the file

    d_png = str(tmp_path / "png")
    png = PngCompression(use_sort=use_sort, verbose=False, n_clusters=256, kmeans_method="fixed")
    png.compress(d_png, splats)
    want = png.decompress(d_png)
    assert list(out) == list(want)
    for k in want:
        assert out[k].shape == want[k].shape and out[k].dtype == want[k].dtype and out[k].device == want[k].device, k
    assert torch.equal(out["means"], want["means"]) and torch.equal(out["shN"], want["shN"])

    kept, side = prepare_splats(splats, 0.005, use_sort, False)
    assert side == 64
    worst = {}
    for k in PLANE_ATTRIBUTES:  # dequantize_grid of the numpy module's reconstruction of the very plane the codec was handed
        (p,), m = quantize_grid(kept[k], side, bits=8, kbit=True)
        assert m == meta[k]
        blob = np.fromfile(os.path.join(d, f"{k}.bin"), np.uint8)
        head = R.parse_container(blob)[0]
        assert (head.qp, head.height, head.width, head.channels, head.stream_len) == (qp, 64, 64, kept[k][0].numel(), 4096)
        assert np.array_equal(blob, R.encode(N(p), qp))
        rec = R.reconstruct(N(p), qp)
        assert torch.equal(out[k], dequantize_grid([T(rec)], m)), k
        worst[k] = int(np.abs(rec.astype(np.int64) - N(p).reshape(rec.shape)).max())
    if qp == 4:  # nearly the PNG codec's values: Qstep = 1
        assert max(worst.values()) <= 2, worst


def test_directory_registry_qp_per_attribute_and_refusals(tmp_path):
    from gscodec_studio_amd.compression import HevcCompression, PngCompression

    splats = _splats()
    with pytest.raises(ValueError, match="should not require entropy_models"):
        HevcCompression(use_sort=False, verbose=False).compress(str(tmp_path / "no"), splats, entropy_models={})
    assert not os.path.exists(tmp_path / "no")
    with pytest.raises(ImportError):  # PLAS, as in the reference
        HevcCompression(verbose=False).compress(str(tmp_path / "plas"), splats)

    # opacities through the plain PNG codec: the PNG codec's values; the other attributes as without the registry
    d = str(tmp_path / "plain")
    HevcCompression(use_sort=False, verbose=False, n_clusters=64, qp=22).compress(d, splats)
    want = HevcCompression().decompress(d)
    reg = {"opacities": {"encode": "_compress_png", "decode": "_decompress_png"}, "scales": {"encode": "_no_such_function"}}
    d2 = str(tmp_path / "registry")
    HevcCompression(use_sort=False, verbose=False, n_clusters=64, qp=22, attribute_codec_registry=reg).compress(d2, splats)
    names = os.listdir(d2)
    assert "opacities.png" in names and "opacities.bin" not in names and "scales.bin" in names
    got = HevcCompression(attribute_codec_registry=reg).decompress(d2)
    d_png = str(tmp_path / "png")
    PngCompression(use_sort=False, verbose=False, n_clusters=64).compress(d_png, splats)
    assert torch.equal(got["opacities"], PngCompression().decompress(d_png)["opacities"])
    assert all(torch.equal(got[k], want[k]) for k in ("means", "scales", "quats", "sh0"))

    # qp_per_attribute: the named attribute's file carries that qp, the others the class's
    d3 = str(tmp_path / "per")
    HevcCompression(use_sort=False, verbose=False, n_clusters=64, qp=22, qp_per_attribute={"sh0": 10, "quats": 40}).compress(d3, splats)
    qps = {k: R.parse_container(np.fromfile(os.path.join(d3, f"{k}.bin"), np.uint8))[0].qp for k in PLANE_ATTRIBUTES}
    assert qps == {"scales": 22, "quats": 40, "opacities": 22, "sh0": 10}
    for k in ("scales", "opacities"):
        assert np.array_equal(np.fromfile(os.path.join(d3, f"{k}.bin"), np.uint8), np.fromfile(os.path.join(d, f"{k}.bin"), np.uint8))
    assert os.path.getsize(os.path.join(d3, "sh0.bin")) > os.path.getsize(os.path.join(d, "sh0.bin"))
    assert os.path.getsize(os.path.join(d3, "quats.bin")) < os.path.getsize(os.path.join(d, "quats.bin"))
    per = HevcCompression().decompress(d3)
    assert torch.equal(per["scales"], want["scales"]) and not torch.equal(per["sh0"], want["sh0"])

    # a directory of the reference's: x265 payloads are refused by name, other damage by the container's checks
    os.rename(os.path.join(d3, "sh0.bin"), os.path.join(d3, "sh0.mp4"))
    with pytest.raises(ValueError, match="x265 payloads are not read here") as e:
        HevcCompression().decompress(d3)
    assert "sh0.mp4" in str(e.value) and "interchangeable" in str(e.value)
    os.rename(os.path.join(d3, "quats.bin"), os.path.join(d3, "quats_u.mp4"))
    os.rename(os.path.join(d3, "sh0.mp4"), os.path.join(d3, "sh0.bin"))
    with pytest.raises(ValueError, match="quats_u.mp4"):
        HevcCompression().decompress(d3)
    blob = np.fromfile(os.path.join(d, "scales.bin"), np.uint8)
    blob[:-3].tofile(os.path.join(d, "scales.bin"))
    with pytest.raises(ValueError, match="scales.bin"):
        HevcCompression().decompress(d)
