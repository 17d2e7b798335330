"""GPU: the spacetime file codec -- ``STGPngCompression`` against the directory the REFERENCE's class wrote and read back
(tests/golden/make_golden_stg_codec.py -> stg_codec.npz), and the one-launch decode ``decode_to_dynamic_inputs`` /
``gs_decode_dynamic_splats`` (csrc/codec.hip) against the per-attribute ``dequantize_grid`` + ``inverse_log_transform`` it
replaces.  Everything is compared bit for bit."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from util import N, T, golden

pytestmark = pytest.mark.gpu

from gscodec_studio_amd import _backend as B  # noqa: E402
from gscodec_studio_amd.compression import (STGPngCompression, decode_to_dynamic_inputs, dequantize_grid,  # noqa: E402
                                            inverse_log_transform, png_read, png_write)
from gscodec_studio_amd.compression.decode import DYNAMIC_ATTRIBUTES  # noqa: E402
from gscodec_studio_amd.compression.stg_compression import STG_ATTRIBUTE_CODECS  # noqa: E402

CASES = ["stg", "sh"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _case(case):
    gd = golden("stg_codec.npz")
    pick = lambda kind: {k.split(".", 2)[2]: gd[k] for k in gd.files if k.startswith(f"{case}.{kind}.")}  # noqa: E731
    return pick("input"), pick("plane"), json.loads(str(gd[f"{case}.meta"])), pick("decoded")


def _write_recorded_dir(d, planes, meta, decoded):
    """A directory as the reference left it: its planes through png_write, its meta.json, its .npz attributes."""
    for fn, img in planes.items():
        png_write(os.path.join(d, fn), img)
    for name in meta:
        if name not in STG_ATTRIBUTE_CODECS:
            np.savez_compressed(os.path.join(d, f"{name}.npz"), arr=decoded[name])
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump(meta, f)


@pytest.mark.parametrize("case", CASES)
def test_compress_writes_the_references_planes_and_meta(case, tmp_path):
    inputs, planes, meta, _ = _case(case)
    splats = {k: T(v) for k, v in inputs.items()}
    before = {k: (v, v.clone()) for k, v in splats.items()}
    STGPngCompression(use_sort=False, verbose=False).compress(str(tmp_path), splats)
    assert all(splats[k] is v and torch.equal(v, c) for k, (v, c) in before.items()) and list(splats) == list(before)
    written = sorted(p.name for p in tmp_path.iterdir())
    assert written == sorted(list(planes) + [f"{k}.npz" for k in meta if k not in STG_ATTRIBUTE_CODECS] + ["meta.json"])
    for fn, img in planes.items():
        got = png_read(str(tmp_path / fn))
        diff = int((got.astype(np.int32) != img.astype(np.int32)).sum()) if got.shape == img.shape else -1
        print(f"{case} {fn}: shape {got.shape}, {diff} byte(s) differ")
        assert got.shape == img.shape and got.dtype == np.uint8 and diff == 0, fn
    with open(tmp_path / "meta.json") as f:
        mine = json.load(f)
    assert list(mine) == list(meta)
    for name, m in meta.items():
        assert set(mine[name]) == set(m), name
        for key, v in m.items():
            if key in ("mins", "maxs"):
                assert np.array_equal(np.asarray(mine[name][key], np.float32), np.asarray(v, np.float32)), (name, key)
            else:
                assert mine[name][key] == v, (name, key)
    for name in meta:
        if name not in STG_ATTRIBUTE_CODECS:
            keep = np.argsort(-inputs["opacities"], kind="stable")[:289]
            assert np.array_equal(np.load(tmp_path / f"{name}.npz")["arr"], inputs[name][keep]), name


@pytest.mark.parametrize("case", CASES)
def test_decompress_reads_the_references_directory(case, tmp_path):
    """A directory as the reference wrote it decodes to the tensors the reference decoded, bit for bit (int32 views), the .npz
    attributes and the cropped count 289 included.  The means too: the inverse log transform rounds as torch's CPU expm1 does
    (``expm1_ref`` in csrc/codec.hip); with the device library's expm1f 101 / 867 (stg) and 103 / 867 (sh) of them were one ulp
    off."""
    _, planes, meta, decoded = _case(case)
    _write_recorded_dir(str(tmp_path), planes, meta, decoded)
    out = STGPngCompression(use_sort=False, verbose=False).decompress(str(tmp_path))
    assert list(out) == list(meta)
    differ = {}
    for name, ref in decoded.items():
        got = N(out[name])
        assert out[name].is_cuda and got.dtype == ref.dtype and got.shape == ref.shape and got.shape[0] == 289, name
        bad = int((_bits(got) != _bits(ref)).sum())
        print(f"{case} {name}: {bad} / {ref.size} values differ, max |diff| {np.abs(got - ref).max():.3g}")
        if bad:
            differ[name] = bad
    assert not differ, differ


def _random_file(n, seed, with_features, motion_images):
    """Random planes and meta of n splats: the means 16-bit, scales / quats at a bit depth drawn from {8, 6, 1}."""
    rng = np.random.default_rng(seed)
    arrays, meta = {}, {}
    for name, width in DYNAMIC_ATTRIBUTES:
        if not with_features and name in ("features_dir", "features_time"):
            continue
        lo = rng.normal(0, 2, width).astype(np.float32)
        m = {"shape": [n] if name == "opacities" else [n, width], "dtype": "float32", "mins": lo.tolist(),
             "maxs": (lo + rng.uniform(0.01, 5, width).astype(np.float32)).tolist()}
        bits = 8
        if STG_ATTRIBUTE_CODECS[name][0] == "kbit":
            bits = m["quantization"] = int(rng.choice([8, 6, 1]))
        plane = lambda w: torch.from_numpy((rng.integers(0, 1 << bits, (n, w)) << (8 - bits)).astype(np.uint8))  # noqa: E731
        if name == "means":
            arrays[name] = [plane(3), plane(3)]
        elif name == "motion":
            m["num_img"] = 3
            arrays[name] = [plane(3), plane(3), plane(3)]
            if not motion_images:
                arrays[name] = [torch.cat(arrays[name], dim=-1)]
        else:
            arrays[name] = [plane(width)]
        meta[name] = m
    return arrays, meta


def _composed(arrays, meta):
    """The decode as it composes from the per-attribute kernels."""
    out = {}
    for name, planes in arrays.items():
        if name == "motion" and len(planes) == 3:
            planes = [torch.cat(planes, dim=-1)]
        out[name] = dequantize_grid(planes, meta[name], device="cuda")
    out["means"] = inverse_log_transform(out["means"])
    return out


# 1: one lane; 255 / 256 / 257: a wave-group edge of the flat walk; 1023 / 1024 / 1025: both sides of the run of splats one
# workgroup owns; 4097: four full workgroups and a tail of one splat
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025, 4097])
@pytest.mark.parametrize("with_features", [True, False])
@pytest.mark.parametrize("motion_images", [True, False])
def test_fused_decode_equals_the_per_attribute_path(n, with_features, motion_images):
    arrays, meta = _random_file(n, 1000 * n + 2 * with_features + motion_images, with_features, motion_images)
    got = decode_to_dynamic_inputs(arrays, meta)
    ref = _composed(arrays, meta)
    assert list(got) == [k for k, _ in DYNAMIC_ATTRIBUTES if k in arrays]
    for name in ref:
        assert got[name].dtype == torch.float32 and list(got[name].shape) == meta[name]["shape"], name
        bad = int((got[name].view(torch.int32) != ref[name].view(torch.int32)).sum())
        assert bad == 0, (name, bad)
    # device planes are taken as they are
    again = decode_to_dynamic_inputs({k: [p.cuda() for p in v] for k, v in arrays.items()}, meta)
    assert all(torch.equal(again[k].view(torch.int32), got[k].view(torch.int32)) for k in got)


def test_extremes_decode_to_the_bounds():
    """All-0 planes decode to mins and all-255 planes to maxs exactly (bounds on a grid of eighths: maxs - mins and mins + range
    are exact in fp32, so the property is the arithmetic's, not luck); a means value that dequantises to 0 gives 0."""
    n = 300
    rng = np.random.default_rng(5)
    for fill in (0, 255):
        arrays, meta = {}, {}
        for name, width in DYNAMIC_ATTRIBUTES:
            lo = rng.integers(-40, 40, width).astype(np.float32) / 8
            hi = lo + rng.integers(1, 40, width).astype(np.float32) / 8
            meta[name] = {"shape": [n, width], "dtype": "float32", "mins": lo.tolist(), "maxs": hi.tolist()}
            if STG_ATTRIBUTE_CODECS[name][0] == "kbit":
                meta[name]["quantization"] = 8
            arrays[name] = [torch.full((n, width), fill, dtype=torch.uint8) for _ in range(2 if name == "means" else 1)]
        out = decode_to_dynamic_inputs(arrays, meta)
        for name, width in DYNAMIC_ATTRIBUTES:
            want = T(np.asarray(meta[name]["mins" if fill == 0 else "maxs"], np.float32))
            if name == "means":
                want = inverse_log_transform(want)
            assert torch.equal(out[name].view(torch.int32), want.expand(n, width).contiguous().view(torch.int32)), (name, fill)
    # q = 0x5555 = 21845 = 65535 / 3 on [-1, 2]: (1/3 in float64) * 3 - 1 = 0
    meta["means"].update(mins=[-1.0, -1.0, -1.0], maxs=[2.0, 2.0, 2.0])
    arrays["means"] = [torch.full((n, 3), 0x55, dtype=torch.uint8), torch.full((n, 3), 0x55, dtype=torch.uint8)]
    zero = decode_to_dynamic_inputs(arrays, meta)["means"]
    assert (zero == 0).all() and not torch.signbit(zero).any()


def test_round_trip_into_the_renderer(tmp_path):
    """compress -> decompress of the ``stg`` case goes straight into render_dynamic(features="stg") at 32 x 32, one camera: finite,
    something drawn, and the same image, bit for bit, as the tensors decompressed from the directory the reference wrote (those of
    test_decompress_reads_the_references_directory) and as the tensors the reference itself decoded."""
    from gscodec_studio_amd.dynamic import render_dynamic

    inputs, planes, meta, decoded = _case("stg")
    codec = STGPngCompression(use_sort=False, verbose=False)
    codec.compress(str(tmp_path / "mine"), {k: T(v) for k, v in inputs.items()})
    (tmp_path / "recorded").mkdir()
    _write_recorded_dir(str(tmp_path / "recorded"), planes, meta, decoded)
    viewmat = np.eye(4, dtype=np.float32)
    viewmat[2, 3] = 20.0
    viewmats, Ks = T(viewmat[None]), T(np.array([[[32.0, 0, 16.0], [0, 32.0, 16.0], [0, 0, 1]]], np.float32))
    images = []
    for splats in (codec.decompress(str(tmp_path / "mine")), codec.decompress(str(tmp_path / "recorded")),
                   {k: T(v) for k, v in decoded.items()}):
        rc, ra, _ = render_dynamic(splats, 0.4, viewmats, Ks, 32, 32, features="stg", packed=False)
        assert rc.shape == (1, 32, 32, 9) and torch.isfinite(rc).all() and torch.isfinite(ra).all()
        assert float(ra.max()) > 0  # something was drawn
        images.append((rc, ra))
    print(f"max |render - render of the reference's tensors| = {float((images[1][0] - images[2][0]).abs().max()):.3g}")
    for rc, ra in images[1:]:
        assert torch.equal(images[0][0].view(torch.int32), rc.view(torch.int32))
        assert torch.equal(images[0][1].view(torch.int32), ra.view(torch.int32))


def test_orderings_and_empty_attributes_round_trip(tmp_path):
    """use_sort="morton" / "grid" permute the splats and nothing else (the bounds are the same, so the decoded values are those
    of use_sort=False, bit for bit, in another order); an attribute with a zero in its shape is meta only and comes back as
    zeros."""
    inputs, _, _, _ = _case("stg")
    decoded = {}
    for order in (False, "morton", "grid"):
        d = tmp_path / str(order)
        splats = {k: T(v) for k, v in inputs.items()}
        splats["empty"] = torch.zeros((292, 0), device="cuda")
        STGPngCompression(use_sort=order, verbose=False).compress(str(d), splats)
        assert not (d / "empty.npz").exists() and not (d / "empty.png").exists()
        out = STGPngCompression(use_sort=order, verbose=False).decompress(str(d))
        assert list(out) == list(splats) and out["empty"].shape == (289, 0) and out["empty"].is_cuda
        key = N(out["extra"])[:, 0]  # (an .npz attribute: the same values under every order)
        decoded[order] = {k: N(v)[np.argsort(key, kind="stable")] for k, v in out.items()}
        if order:
            assert not np.array_equal(key, N(first["extra"])[:, 0]), order  # the order did change
            for name, v in decoded[False].items():
                assert np.array_equal(_bits(decoded[order][name]), _bits(v)), (order, name)
        else:
            first = out


def test_inverse_log_transform_is_the_references():
    """The library's inverse_log_transform on device tensors (gs_inverse_log_transform) equals torch's on the CPU, where the
    reference decodes, bit for bit: 4097 values over the range of log-means and beyond, signed zeros, tiny values, the overflow
    threshold, infinities and NaN."""
    rng = np.random.default_rng(7)
    y = np.concatenate([rng.uniform(-20, 20, 2000), rng.normal(0, 1, 2000), rng.uniform(-1e-4, 1e-4, 87),
                        [0.0, -0.0, 1e-40, -1e-40, 88.72283, 88.8, -88.8, np.inf, -np.inf, np.nan]]).astype(np.float32)
    ref = (torch.sign(torch.from_numpy(y)) * torch.expm1(torch.abs(torch.from_numpy(y)))).numpy()
    got = N(inverse_log_transform(T(y)))
    same = (_bits(got) == _bits(ref)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), (y[~same], got[~same], ref[~same])


def test_c_abi_guards():
    # n = 0: nothing is read, not even the pointer tables
    B.call("gs_decode_dynamic_splats", 0, None, None, None, None, None, None)
    n = 4
    planes = [torch.zeros(n * 9, dtype=torch.uint8, device="cuda") for _ in range(14)]
    outs = [torch.zeros(n * 9, device="cuda") for _ in range(11)]
    c_planes = (ctypes.c_void_p * 14)(*[B.ptr(p) for p in planes])
    c_outs = (ctypes.c_void_p * 11)(*[B.ptr(o) for o in outs])
    mins, maxs = (ctypes.c_float * 35)(*([0.25] * 35)), (ctypes.c_float * 35)(*([1.0] * 35))
    stream = torch.cuda.current_stream().cuda_stream

    def call(bits, c_planes=c_planes, c_outs=c_outs):
        c_bits = (ctypes.c_uint32 * 11)(*bits)
        B.call("gs_decode_dynamic_splats", n, ctypes.addressof(c_planes), ctypes.addressof(mins), ctypes.addressof(maxs),
               ctypes.addressof(c_bits), ctypes.addressof(c_outs), stream)

    with pytest.raises(RuntimeError, match="bit depths must be in 1..8"):
        call([16, 9] + [8] * 9)
    with pytest.raises(RuntimeError, match="bit depths must be in 1..8"):
        call([16] + [8] * 9 + [0])
    with pytest.raises(RuntimeError, match="16-bit"):
        call([8] * 11)
    no_omega = (ctypes.c_void_p * 14)(*[None if k == 10 else B.ptr(p) for k, p in enumerate(planes)])
    with pytest.raises(RuntimeError, match="required attribute"):
        call([16] + [8] * 10, c_planes=no_omega)
    two_images = (ctypes.c_void_p * 14)(*[None if k == 9 else B.ptr(p) for k, p in enumerate(planes)])
    with pytest.raises(RuntimeError, match="three images"):
        call([16] + [8] * 10, c_planes=two_images)
    assert all(float(o.abs().max()) == 0 for o in outs)  # none of the refused calls wrote anything
    call([16] + [8] * 10)  # and the well-formed call goes through: all-0 planes decode to the lower bound, n x C values each
    torch.cuda.synchronize()
    for o, (name, w) in zip(outs, DYNAMIC_ATTRIBUTES):
        want = float(np.expm1(np.float32(0.25))) if name == "means" else 0.25
        assert o[: n * w].cpu().numpy() == pytest.approx(want, rel=1e-6) and float(o[n * w:].abs().max() if n * w < o.numel() else 0) == 0, name
