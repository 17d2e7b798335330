"""File level of the reference's ``HevcCompression`` (gsplat/compression/hevc_compression.py:19-168): the ``--compression hevc``
choice of the trainer, the codec whose ``qp`` trades bytes for quality, with the reference's directory layout --

    meta.json                      one entry per attribute: shape, dtype, mins, maxs, quantization (plus what K-means adds)
    means_l.png, means_u.png       low / high byte of the 16-bit grid of the log-transformed means
    scales.bin quats.bin opacities.bin sh0.bin
                                   the 8-bit grid of the attribute, transform-coded at ``qp``
    shN.npz, mask.bin              masked K-means codebook, as PngCompression writes it
    <other>.npz                    anything else, under the key "arr"

The reference builds the lossy planes by shelling out to ``ffmpeg -c:v libx265 -x265-params qp=<qp>`` and reads the ``.mp4`` back
through imageio-ffmpeg.  Neither belongs on this backend: the class, its fields, the registry names, the directory and
``meta.json`` are kept, and the payload is this project's own bitstream (``plane_codec_reference`` defines it, csrc/plane_codec.hip
codes it on the GPU).  That bitstream is NOT a replication of x265: it has HEVC's 8 x 8 integer transform and flat quantiser, so
``qp`` keeps its meaning (Qstep = 2^((qp - 4) / 6)), and no intra prediction, no rate-distortion optimisation and no CABAC.
``decompress`` says so when it meets an ``.mp4``.  Two further differences: the quats are ONE four-channel file (the reference
splits them 3 + 1 only because of the video pixel formats), and no debug ``.npy`` or intermediate PNG is written.
"""
from __future__ import annotations

import os
from dataclasses import InitVar, dataclass, field
from typing import Any, Dict, Optional, Union

import numpy as np
import torch
from torch import Tensor

from ._container import prepare_splats, read_directory, write_directory
from .entropy_coding_compression import (_compress_masked_kmeans, _compress_png, _compress_png_16bit, _decompress_masked_kmeans,
                                         _decompress_png, _decompress_png_16bit)
from .grid_codec import dequantize_grid, inverse_log_transform, quantize_grid
from .plane_codec import _check_qp, plane_decode, plane_encode

NO_X265 = ("{path}: this directory holds the reference's x265 video payload ({mp4}) and no {name}.bin.  x265 payloads are not read "
           "here: HevcCompression of this implementation writes its own transform-coded planes (<name>.bin).  Every other file of "
           "the directory (means_l.png, means_u.png, shN.npz, mask.bin, <other>.npz, meta.json) is interchangeable.")


def _compress_hevc_kbit(compress_dir: str, param_name: str, params: Tensor, n_sidelen: int, quantization: int = 8, qp: int = 10,
                        stream_len: int = 4096, **kwargs) -> Dict[str, Any]:
    """250-308: the k-bit min-max grid of the attribute (``gs_grid_quantize``), transform-coded at ``qp`` into ``<name>.bin``.
    Meta: shape, dtype, mins, maxs, quantization."""
    (plane,), meta = quantize_grid(params, n_sidelen, bits=quantization, kbit=True)
    plane_encode(plane, qp, stream_len=stream_len).tofile(os.path.join(compress_dir, f"{param_name}.bin"))
    return meta


def _decompress_hevc_kbit(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    """311-353: decode the plane, then ``gs_grid_dequantize``."""
    path = os.path.join(compress_dir, f"{param_name}.bin")
    if not os.path.exists(path):
        for mp4 in (f"{param_name}.mp4", f"{param_name}_u.mp4", f"{param_name}_l.mp4"):
            if os.path.exists(os.path.join(compress_dir, mp4)):
                raise ValueError(NO_X265.format(path=compress_dir, mp4=mp4, name=param_name))
    plane = plane_decode(np.fromfile(path, dtype=np.uint8), device=device, what=path)
    if plane.shape[0] * plane.shape[1] != meta["shape"][0] or plane.shape[2] != len(np.atleast_1d(meta["mins"])):
        raise ValueError(f"{path}: a plane of {tuple(plane.shape)}, meta.json describes {meta['shape']}")
    return dequantize_grid([plane], meta, device=device)


# the reference keeps two functions because it splits the quats into a 3-channel and a 1-channel video; here they are one file
def _compress_quats_hevc_kbit(compress_dir: str, param_name: str, params: Tensor, n_sidelen: int, **kwargs) -> Dict[str, Any]:
    return _compress_hevc_kbit(compress_dir, param_name, params, n_sidelen, **kwargs)


def _decompress_quats_hevc_kbit(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    return _decompress_hevc_kbit(compress_dir, param_name, meta, device=device)


# the names attribute_codec_registry may use
_AVAILABLE = {fn.__name__: fn for fn in (
    _compress_png_16bit, _compress_png, _compress_hevc_kbit, _compress_quats_hevc_kbit, _compress_masked_kmeans,
    _decompress_png_16bit, _decompress_png, _decompress_hevc_kbit, _decompress_quats_hevc_kbit, _decompress_masked_kmeans)}


@dataclass
class HevcCompression:
    """The reference's ``HevcCompression``: same fields, same directory (see the module docstring for the payload of the ``.bin``
    files).  ``qp`` (0..51) is the quantisation parameter of every transform-coded attribute; ``qp_per_attribute`` overrides it by
    name (an extension, for rate-distortion sweeps).  ``use_sort``, ``kmeans_method`` and ``attribute_codec_registry`` as in
    ``EntropyCodingCompression``: the registry maps an attribute to ``{"encode": <name>, "decode": <name>}`` with the reference's
    function names as strings, e.g. ``{"opacities": {"encode": "_compress_png", "decode": "_decompress_png"}}``.  Works on
    detached copies; the caller's dictionary is not written to."""

    use_sort: Union[bool, str] = True
    verbose: bool = True
    n_clusters: int = 32768
    qp: int = 4
    attribute_codec_registry: InitVar[Optional[Dict[str, Dict[str, str]]]] = None
    opacity_threshold: float = 0.005  # outlier filter (outlier_filter.py:8-9, 32-37)

    compress_fn_map: Dict[str, str] = field(default_factory=lambda: {
        "means": "_compress_png_16bit", "scales": "_compress_hevc_kbit", "quats": "_compress_quats_hevc_kbit",
        "opacities": "_compress_hevc_kbit", "sh0": "_compress_hevc_kbit", "shN": "_compress_masked_kmeans"})
    decompress_fn_map: Dict[str, str] = field(default_factory=lambda: {
        "means": "_decompress_png_16bit", "scales": "_decompress_hevc_kbit", "quats": "_decompress_quats_hevc_kbit",
        "opacities": "_decompress_hevc_kbit", "sh0": "_decompress_hevc_kbit", "shN": "_decompress_masked_kmeans"})
    kmeans_method: str = "torch"
    qp_per_attribute: Optional[Dict[str, int]] = None

    def __post_init__(self, attribute_codec_registry):
        for attr_name, attr_codec in (attribute_codec_registry or {}).items():
            for key, fn_map in (("encode", self.compress_fn_map), ("decode", self.decompress_fn_map)):
                if attr_name in fn_map and key in attr_codec:
                    if attr_codec[key] in _AVAILABLE:
                        fn_map[attr_name] = attr_codec[key]
                    else:
                        print(f"Warning: Unknown func: {attr_codec[key]}")

    def qp_of(self, name: str) -> int:
        return (self.qp_per_attribute or {}).get(name, self.qp)

    @torch.no_grad()
    def compress(self, compress_dir: str, splats: Dict[str, Tensor], entropy_models=None) -> None:
        if entropy_models is not None:
            raise ValueError("HevcCompression should not require entropy_models")
        for name in splats:  # before the directory is touched
            _check_qp(self.qp_of(name))
        splats, side = prepare_splats(splats, self.opacity_threshold, self.use_sort, self.verbose)

        def encode(name, value, _):
            if name not in self.compress_fn_map:
                return None
            return _AVAILABLE[self.compress_fn_map[name]](compress_dir, name, value, n_sidelen=side, n_clusters=self.n_clusters,
                                                          verbose=self.verbose, kmeans_method=self.kmeans_method, qp=self.qp_of(name))

        write_directory(compress_dir, splats, encode)

    @torch.no_grad()
    def decompress(self, compress_dir: str, device="cuda") -> Dict[str, Tensor]:
        def decode(name, m, _):
            if name not in self.decompress_fn_map:
                return None
            return _AVAILABLE[self.decompress_fn_map[name]](compress_dir, name, m, device=device)

        splats = read_directory(compress_dir, decode, device)
        splats["means"] = inverse_log_transform(splats["means"])
        return splats
