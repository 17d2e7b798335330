"""File level of the reference's spacetime codec: ``STGPngCompression.compress(compress_dir, splats)`` / ``decompress(compress_dir)``
(gsplat/compression/stg_compression.py:16-143), what the two dynamic trainers import next to ``PngCompression`` and run as
``--compression stg``.  Same directory layout, file names and ``meta.json``, so either implementation reads the other's directories --

    means_l.png, means_u.png                     16-bit grid of log_transform(means)
    scales.png, quats.png                        k-bit grids (``quantization: 8`` in the meta), the quats normalised first
    opacities.png trbf_center.png trbf_scale.png omega.png colors.png features_dir.png features_time.png
                                                 8-bit grids (grey for 1 channel, RGB for 3, RGBA for 4)
    motion_0.png motion_1.png motion_2.png       ONE 8-bit grid over the nine channels, written three channels per image
                                                 (``num_img: 3`` in the meta)
    <other>.npz                                  anything else under the key "arr" -- ``sh0`` and ``shN`` included: the reference's
                                                 STG map does not list them

Order of operations, the reference's: log transform of the means and normalised quats, crop to a square count by dropping the
lowest raw opacities, the ordering, the per-attribute codec; ``decompress`` ends with the inverse log transform.  There is NO
opacity filter (unlike ``PngCompression`` here).  ``decompress`` decodes the planes of the table with one launch
(``decode.decode_to_dynamic_inputs``, csrc/codec.hip) when the nine attributes ``render_dynamic`` needs are all there, and attribute
by attribute through ``dequantize_grid`` otherwise; the result is the RAW parameter dict ``render_dynamic`` takes.  Every attribute,
the means included, decodes to the reference's bits: the inverse log transform rounds as torch's CPU ``expm1`` does.

Three deliberate differences from the reference:

* ``compress`` works on detached copies; the reference overwrites the caller's dict with the transformed, cropped tensors (the
  trainers do not rely on that).
* the reference's empty-attribute branches are dead or wrong (``torch.numel == 0`` is never true, and ``_decompress_*`` returns the
  meta dict for a zero-size shape): here an attribute with a zero in its shape is written as meta only and decodes to
  ``torch.zeros(shape)``, as in ``PngCompression``.
* CPU tensors raise ``RuntimeError`` (no CPU fallback), as everywhere in ``compression``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from ._container import DEFERRED, plane_files, prepare_splats, read_directory, read_planes, write_directory, write_planes
from .decode import DYNAMIC_ATTRIBUTES, decode_to_dynamic_inputs
from .grid_codec import dequantize_grid, inverse_log_transform, quantize_grid

# attribute -> (codec kind, bits, files): the reference's compress_fn_map / decompress_fn_map (stg_compression.py:47-83);
# "16" = _compress_png_16bit, "kbit" = _compress_png_kbit, "plain" = _compress_png, "multi" = _compress_multiple_png (3 images)
STG_ATTRIBUTE_CODECS: Dict[str, Tuple[str, int, Tuple[str, ...]]] = {
    name: (kind, 16 if kind == "16" else 8, plane_files(name, kind, 3))
    for name, kind in (("means", "16"), ("scales", "kbit"), ("quats", "kbit"), ("opacities", "plain"), ("trbf_center", "plain"),
                       ("trbf_scale", "plain"), ("motion", "multi"), ("omega", "plain"), ("colors", "plain"),
                       ("features_dir", "plain"), ("features_time", "plain"))}
_REQUIRED = tuple(name for name, _ in DYNAMIC_ATTRIBUTES[:9])  # what the one-launch decode cannot do without


def _require_device(where: str, device) -> None:
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"STGPngCompression.{where}: the HIP path needs a GPU device (no CPU fallback)")


def _normalize_quats(q: Tensor) -> Tensor:
    """``F.normalize(q, dim=-1)`` = q / max(||q||, 1e-12) as the reference's CPU run rounds it: the squares summed in channel
    order in fp32, one rounding per operation (separate elementwise launches, so nothing is contracted or reordered), then a
    correctly rounded square root and quotient (taken in float64 and rounded once more, which is exact for both).  A reduction
    kernel may sum in another order, and the last bit of the norm reaches the ``mins`` / ``maxs`` of meta.json."""
    sq = q * q
    s = sq[..., 0]
    for c in range(1, q.shape[-1]):
        s = s + sq[..., c]
    norm = torch.sqrt(s.double()).float().clamp_min(1e-12)
    return (q.double() / norm.double().unsqueeze(-1)).to(q.dtype)


@dataclass
class STGPngCompression:
    """The reference's ``STGPngCompression`` (same constructor arguments, same files).  ``use_sort`` as in ``PngCompression``."""

    use_sort: Union[bool, str] = True
    verbose: bool = True

    @torch.no_grad()
    def compress(self, compress_dir: str, splats: Dict[str, Tensor]) -> None:
        for value in splats.values():
            _require_device("compress", value.device)
        splats, side = prepare_splats(splats, None, self.use_sort, self.verbose, normalize_quats=_normalize_quats,
                                      always_warn=True)  # (the reference prints the crop warning unconditionally)

        def encode(name, value, _):
            if name not in STG_ATTRIBUTE_CODECS:
                return None
            kind, bits = STG_ATTRIBUTE_CODECS[name][:2]
            planes, m = quantize_grid(value, side, bits=bits, kbit=(kind == "kbit"))
            if kind == "multi":  # one grid over all channels, three channels per image
                grid = planes[0].reshape(side, side, -1)
                m["num_img"] = (grid.shape[-1] + 2) // 3
                planes = [grid[..., 3 * i:3 * i + 3] for i in range(m["num_img"])]
            write_planes(compress_dir, name, kind, planes)
            return m

        write_directory(compress_dir, splats, encode)

    @torch.no_grad()
    def decompress(self, compress_dir: str, device="cuda") -> Dict[str, Tensor]:
        _require_device("decompress", device)
        arrays, meta = {}, {}  # of the table's attributes: planes as read, meta.json entries

        def decode(name, m, _):  # only reads the planes: they are decoded together below
            if name not in STG_ATTRIBUTE_CODECS:
                return None
            kind = STG_ATTRIBUTE_CODECS[name][0]
            arrays[name] = read_planes(compress_dir, name, kind, int(m["num_img"]) if kind == "multi" else 0)
            meta[name] = m
            return DEFERRED

        splats = read_directory(compress_dir, decode, device)
        if all(k in arrays for k in _REQUIRED):
            splats.update(decode_to_dynamic_inputs(arrays, meta, device=device))
        else:  # not a full spacetime set (e.g. no colors next to sh0 / shN): the same arithmetic, attribute by attribute
            for name, planes in arrays.items():
                if STG_ATTRIBUTE_CODECS[name][0] == "multi":
                    planes = [torch.cat([p.reshape(p.shape[0], p.shape[1], -1) for p in planes], dim=-1)]
                want = [int(np.prod(meta[name]["shape"]))] * (2 if name == "means" else 1)
                if [int(p.numel()) for p in planes] != want:  # file contents: never a read past a plane
                    raise ValueError(f"STGPngCompression.decompress: {name}: plane sizes {[int(p.numel()) for p in planes]} bytes, "
                                     f"expected {want}")
                splats[name] = dequantize_grid(planes, meta[name], device=device)
            if "means" in arrays:
                splats["means"] = inverse_log_transform(splats["means"])
        return splats
