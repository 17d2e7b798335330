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

``use_sort`` as in ``PngCompression``: True = PLAS through ``sort_splats`` (ImportError without the package, as in the reference),
"morton" / "grid" = this library's own orderings, False = keep the order.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Any, Dict, List, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .decode import DYNAMIC_ATTRIBUTES, decode_to_dynamic_inputs, morton_order, sort_splats
from .grid_codec import _crop_to_square, dequantize_grid, inverse_log_transform, log_transform, quantize_grid
from .grid_sort import sort_splats_grid
from .png_compression import _meta_of, png_read, png_write

# attribute -> (codec kind, bits, files): the reference's compress_fn_map / decompress_fn_map (stg_compression.py:47-83);
# "16" = _compress_png_16bit, "kbit" = _compress_png_kbit, "plain" = _compress_png, "multi" = _compress_multiple_png
STG_ATTRIBUTE_CODECS: Dict[str, Tuple[str, int, Tuple[str, ...]]] = {
    "means": ("16", 16, ("means_l.png", "means_u.png")),
    "scales": ("kbit", 8, ("scales.png",)),
    "quats": ("kbit", 8, ("quats.png",)),
    "opacities": ("plain", 8, ("opacities.png",)),
    "trbf_center": ("plain", 8, ("trbf_center.png",)),
    "trbf_scale": ("plain", 8, ("trbf_scale.png",)),
    "motion": ("multi", 8, ("motion_0.png", "motion_1.png", "motion_2.png")),
    "omega": ("plain", 8, ("omega.png",)),
    "colors": ("plain", 8, ("colors.png",)),
    "features_dir": ("plain", 8, ("features_dir.png",)),
    "features_time": ("plain", 8, ("features_time.png",)),
}
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
    """The reference's ``STGPngCompression`` (same constructor arguments, same files).  ``use_sort``: True = PLAS (external
    package, as in the reference), "morton" = the deterministic Morton order, "grid" = the library's grid sort, False = keep
    the order."""

    use_sort: Union[bool, str] = True
    verbose: bool = True

    @torch.no_grad()
    def compress(self, compress_dir: str, splats: Dict[str, Tensor]) -> None:
        for value in splats.values():
            _require_device("compress", value.device)
        os.makedirs(compress_dir, exist_ok=True)
        splats = {k: v.detach() for k, v in splats.items()}
        splats["means"] = log_transform(splats["means"])
        splats["quats"] = _normalize_quats(splats["quats"])
        n_before = len(splats["means"])
        splats, side = _crop_to_square(splats)
        if len(splats["means"]) != n_before:  # (the reference prints this unconditionally)
            print(f"Warning: Number of Gaussians was not square. Removed {n_before - len(splats['means'])} Gaussians.")
        if self.use_sort == "morton":
            order = morton_order(splats["means"])
            splats = {k: v[order] for k, v in splats.items()}
        elif self.use_sort == "grid":
            splats = sort_splats_grid(splats, verbose=self.verbose)
        elif self.use_sort:
            splats = sort_splats(splats, verbose=self.verbose)

        meta: Dict[str, Any] = {}
        for name, value in splats.items():
            if value.numel() == 0:
                meta[name] = _meta_of(value)
            elif name in STG_ATTRIBUTE_CODECS:
                kind, bits, files = STG_ATTRIBUTE_CODECS[name]
                planes, meta[name] = quantize_grid(value, side, bits=bits, kbit=(kind == "kbit"))
                if kind == "multi":  # one grid over all channels, three channels per image
                    grid = planes[0].reshape(side, side, -1)
                    num_img = (grid.shape[-1] + 2) // 3
                    planes = [grid[..., 3 * i:3 * i + 3] for i in range(num_img)]
                    files = tuple(f"{name}_{i}.png" for i in range(num_img))
                    meta[name]["num_img"] = num_img
                for fn, plane in zip(files, planes):
                    png_write(os.path.join(compress_dir, fn), plane.cpu().numpy())
            else:
                np.savez_compressed(os.path.join(compress_dir, f"{name}.npz"), arr=value.cpu().numpy())
                meta[name] = _meta_of(value)
        with open(os.path.join(compress_dir, "meta.json"), "w") as f:
            json.dump(meta, f)

    @torch.no_grad()
    def decompress(self, compress_dir: str, device="cuda") -> Dict[str, Tensor]:
        _require_device("decompress", device)
        with open(os.path.join(compress_dir, "meta.json"), "r") as f:
            meta = json.load(f)
        splats: Dict[str, Tensor] = {}
        arrays: Dict[str, List[Tensor]] = {}
        for name, m in meta.items():
            if not np.all(m["shape"]):
                splats[name] = torch.zeros(m["shape"], dtype=getattr(torch, m["dtype"]), device=device)
            elif name in STG_ATTRIBUTE_CODECS:
                kind, _, files = STG_ATTRIBUTE_CODECS[name]
                if kind == "multi":
                    files = tuple(f"{name}_{i}.png" for i in range(int(m["num_img"])))
                arrays[name] = [torch.from_numpy(png_read(os.path.join(compress_dir, fn))) for fn in files]
                splats[name] = None  # (keeps the meta's order)
            else:
                arr = np.load(os.path.join(compress_dir, f"{name}.npz"))["arr"]
                splats[name] = torch.tensor(arr).reshape(m["shape"]).to(dtype=getattr(torch, m["dtype"]), device=device)
        if all(k in arrays for k in _REQUIRED):
            splats.update(decode_to_dynamic_inputs(arrays, {k: meta[k] for k in arrays}, device=device))
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
