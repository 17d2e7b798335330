"""File level of the reference's PNG codec: ``PngCompression.compress(compress_dir, splats)`` /
``decompress(compress_dir)`` with the SAME directory layout (gsplat/compression/png_compression.py:17-162) --

    meta.json                      one entry per attribute (shape, dtype, mins, maxs, quantization, mask_bits, ...)
    means_l.png, means_u.png       low / high byte of the 16-bit grid of the log-transformed means
    scales.png quats.png sh0.png   k-bit grids, values in the top bits of the byte
    opacities.png                  8-bit grid
    shN.npz, mask.bin              K-means codebook (uint8 centroids, uint16 labels) of the splats that have higher SH bands at
                                   all, and the packed bit mask that says which
    <other>.npz                    anything else, under the key "arr"

so a directory written by either implementation is read by the other.  The quantisation arithmetic runs in the HIP kernels
of ``grid_codec`` / ``decode``, and the directory itself -- the preparation and ordering of the splats, the loop over the
attributes, ``meta.json``, the PNG files -- is ``_container``'s; what is here is which attribute goes to which of them.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Union

import torch
from torch import Tensor

from ._container import (compress_masked_kmeans, decompress_masked_kmeans, prepare_splats, read_directory, read_planes,
                         write_directory, write_planes)
from .grid_codec import ATTRIBUTE_CODECS, dequantize_grid, inverse_log_transform, quantize_grid


@dataclass
class PngCompression:
    """The reference's ``PngCompression`` (same constructor arguments, same files).  ``use_sort``: True = PLAS (external
    package, as in the reference: ImportError without it), "morton" = the deterministic Morton order of the means, "grid" = the
    library's grid sort over every attribute (``grid_sort``), False = keep the order.  ``kmeans_method``: how the shN codebook is clustered, "torch" (float Lloyd iteration in torch) or "fixed" (the
    fixed-point kernels of csrc/kmeans.hip, reproducible bit for bit); the files have the same form."""

    use_sort: Union[bool, str] = True
    verbose: bool = True
    n_clusters: int = 16384  # of the shN codebook (png_compression.py:132)
    opacity_threshold: float = 0.005  # outlier filter: sigmoid(opacity) below it is dropped (outlier_filter.py:8-9, 32-37)
    kmeans_method: str = "torch"

    @torch.no_grad()
    def compress(self, compress_dir: str, splats: Dict[str, Tensor], entropy_models=None) -> None:
        if entropy_models is not None:
            raise ValueError("PngCompression should not require entropy_models")
        splats, side = prepare_splats(splats, self.opacity_threshold, self.use_sort, self.verbose)

        def encode(name, value, _):
            if name in ATTRIBUTE_CODECS:
                bits, kind = ATTRIBUTE_CODECS[name]
                planes, m = quantize_grid(value, side, bits=bits, kbit=(kind == "kbit"))
                write_planes(compress_dir, name, kind, planes)
                return m
            if name == "shN":
                return compress_masked_kmeans(compress_dir, name, value, self.n_clusters, self.kmeans_method)
            return None

        write_directory(compress_dir, splats, encode)

    @torch.no_grad()
    def decompress(self, compress_dir: str, device="cuda") -> Dict[str, Tensor]:
        def decode(name, m, _):
            if name in ATTRIBUTE_CODECS:
                return dequantize_grid(read_planes(compress_dir, name, ATTRIBUTE_CODECS[name][1]), m, device=device)
            if name == "shN":
                return decompress_masked_kmeans(compress_dir, name, m, device)
            return None

        splats = read_directory(compress_dir, decode, device)
        splats["means"] = inverse_log_transform(splats["means"])
        return splats
