"""File level of the reference's ``EntropyCodingCompression`` (gsplat/compression/entropy_coding_compression.py:20-201): the
``--compression entropy_coding`` choice of the trainer, with the reference's directory layout --

    meta.json                      one entry per attribute: shape, dtype, mins, maxs (plus what K-means adds)
    means_l.png, means_u.png       low / high byte of the 16-bit grid of the log-transformed means
    opacities.png, sh0.png         plain 8-bit grids
    scales.bin, quats.bin          the rANS-coded 8-bit symbols, one categorical model per channel
    scales_prob.npy, quats_prob.npy   the float32 [C, 256] symbol probabilities the coder's tables are derived from
    shN.npz, mask.bin              masked K-means codebook, as PngCompression writes it
    <other>.npz                    anything else, under the key "arr"

Every file but the two ``.bin`` is what the reference writes and is read by either implementation.  The ``.bin`` payload is
this project's own bitstream (``ans_reference`` defines it, csrc/ans.hip codes it on the GPU): the reference takes its coder
from the ``constriction`` package, whose stream cannot be reproduced without it.  ``decompress`` says so when it meets one.

Like the reference's ``_compress_factorized_ans`` (328-395) the factorized coder does not read the entropy model it is handed: it
codes against the empirical histogram of the symbols.  The hash-grid Gaussian codec (``_compress_gaussian_ans``) is not built.

Constant channels: where ``maxs == mins`` the reference divides 0 by 0; here such a channel gets symbol 0 everywhere and decodes
to ``mins``.
"""
from __future__ import annotations

import json
import os
from dataclasses import InitVar, dataclass, field
from typing import Any, Dict, Optional, Union

import numpy as np
import torch
from torch import Tensor

from .ans import ans_decode, ans_encode, probabilities, symbol_histogram
from .grid_codec import dequantize_grid, inverse_log_transform, quantize_grid
from .png_compression import (_meta_of, compress_masked_kmeans, decompress_masked_kmeans, png_read, png_write,
                              prepare_splats)

_GAUSSIAN = ("the hash-grid Gaussian codec is not built: only the factorized prior is (the hash-grid Gaussian "
             "model depends on the reference's CUDA-only _gridencoder extension)")


def _compress_png_16bit(compress_dir: str, param_name: str, params: Tensor, n_sidelen: int, **kwargs) -> Dict[str, Any]:
    (lo, hi), meta = quantize_grid(params, n_sidelen, bits=16)
    png_write(os.path.join(compress_dir, f"{param_name}_l.png"), lo.cpu().numpy())
    png_write(os.path.join(compress_dir, f"{param_name}_u.png"), hi.cpu().numpy())
    return meta


def _decompress_png_16bit(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    planes = [torch.from_numpy(png_read(os.path.join(compress_dir, f"{param_name}_{h}.png"))) for h in "lu"]
    return dequantize_grid(planes, meta, device=device)


def _compress_png(compress_dir: str, param_name: str, params: Tensor, n_sidelen: int, **kwargs) -> Dict[str, Any]:
    """The plain 8-bit form (211-250), not the k-bit one: no "quantization" entry in the meta."""
    (plane,), meta = quantize_grid(params, n_sidelen, bits=8)
    png_write(os.path.join(compress_dir, f"{param_name}.png"), plane.cpu().numpy())
    return meta


def _decompress_png(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    return dequantize_grid([torch.from_numpy(png_read(os.path.join(compress_dir, f"{param_name}.png")))], meta, device=device)


def _compress_factorized_ans(compress_dir: str, param_name: str, params: Tensor, n_sidelen: int, stream_len: int = 1024,
                             **kwargs) -> Dict[str, Any]:
    """328-395: per-channel min-max symbols at 8 bits (``gs_grid_quantize``: the same float32 statements, half-to-even), their
    empirical probabilities as ``<name>_prob.npy`` and the rANS stream ``<name>.bin``."""
    (plane,), meta = quantize_grid(params, n_sidelen, bits=8)
    symbols = plane.reshape(params.shape[0], -1)
    prob = probabilities(symbol_histogram(symbols))
    np.save(os.path.join(compress_dir, f"{param_name}_prob.npy"), prob)
    ans_encode(symbols, prob, stream_len=stream_len).tofile(os.path.join(compress_dir, f"{param_name}.bin"))
    return meta


def _decompress_factorized_ans(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    """398-446: symbols / 255 in float64, times the float32 ``maxs - mins``, plus ``mins``, cast: ``gs_grid_dequantize``."""
    path = os.path.join(compress_dir, f"{param_name}.bin")
    prob = np.load(os.path.join(compress_dir, f"{param_name}_prob.npy")).astype(np.float32)
    symbols = ans_decode(np.fromfile(path, dtype=np.uint8), prob, device=device, what=path)
    if symbols.shape[0] != meta["shape"][0] or symbols.shape[1] != len(meta["mins"]):
        raise ValueError(f"{path}: {tuple(symbols.shape)} symbols, meta.json describes {meta['shape']}")
    return dequantize_grid([symbols], meta, device=device)


def _compress_gaussian_ans(*args, **kwargs):
    raise NotImplementedError(f"_compress_gaussian_ans: {_GAUSSIAN}")


def _decompress_gaussian_ans(*args, **kwargs):
    raise NotImplementedError(f"_decompress_gaussian_ans: {_GAUSSIAN}")


def _compress_masked_kmeans(compress_dir: str, param_name: str, params: Tensor, n_sidelen: int, n_clusters: int = 32768,
                            kmeans_method: str = "torch", **kwargs) -> Dict[str, Any]:
    return compress_masked_kmeans(compress_dir, param_name, params, n_clusters, kmeans_method)


def _decompress_masked_kmeans(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    return decompress_masked_kmeans(compress_dir, param_name, meta, device)


def _compress_npz(compress_dir: str, param_name: str, params: Tensor, **kwargs) -> Dict[str, Any]:
    np.savez_compressed(os.path.join(compress_dir, f"{param_name}.npz"), arr=params.cpu().numpy())
    return _meta_of(params)


def _decompress_npz(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    arr = np.load(os.path.join(compress_dir, f"{param_name}.npz"))["arr"]
    return torch.tensor(arr).reshape(meta["shape"]).to(dtype=getattr(torch, meta["dtype"]), device=device)


# the names attribute_codec_registry may use (entropy_coding_compression.py:74-86)
_AVAILABLE = {fn.__name__: fn for fn in (
    _compress_png_16bit, _compress_png, _compress_factorized_ans, _compress_gaussian_ans, _compress_masked_kmeans,
    _decompress_png_16bit, _decompress_png, _decompress_factorized_ans, _decompress_gaussian_ans, _decompress_masked_kmeans)}


@dataclass
class EntropyCodingCompression:
    """The reference's ``EntropyCodingCompression``: same fields, same files (see the module docstring for the one difference,
    the payload of the ``.bin`` files).  ``use_sort`` as in ``PngCompression`` here: True = PLAS (external package, ImportError
    without it), "morton" = the deterministic Morton order, "grid" = the library's grid sort, False = keep the order.
    ``attribute_codec_registry`` maps an
    attribute to ``{"encode": <name>, "decode": <name>}`` with the reference's function names as strings, e.g.
    ``{"scales": {"encode": "_compress_png", "decode": "_decompress_png"}}``.  Works on detached copies; the caller's dictionary
    is not written to.  A channel with ``maxs == mins`` is coded as symbol 0 and decodes to ``mins``.  ``kmeans_method`` as in
    ``PngCompression``: "torch" or "fixed" clustering of the shN codebook; it reaches every compress function as the keyword
    ``kmeans_method``, next to ``n_sidelen``, ``n_clusters`` and ``verbose`` (they all take ``**kwargs``)."""

    use_sort: Union[bool, str] = True
    verbose: bool = True
    n_clusters: int = 32768
    attribute_codec_registry: InitVar[Optional[Dict[str, Dict[str, str]]]] = None
    opacity_threshold: float = 0.005  # outlier filter (outlier_filter.py:8-9, 32-37)

    compress_fn_map: Dict[str, str] = field(default_factory=lambda: {
        "means": "_compress_png_16bit", "scales": "_compress_factorized_ans", "quats": "_compress_factorized_ans",
        "opacities": "_compress_png", "sh0": "_compress_png", "shN": "_compress_masked_kmeans"})
    decompress_fn_map: Dict[str, str] = field(default_factory=lambda: {
        "means": "_decompress_png_16bit", "scales": "_decompress_factorized_ans", "quats": "_decompress_factorized_ans",
        "opacities": "_decompress_png", "sh0": "_decompress_png", "shN": "_decompress_masked_kmeans"})
    kmeans_method: str = "torch"

    def __post_init__(self, attribute_codec_registry):
        for attr_name, attr_codec in (attribute_codec_registry or {}).items():
            for key, fn_map in (("encode", self.compress_fn_map), ("decode", self.decompress_fn_map)):
                if attr_name in fn_map and key in attr_codec:
                    if attr_codec[key] in _AVAILABLE:
                        fn_map[attr_name] = attr_codec[key]
                    else:
                        print(f"Warning: Unknown func: {attr_codec[key]}")

    def _get_compress_fn(self, param_name: str):
        return _AVAILABLE[self.compress_fn_map[param_name]] if param_name in self.compress_fn_map else _compress_npz

    def _get_decompress_fn(self, param_name: str):
        return _AVAILABLE[self.decompress_fn_map[param_name]] if param_name in self.decompress_fn_map else _decompress_npz

    @torch.no_grad()
    def compress(self, compress_dir: str, splats: Dict[str, Tensor], entropy_models=None) -> None:
        """``entropy_models`` must be given, as in the reference (121-122); the factorized codec does not read them.  The
        reference's decode-the-means-again step (157-159) feeds only the Gaussian codec and is left out."""
        if entropy_models is None:
            raise ValueError("EntropyCodingCompression should require entropy_models")
        os.makedirs(compress_dir, exist_ok=True)
        splats, side = prepare_splats(splats, self.opacity_threshold, self.use_sort, self.verbose)
        meta: Dict[str, Any] = {}
        for name, value in splats.items():
            if value.numel() == 0:
                meta[name] = _meta_of(value)
            else:
                meta[name] = self._get_compress_fn(name)(compress_dir, name, value, n_sidelen=side, n_clusters=self.n_clusters,
                                                         verbose=self.verbose, kmeans_method=self.kmeans_method)
        with open(os.path.join(compress_dir, "meta.json"), "w") as f:
            json.dump(meta, f)

    @torch.no_grad()
    def decompress(self, compress_dir: str, device="cuda") -> Dict[str, Tensor]:
        with open(os.path.join(compress_dir, "meta.json"), "r") as f:
            meta = json.load(f)
        splats: Dict[str, Tensor] = {}
        for name, m in meta.items():
            if not np.all(m["shape"]):
                splats[name] = torch.zeros(m["shape"], dtype=getattr(torch, m["dtype"]), device=device)
            else:
                splats[name] = self._get_decompress_fn(name)(compress_dir, name, m, device=device)
        splats["means"] = inverse_log_transform(splats["means"])
        return splats
