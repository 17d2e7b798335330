"""File level of the reference's ``EntropyCodingCompression`` (gsplat/compression/entropy_coding_compression.py:20-201): the
``--compression entropy_coding`` choice of the trainer, with the reference's directory layout --

    meta.json                      one entry per attribute: shape, dtype, mins, maxs (plus what K-means adds)
    means_l.png, means_u.png       low / high byte of the 16-bit grid of the log-transformed means
    opacities.png, sh0.png         plain 8-bit grids
    scales.bin, quats.bin          the rANS-coded 8-bit symbols
    scales_prob.npy, quats_prob.npy   factorized route: the float32 [C, 256] symbol probabilities the coder's tables are derived from
    <name>_entropy_model_encoding_{xyz,xy,xz,yz}.bin, <name>_entropy_model_mlp.ckpt
                                   hash-grid Gaussian route: the model that predicts a Gaussian per splat and channel from the
                                   splat's position -- the signs of the four hash tables, one bit each, and the regressor's MLP
    shN.npz, mask.bin              masked K-means codebook, as PngCompression writes it
    <other>.npz                    anything else, under the key "arr"

Every file but ``<name>.bin`` is what the reference writes and is read by either implementation.  The ``.bin`` payload of BOTH
routes is this project's own bitstream (``ans_reference`` / ``gauss_ans_reference`` define them, csrc/ans.hip and
csrc/gauss_ans.hip code them on the GPU): the reference takes its coder from the ``constriction`` package, whose stream cannot be
reproduced without it.  ``decompress`` says so when it meets one.

Like the reference's ``_compress_factorized_ans`` (328-395) the factorized coder does not read the entropy model it is handed: it
codes against the empirical histogram of the symbols.  The hash-grid Gaussian route (``_compress_gaussian_ans``, 448-654; chosen
through ``attribute_codec_registry``) spends the trained ``Entropy_gaussian``: every symbol is coded against the Gaussian the model
predicts at the splat's DECODED position -- ``compress`` reads the means back from the PNG files it has just written, so that both
sides hand the model the same float32 positions bit for bit -- and the model itself is evaluated by ``gs_gauss_ans_params`` in one
stated float32 order, so that both sides also get the same integers out of it.

Constant channels: where ``maxs == mins`` the reference divides 0 by 0; here such a channel gets symbol 0 everywhere and decodes
to ``mins``.
"""
from __future__ import annotations

import os
from dataclasses import InitVar, dataclass, field
from typing import Any, Dict, Optional, Union

import numpy as np
import torch
from torch import Tensor

from . import gauss_ans_reference as GR
from .ans import ans_decode, ans_encode, probabilities, symbol_histogram
from .gauss_ans import check_entropy_model, gauss_ans_decode, gauss_ans_encode, gaussian_params
from .grid_codec import dequantize_grid, inverse_log_transform, quantize_grid
from ._container import (compress_masked_kmeans, decompress_masked_kmeans, prepare_splats, read_directory, read_planes,
                         write_directory, write_planes)

_ENCODINGS = ("encoding_xyz", "encoding_xy", "encoding_xz", "encoding_yz")


def _compress_png_16bit(compress_dir: str, param_name: str, params: Tensor, n_sidelen: int, **kwargs) -> Dict[str, Any]:
    planes, meta = quantize_grid(params, n_sidelen, bits=16)
    write_planes(compress_dir, param_name, "16", planes)
    return meta


def _decompress_png_16bit(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    return dequantize_grid(read_planes(compress_dir, param_name, "16"), meta, device=device)


def _compress_png(compress_dir: str, param_name: str, params: Tensor, n_sidelen: int, **kwargs) -> Dict[str, Any]:
    """The plain 8-bit form (211-250), not the k-bit one: no "quantization" entry in the meta."""
    planes, meta = quantize_grid(params, n_sidelen, bits=8)
    write_planes(compress_dir, param_name, "plain", planes)
    return meta


def _decompress_png(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    return dequantize_grid(read_planes(compress_dir, param_name), meta, device=device)


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


def _dequantize_symbols(path: str, symbols: Tensor, meta: Dict[str, Any], device) -> Tensor:
    """What either ANS route does with its decoded symbols: they must be what the meta describes."""
    if symbols.shape[0] != meta["shape"][0] or symbols.shape[1] != len(meta["mins"]):
        raise ValueError(f"{path}: {tuple(symbols.shape)} symbols, meta.json describes {meta['shape']}")
    return dequantize_grid([symbols], meta, device=device)


def _decompress_factorized_ans(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    """398-446: symbols / 255 in float64, times the float32 ``maxs - mins``, plus ``mins``, cast: ``gs_grid_dequantize``."""
    path = os.path.join(compress_dir, f"{param_name}.bin")
    prob = np.load(os.path.join(compress_dir, f"{param_name}_prob.npy")).astype(np.float32)
    return _dequantize_symbols(path, ans_decode(np.fromfile(path, dtype=np.uint8), prob, device=device, what=path), meta, device)


def save_gaussian_entropy_model(param_name: str, entropy_model: torch.nn.Module, compress_dir: str) -> Dict[str, Any]:
    """467-489: the hash tables as ``STE_binary`` leaves them, one bit per entry, LSB first (``to_bin_stream``'s bytes, without
    its Python loop), and ``mlp_regressor.state_dict()``; returns the ``encoding_*_shape`` entries of the meta."""
    check_entropy_model(entropy_model)
    pr = entropy_model.param_regressor
    meta: Dict[str, Any] = {}
    for enc_name in _ENCODINGS:
        params = getattr(pr.hash_grid, enc_name).params.detach()
        if bool(torch.isnan(params).any()):
            raise ValueError(f"{enc_name} of the entropy model of {param_name} holds a NaN: its sign is 0, which the one-bit file cannot hold")
        meta[f"{enc_name}_shape"] = list(params.shape)
        GR.pack_signs(np.where(params.cpu().numpy().reshape(-1) >= 0, 1, -1)).tofile(
            os.path.join(compress_dir, f"{param_name}_entropy_model_{enc_name}.bin"))
    torch.save({k: v.detach().cpu() for k, v in pr.mlp_regressor.state_dict().items()},
               os.path.join(compress_dir, f"{param_name}_entropy_model_mlp.ckpt"))
    return meta


def load_gaussian_entropy_model(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> torch.nn.Module:
    """602-620: a fresh ``Entropy_gaussian`` with the stored signs as its tables and the stored MLP (``strict=True``)."""
    from ..compression_simulation.entropy_model import Entropy_gaussian

    entropy_model = Entropy_gaussian(channel=meta["shape"][-1])
    pr = entropy_model.param_regressor
    state = torch.load(os.path.join(compress_dir, f"{param_name}_entropy_model_mlp.ckpt"), map_location="cpu", weights_only=True)
    pr.mlp_regressor.load_state_dict(state, strict=True)
    for enc_name in _ENCODINGS:
        shape = [int(v) for v in meta[f"{enc_name}_shape"]]
        enc = getattr(pr.hash_grid, enc_name)
        if shape != list(enc.params.shape):
            raise ValueError(f"{param_name}: {enc_name}_shape {shape} in meta.json, the model's table is {list(enc.params.shape)}")
        data = np.fromfile(os.path.join(compress_dir, f"{param_name}_entropy_model_{enc_name}.bin"), dtype=np.uint8)
        enc.params.data = torch.from_numpy(GR.unpack_signs(data, int(np.prod(shape))).reshape(shape))
    return entropy_model.to(device)


def _compress_gaussian_ans(compress_dir: str, param_name: str, params: Tensor, n_sidelen: int, entropy_model=None,
                           decoded_means: Optional[Tensor] = None, stream_len: int = 1024, **kwargs) -> Dict[str, Any]:
    """491-568: the model's files, then the same 8-bit min-max symbols as the factorized route, each coded against the Gaussian
    the model predicts at the splat's decoded position (``gauss_ans``).  Meta: ``encoding_*_shape``, shape, dtype, mins, maxs."""
    if entropy_model is None:
        raise NotImplementedError(
            f"_compress_gaussian_ans: the hash-grid Gaussian codec codes {param_name} against its trained Entropy_gaussian, and "
            f"entropy_models holds no model for {param_name}: pass the simulation's entropy_models, or keep the factorized route")
    if decoded_means is None:
        raise ValueError(f"_compress_gaussian_ans: {param_name} needs the decoded means (compress() hands them over)")
    meta = save_gaussian_entropy_model(param_name, entropy_model, compress_dir)
    (plane,), q_meta = quantize_grid(params, n_sidelen, bits=8)
    symbols = plane.reshape(params.shape[0], -1)
    mu_q, k = gaussian_params(entropy_model, decoded_means.to(symbols.device), q_meta["mins"], q_meta["maxs"])
    gauss_ans_encode(symbols, mu_q, k, stream_len=stream_len).tofile(os.path.join(compress_dir, f"{param_name}.bin"))
    meta.update(q_meta)
    return meta


def _decompress_gaussian_ans(compress_dir: str, param_name: str, meta: Dict[str, Any], decoded_means: Optional[Tensor] = None,
                             device="cuda") -> Tensor:
    """593-654: rebuild the model from its files, evaluate it at the decoded means, decode, dequantize."""
    if not all(f"{e}_shape" in meta for e in _ENCODINGS):
        raise NotImplementedError(
            f"_decompress_gaussian_ans: the meta of {param_name} has no encoding_*_shape keys: this directory was not written by the "
            f"hash-grid Gaussian codec (no entropy model files for {param_name}); decode it with the route that wrote it")
    if decoded_means is None:
        raise ValueError(f"_decompress_gaussian_ans: {param_name} needs the decoded means (decompress() hands them over)")
    path = os.path.join(compress_dir, f"{param_name}.bin")
    entropy_model = load_gaussian_entropy_model(compress_dir, param_name, meta, device)
    mu_q, k = gaussian_params(entropy_model, decoded_means.to(device), meta["mins"], meta["maxs"])
    return _dequantize_symbols(path, gauss_ans_decode(np.fromfile(path, dtype=np.uint8), mu_q, k, device=device, what=path), meta, device)


def _compress_masked_kmeans(compress_dir: str, param_name: str, params: Tensor, n_sidelen: int, n_clusters: int = 32768,
                            kmeans_method: str = "torch", **kwargs) -> Dict[str, Any]:
    return compress_masked_kmeans(compress_dir, param_name, params, n_clusters, kmeans_method)


def _decompress_masked_kmeans(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    return decompress_masked_kmeans(compress_dir, param_name, meta, device)


# the names attribute_codec_registry may use (entropy_coding_compression.py:74-86)
_AVAILABLE = {fn.__name__: fn for fn in (
    _compress_png_16bit, _compress_png, _compress_factorized_ans, _compress_gaussian_ans, _compress_masked_kmeans,
    _decompress_png_16bit, _decompress_png, _decompress_factorized_ans, _decompress_gaussian_ans, _decompress_masked_kmeans)}


@dataclass
class EntropyCodingCompression:
    """The reference's ``EntropyCodingCompression``: same fields, same files (see the module docstring for the one difference,
    the payload of the ``.bin`` files).  ``use_sort`` as in ``PngCompression`` here.  ``attribute_codec_registry`` maps an
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

    @torch.no_grad()
    def compress(self, compress_dir: str, splats: Dict[str, Tensor], entropy_models=None) -> None:
        """``entropy_models`` must be given, as in the reference (121-122); the factorized codec does not read them.  An
        attribute routed to ``_compress_gaussian_ans`` gets its model and the DECODED means (157-159: read back from the files
        just written), so ``means`` must precede it in ``splats``."""
        if entropy_models is None:
            raise ValueError("EntropyCodingCompression should require entropy_models")
        splats, side = prepare_splats(splats, self.opacity_threshold, self.use_sort, self.verbose)

        def encode(name, value, meta):
            if name not in self.compress_fn_map:
                return None
            fn, extra = _AVAILABLE[self.compress_fn_map[name]], {}
            if fn is _compress_gaussian_ans and name in entropy_models and entropy_models[name] is not None:
                if "means" not in meta:
                    raise ValueError(f"{name} is coded against the decoded means: 'means' must precede it in the splats")
                extra = {"entropy_model": entropy_models[name],
                         "decoded_means": self.get_decompressed_means(compress_dir, meta["means"], value.device)}
            return fn(compress_dir, name, value, n_sidelen=side, n_clusters=self.n_clusters, verbose=self.verbose,
                      kmeans_method=self.kmeans_method, **extra)

        write_directory(compress_dir, splats, encode)

    @torch.no_grad()
    def decompress(self, compress_dir: str, device="cuda") -> Dict[str, Tensor]:
        def decode(name, m, splats):
            if name not in self.decompress_fn_map:
                return None
            fn = _AVAILABLE[self.decompress_fn_map[name]]
            if fn is _decompress_gaussian_ans:
                if "means" not in splats:
                    raise ValueError(f"{name} is coded against the decoded means: 'means' must precede it in meta.json")
                return fn(compress_dir, name, m, inverse_log_transform(splats["means"]), device=device)
            return fn(compress_dir, name, m, device=device)

        splats = read_directory(compress_dir, decode, device)
        splats["means"] = inverse_log_transform(splats["means"])
        return splats

    def get_decompressed_means(self, compress_dir: str, meta_means: Dict[str, Any], device="cuda") -> Tensor:
        """193-201: the means as ``decompress`` will see them, from the files of ``compress_dir``."""
        fn = _AVAILABLE[self.decompress_fn_map["means"]]
        return inverse_log_transform(fn(compress_dir, "means", meta_means, device=device))
