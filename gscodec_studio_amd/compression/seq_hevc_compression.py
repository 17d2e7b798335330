"""File level of the reference's ``SeqHevcCompression`` (gsplat/compression/seq_hevc_compression.py): a SEQUENCE of splat
dictionaries -- a dynamic scene exported as one ``.ply`` per frame -- compressed with temporal prediction, the codec behind the
reference's ``examples/compress_ply_sequence.py``.  Fields, call sequence and directory are the reference's --

    codec.reorganize(splats_list)      the frames stacked per attribute, padded to a square count, ordered, as [T, side, side, ...]
    codec.compress(dir)                writes the directory
    videos = codec.decompress(dir)     {name: [T, side, side, ...]}
    codec.deorganize(videos)           back to a list of T dictionaries of the padded count

    meta.json                          per attribute: shape, dtype, mins, maxs, file_extension (".bin")
    means.bin                          the 16-bit grids, lossless: differences to the frame before inside a GOP
    scales.bin quats.bin opacities.bin sh0.bin
                                       the 8-bit grids as a plane sequence at the attribute's qp
    shN_sh{d}_{m}.bin                  one three-channel plane sequence per higher SH coefficient the input has (0, 3, 8 or 15)
    <other>.npz                        anything else, under the key "arr"

The reference stacks every attribute into a video and shells out to ``ffmpeg -c:v libx265``; frame t is predicted from the decoded
frame t - 1, or every frame is coded alone with ``use_all_intra``.  Here the payload is this project's own bitstream
(``plane_seq_codec_reference`` defines it, the sequence kernels of csrc/plane_codec.hip run its closed loop in one launch): HEVC's
8 x 8 transform and quantiser, so ``qp`` keeps its meaning, with the co-located block of the previous reconstruction as the only
prediction -- no motion search, no intra prediction, no rate-distortion optimisation, not an x265 stream.  ``decompress`` says so
when it meets an ``.mp4``.  ``gop`` is an added field: 250, x265's default keyint, the value the reference runs under;
``use_all_intra`` means gop 1.  Further differences: the quats are ONE four-channel file, the means are lossless through the rANS
coder (the reference's ``lossless=1``) and no ``.npy`` debug copy or PNG intermediate is written."""
from __future__ import annotations

import json
import os
from dataclasses import InitVar, dataclass, field
from typing import Any, Dict, List, Optional, Union

import numpy as np
import torch
from torch import Tensor

from . import plane_seq_codec_reference as R
from ._container import compress_npz, decompress_npz, meta_of
from .ans import ans_decode, ans_encode, symbol_histogram
from .decode import morton_order, sort_splats
from .grid_codec import dequantize_grid, quantize_grid_sequence
from .grid_sort import sort_splats_grid
from .plane_codec import _check_qp
from .plane_seq_codec import plane_seq_decode, plane_seq_encode

FILE_EXTENSION = ".bin"
PAD_VALUES = {"opacities": -5.0, "scales": -10.0}  # seq_hevc_compression.py:225-230; 0 elsewhere
SHN_NAMES = tuple(f"sh{d}_{m}" for d in range(1, 4) for m in range(-d, d + 1))
SHN_COUNTS = (0, 3, 8, 15)
NO_X265 = ("{path}: this directory holds the reference's x265 video payload ({mp4}) and no {name}.bin.  x265 payloads are not read "
           "here: SeqHevcCompression of this implementation writes its own transform-coded plane sequences (<name>.bin).  The "
           "<other>.npz files and meta.json are interchangeable.")


def _psnr(a: Tensor, b: Tensor, peak: float = 255.0) -> float:
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else float(20 * np.log10(peak) - 10 * np.log10(mse))


def _open_payload(compress_dir: str, name: str, stems=None) -> str:
    """-> the path of ``<name>.bin``; a directory of the reference's is refused by the name of its video file."""
    path = os.path.join(compress_dir, f"{name}{FILE_EXTENSION}")
    if not os.path.exists(path):
        for stem in stems or (name,):
            for ext in (".mp4", ".265"):
                if os.path.exists(os.path.join(compress_dir, stem + ext)):
                    raise ValueError(NO_X265.format(path=compress_dir, mp4=stem + ext, name=name))
    return path


def _decode_planes(compress_dir: str, name: str, meta: Dict[str, Any], channels: int, device, stems=None) -> Tensor:
    path = _open_payload(compress_dir, name, stems)
    planes = plane_seq_decode(np.fromfile(path, dtype=np.uint8), device=device, what=path)
    if list(planes.shape[:3]) != list(meta["shape"][:3]) or planes.shape[3] != channels:
        raise ValueError(f"{path}: a sequence of {tuple(planes.shape)}, meta.json describes {meta['shape']}")
    return planes


def _encode_planes(planes: Tensor, qp: int, gop: int, want_recon: bool):
    """-> (file bytes, the decoder's frames or None): the reconstruction is stored only for the PSNR report of ``verbose``."""
    return plane_seq_encode(planes, qp, gop, return_recon=True) if want_recon else (plane_seq_encode(planes, qp, gop), None)


def _compress_video_hevc(compress_dir: str, param_name: str, params: Tensor, qp: int = 10, gop: int = 250, verbose: bool = False,
                         **kwargs) -> Dict[str, Any]:
    """306-359: the 8-bit min-max grids of the attribute, one range over frames and pixels, as a plane sequence at ``qp``."""
    (planes,), meta = quantize_grid_sequence(params, bits=8)
    blob, recon = _encode_planes(planes, qp, gop, verbose)
    blob.tofile(os.path.join(compress_dir, f"{param_name}{FILE_EXTENSION}"))
    if verbose:
        print(f"QP value of {param_name} is: {qp}; PSNR of \"{param_name}\" map after coding: {_psnr(planes, recon):.2f} dB, {blob.size} bytes")
    return {**meta, "file_extension": FILE_EXTENSION}


def _decompress_video_hevc(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    """361-390."""
    channels = len(np.atleast_1d(meta["mins"]))
    stems = (param_name, f"{param_name}_w", f"{param_name}_xyz")
    return dequantize_grid([_decode_planes(compress_dir, param_name, meta, channels, device, stems)], meta, device=device)


# the reference keeps two functions because it splits the quats into a 1-channel and a 3-channel video; here they are one file
def _compress_quats_video_hevc(compress_dir: str, param_name: str, params: Tensor, **kwargs) -> Dict[str, Any]:
    return _compress_video_hevc(compress_dir, param_name, params, **kwargs)


def _decompress_quats_video_hevc(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    return _decompress_video_hevc(compress_dir, param_name, meta, device=device)


def _means_symbols(grid: Tensor, gop: int):
    """``plane_seq_codec_reference.means_symbols`` on the device: int32 values of a 16-bit grid [T, H, W, C] -> the byte columns
    of the I frames and of the P frames (None without one), uint8 [n H W, 2 C]."""
    intra = R.is_intra(grid.shape[0], gop)
    d = grid.clone()
    d[1:] -= grid[:-1]
    d = torch.remainder(d + 32768, 65536) - 32768
    mask = torch.from_numpy(intra).to(grid.device)[:, None, None, None]
    u = torch.where(mask, grid, ((d << 1) ^ (d >> 15)) & 0xFFFF)
    both = torch.cat([u & 0xFF, u >> 8], dim=3).to(torch.uint8)
    rows = lambda keep: both[torch.from_numpy(np.flatnonzero(keep)).to(grid.device)].reshape(-1, both.shape[3]).contiguous()
    return rows(intra), (None if intra.all() else rows(~intra))


def _means_from_symbols(sym_i: Tensor, sym_p: Optional[Tensor], head: R.MeansHeader) -> Tensor:
    """``plane_seq_codec_reference.means_from_symbols`` on the device -> int32 [T, H, W, C]."""
    intra = R.is_intra(head.frames, head.gop)
    c, dev = head.channels, sym_i.device

    def join(sym):
        s = sym.to(torch.int32).reshape(-1, head.height, head.width, 2 * c)
        return s[..., :c] | (s[..., c:] << 8)

    u = torch.empty((head.frames, head.height, head.width, c), dtype=torch.int32, device=dev)
    u[torch.from_numpy(np.flatnonzero(intra)).to(dev)] = join(sym_i)
    if sym_p is not None:
        u[torch.from_numpy(np.flatnonzero(~intra)).to(dev)] = join(sym_p)
    out = torch.empty_like(u)
    for t in range(head.frames):
        out[t] = u[t] if intra[t] else torch.remainder(out[t - 1] + ((u[t] >> 1) ^ -(u[t] & 1)), 65536)
    return out


def _compress_video_hevc_16bit(compress_dir: str, param_name: str, params: Tensor, gop: int = 250, verbose: bool = False,
                               **kwargs) -> Dict[str, Any]:
    """392-452 (``lossless=1``): the 16-bit grids, no log transform, as temporal differences through the rANS coder."""
    (lo, hi), meta = quantize_grid_sequence(params, bits=16)
    grid = lo.to(torch.int32) | (hi.to(torch.int32) << 8)
    if grid.shape[3] > R.MEANS_MAX_CHANNELS:
        raise ValueError(f"{param_name}: {grid.shape[3]} channels, the lossless grid sequence takes up to {R.MEANS_MAX_CHANNELS}")
    parts = []
    for sym in _means_symbols(grid, gop):
        if sym is not None:
            freq = R.tables_from_counts(symbol_histogram(sym).cpu().numpy())
            parts += [freq, ans_encode(sym, R.table_probabilities(freq, R.A.DEFAULT_BITS))]
    head = R.MeansHeader(R.A.DEFAULT_BITS, *grid.shape, gop, 0, 0)
    blob = R.build_means_container(head, *parts)
    blob.tofile(os.path.join(compress_dir, f"{param_name}{FILE_EXTENSION}"))
    if verbose:
        print(f"\"{param_name}\" map coded without loss, {blob.size} bytes")
    return {**meta, "file_extension": FILE_EXTENSION}


def _decompress_video_hevc_16bit(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    """454-486."""
    path = _open_payload(compress_dir, param_name, (f"{param_name}_l", f"{param_name}_u"))
    head, freq_i, blob_i, freq_p, blob_p = R.parse_means_container(np.fromfile(path, dtype=np.uint8), path)
    if [head.frames, head.height, head.width] != list(meta["shape"][:3]) or head.channels != len(np.atleast_1d(meta["mins"])):
        raise ValueError(f"{path}: grids of {tuple(head[1:5])}, meta.json describes {meta['shape']}")
    sym_i = ans_decode(blob_i, R.table_probabilities(freq_i, head.bits), device=device, what=path)
    sym_p = None if blob_p is None else ans_decode(blob_p, R.table_probabilities(freq_p, head.bits), device=device, what=path)
    grid = _means_from_symbols(sym_i, sym_p, head)
    return dequantize_grid([(grid & 0xFF).to(torch.uint8), (grid >> 8).to(torch.uint8)], meta, device=device)


def _compress_shN_video_hevc(compress_dir: str, param_name: str, params: Tensor, qp: Dict[str, int] = None, gop: int = 250,
                             verbose: bool = False, **kwargs) -> Dict[str, Any]:
    """580-632: ``params`` [T, side, side, K, 3]; one three-channel plane sequence per coefficient, the qp by its degree; one
    min-max range per (coefficient, colour) over frames and pixels.  K = 0 leaves a meta entry alone."""
    if params.shape[3] == 0:
        return {**meta_of(params), "mins": [], "maxs": [], "file_extension": FILE_EXTENSION}
    (planes,), meta = quantize_grid_sequence(params, bits=8)  # [T, side, side, 3 K]
    k = params.shape[3]
    for i, sh_name in enumerate(SHN_NAMES[:k]):
        one = planes[..., 3 * i:3 * i + 3].contiguous()
        blob, recon = _encode_planes(one, qp[sh_name[:3]], gop, verbose)
        blob.tofile(os.path.join(compress_dir, f"{param_name}_{sh_name}{FILE_EXTENSION}"))
        if verbose:
            print(f"QP value of {sh_name} is: {qp[sh_name[:3]]}; PSNR after coding: {_psnr(one, recon):.2f} dB, {blob.size} bytes")
    meta["mins"] = torch.tensor(meta["mins"]).reshape(k, 3).tolist()
    meta["maxs"] = torch.tensor(meta["maxs"]).reshape(k, 3).tolist()
    return {**meta, "file_extension": FILE_EXTENSION}


def _decompress_shN_video_hevc(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    """634-668."""
    k = int(meta["shape"][3])
    if k == 0 or not np.all(meta["shape"]):
        return torch.zeros(meta["shape"], dtype=getattr(torch, meta["dtype"]), device=device)
    if k not in SHN_COUNTS:
        raise ValueError(f"{compress_dir}: {k} higher SH coefficients in meta.json, a whole degree has 3, 8 or 15")
    planes = torch.cat([_decode_planes(compress_dir, f"{param_name}_{sh_name}", meta, 3, device) for sh_name in SHN_NAMES[:k]], dim=3)
    flat = {**meta, "mins": np.asarray(meta["mins"], np.float64).reshape(-1).tolist(), "maxs": np.asarray(meta["maxs"], np.float64).reshape(-1).tolist()}
    return dequantize_grid([planes], flat, device=device)


# the names attribute_codec_registry may use
_AVAILABLE = {fn.__name__: fn for fn in (
    _compress_video_hevc_16bit, _compress_video_hevc, _compress_quats_video_hevc, _compress_shN_video_hevc,
    _decompress_video_hevc_16bit, _decompress_video_hevc, _decompress_quats_video_hevc, _decompress_shN_video_hevc)}


@dataclass
class SeqHevcCompression:
    """The reference's ``SeqHevcCompression``: same fields and call sequence (see the module docstring for the payload).  ``qp`` maps
    an attribute to its quantisation parameter (0..51), ``shN`` to a dictionary by degree; the entry of the means is not used (they
    are lossless).  ``use_sort``: True = PLAS (ImportError without the package), "grid", "morton" or False; the order is frame 0's,
    without shN, or every frame's own with ``use_all_intra``.  ``gop``: an I frame every ``gop`` frames (``use_all_intra``: 1).
    ``attribute_codec_registry`` maps an attribute to ``{"encode": <name>, "decode": <name>}`` with the reference's function names
    as strings.  Works on detached copies; the caller's dictionaries are not written to."""

    use_sort: Union[bool, str] = True
    verbose: bool = True
    qp: Dict[str, Union[int, Dict[str, Any]]] = field(default_factory=lambda: {
        "means": -1, "opacities": 4, "quats": 4, "scales": 4, "sh0": 16, "shN": {"sh1": 20, "sh2": 24, "sh3": 28}})
    n_clusters: int = 32768
    debug: bool = False
    use_all_intra: bool = False
    attribute_codec_registry: InitVar[Optional[Dict[str, Dict[str, str]]]] = None
    gop: int = 250  # x265's default keyint

    compress_fn_map: Dict[str, str] = field(default_factory=lambda: {
        "means": "_compress_video_hevc_16bit", "scales": "_compress_video_hevc", "quats": "_compress_quats_video_hevc",
        "opacities": "_compress_video_hevc", "sh0": "_compress_video_hevc", "shN": "_compress_shN_video_hevc"})
    decompress_fn_map: Dict[str, str] = field(default_factory=lambda: {
        "means": "_decompress_video_hevc_16bit", "scales": "_decompress_video_hevc", "quats": "_decompress_quats_video_hevc",
        "opacities": "_decompress_video_hevc", "sh0": "_decompress_video_hevc", "shN": "_decompress_shN_video_hevc"})

    def __post_init__(self, attribute_codec_registry):
        self.splats_videos: Optional[Dict[str, Tensor]] = None
        for attr_name, attr_codec in (attribute_codec_registry or {}).items():
            for key, fn_map in (("encode", self.compress_fn_map), ("decode", self.decompress_fn_map)):
                if attr_name in fn_map and key in attr_codec:
                    if attr_codec[key] in _AVAILABLE:
                        fn_map[attr_name] = attr_codec[key]
                    else:
                        print(f"Warning: Unknown func: {attr_codec[key]}")

    @property
    def effective_gop(self) -> int:
        return 1 if self.use_all_intra else self.gop

    def _check_settings(self, names) -> None:
        """ValueError for a gop below 1 and for a ``qp`` that does not give every lossy attribute in ``names`` a value in 0..51."""
        R.check_gop(self.gop)
        if not isinstance(self.qp, dict):
            raise ValueError(f"qp must map attribute names to quantisation parameters, got {self.qp!r}")
        for name in names:
            fn = self.compress_fn_map.get(name)
            if fn in ("_compress_video_hevc", "_compress_quats_video_hevc"):
                if name not in self.qp:
                    raise ValueError(f"qp has no entry for {name!r}")
                _check_qp(self.qp[name])
            elif fn == "_compress_shN_video_hevc":
                by_degree = self.qp.get(name)
                if not isinstance(by_degree, dict) or any(d not in by_degree for d in ("sh1", "sh2", "sh3")):
                    raise ValueError(f"qp[{name!r}] must map 'sh1', 'sh2' and 'sh3' to quantisation parameters, got {by_degree!r}")
                for d in ("sh1", "sh2", "sh3"):
                    _check_qp(by_degree[d])

    def _order(self, frame: Dict[str, Tensor]) -> Optional[Tensor]:
        """The permutation ``use_sort`` gives one padded frame (sort_with_frame_index, 178-199), None for no sorting."""
        if self.use_sort == "morton":
            return morton_order(frame["means"])
        if self.use_sort == "grid":
            return sort_splats_grid(frame, verbose=self.verbose, return_indices=True, sort_with_shN=False)[1]
        if self.use_sort:
            return sort_splats(frame, verbose=self.verbose, return_indices=True, sort_with_shN=False)[1]
        return None

    @torch.no_grad()
    def reorganize(self, splats_list: List[Dict[str, Tensor]]) -> Dict[str, Tensor]:
        """236-274: list of T dictionaries -> {name: [T, side, side, ...]}, kept for ``compress``."""
        if not isinstance(splats_list, (list, tuple)) or len(splats_list) == 0:
            raise ValueError("reorganize takes a non-empty list of splat dictionaries, one per frame")
        names = list(splats_list[0].keys())
        for t, frame in enumerate(splats_list):
            if list(frame.keys()) != names:
                raise ValueError(f"frame {t} has the attributes {list(frame.keys())}, frame 0 has {names}")
            for k in names:
                if tuple(frame[k].shape) != tuple(splats_list[0][k].shape):
                    raise ValueError(f"frame {t}: {k} has the shape {tuple(frame[k].shape)}, frame 0 has {tuple(splats_list[0][k].shape)}")
        for k in ("means", "quats"):
            if k not in names:
                raise ValueError(f"the splat dictionaries need {k!r}")
        if "shN" in names and (splats_list[0]["shN"].dim() != 3 or splats_list[0]["shN"].shape[1] not in SHN_COUNTS):
            raise ValueError(f"shN must be [N, K, 3] with K in {SHN_COUNTS}, got {tuple(splats_list[0]['shN'].shape)}")
        self._check_settings(names)
        if any(not frame[k].is_cuda for frame in splats_list for k in names):
            raise RuntimeError("SeqHevcCompression runs on the GPU: the splats must be device tensors (no CPU fallback)")
        videos = {k: torch.stack([frame[k].detach() for frame in splats_list], dim=0) for k in names}  # stack copies
        n = videos["means"].shape[1]
        side = int(np.ceil(n ** 0.5))
        n_pad = side * side - n
        if n_pad:
            if self.verbose:
                print(f"Warning: Number of Gaussians was not square. Padded {n_pad} Gaussians.")
            for k, v in videos.items():
                pad = torch.full((v.shape[0], n_pad) + tuple(v.shape[2:]), PAD_VALUES.get(k, 0.0), dtype=v.dtype, device=v.device)
                videos[k] = torch.cat([v, pad], dim=1)
        sort_names = [k for k in names if k != "shN"]
        if self.use_sort:
            if not self.use_all_intra:
                order = self._order({k: videos[k][0] for k in sort_names})
                videos = {k: v[:, order] for k, v in videos.items()}
            else:
                for t in range(len(splats_list)):
                    order = self._order({k: videos[k][t] for k in sort_names})
                    for k in names:
                        videos[k][t] = videos[k][t][order]
        videos = {k: v.reshape((v.shape[0], side, side) + tuple(v.shape[2:])) for k, v in videos.items()}
        videos["quats"] = torch.nn.functional.normalize(videos["quats"], dim=-1)
        self.splats_videos = videos
        return videos

    @torch.no_grad()
    def compress(self, compress_dir: str) -> None:
        """130-155: writes the directory from what ``reorganize`` kept."""
        if self.splats_videos is None:
            raise ValueError("compress: call reorganize(splats_list) first")
        self._check_settings(self.splats_videos)  # before the directory is touched
        os.makedirs(compress_dir, exist_ok=True)
        meta: Dict[str, Any] = {}
        for name, video in self.splats_videos.items():
            if name in self.compress_fn_map:
                meta[name] = _AVAILABLE[self.compress_fn_map[name]](compress_dir, name, video, qp=self.qp.get(name), gop=self.effective_gop,
                                                                    verbose=self.verbose)
            else:
                meta[name] = compress_npz(compress_dir, name, video)
        with open(os.path.join(compress_dir, "meta.json"), "w") as f:
            json.dump(meta, f)

    @torch.no_grad()
    def decompress(self, compress_dir: str, device="cuda") -> Dict[str, Tensor]:
        """157-176: -> {name: [T, side, side, ...]} on ``device``; needs none of the encoder's settings."""
        with open(os.path.join(compress_dir, "meta.json"), "r") as f:
            meta = json.load(f)
        videos = {}
        for name, m in meta.items():
            if name in self.decompress_fn_map and "file_extension" in m:
                videos[name] = _AVAILABLE[self.decompress_fn_map[name]](compress_dir, name, m, device=device)
            else:
                videos[name] = decompress_npz(compress_dir, name, m, device)
        return videos

    def deorganize(self, splats_videos_c: Dict[str, Tensor]) -> List[Dict[str, Tensor]]:
        """276-294: {name: [T, side, side, ...]} -> T dictionaries of [side^2, ...]."""
        flat = {k: v.reshape((v.shape[0], v.shape[1] * v.shape[2]) + tuple(v.shape[3:])) for k, v in splats_videos_c.items()}
        return [{k: v[t] for k, v in flat.items()} for t in range(flat["means"].shape[0])]
