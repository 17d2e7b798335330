"""The directory level under ``PngCompression``, ``STGPngCompression`` and ``EntropyCodingCompression``: what the three share once
their attribute codecs are taken out, and nothing that knows one of them.  From the top:

* ``prepare_splats`` / ``order_splats``: the filter, transform, crop and ordering in front of the attribute codecs, on detached
  copies.  Nothing has touched the directory when the ordering fails.
* ``write_directory`` / ``read_directory``: the loop over the attributes around a codec's callback, with the rules of the
  layout: the key order of ``meta.json``, the attribute without elements, the ``<name>.npz`` of an attribute no codec takes.
* ``write_planes`` / ``read_planes``: the image grids of an attribute as PNG files, named by ``plane_files``.
* ``png_write`` / ``png_read``: 8-bit grey / grey+alpha / RGB / RGBA, non-interlaced -- what ``imageio.imwrite`` produces for these
  arrays (the image has no imageio / Pillow; a PNG is a zlib stream of filtered scanlines, PNG specification sections 5, 9, 10).
  Reading undoes all five filter types (the sequential part is ``gs_png_unfilter`` of the library); writing picks None / Sub / Up
  per row by the usual minimum-sum-of-absolute-differences heuristic.
"""
from __future__ import annotations

import json
import os
import struct
import zlib
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import _backend as B
from .decode import kmeans_decode, kmeans_encode, morton_order, sort_splats
from .grid_codec import transform_and_crop
from .grid_sort import sort_splats_grid

_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"
_COLOR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}  # channels -> PNG colour type
_CHANNELS = {0: 1, 4: 2, 2: 3, 6: 4}

DEFERRED = object()  # what a ``read_directory`` callback returns for an attribute it decodes after the loop


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_write(path: str, img: np.ndarray, level: int = 6) -> None:
    """Write a uint8 image [H, W] or [H, W, C] (C = 1..4) as a PNG file."""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3), (img.dtype, img.shape)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, c = img.shape
    assert c in _COLOR_TYPE and h > 0 and w > 0, img.shape
    rows = img.reshape(h, w * c)
    # per-row filter choice among None (0), Sub (1), Up (2): smallest sum of |signed residual|
    sub = rows.copy()
    sub[:, c:] = rows[:, c:] - rows[:, :-c]
    up = rows.copy()
    up[1:] = rows[1:] - rows[:-1]
    cand = np.stack([rows, sub, up])  # [3, h, w*c]
    cost = np.abs(cand.view(np.int8).astype(np.int32)).sum(axis=2)  # [3, h]
    ft = cost.argmin(axis=0).astype(np.uint8)  # [h]
    body = np.empty((h, 1 + w * c), dtype=np.uint8)
    body[:, 0] = ft
    body[:, 1:] = cand[ft, np.arange(h)]
    ihdr = struct.pack(">IIBBBBB", w, h, 8, _COLOR_TYPE[c], 0, 0, 0)
    with open(path, "wb") as f:
        f.write(_PNG_MAGIC + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(body.tobytes(), level)) + _chunk(b"IEND", b""))


def png_read(path: str) -> np.ndarray:
    """Read an 8-bit non-interlaced grey / grey+alpha / RGB / RGBA PNG -> uint8 [H, W] or [H, W, C] (as imageio.imread)."""
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:8] != _PNG_MAGIC:
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos + 8 <= len(buf):
        (n,), tag = struct.unpack(">I", buf[pos:pos + 4]), buf[pos + 4:pos + 8]
        data = buf[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", buf[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(tag + data) & 0xFFFFFFFF != crc:
            raise ValueError(f"{path}: CRC mismatch in chunk {tag!r}")
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", data)
        elif tag == b"IDAT":
            idat.append(data)
        elif tag == b"IEND":
            break
        pos += 12 + n
    if hdr is None or not idat:
        raise ValueError(f"{path}: missing IHDR / IDAT")
    w, h, depth, ctype, comp, filt, interlace = hdr
    if depth != 8 or ctype not in _CHANNELS or comp != 0 or filt != 0 or interlace != 0:
        raise ValueError(f"{path}: only 8-bit non-interlaced grey / grey+alpha / RGB / RGBA images are supported "
                         f"(bit depth {depth}, colour type {ctype}, interlace {interlace})")
    c = _CHANNELS[ctype]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if raw.size != h * (1 + w * c):
        raise ValueError(f"{path}: {raw.size} bytes of image data, expected {h * (1 + w * c)}")
    raw = np.ascontiguousarray(raw)
    out = np.empty((h, w * c), dtype=np.uint8)
    B.call("gs_png_unfilter", raw.ctypes.data, h, w * c, c, out.ctypes.data)
    return out.reshape(h, w) if c == 1 else out.reshape(h, w, c)


def plane_files(name: str, kind: str = "plain", num_img: int = 0) -> Tuple[str, ...]:
    """The files of an attribute's image grid by the kind of its codec: "multi" = ``num_img`` images of three channels, "16" = the
    low and the high byte, "plain" / "kbit" = one image."""
    if kind == "multi":
        return tuple(f"{name}_{i}.png" for i in range(num_img))
    return (f"{name}_l.png", f"{name}_u.png") if kind == "16" else (f"{name}.png",)


def write_planes(compress_dir: str, name: str, kind: str, planes: Sequence[Tensor]) -> None:
    for fn, plane in zip(plane_files(name, kind, len(planes)), planes):
        png_write(os.path.join(compress_dir, fn), plane.cpu().numpy())


def read_planes(compress_dir: str, name: str, kind: str = "plain", num_img: int = 0) -> List[Tensor]:
    return [torch.from_numpy(png_read(os.path.join(compress_dir, fn))) for fn in plane_files(name, kind, num_img)]


def meta_of(params: Tensor) -> Dict[str, Any]:
    return {"shape": list(params.shape), "dtype": str(params.dtype).split(".")[1]}


def compress_npz(compress_dir: str, param_name: str, params: Tensor) -> Dict[str, Any]:
    np.savez_compressed(os.path.join(compress_dir, f"{param_name}.npz"), arr=params.cpu().numpy())
    return meta_of(params)


def decompress_npz(compress_dir: str, param_name: str, meta: Dict[str, Any], device="cuda") -> Tensor:
    arr = np.load(os.path.join(compress_dir, f"{param_name}.npz"))["arr"]
    return torch.tensor(arr).reshape(meta["shape"]).to(dtype=getattr(torch, meta["dtype"]), device=device)


def compress_masked_kmeans(compress_dir: str, param_name: str, params: Tensor, n_clusters: int, method: str = "torch") -> Dict[str, Any]:
    """png_compression.py:521-600: the splats with any positive higher-band coefficient are clustered (``method``: see
    ``kmeans_encode``), the rest is a bit in mask.bin."""
    mask = (params > 0).any(dim=1).any(dim=1).reshape(-1)
    n = int(mask.numel())
    np.packbits(mask.cpu().numpy().astype(bool))[: (n + 7) // 8].tofile(os.path.join(compress_dir, "mask.bin"))
    if int(mask.sum()) == 0:  # nothing to cluster: an empty codebook, every splat decodes to zeros
        np.savez_compressed(os.path.join(compress_dir, f"{param_name}.npz"), centroids=np.zeros((0, params[0].numel()), np.uint8),
                            labels=np.zeros(0, np.uint16))
        meta = {**meta_of(params), "mins": 0.0, "maxs": 0.0, "quantization": 8}
    else:
        cq, labels, meta = kmeans_encode(params[mask], n_clusters=n_clusters, method=method)
        np.savez_compressed(os.path.join(compress_dir, f"{param_name}.npz"), centroids=cq.cpu().numpy(),
                            labels=labels.cpu().numpy().astype(np.uint16))
    meta.update({"shape": list(params.shape), "mask_bits": n, "mask_byte": (n + 7) // 8})
    return meta


def decompress_masked_kmeans(compress_dir: str, param_name: str, m: Dict[str, Any], device) -> Tensor:
    """png_compression.py:603-640: mask.bin + the codebook -> the higher bands, zeros where the mask is clear."""
    bits_loaded = np.fromfile(os.path.join(compress_dir, "mask.bin"), dtype=np.uint8)
    mask = torch.from_numpy(np.unpackbits(bits_loaded)[: m["mask_bits"]].astype(bool))
    z = np.load(os.path.join(compress_dir, f"{param_name}.npz"))
    if z["labels"].size == 0:
        return torch.zeros(m["shape"], dtype=getattr(torch, m["dtype"]), device=device)
    return kmeans_decode(torch.from_numpy(z["centroids"]), torch.from_numpy(z["labels"].astype(np.int32)), m, device=device, mask=mask)


def order_splats(splats: Dict[str, Tensor], use_sort: Union[bool, str], verbose: bool) -> Dict[str, Tensor]:
    """``use_sort``: False = keep the order, "morton" = ``morton_order`` of the (log-transformed) means, "grid" =
    ``sort_splats_grid``, anything else that is true = PLAS through ``sort_splats`` (ImportError without the package)."""
    if use_sort == "morton":
        order = morton_order(splats["means"])
        return {k: v[order] for k, v in splats.items()}
    if use_sort == "grid":
        return sort_splats_grid(splats, verbose=verbose)
    return sort_splats(splats, verbose=verbose) if use_sort else splats


def prepare_splats(splats: Dict[str, Tensor], opacity_threshold: Optional[float], use_sort: Union[bool, str], verbose: bool,
                   normalize_quats: Optional[Callable] = None, always_warn: bool = False) -> Tuple[Dict[str, Tensor], int]:
    """What the reference's compress() does in front of the per-attribute codecs (png_compression.py:101-125), on detached
    copies: the opacity filter (``sigmoid(opacities) >= opacity_threshold``; None = no filter), the log transform of the means,
    the normalised quats (``normalize_quats``: default ``F.normalize``), the crop to a square count -- announced when ``verbose``,
    or whenever it happens with ``always_warn`` -- and the ordering (``order_splats``).  Returns (splats, side length)."""
    splats = {k: v.detach() for k, v in splats.items()}
    if opacity_threshold is not None:
        keep = torch.sigmoid(splats["opacities"]) >= opacity_threshold
        splats = {k: v[keep] for k, v in splats.items()}
    n_before = len(splats["means"])
    splats, side = transform_and_crop(splats, normalize_quats)
    if (verbose or always_warn) and len(splats["means"]) != n_before:
        print(f"Warning: Number of Gaussians was not square. Removed {n_before - len(splats['means'])} Gaussians.")
    return order_splats(splats, use_sort, verbose), side


def write_directory(compress_dir: str, splats: Dict[str, Tensor], encode: Callable[..., Optional[Dict[str, Any]]]) -> None:
    """``encode(name, value, meta)`` writes the files of one attribute and returns its meta entry, or None for an attribute that
    is not the codec's: that one goes to ``<name>.npz``.  ``meta`` holds the entries of the attributes in front of it."""
    os.makedirs(compress_dir, exist_ok=True)
    meta: Dict[str, Any] = {}
    for name, value in splats.items():
        entry = meta_of(value) if value.numel() == 0 else encode(name, value, meta)
        meta[name] = compress_npz(compress_dir, name, value) if entry is None else entry
    with open(os.path.join(compress_dir, "meta.json"), "w") as f:
        json.dump(meta, f)


def read_directory(compress_dir: str, decode: Callable[..., Any], device) -> Dict[str, Tensor]:
    """``decode(name, m, splats)`` returns the attribute from its files and its meta entry, None for an attribute that is not the
    codec's (read from ``<name>.npz``), or ``DEFERRED``: the attribute keeps its place in the result, as None, and the codec
    fills it in after the loop.  ``splats`` holds the attributes in front of it."""
    with open(os.path.join(compress_dir, "meta.json"), "r") as f:
        meta = json.load(f)
    splats: Dict[str, Tensor] = {}
    for name, m in meta.items():
        if not np.all(m["shape"]):
            splats[name] = torch.zeros(m["shape"], dtype=getattr(torch, m["dtype"]), device=device)
            continue
        value = decode(name, m, splats)
        splats[name] = None if value is DEFERRED else decompress_npz(compress_dir, name, m, device) if value is None else value
    return splats
