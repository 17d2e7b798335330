"""Splat sets as ``.ply`` files in the INRIA 3DGS layout, without the ``plyfile`` package: the counterpart of ``save_ply`` /
``load_ply`` of the reference's trainers (``examples/simple_trainer.py:414-510``, ``examples/utils.py:228-287``,
``ply_loader_renderer.py:417-510``), through the kernels of csrc/ply.hip.

    load_ply(path, device="cuda")                     -> ParameterDict: means, sh0, shN, opacities, scales, quats
    save_ply(splats, path, normals=True)              -> None
    load_ply_to_rasterizer_inputs(path, device=...)   -> dict of what ``rasterization()`` takes, by one kernel per chunk
    read_ply_header(path)                             -> PlyHeader (host only)
    column_table(header, fused=False)                 -> PlyColumns: the table the kernels transpose by (host only)

The raw vertex rows go to the GPU as they are (pinned staging buffers of at most 64 MB, the upload of one chunk under the
unpack of the one before) and ``gs_ply_unpack`` writes every tensor; ``gs_ply_pack`` is the way back.  The reader takes
``binary_little_endian 1.0`` files whose first element is ``vertex`` with scalar properties; the properties that are read
(``x y z``, ``f_dc_*``, ``f_rest_*``, ``opacity``, ``scale_*``, ``rot_*``) are ``float`` or ``double`` and may stand in any
order among columns that are skipped.  Everything else is a ``ValueError`` that names the problem, before any launch.  No CPU
fallback: without a GPU the three device functions raise ``RuntimeError``."""
from __future__ import annotations

import ctypes
import os
import threading
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _backend as B

__all__ = ["load_ply", "save_ply", "load_ply_to_rasterizer_inputs", "read_ply_header", "column_table", "ply_header_text",
           "PlyHeader", "PlyProperty", "PlyColumns"]

# PLY scalar types under both spellings -> (canonical name, bytes)
_TYPES = {"char": ("char", 1), "int8": ("char", 1), "uchar": ("uchar", 1), "uint8": ("uchar", 1), "short": ("short", 2),
          "int16": ("short", 2), "ushort": ("ushort", 2), "uint16": ("ushort", 2), "int": ("int", 4), "int32": ("int", 4),
          "uint": ("uint", 4), "uint32": ("uint", 4), "float": ("float", 4), "float32": ("float", 4), "double": ("double", 8),
          "float64": ("double", 8)}
_NUMPY = {"char": "i1", "uchar": "u1", "short": "<i2", "ushort": "<u2", "int": "<i4", "uint": "<u4", "float": "<f4", "double": "<f8"}
_KEYS = ("means", "sh0", "shN", "opacities", "scales", "quats")
_DOUBLE = 1 << 16  # the type flag of a column-table entry (csrc/ply.hip)
_HEADER_LIMIT = 1 << 20  # a header is a few KB; a file without `end_header` in its first MiB is refused
_STAGING_BYTES = 64 << 20


@dataclass(frozen=True)
class PlyProperty:
    name: str
    type: str  # canonical: char uchar short ushort int uint float double
    offset: int  # byte offset inside a vertex row


@dataclass(frozen=True)
class PlyHeader:
    """The header of a binary little-endian ``.ply`` as far as the vertex element goes."""
    format: str  # "binary_little_endian"
    count: int  # vertices
    properties: Tuple[PlyProperty, ...]
    stride: int  # bytes per vertex row
    payload_offset: int  # byte of the file where the first row starts
    elements_after: Tuple[Tuple[str, int], ...] = ()  # (name, count) of the elements behind `vertex`, which are ignored

    def numpy_dtype(self) -> np.dtype:
        """The structured dtype of a vertex row (what ``np.frombuffer`` reads the payload with)."""
        return np.dtype({"names": [p.name for p in self.properties], "formats": [_NUMPY[p.type] for p in self.properties],
                         "offsets": [p.offset for p in self.properties], "itemsize": self.stride})


@dataclass(frozen=True)
class PlyColumns:
    """The column table of ``gs_ply_unpack`` / ``gs_ply_pack``: per float of an output row -- group after group, in output
    order -- ``byte offset | 1 << 16 for a double``; ``widths``: floats per row of means, sh0, shN, opacities, scales, quats
    (``fused``: sh0 and shN as ONE colour group in slot 1, slot 2 empty)."""
    entries: Tuple[int, ...]
    widths: Tuple[int, int, int, int, int, int]
    S0: int
    SN: int
    S: int
    Q: int
    route: str = "words"  # "words": stride and every offset a multiple of 4; else "unaligned" (byte-wise reads)


def _fail(path, what: str):
    return ValueError(f"{path}: {what}")


def parse_ply_header(data: bytes, name: str = "<bytes>") -> PlyHeader:
    """``read_ply_header`` of the leading bytes of a file."""
    if data[:3] != b"ply" or data[3:4] not in (b"\n", b"\r"):
        raise _fail(name, "not a PLY file (no `ply` magic)")
    end = data.find(b"end_header")
    nl = data.find(b"\n", end) if end >= 0 else -1
    if end < 0 or nl < 0:
        raise _fail(name, f"no `end_header` line in the first {min(len(data), _HEADER_LIMIT)} bytes")
    try:
        lines = [ln.rstrip("\r") for ln in data[:nl].decode("ascii").split("\n")]
    except UnicodeDecodeError:
        raise _fail(name, "the header is not ASCII text") from None
    fmt = None
    elements: List[Tuple[str, int]] = []
    props: List[PlyProperty] = []
    offset = 0
    for ln in lines[1:]:
        words = ln.split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "end_header":
            break
        if words[0] == "format":
            if len(words) != 3 or words[2] != "1.0":
                raise _fail(name, f"unsupported format line `{ln}`")
            if words[1] != "binary_little_endian":
                raise _fail(name, f"format {words[1]} is not supported (binary_little_endian 1.0 only)")
            fmt = words[1]
        elif words[0] == "element":
            if len(words) != 3 or not words[2].isdigit():
                raise _fail(name, f"malformed element line `{ln}`")
            if not elements and words[1] != "vertex":
                raise _fail(name, f"element {words[1]} before vertex (vertex must be the first element)")
            elements.append((words[1], int(words[2])))
        elif words[0] == "property":
            if not elements:
                raise _fail(name, f"property line before any element: `{ln}`")
            if len(elements) > 1:
                continue  # elements behind vertex are not read
            if len(words) >= 2 and words[1] == "list":
                raise _fail(name, f"list property inside vertex: `{ln}`")
            if len(words) != 3 or words[1] not in _TYPES:
                raise _fail(name, f"malformed or unknown property line `{ln}`")
            kind, size = _TYPES[words[1]]
            if any(p.name == words[2] for p in props):
                raise _fail(name, f"property {words[2]} twice")
            props.append(PlyProperty(words[2], kind, offset))
            offset += size
        else:
            raise _fail(name, f"unknown header line `{ln}`")
    if fmt is None:
        raise _fail(name, "no format line")
    if not elements:
        raise _fail(name, "no vertex element")
    if elements[0][1] >= 1 << 31:
        raise _fail(name, f"{elements[0][1]} vertices: fewer than 2^31 are supported")
    return PlyHeader(fmt, elements[0][1], tuple(props), offset, nl + 1, tuple(elements[1:]))


def read_ply_header(path) -> PlyHeader:
    """Parse the header of the ``.ply`` at ``path`` (host only, no GPU).  ValueError for anything this reader refuses at the
    level of the header: no magic, ``ascii`` / ``binary_big_endian``, a list property inside ``vertex``, an element before
    ``vertex``, 2^31 vertices or more."""
    with open(path, "rb") as f:
        return parse_ply_header(f.read(_HEADER_LIMIT), str(path))


def _group(header: PlyHeader, prefix: str, name) -> List[PlyProperty]:
    """The properties ``<prefix>0 .. <prefix>{k-1}`` in the order of their numbers; a gap is refused."""
    by_name = {p.name: p for p in header.properties}
    mine = [p for p in header.properties if p.name.startswith(prefix)]
    out = []
    for i in range(len(mine)):
        if f"{prefix}{i}" not in by_name:
            raise _fail(name, f"gap in the numbered group {prefix}*: {len(mine)} properties but no {prefix}{i}")
        out.append(by_name[f"{prefix}{i}"])
    return out


def column_table(header: PlyHeader, fused: bool = False, name: str = "<header>") -> PlyColumns:
    """The column table for the splat tensors of a file with this header, or ValueError: a missing ``x`` / ``y`` / ``z`` /
    ``opacity``, a gap in a numbered group, ``f_dc_*`` or ``f_rest_*`` counts not divisible by 3, a needed property of an
    integer type, a row stride or a column count above the kernel's limits."""
    by_name = {p.name: p for p in header.properties}
    for need in ("x", "y", "z", "opacity"):
        if need not in by_name:
            raise _fail(name, f"missing property {need}")
    dc, rest = _group(header, "f_dc_", name), _group(header, "f_rest_", name)
    scale, rot = _group(header, "scale_", name), _group(header, "rot_", name)
    for what, g in (("f_dc_*", dc), ("f_rest_*", rest)):
        if len(g) % 3:
            raise _fail(name, f"{len(g)} {what} properties: not divisible by 3")

    def channel_major(g):  # output [K, 3] element (k, c) is column c * K + k: reshape(-1, 3, K).transpose(0, 2, 1)
        K = len(g) // 3
        return [g[c * K + k] for k in range(K) for c in range(3)]

    groups = [[by_name["x"], by_name["y"], by_name["z"]], channel_major(dc), channel_major(rest), [by_name["opacity"]], scale, rot]
    if fused:
        groups[1], groups[2] = groups[1] + groups[2], []
    entries = []
    for g in groups:
        for p in g:
            if p.type not in ("float", "double"):
                raise _fail(name, f"property {p.name} has the integer type {p.type}: float or double is needed")
            entries.append(p.offset | (_DOUBLE if p.type == "double" else 0))
    max_stride, max_cols = _limits()
    if header.stride > max_stride:
        raise _fail(name, f"row stride {header.stride} bytes above the limit of {max_stride}")
    if len(entries) > max_cols:
        raise _fail(name, f"{len(entries)} columns to read, above the limit of {max_cols}")
    words = header.stride % 4 == 0 and all((e & 0xFFFF) % 4 == 0 for e in entries)
    return PlyColumns(tuple(entries), tuple(len(g) for g in groups), len(dc), len(rest), len(scale), len(rot),
                      "words" if words else "unaligned")


def _limits() -> Tuple[int, int]:
    return int(B.query("gs_ply_max_stride")), int(B.query("gs_ply_max_columns"))


def _property_names(S0: int, SN: int, S: int, Q: int, normals: bool) -> List[str]:
    return (["x", "y", "z"] + (["nx", "ny", "nz"] if normals else []) + [f"f_dc_{i}" for i in range(S0)]
            + [f"f_rest_{i}" for i in range(SN)] + ["opacity"] + [f"scale_{i}" for i in range(S)] + [f"rot_{i}" for i in range(Q)])


def ply_header_text(n: int, S0: int = 3, SN: int = 45, S: int = 3, Q: int = 4, normals: bool = True) -> bytes:
    """The header ``save_ply`` writes, from the PLY specification: every property a ``float``."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    lines += [f"property float {p}" for p in _property_names(S0, SN, S, Q, normals)]
    return ("\n".join(lines) + "\nend_header\n").encode("ascii")


# ---------------------------------------------------------------------------------------------------------------------
# device side

def _need_gpu(who: str) -> None:
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who}: no GPU (the rows are transposed on the GPU, no CPU fallback)")


def _device_of(who: str, device) -> Tuple[torch.device, bool]:
    """(the GPU to work on, whether the result goes back to the host)."""
    dev = torch.device(device)
    if dev.type not in ("cuda", "cpu"):
        raise ValueError(f"{who}: device must be a GPU or \"cpu\", got {device!r}")
    _need_gpu(who)
    if dev.type == "cpu":
        return torch.device("cuda", torch.cuda.current_device()), True
    return (dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())), False


class _Staging:
    """Two pinned host buffers (grown on demand to at most 64 MB each, kept for the next call), one copy stream per device,
    and the lock that keeps two calls from sharing them."""

    def __init__(self):
        self.lock = threading.Lock()
        self.pinned: List[Optional[Tensor]] = [None, None]
        self.streams: Dict[int, torch.cuda.Stream] = {}

    def buffers(self, nbytes: int) -> List[Tensor]:
        for i in range(2):
            if self.pinned[i] is None or self.pinned[i].numel() < nbytes:
                self.pinned[i] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return self.pinned  # type: ignore[return-value]

    def stream(self, dev: torch.device) -> torch.cuda.Stream:
        s = self.streams.get(dev.index)
        if s is None:
            s = self.streams[dev.index] = torch.cuda.Stream(dev)
        return s


_STAGING = _Staging()


def _rows_per_chunk(stride: int, n: int, forced: Optional[int]) -> int:
    """Rows per chunk: whole row blocks (a multiple of 256 rows, so every chunk starts 16-byte aligned in a buffer of its own
    anyway and no block straddles two chunks), at most 64 MB."""
    rows = forced if forced is not None else _STAGING_BYTES // stride
    rows = max(256, rows // 256 * 256)
    return min(rows, (n + 255) // 256 * 256)


def _c_u32(values) -> ctypes.Array:
    return (ctypes.c_uint32 * len(values))(*values)


def _unpack_file(who: str, path, device, fused: bool, activate: bool, normalize_quats: bool,
                 chunk_rows: Optional[int], force_bytes: bool = False) -> Tuple[PlyColumns, List[Optional[Tensor]], bool]:
    """Header, checks (the file's first: a refused file is a ValueError with or without a GPU), allocation and the chunked
    upload + unpack.  Returns the table, the six group tensors [n, width] on the GPU (None for an empty group) and whether
    the caller asked for them on the host."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        header = parse_ply_header(f.read(_HEADER_LIMIT), path)
        cols = column_table(header, fused, path)
        n, stride = header.count, header.stride
        size = os.fstat(f.fileno()).st_size
        if size - header.payload_offset < n * stride:
            raise _fail(path, f"payload shorter than {n} rows of {stride} bytes ({size - header.payload_offset} < {n * stride}): truncated file")
        dev, to_host = _device_of(who, device)
        outs: List[Optional[Tensor]] = [torch.empty((n, w), dtype=torch.float32, device=dev) if (w or not fused or g != 2) else None
                                        for g, w in enumerate(cols.widths)]
        if n == 0:
            return cols, outs, to_host
        rows_per = _rows_per_chunk(stride, n, chunk_rows)
        nbytes = rows_per * stride
        table, widths = _c_u32(cols.entries), _c_u32(cols.widths)
        f.seek(header.payload_offset)
        with _STAGING.lock, torch.cuda.device(dev):
            pinned = _STAGING.buffers(nbytes)
            host = [p.numpy() for p in pinned]
            main, side = torch.cuda.current_stream(dev), _STAGING.stream(dev)
            staged = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2)]
            uploaded: List[Optional[torch.cuda.Event]] = [None, None]
            unpacked: List[Optional[torch.cuda.Event]] = [None, None]
            side.wait_stream(main)  # the staging tensors were allocated on the caller's stream
            try:
                for i, row0 in enumerate(range(0, n, rows_per)):
                    b, count = i & 1, min(rows_per, n - row0)
                    if uploaded[b] is not None:
                        uploaded[b].synchronize()  # the pinned buffer is free again (a copy, not a kernel, is waited for)
                    got = f.readinto(memoryview(host[b])[:count * stride])
                    if got != count * stride:
                        raise _fail(path, f"payload shorter than {n} rows of {stride} bytes: read ended in row block {i}")
                    with torch.cuda.stream(side):
                        if unpacked[b] is not None:
                            side.wait_event(unpacked[b])  # the device buffer is free again
                        staged[b][:count * stride].copy_(pinned[b][:count * stride], non_blocking=True)
                        uploaded[b] = torch.cuda.Event()
                        uploaded[b].record(side)
                    main.wait_event(uploaded[b])
                    ptrs = (ctypes.c_void_p * 6)(*[None if (t is None or t.shape[1] == 0) else t.data_ptr() + row0 * t.shape[1] * 4
                                                   for t in outs])
                    B.call("gs_ply_unpack", count, stride, B.ptr(staged[b]), ctypes.addressof(table), ctypes.addressof(widths),
                           ctypes.addressof(ptrs), int(activate), int(normalize_quats), int(force_bytes), main.cuda_stream)
                    unpacked[b] = torch.cuda.Event()
                    unpacked[b].record(main)
            finally:
                for e in uploaded:  # the pinned buffers belong to the next call
                    if e is not None:
                        e.synchronize()
    return cols, outs, to_host


@torch.no_grad()
def load_ply(path, device="cuda", _chunk_rows: Optional[int] = None) -> torch.nn.ParameterDict:
    """The reference's ``load_ply``: a ``ParameterDict`` with ``means [N,3]``, ``sh0 [N,S0/3,3]``, ``shN [N,SN/3,3]``,
    ``opacities [N]``, ``scales [N,S]``, ``quats [N,Q]``, float32 on ``device``; ``S0``, ``SN``, ``S``, ``Q`` count the
    properties ``f_dc_*``, ``f_rest_*``, ``scale_*``, ``rot_*``.  Column ``i`` of a group is the property ``<prefix>{i}``
    wherever it stands in the file; a ``double`` is rounded to float32.  ``device="cpu"`` works on the current GPU and copies
    the result back.  ValueError for a file that is refused, RuntimeError without a GPU."""
    cols, outs, to_host = _unpack_file("load_ply", path, device, False, False, False, _chunk_rows)
    n = int(outs[0].shape[0])
    shaped = {"means": outs[0], "sh0": outs[1].view(n, cols.S0 // 3, 3), "shN": outs[2].view(n, cols.SN // 3, 3),
              "opacities": outs[3].view(n), "scales": outs[4], "quats": outs[5]}
    splats = torch.nn.ParameterDict()  # (filled key by key: built from a plain dict it would sort them)
    for k, v in shaped.items():
        splats[k] = torch.nn.Parameter(v.cpu() if to_host else v)
    return splats


@torch.no_grad()
def load_ply_to_rasterizer_inputs(path, device="cuda", activate: bool = True, normalize_quats: bool = True,
                                  _chunk_rows: Optional[int] = None, _force_bytes: bool = False) -> Dict[str, Tensor]:
    """A ``.ply`` straight into what ``rasterization()`` takes, with the keys and semantics of
    ``compression.decode_to_rasterizer_inputs``: ``means``, ``quats`` (``/ max(||q||, 1e-12)`` with ``normalize_quats``),
    ``scales`` (``exp`` with ``activate``), ``opacities`` (``sigmoid`` with ``activate``), ``sh0``, ``shN`` -- and ``colors
    [N, (S0 + SN) / 3, 3]``, the ``cat(sh0, shN)`` the renderer wants, of which ``sh0`` and ``shN`` are views.  The kernel
    applies the activations while it transposes: no raw-parameter intermediate."""
    cols, outs, to_host = _unpack_file("load_ply_to_rasterizer_inputs", path, device, True, activate, normalize_quats, _chunk_rows,
                                       _force_bytes)
    n = int(outs[0].shape[0])
    colors = outs[1].view(n, (cols.S0 + cols.SN) // 3, 3)
    if to_host:
        outs, colors = [None if t is None else t.cpu() for t in outs], colors.cpu()
    return {"means": outs[0], "quats": outs[5], "scales": outs[4], "opacities": outs[3].view(n), "sh0": colors[:, :cols.S0 // 3],
            "shN": colors[:, cols.S0 // 3:], "colors": colors}


def _checked_splats(splats) -> Tuple[List[Tensor], int]:
    """save_ply's refusals: ValueError for a missing key, a shape that is not the layout's, mismatched N or a dtype other than
    float32; RuntimeError for host tensors."""
    for k in _KEYS:
        if k not in splats:
            raise ValueError(f"save_ply: key {k!r} missing (needs {', '.join(_KEYS)})")
    t = {k: splats[k].detach() for k in _KEYS}
    for k, v in t.items():
        if v.dtype != torch.float32:
            raise ValueError(f"save_ply: {k} must be float32, got {v.dtype}")
    dims = {"means": 2, "sh0": 3, "shN": 3, "opacities": 1, "scales": 2, "quats": 2}
    for k, v in t.items():
        if v.dim() != dims[k] or (k == "means" and v.shape[1] != 3) or (k in ("sh0", "shN") and v.shape[2] != 3):
            raise ValueError(f"save_ply: {k} has shape {tuple(v.shape)}")
    n = int(t["means"].shape[0])
    for k, v in t.items():
        if v.shape[0] != n:
            raise ValueError(f"save_ply: mismatched N: means has {n} rows, {k} has {v.shape[0]}")
    if n >= 1 << 31:
        raise ValueError(f"save_ply: fewer than 2^31 splats, got {n}")
    for k, v in t.items():
        if not v.is_cuda:
            raise RuntimeError(f"save_ply: device tensors only ({k} is on {v.device}; the rows are packed on the GPU, no CPU fallback)")
        if v.device != t["means"].device:
            raise ValueError(f"save_ply: means on {t['means'].device}, {k} on {v.device}")
    # a view (a slice of a wider tensor, a transpose) is copied to a dense tensor first: any strides work
    return [t[k].contiguous().view(n, int(np.prod(t[k].shape[1:]))) for k in _KEYS], n


@torch.no_grad()
def save_ply(splats, path, normals: bool = True, _chunk_rows: Optional[int] = None) -> None:
    """The reference's ``save_ply``: the vertex element ``x y z nx ny nz f_dc_* f_rest_* opacity scale_* rot_*`` (the normals
    zeros; ``normals=False`` leaves them out), every property a ``float``, ``binary_little_endian 1.0``.  ``splats``: dict or
    ``ParameterDict`` of float32 device tensors ``means [N,3]``, ``sh0 [N,K0,3]``, ``shN [N,KN,3]``, ``opacities [N]``,
    ``scales [N,S]``, ``quats [N,Q]``, dense or not.  The file is written beside ``path`` and renamed onto it, so an
    interrupted save leaves no truncated ``.ply``."""
    path = os.fspath(path)
    flat, n = _checked_splats(splats)
    S0, SN, S, Q = (int(flat[i].shape[1]) for i in (1, 2, 4, 5))
    names = _property_names(S0, SN, S, Q, normals)
    stride = 4 * len(names)
    max_stride, max_cols = _limits()
    if stride > max_stride or stride - (12 if normals else 0) > 4 * max_cols:
        raise ValueError(f"save_ply: a row of {stride} bytes is above the limit of {max_stride} bytes / {max_cols} columns")
    at = {p: 4 * i for i, p in enumerate(names)}
    K0, KN = S0 // 3, SN // 3
    # input element (k, c) of sh0 / shN goes to the channel-major column c * K + k: transpose(1, 2).flatten(1)
    entries = ([at["x"], at["y"], at["z"]] + [at[f"f_dc_{c * K0 + k}"] for k in range(K0) for c in range(3)]
               + [at[f"f_rest_{c * KN + k}"] for k in range(KN) for c in range(3)] + [at["opacity"]]
               + [at[f"scale_{i}"] for i in range(S)] + [at[f"rot_{i}"] for i in range(Q)])
    dev = flat[0].device
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(ply_header_text(n, S0, SN, S, Q, normals))
            if n:
                rows_per = _rows_per_chunk(stride, n, _chunk_rows)
                nbytes = rows_per * stride
                table, widths = _c_u32(entries), _c_u32([int(t.shape[1]) for t in flat])
                with _STAGING.lock, torch.cuda.device(dev):
                    pinned = _STAGING.buffers(nbytes)
                    host = [p.numpy() for p in pinned]
                    main = torch.cuda.current_stream(dev)
                    staged = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2)]
                    done: List[Optional[Tuple[torch.cuda.Event, int]]] = [None, None]

                    def flush(b: int) -> None:  # chunk b has arrived in its pinned buffer: to the file
                        if done[b] is not None:
                            done[b][0].synchronize()
                            host[b][:done[b][1]].tofile(f)
                            done[b] = None

                    for i, row0 in enumerate(range(0, n, rows_per)):
                        b, count = i & 1, min(rows_per, n - row0)
                        ptrs = (ctypes.c_void_p * 6)(*[None if t.shape[1] == 0 else t.data_ptr() + row0 * t.shape[1] * 4 for t in flat])
                        B.call("gs_ply_pack", count, stride, ctypes.addressof(table), ctypes.addressof(widths), ctypes.addressof(ptrs),
                               B.ptr(staged[b]), main.cuda_stream)
                        pinned[b][:count * stride].copy_(staged[b][:count * stride], non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(main)
                        done[b] = (ev, count * stride)
                        flush(b ^ 1)  # the write of chunk i - 1, while the GPU packs chunk i
                    flush(0)
                    flush(1)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise

