"""The transform-coded attribute planes of ``HevcCompression`` on the GPU: an 8-bit plane ``[H, W, ch]`` and HEVC's quantisation
parameter  <->  the ``<name>.bin`` container of ``plane_codec_reference`` (which defines the format; the kernels of
csrc/plane_codec.hip compute the same levels, planes and bytes).

    plane_encode(plane, qp, stream_len=4096)  -> container bytes   (transform + quantiser, symbols, histogram, rANS, pack)
    plane_decode(blob, device)                -> uint8 [H, W, ch]  (container validated on the host before any launch)
    transform_levels(plane, qp)               -> int16 [ch, n_blocks, 64]     gs_plane_transform_fwd alone
    inverse_transform(levels, qp, H, W)       -> uint8 [H, W, ch]             gs_plane_transform_inv alone

Between the two kernels of a direction sit the steps the format defines on whole arrays -- the DC differences, the fold, the
escapes, the per-context histogram and their inverses -- as torch operations on the device (``cumsum``, ``nonzero`` in flat order,
``bincount``): once per file, and each is one statement of the numpy module.  The frequency tables are derived from the histogram
on the host by the numpy module's own ``tables_from_histogram``, so both sides normalise with the same code."""
from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

from .. import _backend as B
from . import plane_codec_reference as R
from ._ans_streams import _stream, decode_buffers, encode_streams


def _check_plane(plane: Tensor, qp) -> Tensor:
    """-> the contiguous uint8 [H, W, ch] device plane; ValueError for a wrong dtype, shape, channel count or qp, RuntimeError
    for a host tensor."""
    if not isinstance(plane, Tensor):
        raise ValueError(f"the plane must be a uint8 device tensor, got {type(plane).__name__}")
    if plane.dtype != torch.uint8 or plane.dim() not in (2, 3):
        raise ValueError(f"the plane must be a uint8 [H, W] or [H, W, ch] tensor, got {plane.dtype} {tuple(plane.shape)}")
    if plane.dim() == 2:
        plane = plane[:, :, None]
    h, w, ch = plane.shape
    if not 1 <= ch <= R.MAX_CHANNELS or h < 1 or w < 1 or 64 * ch * R.n_blocks(h, w) >= 1 << 31:
        raise ValueError(f"the plane must be non-empty with 1..{R.MAX_CHANNELS} channels and fewer than 2^31 coefficients, got {tuple(plane.shape)}")
    _check_qp(qp)
    if not plane.is_cuda:
        raise RuntimeError("the plane codec runs on the GPU: the plane must be a device tensor (no CPU fallback); "
                           "plane_codec_reference.encode is the numpy form")
    return plane.contiguous()


def _check_qp(qp) -> None:
    if isinstance(qp, bool) or not isinstance(qp, (int, np.integer)) or not 0 <= qp <= R.MAX_QP:
        raise ValueError(f"qp must be an integer in 0..{R.MAX_QP}, got {qp!r}")


@torch.no_grad()
def transform_levels(plane: Tensor, qp: int) -> Tensor:
    """uint8 device plane -> int16 levels [ch, n_blocks, 64] in scan order, equal to ``plane_codec_reference.forward_levels``."""
    plane = _check_plane(plane, qp)
    h, w, ch = plane.shape
    levels = torch.empty((ch, R.n_blocks(h, w), 64), dtype=torch.int16, device=plane.device)
    with torch.cuda.device(plane.device):
        B.call("gs_plane_transform_fwd", h, w, ch, int(qp), B.ptr(plane), B.ptr(levels), _stream(plane))
    return levels


@torch.no_grad()
def inverse_transform(levels: Tensor, qp: int, height: int, width: int) -> Tensor:
    """int16 device levels [ch, n_blocks, 64] (any values) -> uint8 plane [H, W, ch], equal to
    ``plane_codec_reference.inverse_levels``."""
    if not isinstance(levels, Tensor) or not levels.is_cuda:
        raise RuntimeError("the plane codec runs on the GPU: the levels must be a device tensor (no CPU fallback)")
    _check_qp(qp)
    if (levels.dtype != torch.int16 or levels.dim() != 3 or height < 1 or width < 1 or not 1 <= levels.shape[0] <= R.MAX_CHANNELS
            or tuple(levels.shape[1:]) != (R.n_blocks(height, width), 64)):
        raise ValueError(f"levels {levels.dtype} {tuple(levels.shape)} do not belong to a {height} x {width} plane of 1..{R.MAX_CHANNELS} channels")
    levels = levels.contiguous()
    ch = levels.shape[0]
    plane = torch.empty((height, width, ch), dtype=torch.uint8, device=levels.device)
    with torch.cuda.device(levels.device):
        B.call("gs_plane_transform_inv", height, width, ch, int(qp), B.ptr(levels), B.ptr(plane), _stream(levels))
    return plane


def _context_index(n: int, dev: torch.device) -> Tensor:
    """int64 [n]: 256 CTX[i % 64], the row of symbol i in the [15, 256] histogram."""
    return (torch.from_numpy(R.CTX * 256).to(dev)).repeat(n // 64)


def encode_levels(levels: Tensor, dc_differences: bool, stream_len: int, bits: int):
    """int16 device levels [rows, n_blocks, 64] -> (freq uint32 [15, 256], offsets, payload, escapes), all numpy: the module's
    ``levels_to_symbols`` (DC differences along the blocks of a row when ``dc_differences``, fold, escapes), the per-context
    histogram, the host-side tables and ``gs_plane_ans_encode``.  The plane codec calls it once, the plane-sequence codec once per
    group of frames."""
    dev = levels.device
    l = levels.to(torch.int32)
    if dc_differences:
        l[:, 1:, 0] = l[:, 1:, 0] - l[:, :-1, 0]
    u = (2 * l.abs() - (l < 0).to(torch.int32)).reshape(-1)
    symbols = u.clamp(max=R.ESCAPE).to(torch.uint8)
    escapes = (u[torch.nonzero(u >= R.ESCAPE).reshape(-1)] - R.ESCAPE).cpu().numpy().astype(np.uint16)
    n = symbols.numel()
    hist = torch.bincount(_context_index(n, dev) + symbols.long(), minlength=R.N_CONTEXTS * 256).reshape(R.N_CONTEXTS, 256)
    freq = R.tables_from_histogram(hist.cpu().numpy(), bits)
    cum = torch.from_numpy(R.cumulative16(freq).view(np.int16)).to(dev)
    sym2d = symbols.reshape(n, 1)

    def launch(scratch, lengths, states, status, stream):
        B.call("gs_plane_ans_encode", n, int(stream_len), bits, B.ptr(symbols), B.ptr(cum), B.ptr(scratch), scratch.numel(),
               B.ptr(lengths), B.ptr(states), B.ptr(status), stream)

    offsets, payload = encode_streams(sym2d, int(stream_len), int(B.query("gs_plane_ans_slot_bytes", int(stream_len), bits)), launch,
                                      "gs_plane_ans_encode", "1: a symbol with frequency 0, 2: slot too small")
    return freq, offsets, payload, escapes


def decode_levels(freq: np.ndarray, offsets: np.ndarray, payload: np.ndarray, escapes: np.ndarray, n: int, rows: int, dc_sums: bool,
                  stream_len: int, bits: int, dev: torch.device, what: str) -> Tensor:
    """The inverse of ``encode_levels`` on a parsed group of ``n`` symbols -> int16 device levels [rows, n / (64 rows), 64]:
    ``gs_plane_ans_decode``, then the module's ``symbols_to_levels`` (escapes, unfold, DC sums when ``dc_sums``, clamp)."""
    d_off, d_payload, symbols = decode_buffers(n, 1, stream_len, 1, offsets, payload, dev, what)
    if d_payload.numel() == 0:  # unreachable behind parse_container (a stream has its 4 state bytes); the kernel takes no null
        raise ValueError(f"{what}: empty payload")
    cum = torch.from_numpy(R.cumulative16(freq).view(np.int16)).to(dev)
    with torch.cuda.device(dev):
        B.call("gs_plane_ans_decode", n, stream_len, bits, B.ptr(d_payload), d_payload.numel(), B.ptr(d_off), B.ptr(cum),
               B.ptr(symbols), _stream(symbols))
    u = symbols.reshape(-1).to(torch.int64)
    esc = torch.from_numpy(np.concatenate([escapes.astype(np.int64), [0]])).to(dev)
    is_esc = u == R.ESCAPE
    rank = (torch.cumsum(is_esc, dim=0) - 1).clamp(min=0, max=esc.numel() - 1)
    u = torch.where(is_esc, R.ESCAPE + esc[rank], u)
    l = torch.where((u & 1) != 0, -((u + 1) >> 1), u >> 1).reshape(rows, -1, 64)
    if dc_sums:
        l[:, :, 0] = torch.cumsum(l[:, :, 0], dim=1)
    return l.clamp(-R.LEVEL_MAX, R.LEVEL_MAX).to(torch.int16)


@torch.no_grad()
def plane_encode(plane: Tensor, qp: int, stream_len: int = R.DEFAULT_STREAM_LEN, bits: int = R.DEFAULT_BITS) -> np.ndarray:
    """Encode a uint8 device plane [H, W] or [H, W, ch] (ch = 1..4) at ``qp`` (0..51) -> the container as a numpy uint8 array,
    byte-identical to ``plane_codec_reference.encode``.  Refused before any launch: a host tensor (RuntimeError), a wrong dtype,
    shape, channel count, qp, stream length or resolution (ValueError)."""
    plane = _check_plane(plane, qp)
    if isinstance(stream_len, bool) or not isinstance(stream_len, (int, np.integer)) or not 1 <= stream_len <= R.MAX_STREAM_LEN:
        raise ValueError(f"stream_len = {stream_len!r}")
    if not R.A.MIN_BITS <= bits <= R.A.MAX_BITS:
        raise ValueError(f"probability resolution of {bits} bits, supported: {R.A.MIN_BITS}..{R.A.MAX_BITS}")
    h, w, ch = plane.shape
    freq, offsets, payload, escapes = encode_levels(transform_levels(plane, qp), True, int(stream_len), bits)
    return R.build_container(R.Header(bits, int(stream_len), int(qp), h, w, ch, escapes.size), freq, offsets, payload, escapes)


@torch.no_grad()
def plane_decode(blob, device="cuda", what: str = "the buffer") -> Tensor:
    """Decode a container (bytes or uint8 array) -> uint8 [H, W, ch] on ``device``, the layout ``dequantize_grid`` reads, equal to
    ``plane_codec_reference.decode``.  The container is validated on the host first (ValueError naming ``what``; nothing is launched
    on a file ``parse_container`` refuses); the kernels also bound their own reads and clamp the levels."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("the plane codec runs on the GPU (no CPU fallback); plane_codec_reference.decode is the numpy form")
    head, freq, offsets, payload, escapes = R.parse_container(blob, what)
    n = 64 * head.channels * R.n_blocks(head.height, head.width)
    levels = decode_levels(freq, offsets, payload, escapes, n, head.channels, True, head.stream_len, head.bits, dev, what)
    return inverse_transform(levels, head.qp, head.height, head.width)
