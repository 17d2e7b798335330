"""The ``<name>.bin`` bitstream of ``HevcCompression``, written down in plain numpy.  THIS MODULE IS THE DEFINITION OF THE FORMAT:
the HIP coder (csrc/plane_codec.hip behind ``plane_codec.py``) must produce the same bytes and the same planes, and does -- the
arithmetic is integer-only.

A small intra transform codec for 8-bit planes ``[H, W, ch]`` (ch = 1..4) with HEVC's quantisation parameter ``qp`` in 0..51.
It is NOT an HEVC bitstream and no replication of x265: no intra prediction, no rate-distortion optimisation, no CABAC.  What it
keeps of H.265 is the 8-point integer transform and the flat quantiser, so that ``qp`` means what it means there
(Qstep = 2^((qp - 4) / 6): six steps halve the precision).

* blocks: H and W are padded to multiples of 8 by edge replication (the header holds H and W, decoding crops); every image
  channel is coded on its own as 8x8 blocks in raster order, n_blocks = ceil(H / 8) ceil(W / 8);
* transform: ``M`` below, ``rs(v, s) = (v + (1 << (s - 1))) >> s`` (arithmetic shift).  Forward: along x with rs(., 2), then
  along y with rs(., 9).  Inverse: along y with rs(., 7), clip to int16, then along x with rs(., 12), clip to 0..255.
  |coefficient| <= 32640; a constant block has the one coefficient 128 v;
* quantiser: qbits = 18 + qp // 6, ``level = sign(c) ((|c| QS[qp % 6] + (171 << (qbits - 9))) >> qbits)``; dequantiser:
  ``clip16(((level LS[qp % 6] << (qp // 6)) + 2) >> 2)`` on levels clamped to +-32767 (every product fits int32);
* symbols: the 64 levels of a block in the scan ``SCAN`` (by anti-diagonal d = i + j of the coefficient at row i, column j;
  within a diagonal by ascending i); the DC level becomes the difference to the DC level of the block before it in the channel
  (0 in front of the first); fold ``u = 2 |l| - (l < 0)``; the symbol is min(u, 255), and a symbol of 255 is an escape whose
  ``u - 255`` goes as a u16 into a side list, in flat symbol order.  The flat sequence is ordered (channel, block, scan position);
* entropy stage: 15 contexts, context of flat symbol i = ``CTX[i % 64]`` = the anti-diagonal of its scan position; one static
  frequency table per context, ``tables_from_histogram`` (``ans_reference.normalize_frequencies`` of the context's histogram) at
  resolution 2^P; the flat sequence is ONE channel of ``ans_reference``'s streams, cut every S symbols (S = 4096 by default: state
  and offset cost 8 bytes per stream), coded by ``ans_reference._encode_streams`` / ``_decode_streams``.  The decoder names the
  symbol of a slot by an 8-step binary search on the cumulative table.

Container, little-endian::

    8 bytes   magic  b"GSTCv1\\0\\0"
    u32 version (1), u32 P, u32 S, u32 qp, u32 H, u32 W, u32 ch, u32 n_escapes
    15 tables: u16 count, then count x (u8 symbol, u16 frequency), symbols ascending, only the symbols that occur; each
               table sums to 2^P.  The integer frequencies themselves: nothing is re-derived from floats on the reading side
    u32 offsets[n_streams + 1]       n_streams = ceil(64 ch n_blocks / S)
    payload                          per stream: u32 final state, then the renormalisation bytes (``ans_reference``)
    u16 escapes[n_escapes]

No torch, no native library: importable anywhere."""
from __future__ import annotations

import struct
from typing import NamedTuple, Tuple

import numpy as np

from . import ans_reference as A

MAGIC = b"GSTCv1\x00\x00"
VERSION = 1
DEFAULT_BITS = A.DEFAULT_BITS  # P
DEFAULT_STREAM_LEN = 4096  # S
MAX_STREAM_LEN = 1 << 24
MAX_QP = 51
MAX_CHANNELS = 4
N_CONTEXTS = 15
ESCAPE = 255
LEVEL_MAX = 32767
_HEADER = struct.Struct("<8sIIIIIIII")

M = np.array([[64, 64, 64, 64, 64, 64, 64, 64],
              [89, 75, 50, 18, -18, -50, -75, -89],
              [83, 36, -36, -83, -83, -36, 36, 83],
              [75, -18, -89, -50, 50, 89, 18, -75],
              [64, -64, -64, 64, 64, -64, -64, 64],
              [50, -89, 18, 75, -75, -18, 89, -50],
              [36, -83, 83, -36, -36, 83, -83, 36],
              [18, -50, 75, -89, 89, -75, 50, -18]], dtype=np.int64)
QS = (26214, 23302, 20560, 18396, 16384, 14564)
LS = (40, 45, 51, 57, 64, 72)

# scan position k -> the coefficient at row i (vertical frequency), column j: SCAN[k] = 8 i + j
SCAN = np.array([8 * i + (d - i) for d in range(15) for i in range(8) if 0 <= d - i < 8], dtype=np.int64)
CTX = (SCAN // 8 + SCAN % 8).astype(np.int64)  # the context of scan position k

NOT_OURS = ("{what} does not start with the magic of this project's transform-coded plane container.  The reference's "
            "HevcCompression writes x265 video payloads (<name>.mp4), which are not read here; every other file of the directory "
            "(means_l.png, means_u.png, shN.npz, mask.bin, meta.json) is interchangeable.")


class Header(NamedTuple):
    bits: int
    stream_len: int
    qp: int
    height: int
    width: int
    channels: int
    n_escapes: int


def rs(v: np.ndarray, s: int) -> np.ndarray:
    return (v + (1 << (s - 1))) >> s


def n_blocks(height: int, width: int) -> int:
    return (-(-height // 8)) * (-(-width // 8))


def check_plane(plane, qp) -> np.ndarray:
    """-> the plane as uint8 [H, W, ch]; ValueError for anything else, and for a qp outside 0..51."""
    p = np.asarray(plane)
    if p.dtype != np.uint8 or p.ndim not in (2, 3):
        raise ValueError(f"the plane must be a uint8 [H, W] or [H, W, ch] array, got {p.dtype} {p.shape}")
    if p.ndim == 2:
        p = p[:, :, None]
    if not 1 <= p.shape[2] <= MAX_CHANNELS or p.shape[0] < 1 or p.shape[1] < 1:
        raise ValueError(f"the plane must be non-empty with 1..{MAX_CHANNELS} channels, got {p.shape}")
    if isinstance(qp, bool) or not isinstance(qp, (int, np.integer)) or not 0 <= qp <= MAX_QP:
        raise ValueError(f"qp must be an integer in 0..{MAX_QP}, got {qp!r}")
    return p


def _blocks(plane: np.ndarray) -> np.ndarray:
    """uint8 [H, W, ch] -> int64 [ch, n_blocks, 8 (y), 8 (x)], padded by edge replication."""
    h, w, ch = plane.shape
    hp, wp = -(-h // 8) * 8, -(-w // 8) * 8
    p = np.pad(plane, ((0, hp - h), (0, wp - w), (0, 0)), mode="edge").astype(np.int64)
    return p.reshape(hp // 8, 8, wp // 8, 8, ch).transpose(4, 0, 2, 1, 3).reshape(ch, -1, 8, 8)


def transform_blocks(blocks: np.ndarray) -> np.ndarray:
    """int64 [ch, n_blocks, 8 (y), 8 (x)] (pixels, or residuals in -255..255) -> coefficients int64 [ch, n_blocks, 8 (v), 8 (u)]:
    the forward transform, |coefficient| <= 32640."""
    t = rs(np.einsum("ux,cbyx->cbyu", M, blocks), 2)  # along x
    return rs(np.einsum("vy,cbyu->cbvu", M, t), 9)  # along y


def forward_blocks(blocks: np.ndarray, qp: int) -> np.ndarray:
    """int64 [ch, n_blocks, 8, 8] -> int64 levels [ch, n_blocks, 64] in scan order: transform and quantiser (on sign and magnitude)."""
    c = transform_blocks(blocks)
    qbits = 18 + qp // 6
    level = np.sign(c) * ((np.abs(c) * QS[qp % 6] + (171 << (qbits - 9))) >> qbits)
    return level.reshape(level.shape[0], level.shape[1], 64)[:, :, SCAN]


def inverse_blocks(levels: np.ndarray, qp: int) -> np.ndarray:
    """levels [ch, n_blocks, 64] in scan order (any values: clamped to +-32767) -> int64 [ch, n_blocks, 8 (y), 8 (x)]: dequantiser
    and inverse transform up to the last ``rs(., 12)``, NOT clipped to 0..255 (a plane clips it; a residual is added to its
    prediction first)."""
    lv = np.asarray(levels)
    level = np.zeros(lv.shape, np.int64)
    level[:, :, SCAN] = np.clip(lv.astype(np.int64), -LEVEL_MAX, LEVEL_MAX)
    c = np.clip((((level * LS[qp % 6]) << (qp // 6)) + 2) >> 2, -32768, 32767).reshape(lv.shape[0], -1, 8, 8)
    t = np.clip(rs(np.einsum("vy,cbvu->cbyu", M, c), 7), -32768, 32767)  # along y
    return rs(np.einsum("ux,cbyu->cbyx", M, t), 12)  # along x


def _unblocks(x: np.ndarray, height: int, width: int) -> np.ndarray:
    """The inverse of ``_blocks``: [ch, n_blocks, 8, 8] with values in 0..255 -> uint8 [H, W, ch], the padding cropped."""
    ch = x.shape[0]
    hb, wb = -(-height // 8), -(-width // 8)
    full = x.reshape(ch, hb, wb, 8, 8).transpose(1, 3, 2, 4, 0).reshape(hb * 8, wb * 8, ch)
    return np.ascontiguousarray(full[:height, :width]).astype(np.uint8)


def forward_levels(plane, qp: int) -> np.ndarray:
    """uint8 plane -> int16 levels [ch, n_blocks, 64] in scan order: transform and quantiser."""
    return forward_blocks(_blocks(check_plane(plane, qp)), qp).astype(np.int16)


def inverse_levels(levels, qp: int, height: int, width: int) -> np.ndarray:
    """int16 levels [ch, n_blocks, 64] in scan order (any values: they are clamped to +-32767) -> uint8 plane [H, W, ch]."""
    lv = np.asarray(levels)
    ch = lv.shape[0]
    if lv.ndim != 3 or lv.shape[1:] != (n_blocks(height, width), 64) or not 1 <= ch <= MAX_CHANNELS or not 0 <= qp <= MAX_QP:
        raise ValueError(f"levels {lv.shape} do not belong to a {height} x {width} plane of 1..{MAX_CHANNELS} channels at qp {qp}")
    return _unblocks(np.clip(inverse_blocks(lv, qp), 0, 255), height, width)


def reconstruct(plane, qp: int) -> np.ndarray:
    """What decoding the encoded plane gives: uint8 [H, W, ch]."""
    p = check_plane(plane, qp)
    return inverse_levels(forward_levels(p, qp), qp, p.shape[0], p.shape[1])


def levels_to_symbols(levels: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """int16 levels [ch, n_blocks, 64] -> (symbols uint8 [64 ch n_blocks] in flat order, escapes uint16): DC differences, fold,
    escapes.  ValueError for a folded value that no u16 escape holds (levels of ``forward_levels`` stay far below)."""
    l = np.asarray(levels).astype(np.int64)
    l[:, 1:, 0] = l[:, 1:, 0] - l[:, :-1, 0]
    u = (2 * np.abs(l) - (l < 0)).reshape(-1)
    if u.max() - ESCAPE > 0xFFFF:
        raise ValueError("a level is too large for a u16 escape")
    return np.minimum(u, ESCAPE).astype(np.uint8), (u[u >= ESCAPE] - ESCAPE).astype(np.uint16)


def symbols_to_levels(symbols: np.ndarray, escapes: np.ndarray, channels: int) -> np.ndarray:
    """The inverse of ``levels_to_symbols`` -> int16 [ch, n_blocks, 64], clamped to +-32767.  The k-th symbol of 255 takes the
    k-th escape, 0 behind the end of the list (a damaged stream gives wrong levels, nothing else)."""
    u = np.asarray(symbols).astype(np.int64).reshape(-1)
    esc = np.concatenate([np.asarray(escapes).astype(np.int64).reshape(-1), [0]])
    is_esc = u == ESCAPE
    rank = np.minimum(np.cumsum(is_esc) - 1, esc.size - 1)
    u = np.where(is_esc, ESCAPE + esc[rank], u)
    l = np.where(u & 1, -((u + 1) >> 1), u >> 1).reshape(channels, -1, 64)
    l[:, :, 0] = np.cumsum(l[:, :, 0], axis=1)
    return np.clip(l, -LEVEL_MAX, LEVEL_MAX).astype(np.int16)


def context_histogram(symbols: np.ndarray) -> np.ndarray:
    """flat symbols uint8 [N] (N a multiple of 64) -> int64 [15, 256]: how often each symbol occurs under each context."""
    s = np.asarray(symbols).reshape(-1, 64).astype(np.int64)
    return np.bincount((CTX[None, :] * 256 + s).reshape(-1), minlength=N_CONTEXTS * 256).reshape(N_CONTEXTS, 256)


def tables_from_histogram(hist: np.ndarray, bits: int = DEFAULT_BITS) -> np.ndarray:
    """int64 [15, 256] counts -> uint32 [15, 256] frequencies that sum to 2^bits per context and are positive exactly where the
    count is: ``normalize_frequencies`` of the float32 relative frequencies (count / total, divided in float64)."""
    h = np.asarray(hist, dtype=np.float64)
    return A.normalize_frequencies((h / h.sum(axis=1, keepdims=True)).astype(np.float32), bits)


def cumulative16(freq: np.ndarray) -> np.ndarray:
    """uint32 [15, 256] -> uint16 [15, 257]: cum[c][s] = the frequencies below s, cum[c][256] = 2^P (<= 2^14: it fits)."""
    cum = np.zeros((freq.shape[0], 257), np.uint16)
    cum[:, 1:] = np.cumsum(freq, axis=1)
    return cum


def slot_bytes(stream_len: int, bits: int) -> int:
    return A.slot_bytes(stream_len, bits)


def _pack_tables(freq: np.ndarray) -> bytes:
    out = []
    for row in freq:
        sym = np.flatnonzero(row)
        rec = np.zeros(sym.size, dtype=[("s", "u1"), ("f", "<u2")])
        rec["s"], rec["f"] = sym, row[sym]
        out.append(struct.pack("<H", sym.size) + rec.tobytes())
    return b"".join(out)


def _unpack_tables(buf: np.ndarray, pos: int, bits: int, what: str, n_tables: int = N_CONTEXTS) -> Tuple[np.ndarray, int]:
    """The inverse of ``_pack_tables`` at ``buf[pos:]`` -> (freq uint32 [n_tables, 256], the position behind the tables); ValueError
    for a table that is truncated, empty, out of order, holds a zero or does not sum to 2^bits."""
    freq = np.zeros((n_tables, 256), np.uint32)
    for c in range(n_tables):
        count = int(buf[pos:pos + 2].view("<u2")[0]) if pos + 2 <= buf.size else -1
        if not 1 <= count <= 256 or pos + 2 + 3 * count > buf.size:
            raise ValueError(f"{what}: truncated or empty frequency table of context {c}")
        rec = buf[pos + 2:pos + 2 + 3 * count].view([("s", "u1"), ("f", "<u2")])
        pos += 2 + 3 * count
        if np.any(np.diff(rec["s"].astype(np.int64)) <= 0) or np.any(rec["f"] == 0) or int(rec["f"].astype(np.int64).sum()) != 1 << bits:
            raise ValueError(f"{what}: the frequency table of context {c} is out of order, holds a zero or does not sum to 2^{bits}")
        freq[c, rec["s"]] = rec["f"]
    return freq, pos


def build_container(head: Header, freq: np.ndarray, offsets: np.ndarray, payload: np.ndarray, escapes: np.ndarray) -> np.ndarray:
    """Header + tables + offset table + payload + escapes -> the file's bytes (uint8 array)."""
    front = _HEADER.pack(MAGIC, VERSION, head.bits, head.stream_len, head.qp, head.height, head.width, head.channels,
                         head.n_escapes) + _pack_tables(freq)
    return np.concatenate([A._container(front, offsets, payload), np.asarray(escapes).astype("<u2").view(np.uint8)])


def parse_container(blob, what: str = "the buffer") -> Tuple[Header, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Validate a container and split it: (header, freq uint32 [15, 256], offsets int64 [n_streams + 1], payload uint8, escapes
    uint16).  Raises ValueError, naming ``what``, for anything a decoder must not be started on: a foreign or short file, an
    unknown version, P, S, qp or ch out of range, an empty plane, a table that is truncated, out of order or does not sum to 2^P,
    offsets that decrease, point outside the file or leave a stream fewer than its 4 state bytes, and an escape list that is not
    what the header claims."""
    buf = A._as_bytes(blob)
    if buf.size < len(MAGIC) or buf[:len(MAGIC)].tobytes() != MAGIC:
        raise ValueError(NOT_OURS.format(what=what))
    if buf.size < _HEADER.size:
        raise ValueError(f"{what}: truncated plane header")
    _, version, bits, stream_len, qp, height, width, channels, n_escapes = _HEADER.unpack(buf[:_HEADER.size].tobytes())
    if version != VERSION:
        raise ValueError(f"{what}: plane container version {version}, this reader knows version {VERSION}")
    if not A.MIN_BITS <= bits <= A.MAX_BITS or not 1 <= stream_len <= MAX_STREAM_LEN or qp > MAX_QP or not 1 <= channels <= MAX_CHANNELS:
        raise ValueError(f"{what}: bad plane header (P = {bits}, S = {stream_len}, qp = {qp}, ch = {channels})")
    if height * width < 1 or 64 * channels * n_blocks(height, width) >= 1 << 31:
        raise ValueError(f"{what}: bad plane header (H = {height}, W = {width})")
    freq, pos = _unpack_tables(buf, _HEADER.size, bits, what)
    n_streams = -(-64 * channels * n_blocks(height, width) // stream_len)
    offsets, rest = A._split_container(buf, pos, n_streams, what)
    end = int(offsets[-1])
    if rest.size - end != 2 * n_escapes:
        raise ValueError(f"{what}: {rest.size - end} bytes behind the payload, the header claims {n_escapes} escapes of 2 bytes")
    escapes = np.ascontiguousarray(rest[end:]).view("<u2").astype(np.uint16)
    return Header(bits, stream_len, qp, height, width, channels, n_escapes), freq, offsets, rest[:end], escapes


def _contexts(n: int, stream_len: int) -> np.ndarray:
    """[n_streams, S]: the context of symbol j of stream r, CTX[(r S + j) % 64]."""
    n_streams = -(-n // stream_len)
    return CTX[np.arange(n_streams * stream_len, dtype=np.int64).reshape(n_streams, stream_len) % 64]


def encode_symbols(symbols: np.ndarray, freq: np.ndarray, stream_len: int, bits: int) -> Tuple[np.ndarray, np.ndarray]:
    """flat symbols uint8 [N] against the tables -> (offsets int64 [n_streams + 1], payload uint8)."""
    sym = np.asarray(symbols, np.uint8).reshape(-1, 1)
    n = sym.shape[0]
    ctx, padded = _contexts(n, stream_len), A._pad(sym, stream_len)
    if np.any(freq[ctx.reshape(-1)[:n], sym[:, 0]] == 0):
        raise ValueError("a symbol occurs whose frequency is 0")
    cum = cumulative16(freq).astype(np.uint32)
    return A._encode_streams(n, 1, stream_len, bits, slot_bytes(stream_len, bits),
                             lambda j: (freq[ctx[:, j], padded[:, j]], cum[ctx[:, j], padded[:, j]]))


def decode_symbols(offsets: np.ndarray, payload: np.ndarray, n: int, freq: np.ndarray, stream_len: int, bits: int) -> np.ndarray:
    """-> flat symbols uint8 [N].  Reads are bounded to each stream's byte range; a byte beyond it is 0."""
    ctx = _contexts(n, stream_len)
    cum = cumulative16(freq).astype(np.int64)

    def lookup(j, slot):
        c = ctx[:, j]
        s = np.zeros(slot.size, np.int64)
        step = 128
        while step >= 1:  # the last s with cum(s) <= slot: 8 steps, always
            s = np.where(cum[c, s + step] <= slot, s + step, s)
            step >>= 1
        return s, cum[c, s + 1] - cum[c, s], cum[c, s]

    return A._decode_streams(offsets, payload, n, 1, stream_len, bits, lookup).reshape(-1)


def encode(plane, qp: int, stream_len: int = DEFAULT_STREAM_LEN, bits: int = DEFAULT_BITS) -> np.ndarray:
    """uint8 plane [H, W] or [H, W, ch] -> container bytes (uint8 array)."""
    p = check_plane(plane, qp)
    if not 1 <= stream_len <= MAX_STREAM_LEN:
        raise ValueError(f"stream_len = {stream_len}")
    symbols, escapes = levels_to_symbols(forward_levels(p, qp))
    freq = tables_from_histogram(context_histogram(symbols), bits)
    offsets, payload = encode_symbols(symbols, freq, stream_len, bits)
    return build_container(Header(bits, stream_len, qp, p.shape[0], p.shape[1], p.shape[2], escapes.size), freq, offsets, payload, escapes)


def decode(blob, what: str = "the buffer") -> np.ndarray:
    """container bytes -> uint8 plane [H, W, ch].  A damaged payload decodes to some plane; what ``parse_container`` refuses
    raises ValueError."""
    head, freq, offsets, payload, escapes = parse_container(blob, what)
    n = 64 * head.channels * n_blocks(head.height, head.width)
    symbols = decode_symbols(offsets, payload, n, freq, head.stream_len, head.bits)
    return inverse_levels(symbols_to_levels(symbols, escapes, head.channels), head.qp, head.height, head.width)
