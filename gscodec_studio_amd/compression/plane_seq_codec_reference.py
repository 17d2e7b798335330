"""The ``<name>.bin`` bitstream of ``SeqHevcCompression``, written down in plain numpy.  THIS MODULE IS THE DEFINITION OF THE FORMAT:
the HIP coder (``plane_seq_fwd_kernel`` / ``plane_seq_inv_kernel`` of csrc/plane_codec.hip behind ``plane_seq_codec.py``) must
produce the same levels, frames and bytes, and does -- the arithmetic is integer-only.

A sequence of T 8-bit planes ``[T, H, W, ch]`` (ch = 1..4) under HEVC's quantisation parameter ``qp`` (0..51), coded with the stages
of ``plane_codec_reference`` (blocks, transform ``M``, quantiser, dequantiser, scan ``SCAN``, fold, escapes, the 15 context tables
and the rANS streams are THAT module's, imported, not restated) plus temporal prediction:

* frame types: frame t is an I frame when ``t % gop == 0``, otherwise a P frame; ``gop = 1`` is all-intra;
* state: the padded reconstruction, int ``[ch, n_blocks, 8, 8]`` with values in 0..255 on all 64 pixels of every block, the padding
  pixels included -- encoder and decoder carry the same state, nothing of it is stored;
* I frame: levels = ``plane_codec_reference.forward_levels(x_t, qp)``; state = that module's inverse on them, uncropped;
* P frame: residual = ``_blocks(x_t) - state`` on the edge-replicated source, in -255..255, through the same forward transform and
  quantiser (which works on sign and magnitude).  |coefficient| <= 32640 holds for signed input too: every row of ``M`` has an L1
  norm <= 512, so |first pass| <= rs(512 * 255, 2) = 32640 and |second pass| <= rs(512 * 32640, 9) = 32640.
  state = ``clip(state + inv(levels), 0, 255)`` with ``inv`` = the plane codec's dequantiser and inverse transform with its int16
  clips, ending in ``rs(., 12)`` WITHOUT the clip to 0..255;
* decoded frame t: the state behind frame t, cropped to H x W.  No motion search and no spatial prediction: a block depends on the
  co-located block of the frame before alone;
* symbols: two flat sequences, each ordered (frame, channel, block, scan position): the levels of the I frames in frame order, and
  the levels of the P frames.  I frames keep the plane codec's DC differences (restarting at every frame and channel); P frames
  have none (residual DCs are not spatially correlated).  Fold and escapes as in the plane codec;
* entropy stage: each group has its own 15 context tables from its own histogram and is coded by the plane codec's
  ``encode_symbols`` / ``decode_symbols`` (the context of flat symbol i is still ``CTX[i % 64]``).

Container, little-endian::

    8 bytes   magic  b"GSTSv1\\0\\0"
    u32 version (1), u32 P, u32 S, u32 qp, u32 H, u32 W, u32 ch, u32 T, u32 gop, u32 n_escapes_I, u32 n_escapes_P
    the I group (frames 0, gop, 2 gop, ...: n_I = ceil(T / gop) frames, N_I = 64 ch n_blocks n_I symbols):
        15 tables                        as in the plane container
        u32 offsets[n_streams + 1]       n_streams = ceil(N_I / S)
        payload
        u16 escapes[n_escapes_I]
    the P group (the other T - n_I frames), in the same layout; ABSENT when there is no P frame

The lossless 16-bit grids of ``means.bin`` (the reference's ``lossless=1`` videos of the low and the high byte) are a small wrapper
around two containers of ``ans_reference``, defined at the end of this module.

No torch, no native library: importable anywhere."""
from __future__ import annotations

import struct
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import ans_reference as A
from . import plane_codec_reference as P

MAGIC = b"GSTSv1\x00\x00"
VERSION = 1
DEFAULT_BITS = P.DEFAULT_BITS
DEFAULT_STREAM_LEN = P.DEFAULT_STREAM_LEN
_HEADER = struct.Struct("<8s11I")

NOT_OURS = ("{what} does not start with the magic of this project's transform-coded plane-sequence container.  The reference's "
            "SeqHevcCompression writes x265 video payloads (<name>.mp4), which are not read here.")


class Header(NamedTuple):
    bits: int
    stream_len: int
    qp: int
    height: int
    width: int
    channels: int
    frames: int
    gop: int
    n_escapes_i: int
    n_escapes_p: int


class Group(NamedTuple):
    """One of the two symbol groups of a file, parsed: what ``decode_symbols`` takes."""
    freq: np.ndarray  # uint32 [15, 256]
    offsets: np.ndarray  # int64 [n_streams + 1]
    payload: np.ndarray  # uint8
    escapes: np.ndarray  # uint16


def is_intra(frames: int, gop: int) -> np.ndarray:
    """bool [T]: frame t is an I frame."""
    return np.arange(frames) % gop == 0


def check_gop(gop) -> None:
    if isinstance(gop, bool) or not isinstance(gop, (int, np.integer)) or not 1 <= gop < 1 << 32:
        raise ValueError(f"gop must be a positive integer below 2^32 (the header's field), got {gop!r}")


def check_frames(frames, qp, gop) -> np.ndarray:
    """-> the sequence as uint8 [T, H, W, ch]; ValueError for anything else, for a qp outside 0..51 and a gop below 1."""
    f = np.asarray(frames)
    if f.dtype != np.uint8 or f.ndim not in (3, 4):
        raise ValueError(f"the sequence must be a uint8 [T, H, W] or [T, H, W, ch] array, got {f.dtype} {f.shape}")
    if f.ndim == 3:
        f = f[..., None]
    if f.shape[0] < 1:
        raise ValueError(f"the sequence must hold at least one frame, got {f.shape}")
    P.check_plane(f[0], qp)
    check_gop(gop)
    if 64 * f.shape[3] * P.n_blocks(f.shape[1], f.shape[2]) * f.shape[0] >= 1 << 31:
        raise ValueError(f"the sequence must have fewer than 2^31 coefficients, got {f.shape}")
    return f


def _closed_loop(frames: np.ndarray, qp: int, gop: int) -> Tuple[np.ndarray, np.ndarray]:
    t_n, h, w, ch = frames.shape
    levels = np.zeros((t_n, ch, P.n_blocks(h, w), 64), np.int16)
    out = np.zeros(frames.shape, np.uint8)
    state = None
    for t in range(t_n):
        if t % gop == 0:
            levels[t] = P.forward_levels(frames[t], qp)
            state = np.clip(P.inverse_blocks(levels[t], qp), 0, 255)
        else:
            levels[t] = P.forward_blocks(P._blocks(frames[t]) - state, qp).astype(np.int16)
            state = np.clip(state + P.inverse_blocks(levels[t], qp), 0, 255)
        out[t] = P._unblocks(state, h, w)
    return levels, out


def forward_levels(frames, qp: int, gop: int) -> np.ndarray:
    """uint8 [T, H, W, ch] -> int16 levels [T, ch, n_blocks, 64] in scan order: the encoder's closed loop."""
    return _closed_loop(check_frames(frames, qp, gop), qp, gop)[0]


def reconstruct(frames, qp: int, gop: int) -> np.ndarray:
    """What decoding the encoded sequence gives: uint8 [T, H, W, ch]."""
    return _closed_loop(check_frames(frames, qp, gop), qp, gop)[1]


def inverse_levels(levels, qp: int, gop: int, height: int, width: int) -> np.ndarray:
    """int16 levels [T, ch, n_blocks, 64] (any values: they are clamped to +-32767) -> uint8 [T, H, W, ch]: the decoder's loop."""
    lv = np.asarray(levels)
    check_gop(gop)
    if (lv.ndim != 4 or lv.shape[0] < 1 or lv.shape[2:] != (P.n_blocks(height, width), 64) or not 1 <= lv.shape[1] <= P.MAX_CHANNELS
            or not 0 <= qp <= P.MAX_QP):
        raise ValueError(f"levels {lv.shape} do not belong to a sequence of {height} x {width} planes of 1..{P.MAX_CHANNELS} channels at qp {qp}")
    out = np.zeros((lv.shape[0], height, width, lv.shape[1]), np.uint8)
    state = 0
    for t in range(lv.shape[0]):
        state = np.clip((0 if t % gop == 0 else state) + P.inverse_blocks(lv[t], qp), 0, 255)
        out[t] = P._unblocks(state, height, width)
    return out


def levels_to_symbols(levels: np.ndarray, gop: int) -> Tuple[Tuple[np.ndarray, np.ndarray], Optional[Tuple[np.ndarray, np.ndarray]]]:
    """int16 [T, ch, n_blocks, 64] -> ((symbols, escapes) of the I group, the same of the P group or None).  The plane codec's
    ``levels_to_symbols`` on both: the I frames as n_I ch channels (DC differences along the blocks of one frame and channel), the
    P frames as one block per "channel", which leaves their DC levels as they are."""
    lv = np.asarray(levels)
    intra = is_intra(lv.shape[0], gop)
    group_i = P.levels_to_symbols(lv[intra].reshape(-1, lv.shape[2], 64))
    return group_i, (P.levels_to_symbols(lv[~intra].reshape(-1, 1, 64)) if not intra.all() else None)


def symbols_to_levels(group_i, group_p, frames: int, gop: int, channels: int) -> np.ndarray:
    """The inverse of ``levels_to_symbols`` -> int16 [T, ch, n_blocks, 64], clamped to +-32767."""
    intra = is_intra(frames, gop)
    n_i = int(intra.sum())
    lv_i = P.symbols_to_levels(group_i[0], group_i[1], n_i * channels)
    out = np.zeros((frames, channels, lv_i.shape[1], 64), np.int16)
    out[intra] = lv_i.reshape(n_i, channels, -1, 64)
    if n_i < frames:
        n = np.asarray(group_p[0]).size // 64
        out[~intra] = P.symbols_to_levels(group_p[0], group_p[1], n).reshape(frames - n_i, channels, -1, 64)
    return out


def _pack_group(freq: np.ndarray, offsets: np.ndarray, payload: np.ndarray, escapes: np.ndarray) -> np.ndarray:
    return np.concatenate([A._container(P._pack_tables(freq), offsets, payload), np.asarray(escapes).astype("<u2").view(np.uint8)])


def build_container(head: Header, group_i: Group, group_p: Optional[Group]) -> np.ndarray:
    """Header + the I group + the P group (None without a P frame) -> the file's bytes (uint8 array)."""
    front = np.frombuffer(_HEADER.pack(MAGIC, VERSION, *head), np.uint8)
    return np.concatenate([front, _pack_group(*group_i)] + ([_pack_group(*group_p)] if group_p is not None else []))


def _parse_group(buf: np.ndarray, pos: int, n: int, head: Header, n_escapes: int, what: str) -> Tuple[Group, int]:
    freq, pos = P._unpack_tables(buf, pos, head.bits, what)
    n_streams = -(-n // head.stream_len)
    offsets, rest = A._split_container(buf, pos, n_streams, what)
    end = int(offsets[-1])
    if rest.size - end < 2 * n_escapes:
        raise ValueError(f"{what}: {rest.size - end} bytes behind a payload, the header claims {n_escapes} escapes of 2 bytes")
    escapes = np.ascontiguousarray(rest[end:end + 2 * n_escapes]).view("<u2").astype(np.uint16)
    return Group(freq, offsets, rest[:end], escapes), pos + 4 * (n_streams + 1) + end + 2 * n_escapes


def parse_container(blob, what: str = "the buffer") -> Tuple[Header, Group, Optional[Group]]:
    """Validate a container and split it: (header, the I group, the P group or None).  Raises ValueError, naming ``what``, for
    anything a decoder must not be started on: what ``plane_codec_reference.parse_container`` refuses (a foreign or short file, an
    unknown version, P, S, qp or ch out of range, an empty plane, bad tables, bad offsets, an escape list that is not what the header
    claims), and T = 0, gop = 0, a group of 2^31 coefficients or more, a P group that T and gop imply and the file lacks, and bytes
    behind the last group (a P group, or escapes of one, that T and gop exclude)."""
    buf = A._as_bytes(blob)
    if buf.size < len(MAGIC) or buf[:len(MAGIC)].tobytes() != MAGIC:
        raise ValueError(NOT_OURS.format(what=what))
    if buf.size < _HEADER.size:
        raise ValueError(f"{what}: truncated plane-sequence header")
    version, *fields = _HEADER.unpack(buf[:_HEADER.size].tobytes())[1:]
    if version != VERSION:
        raise ValueError(f"{what}: plane-sequence container version {version}, this reader knows version {VERSION}")
    head = Header(*fields)
    if (not A.MIN_BITS <= head.bits <= A.MAX_BITS or not 1 <= head.stream_len <= P.MAX_STREAM_LEN or head.qp > P.MAX_QP
            or not 1 <= head.channels <= P.MAX_CHANNELS):
        raise ValueError(f"{what}: bad plane-sequence header (P = {head.bits}, S = {head.stream_len}, qp = {head.qp}, ch = {head.channels})")
    if head.frames < 1 or head.gop < 1:
        raise ValueError(f"{what}: bad plane-sequence header (T = {head.frames}, gop = {head.gop})")
    n_i = -(-head.frames // head.gop)
    n_p = head.frames - n_i
    per_frame = 64 * head.channels * P.n_blocks(head.height, head.width)
    if head.height * head.width < 1 or per_frame * max(n_i, n_p) >= 1 << 31:
        raise ValueError(f"{what}: bad plane-sequence header (H = {head.height}, W = {head.width}, T = {head.frames}, gop = {head.gop})")
    if n_p == 0 and head.n_escapes_p:
        raise ValueError(f"{what}: the header claims {head.n_escapes_p} escapes of P frames, T = {head.frames} and gop = {head.gop} leave none")
    group_i, pos = _parse_group(buf, _HEADER.size, per_frame * n_i, head, head.n_escapes_i, what)
    group_p = None
    if n_p:
        if pos == buf.size:
            raise ValueError(f"{what}: the file ends behind the I group, T = {head.frames} and gop = {head.gop} imply a P group")
        group_p, pos = _parse_group(buf, pos, per_frame * n_p, head, head.n_escapes_p, what)
    if pos != buf.size:
        raise ValueError(f"{what}: {buf.size - pos} bytes behind the last group" + ("" if n_p else
                         f" (a P group? T = {head.frames} and gop = {head.gop} leave no P frame)"))
    return head, group_i, group_p


def _encode_group(symbols: np.ndarray, escapes: np.ndarray, stream_len: int, bits: int) -> Group:
    freq = P.tables_from_histogram(P.context_histogram(symbols), bits)
    offsets, payload = P.encode_symbols(symbols, freq, stream_len, bits)
    return Group(freq, offsets, payload, escapes)


def encode(frames, qp: int, gop: int, stream_len: int = DEFAULT_STREAM_LEN, bits: int = DEFAULT_BITS) -> np.ndarray:
    """uint8 [T, H, W] or [T, H, W, ch] -> container bytes (uint8 array)."""
    f = check_frames(frames, qp, gop)
    if not 1 <= stream_len <= P.MAX_STREAM_LEN:
        raise ValueError(f"stream_len = {stream_len}")
    sym_i, sym_p = levels_to_symbols(_closed_loop(f, qp, gop)[0], gop)
    head = Header(bits, stream_len, qp, f.shape[1], f.shape[2], f.shape[3], f.shape[0], gop, sym_i[1].size, 0 if sym_p is None else sym_p[1].size)
    return build_container(head, _encode_group(*sym_i, stream_len, bits), None if sym_p is None else _encode_group(*sym_p, stream_len, bits))


def decode(blob, what: str = "the buffer") -> np.ndarray:
    """container bytes -> uint8 [T, H, W, ch].  A damaged payload decodes to some frames; what ``parse_container`` refuses raises
    ValueError."""
    head, group_i, group_p = parse_container(blob, what)
    n_i = -(-head.frames // head.gop)
    per_frame = 64 * head.channels * P.n_blocks(head.height, head.width)

    def symbols(group, n_frames):
        return P.decode_symbols(group.offsets, group.payload, per_frame * n_frames, group.freq, head.stream_len, head.bits), group.escapes

    levels = symbols_to_levels(symbols(group_i, n_i), None if group_p is None else symbols(group_p, head.frames - n_i), head.frames,
                               head.gop, head.channels)
    return inverse_levels(levels, head.qp, head.gop, head.height, head.width)


# ---- means.bin: lossless 16-bit grids with temporal differences ------------------------------------------------------------------
#
# grid uint16 [T, H, W, C] (the 16-bit min-max grid of the means, C = 3).  Inside a GOP frame t stores d = (grid[t] - grid[t - 1]) mod
# 2^16, read as int16 and folded by zig-zag, u = (d << 1) ^ (d >> 15), a GOP's first frame stores its values raw; either u16 is split
# into its low and its high byte.  The bytes of the I frames, uint8 [n_I H W, 2 C] (C low bytes, then C high bytes), and those of
# the P frames are coded as two containers of ``ans_reference`` against their own histograms.  Little-endian::
#
#     8 bytes   magic  b"GSTMv1\0\0"
#     u32 version (1), u32 P, u32 T, u32 H, u32 W, u32 C, u32 gop, u32 bytes_I, u32 bytes_P
#     the I group: 2 C frequency tables (the plane container's table records; each sums to 2^P), then bytes_I bytes: a GSANSv1
#                  container (its probability table is frequency / 2^P, which ``normalize_frequencies`` maps back exactly)
#     the P group, in the same layout; absent (bytes_P = 0) when there is no P frame

MEANS_MAGIC = b"GSTMv1\x00\x00"
_MEANS_HEADER = struct.Struct("<8s9I")
MEANS_MAX_CHANNELS = 8  # 2 C byte columns: what one call of the ANS coder takes (16)


class MeansHeader(NamedTuple):
    bits: int
    frames: int
    height: int
    width: int
    channels: int
    gop: int
    bytes_i: int
    bytes_p: int


def means_symbols(grid, gop: int) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """uint16 [T, H, W, C] -> (uint8 [n_I H W, 2 C], uint8 [n_P H W, 2 C] or None)."""
    g = np.asarray(grid)
    check_gop(gop)
    if g.dtype != np.uint16 or g.ndim != 4 or min(g.shape) < 1 or g.shape[3] > MEANS_MAX_CHANNELS:
        raise ValueError(f"the grids must be a non-empty uint16 [T, H, W, C] array with C <= {MEANS_MAX_CHANNELS}, got {g.dtype} {g.shape}")
    intra = is_intra(g.shape[0], gop)
    d = g.astype(np.int64)
    d[1:] -= g[:-1].astype(np.int64)
    d = ((d + 32768) % 65536) - 32768  # the difference mod 2^16 as int16
    u = np.where(intra[:, None, None, None], g.astype(np.int64), ((d << 1) ^ (d >> 15)) & 0xFFFF)
    both = np.concatenate([u & 0xFF, u >> 8], axis=3).astype(np.uint8)
    return both[intra].reshape(-1, 2 * g.shape[3]), (both[~intra].reshape(-1, 2 * g.shape[3]) if not intra.all() else None)


def means_from_symbols(sym_i: np.ndarray, sym_p: Optional[np.ndarray], head: MeansHeader) -> np.ndarray:
    """The inverse of ``means_symbols`` -> uint16 [T, H, W, C]."""
    intra = is_intra(head.frames, head.gop)
    c = head.channels
    u = np.zeros((head.frames, head.height, head.width, c), np.int64)

    def join(sym):
        s = np.asarray(sym).astype(np.int64).reshape(-1, head.height, head.width, 2 * c)
        return s[..., :c] | (s[..., c:] << 8)

    u[intra] = join(sym_i)
    if not intra.all():
        u[~intra] = join(sym_p)
    out = np.zeros(u.shape, np.int64)
    for t in range(head.frames):
        out[t] = u[t] if intra[t] else (out[t - 1] + ((u[t] >> 1) ^ -(u[t] & 1))) % 65536
    return out.astype(np.uint16)


def tables_from_counts(hist: np.ndarray, bits: int = A.DEFAULT_BITS) -> np.ndarray:
    """counts [2 C, 256] -> uint32 [2 C, 256]: ``normalize_frequencies`` of the float32 relative frequencies (count / total, divided
    in float64) of every byte column."""
    h = np.asarray(hist, dtype=np.float64)
    return A.normalize_frequencies((h / h.sum(axis=1, keepdims=True)).astype(np.float32), bits)


def means_tables(symbols: np.ndarray, bits: int = A.DEFAULT_BITS) -> np.ndarray:
    """uint8 [N, 2 C] -> uint32 [2 C, 256]: ``tables_from_counts`` of the columns' histograms."""
    s = np.asarray(symbols)
    return tables_from_counts(np.stack([np.bincount(s[:, k], minlength=256) for k in range(s.shape[1])]), bits)


def table_probabilities(freq: np.ndarray, bits: int) -> np.ndarray:
    """The float32 table to hand ``ans_encode`` / ``ans_decode`` so that they code with exactly ``freq``: freq / 2^bits is exact in
    float32 and ``normalize_frequencies`` maps it back to ``freq``."""
    return (np.asarray(freq, np.float64) / (1 << bits)).astype(np.float32)


def build_means_container(head: MeansHeader, freq_i: np.ndarray, blob_i: np.ndarray, freq_p: Optional[np.ndarray] = None,
                          blob_p: Optional[np.ndarray] = None) -> np.ndarray:
    """``head.bytes_i`` / ``bytes_p`` are taken from the blobs."""
    blob_i = A._as_bytes(blob_i)
    parts = [np.frombuffer(P._pack_tables(freq_i), np.uint8), blob_i]
    if blob_p is not None:
        blob_p = A._as_bytes(blob_p)
        parts += [np.frombuffer(P._pack_tables(freq_p), np.uint8), blob_p]
    head = head._replace(bytes_i=blob_i.size, bytes_p=0 if blob_p is None else blob_p.size)
    return np.concatenate([np.frombuffer(_MEANS_HEADER.pack(MEANS_MAGIC, VERSION, *head), np.uint8)] + parts)


def parse_means_container(blob, what: str = "the buffer"):
    """-> (header, freq_I uint32 [2 C, 256], the I group's ANS container, freq_P or None, the P group's container or None);
    ValueError naming ``what`` for a foreign, short or inconsistent file.  The ANS containers are validated by their own parser."""
    buf = A._as_bytes(blob)
    if buf.size < len(MEANS_MAGIC) or buf[:len(MEANS_MAGIC)].tobytes() != MEANS_MAGIC:
        raise ValueError(f"{what} does not start with the magic of this project's lossless grid-sequence container.  The reference's "
                         "SeqHevcCompression writes x265 video payloads (<name>_l.mp4, <name>_u.mp4), which are not read here.")
    if buf.size < _MEANS_HEADER.size:
        raise ValueError(f"{what}: truncated grid-sequence header")
    version, *fields = _MEANS_HEADER.unpack(buf[:_MEANS_HEADER.size].tobytes())[1:]
    if version != VERSION:
        raise ValueError(f"{what}: grid-sequence container version {version}, this reader knows version {VERSION}")
    head = MeansHeader(*fields)
    if (not A.MIN_BITS <= head.bits <= A.MAX_BITS or head.frames < 1 or head.gop < 1 or head.height * head.width < 1
            or not 1 <= head.channels <= MEANS_MAX_CHANNELS):
        raise ValueError(f"{what}: bad grid-sequence header {tuple(head)}")
    n_i = -(-head.frames // head.gop)
    if (head.bytes_p == 0) != (n_i == head.frames):
        raise ValueError(f"{what}: a P group of {head.bytes_p} bytes against T = {head.frames} and gop = {head.gop}")

    def group(pos, size, n_frames):
        freq, pos = P._unpack_tables(buf, pos, head.bits, what, 2 * head.channels)
        if pos + size > buf.size:
            raise ValueError(f"{what}: truncated ANS container ({size} bytes expected at {pos}, the file has {buf.size})")
        bits, c, _, n = A.parse_container(buf[pos:pos + size], what)[:4]
        if (bits, c, n) != (head.bits, 2 * head.channels, n_frames * head.height * head.width):
            raise ValueError(f"{what}: an ANS container of P = {bits}, C = {c}, N = {n} against the header {tuple(head)}")
        return freq, buf[pos:pos + size], pos + size

    freq_i, blob_i, pos = group(_MEANS_HEADER.size, head.bytes_i, n_i)
    freq_p = blob_p = None
    if head.bytes_p:
        freq_p, blob_p, pos = group(pos, head.bytes_p, head.frames - n_i)
    if pos != buf.size:
        raise ValueError(f"{what}: {buf.size - pos} bytes behind the last group")
    return head, freq_i, blob_i, freq_p, blob_p


def encode_means(grid, gop: int, stream_len: int = A.DEFAULT_STREAM_LEN, bits: int = A.DEFAULT_BITS) -> np.ndarray:
    """uint16 [T, H, W, C] -> container bytes; lossless."""
    sym_i, sym_p = means_symbols(grid, gop)
    g = np.asarray(grid)
    freq_i = means_tables(sym_i, bits)
    blob_i = A.encode(sym_i, table_probabilities(freq_i, bits), stream_len, bits)
    freq_p = blob_p = None
    if sym_p is not None:
        freq_p = means_tables(sym_p, bits)
        blob_p = A.encode(sym_p, table_probabilities(freq_p, bits), stream_len, bits)
    return build_means_container(MeansHeader(bits, g.shape[0], g.shape[1], g.shape[2], g.shape[3], gop, 0, 0), freq_i, blob_i, freq_p, blob_p)


def decode_means(blob, what: str = "the buffer") -> np.ndarray:
    """container bytes -> uint16 [T, H, W, C]."""
    head, freq_i, blob_i, freq_p, blob_p = parse_means_container(blob, what)
    sym_i = A.decode(blob_i, table_probabilities(freq_i, head.bits))
    sym_p = None if blob_p is None else A.decode(blob_p, table_probabilities(freq_p, head.bits))
    return means_from_symbols(sym_i, sym_p, head)
