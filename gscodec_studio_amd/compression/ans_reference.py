"""The ``<name>.bin`` bitstream of ``EntropyCodingCompression``, written down in plain numpy.  THIS MODULE IS THE DEFINITION OF THE
FORMAT: the HIP coder (csrc/ans.hip behind ``ans.py``) must produce the same bytes, and does -- the arithmetic is integer-only.

A static, table-based, byte-wise rANS coder over many independent streams:

* state ``x``: 32 bits, in [L, 2^31) between symbols, L = 2^23; probability resolution M = 2^P (P = 14 by default);
* encode symbol s (frequency f, cumulative frequency c):  ``while x >= f << (31 - P): emit x & 255; x >>= 8``, then
  ``x = (x // f << P) + x % f + c``;  decode: ``slot = x & (M - 1)``, s = the symbol whose [c, c + f) holds slot,
  ``x = f * (x >> P) + slot - c``, then ``while x < L: x = x << 8 | next byte``;
* channel c of N symbols is cut into ``n_streams = ceil(N / S)`` streams, stream k = symbols [k S, min(N, (k + 1) S)) in splat
  order.  A stream starts at x = L, is encoded LAST SYMBOL FIRST and stores its final state, so the decoder reads it forwards;
* the integer frequencies are derived by BOTH sides from the float32 probability table that travels beside the stream
  (``<name>_prob.npy``, exactly the reference's file) with ``normalize_frequencies``.

Container, little-endian::

    8 bytes   magic  b"GSANSv1\\0"
    u32 version (1), u32 P, u32 C, u32 S, u64 N
    u32 offsets[C * n_streams + 1]     into the payload; stream (c, k) is payload[offsets[c * n_streams + k] : offsets[... + 1]]
    payload                            per stream: u32 final state, then the renormalisation bytes in the order the decoder
                                       consumes them (the reverse of the order the encoder emitted them in)

Everything about one stream -- ``_streams`` / ``_pad``, the encode and the decode loop, the container behind its header -- takes the
model as a callable and serves ``gauss_ans_reference`` as well; only header, magic and model differ between the two formats.

No torch, no native library: importable anywhere."""
from __future__ import annotations

import struct
from typing import Tuple

import numpy as np

MAGIC = b"GSANSv1\x00"
VERSION = 1
STATE_LOW = 1 << 23  # L
DEFAULT_BITS = 14  # P
DEFAULT_STREAM_LEN = 1024  # S
MIN_BITS, MAX_BITS = 8, 14  # 256 symbols need 2^8 slots; the decode kernel keeps the 2^P-byte slot table in LDS
_HEADER = struct.Struct("<8sIIIIQ")

NOT_OURS = ("{what} does not start with the magic of this project's ANS container.  The ANS payloads of this implementation and "
            "of the reference's (written with the `constriction` package) are not interchangeable; every other file of the "
            "directory (PNG grids, shN.npz, mask.bin, *_prob.npy, meta.json) is.")


def normalize_frequencies(prob: np.ndarray, bits: int = DEFAULT_BITS) -> np.ndarray:
    """float32 probabilities [C, 256] -> integer frequencies uint32 [C, 256] that sum to 2^bits per channel: ``floor(p * 2^bits)``
    in float64, at least 1 wherever p > 0, 0 elsewhere; the difference to 2^bits is then added to, or taken from, the currently
    largest entry (never below 1; the lowest index on ties).  Encoder and decoder both call this on the stored table."""
    if not MIN_BITS <= bits <= MAX_BITS:
        raise ValueError(f"probability resolution of {bits} bits, supported: {MIN_BITS}..{MAX_BITS}")
    p = np.asarray(prob, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 256:
        raise ValueError(f"the probability table must be [C, 256], got {p.shape}")
    if not np.all(np.isfinite(p)) or np.any(p < 0) or np.any(p.max(axis=1) <= 0):
        raise ValueError("the probability table needs finite, non-negative rows with at least one positive entry")
    total = 1 << bits
    freq = np.floor(p.astype(np.float64) * total).astype(np.int64)
    freq[(p > 0) & (freq < 1)] = 1
    for row in freq:
        diff = total - int(row.sum())
        while diff != 0:
            i = int(row.argmax())  # the first of equal maxima
            step = diff if diff > 0 else -min(-diff, int(row[i]) - 1)
            if step == 0:
                raise ValueError("the probability table cannot be normalised")  # unreachable for 256 symbols and bits >= 8
            row[i] += step
            diff -= step
    return freq.astype(np.uint32)


def cumulative(freq: np.ndarray) -> np.ndarray:
    """Exclusive prefix sums of the frequencies along the symbol axis."""
    return (np.cumsum(freq, axis=1, dtype=np.uint64) - freq).astype(np.uint32)


def slot_bytes(stream_len: int, bits: int) -> int:
    """Worst-case renormalisation bytes of one stream, with slack: ceil(S P / 8) + 8."""
    return (stream_len * bits + 7) // 8 + 8


def _container(head: bytes, offsets: np.ndarray, payload: np.ndarray) -> np.ndarray:
    """What both containers are behind their own header: the u32 offset table, then the payload."""
    if int(offsets[-1]) >= 1 << 32:
        raise ValueError("ANS payload of 4 GiB or more: the container's offsets are 32-bit")
    return np.concatenate([np.frombuffer(head, np.uint8), np.asarray(offsets).astype("<u4").view(np.uint8),
                           np.asarray(payload, np.uint8)])


def _as_bytes(blob) -> np.ndarray:
    return np.frombuffer(bytes(blob), np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob).view(np.uint8).ravel()


def _split_container(buf: np.ndarray, head_size: int, n_total: int, what: str) -> Tuple[np.ndarray, np.ndarray]:
    """The part of a container behind its (validated) header -> (offsets int64 [n_total + 1], payload uint8); ValueError for
    offsets that decrease, point outside the file or leave a stream fewer than its 4 state bytes."""
    table_end = head_size + 4 * (n_total + 1)
    if buf.size < table_end:
        raise ValueError(f"{what}: truncated ANS offset table ({n_total + 1} entries expected)")
    offsets = buf[head_size:table_end].view("<u4").astype(np.int64)
    payload = buf[table_end:]
    if offsets[0] != 0 or np.any(np.diff(offsets) < 4):
        raise ValueError(f"{what}: ANS stream offsets must start at 0 and leave every stream at least its 4 state bytes")
    if offsets[-1] > payload.size:
        raise ValueError(f"{what}: ANS stream offsets point past the end of the file ({int(offsets[-1])} > {payload.size} payload bytes)")
    return offsets, payload


def build_container(bits: int, n_channels: int, stream_len: int, n: int, offsets: np.ndarray, payload: np.ndarray) -> np.ndarray:
    """Header + offset table + payload -> the file's bytes (uint8 array)."""
    return _container(_HEADER.pack(MAGIC, VERSION, bits, n_channels, stream_len, n), offsets, payload)


def parse_container(blob, what: str = "the buffer") -> Tuple[int, int, int, int, np.ndarray, np.ndarray]:
    """Validate a container and split it: (P, C, S, N, offsets int64 [C * n_streams + 1], payload uint8).  Raises ValueError for
    anything a decoder must not be started on: a foreign or short file, an unknown version, offsets that decrease, point outside
    the file or leave a stream fewer than its 4 state bytes."""
    buf = _as_bytes(blob)
    if buf.size < len(MAGIC) or buf[:len(MAGIC)].tobytes() != MAGIC:
        raise ValueError(NOT_OURS.format(what=what))
    if buf.size < _HEADER.size:
        raise ValueError(f"{what}: truncated ANS header")
    _, version, bits, n_channels, stream_len, n = _HEADER.unpack(buf[:_HEADER.size].tobytes())
    if version != VERSION:
        raise ValueError(f"{what}: ANS container version {version}, this reader knows version {VERSION}")
    if not MIN_BITS <= bits <= MAX_BITS or n_channels < 1 or stream_len < 1 or n < 1:
        raise ValueError(f"{what}: bad ANS header (P = {bits}, C = {n_channels}, S = {stream_len}, N = {n})")
    return (bits, n_channels, stream_len, n) + _split_container(buf, _HEADER.size, n_channels * (-(-n // stream_len)), what)


def _streams(n: int, n_channels: int, stream_len: int) -> Tuple[np.ndarray, np.ndarray]:
    """One row per stream, channel after channel: (its length, its channel), both [C * n_streams]."""
    n_streams = -(-n // stream_len)
    lens = np.tile(np.minimum(stream_len, n - np.arange(n_streams, dtype=np.int64) * stream_len), n_channels)
    return lens, np.repeat(np.arange(n_channels), n_streams)


def _pad(a: np.ndarray, stream_len: int) -> np.ndarray:
    """[N, C] -> [C * n_streams, S]: the rows of ``_streams``, zero-padded behind N."""
    n, c = a.shape
    p = np.zeros((c, -(-n // stream_len) * stream_len), a.dtype)
    p[:, :n] = a.T
    return p.reshape(-1, stream_len)


def _encode_streams(n: int, n_channels: int, stream_len: int, bits: int, slot: int, model) -> Tuple[np.ndarray, np.ndarray]:
    """THE ENCODER of both routes.  All streams (rows) advance together, last symbol first; ``model(j)`` gives the frequency and
    the cumulative frequency of symbol j of every row at resolution 2^bits (what it gives for a row that has no symbol j is not
    used).  Each row fills a private slot of ``slot`` bytes from the back.  -> (offsets int64 [rows + 1], payload uint8)."""
    lens = _streams(n, n_channels, stream_len)[0]
    rows = np.arange(lens.size)
    buf = np.zeros((rows.size, slot), np.uint8)
    pos = np.full(rows.size, slot, np.int64)
    x = np.full(rows.size, STATE_LOW, np.uint64)
    for j in range(int(lens.max()) - 1, -1, -1):  # no row has a symbol behind the longest one's
        act = j < lens
        f, cum = model(j)
        f = np.where(act, f, 1).astype(np.uint64)
        while True:
            m = act & (x >= (f << np.uint64(31 - bits)))
            if not m.any():
                break
            if np.any(pos[m] == 0):
                raise RuntimeError("slot full: a stream outgrew its worst-case bound")  # unreachable (the slot_bytes derivations)
            pos[m] -= 1
            buf[rows[m], pos[m]] = (x[m] & np.uint64(0xFF)).astype(np.uint8)
            x[m] >>= np.uint64(8)
        x = np.where(act, ((x // f) << np.uint64(bits)) + x % f + np.asarray(cum).astype(np.uint64), x)
    offsets = np.concatenate([[0], np.cumsum(4 + (slot - pos))]).astype(np.int64)
    payload = np.empty(int(offsets[-1]), np.uint8)
    states = x.astype("<u4").view(np.uint8).reshape(-1, 4)
    for i in rows:
        payload[offsets[i]:offsets[i] + 4] = states[i]
        payload[offsets[i] + 4:offsets[i + 1]] = buf[i, pos[i]:]
    return offsets, payload


def _decode_streams(offsets: np.ndarray, payload: np.ndarray, n: int, n_channels: int, stream_len: int, bits: int, lookup) -> np.ndarray:
    """THE DECODER of both routes -> symbols uint8 [N, C].  ``lookup(j, slot)`` names, for symbol j of every row, the symbol
    whose [cum, cum + f) holds ``slot`` (int64), with f and cum.  Reads are bounded to each stream's byte range; a byte beyond it
    is 0 (a damaged stream gives wrong symbols, nothing else)."""
    lens = _streams(n, n_channels, stream_len)[0]
    data = np.concatenate([payload, np.zeros(1, np.uint8)])  # index payload.size = the substituted 0
    rd, end = offsets[:-1].copy(), offsets[1:]

    def next_byte(mask):
        got = data[np.where(mask & (rd < end), rd, payload.size)].astype(np.uint64)
        rd[mask] += 1
        return got

    everyone = np.ones(rd.size, bool)
    x = np.zeros(rd.size, np.uint64)
    for b in range(4):
        x |= next_byte(everyone) << np.uint64(8 * b)
    out = np.zeros((rd.size, stream_len), np.uint8)
    for j in range(int(lens.max())):
        act = j < lens
        slot = (x & np.uint64((1 << bits) - 1)).astype(np.int64)
        s, f, cum = lookup(j, slot)
        out[act, j] = s[act]
        x = np.where(act, (np.asarray(f).astype(np.uint64) * (x >> np.uint64(bits)) + (slot - cum).astype(np.uint64))
                     & np.uint64(0xFFFFFFFF), x)
        for _ in range(2):  # a valid stream needs at most two bytes per symbol
            m = act & (x < STATE_LOW)
            x = np.where(m, (x << np.uint64(8)) | next_byte(m), x)
    return np.ascontiguousarray(out.reshape(n_channels, -1)[:, :n].T)


def encode(symbols: np.ndarray, prob: np.ndarray, stream_len: int = DEFAULT_STREAM_LEN, bits: int = DEFAULT_BITS) -> np.ndarray:
    """symbols uint8 [N, C], prob float32 [C, 256] -> container bytes."""
    sym = np.asarray(symbols)
    if sym.dtype != np.uint8 or sym.ndim != 2 or sym.shape[0] < 1 or stream_len < 1:
        raise ValueError("symbols must be a non-empty uint8 [N, C] array and stream_len positive")
    n, n_channels = sym.shape
    freq = normalize_frequencies(prob, bits)
    if freq.shape[0] != n_channels:
        raise ValueError(f"{n_channels} channels of symbols, {freq.shape[0]} rows of probabilities")
    if np.any(freq[np.arange(n_channels)[None, :], sym] == 0):
        raise ValueError("a symbol occurs whose probability is 0")
    cum = cumulative(freq)
    ch, padded = _streams(n, n_channels, stream_len)[1], _pad(sym, stream_len)
    offsets, payload = _encode_streams(n, n_channels, stream_len, bits, slot_bytes(stream_len, bits),
                                       lambda j: (freq[ch, padded[:, j]], cum[ch, padded[:, j]]))
    return build_container(bits, n_channels, stream_len, n, offsets, payload)


def decode(blob, prob: np.ndarray) -> np.ndarray:
    """container bytes, prob float32 [C, 256] -> symbols uint8 [N, C].  Reads are bounded to each stream's byte range; a byte
    beyond it is 0 (a damaged stream gives wrong symbols, nothing else)."""
    bits, n_channels, stream_len, n, offsets, payload = parse_container(blob)
    freq = normalize_frequencies(prob, bits)
    if freq.shape[0] != n_channels:
        raise ValueError(f"the container has {n_channels} channels, the probability table {freq.shape[0]}")
    cum = cumulative(freq)
    symbol_of = np.stack([np.repeat(np.arange(256, dtype=np.uint8), row) for row in freq])  # [C, 2^P]
    ch = _streams(n, n_channels, stream_len)[1]

    def lookup(j, slot):
        s = symbol_of[ch, slot]
        return s, freq[ch, s], cum[ch, s]

    return _decode_streams(offsets, payload, n, n_channels, stream_len, bits, lookup)
