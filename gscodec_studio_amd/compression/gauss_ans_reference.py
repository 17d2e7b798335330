"""The ``<name>.bin`` bitstream of the hash-grid Gaussian route of ``EntropyCodingCompression``, written down in plain numpy.
THIS MODULE IS THE DEFINITION OF THE FORMAT: the HIP coder (csrc/gauss_ans.hip behind ``gauss_ans.py``) must produce the same
bytes, and does -- everything after ``regress_params`` is integer arithmetic, and ``regress_params`` states its float32 order.

The streams are ``ans_reference``'s, whose encode and decode loops and container tail run here too: a 32-bit state in [L, 2^31), L = 2^23, byte-wise renormalisation, channel c of the N
symbols cut into ``ceil(N / S)`` streams of S consecutive symbols, each stream encoded LAST SYMBOL FIRST from x = L and stored as
its final state followed by the bytes in the order the decoder consumes them.  What differs is the model: the probability
resolution is M = 2^P with P = 16, and EVERY SYMBOL HAS ITS OWN FREQUENCIES, given by two small integers --

* ``mu_q``, the mean on a grid of F = 8 steps per symbol, 0..2040;
* ``k``, a scale level 0..K-1 (K = 64): sigma_k = 2^((k - 22) / 5) symbol widths, about 0.047 .. 294.

and one integer table ``G[k][t] = rint((2^16 - 256) Phi(t / (8 sigma_k)))``, t = -2036..2036 (uint16 [64, 4073], float64 and
``math.erf``)::

    cum(0) = 0,  cum(256) = 2^16,  cum(s) = G[k][clamp(8 s - 4 - mu_q)] + s  for s = 1..255,   f(s) = cum(s + 1) - cum(s)

G is non-decreasing in t and at most 2^16 - 256, so the ``+ s`` gives every symbol a frequency of at least 1 whatever (mu_q, k)
says: correctness never depends on the model, only the size does.  The decoder finds s by an 8-step binary search on cum.

``quantize_params`` maps the normalised float32 mean and standard deviation to (mu_q, k); ``regress_params`` is the whole way from
the hash-grid features of a splat to them, in a stated float32 order, so that a splat's model depends on nothing but its features,
the stored weights and mins / maxs.

Container, little-endian::

    8 bytes   magic  b"GSGANSv1"
    u32 version (1), u32 P (16), u32 C, u32 S, u64 N, u32 K (64), u32 F (8), u32 CRC32 of G's bytes followed by the thresholds'
    u32 offsets[C * n_streams + 1]     into the payload, as in ans_reference
    payload                            per stream: u32 final state, then the renormalisation bytes

The CRC is recomputed by every reader: a host whose ``erf`` or ``pow`` differs in one table entry refuses the file instead of
decoding noise.

Worst-case bytes of one stream (``slot_bytes``).  Encoding one symbol of frequency f takes the state x to x' = x >> 8b (b bytes
emitted) and then to x'' = (x' // f << P) + x' % f + cum < (q + 1) 2^P with q = x' // f.  q >= 2^7: without a shift x' >= 2^23 and
f < 2^16; after a shift the previous value was >= f << 15, so x' >= f << 7.  Hence q + 1 <= q (1 + 2^-7) and
x'' < x 2^(-8b) (2^P / f) (1 + 2^-7): the floor of the division loses less than one part in 2^7 (it was 2^9 at P = 14).  Over a
stream of S symbols that starts at 2^23 and ends at >= 2^23:  8 B < S (16 + log2(1 + 2^-7)) = S (16 + 0.011227), that is
B < 2 S + 0.0014034 S <= 2 S + S / 512, and B being an integer, B <= 2 S + S // 512.  ``slot_bytes`` adds 8 bytes of slack.  (The
same two facts give the decoder's bound of two bytes per symbol: x'' >= 2^7 2^16 = 2^23 needs q >= 2^7, and x < 2^31 is below
f << 15 after two shifts.)

No torch, no native library: importable anywhere."""
from __future__ import annotations

import math
import struct
import zlib
from functools import lru_cache
from typing import Tuple

import numpy as np

from . import ans_reference as S  # the stream layer: one state machine, one layout, one container tail

MAGIC = b"GSGANSv1"
VERSION = 1
STATE_LOW = S.STATE_LOW  # L
BITS = 16  # P
DEFAULT_STREAM_LEN = 1024  # S
N_LEVELS = 64  # K
MEAN_STEPS = 8  # F
MU_Q_MAX = 255 * MEAN_STEPS  # 2040
T_MAX = MU_Q_MAX - MEAN_STEPS // 2  # 2036: |8 s - 4 - mu_q| for s in 1..255
TABLE_WIDTH = 2 * T_MAX + 1  # 4073
G_TOP = (1 << BITS) - 256
HIDDEN_PER_CHANNEL = 5  # the regressor is Linear(48, 5 C), ReLU, Linear(5 C, 2 C)
N_FEATURES = 48
SCALE_MIN = np.float32(1e-9)
_HEADER = struct.Struct("<8sIIIIQIII")

NOT_OURS = ("{what} does not start with the magic of this project's Gaussian ANS container.  The ANS payloads of this "
            "implementation and of the reference's (written with the `constriction` package) are not interchangeable, nor are "
            "this project's factorized and Gaussian containers; every other file of the directory is.")


def level_sigmas() -> np.ndarray:
    """sigma_k = 2^((k - 22) / 5), float64 [K]."""
    return np.array([2.0 ** ((k - 22) / 5.0) for k in range(N_LEVELS)], np.float64)


@lru_cache(maxsize=1)
def _tables() -> Tuple[np.ndarray, np.ndarray, int]:
    sig = level_sigmas()
    g = np.empty((N_LEVELS, TABLE_WIDTH), np.uint16)
    for k in range(N_LEVELS):
        d = 8.0 * sig[k] * math.sqrt(2.0)
        phi = np.array([0.5 * (1.0 + math.erf(t / d)) for t in range(-T_MAX, T_MAX + 1)], np.float64)
        g[k] = np.rint(G_TOP * phi).astype(np.uint16)
    tau = np.array([2.0 ** ((j - 22.5) / 5.0) for j in range(1, N_LEVELS)], np.float64).astype(np.float32)
    crc = zlib.crc32(tau.astype("<f4").tobytes(), zlib.crc32(g.astype("<u2").tobytes())) & 0xFFFFFFFF
    g.setflags(write=False)
    tau.setflags(write=False)
    return g, tau, crc


def gaussian_table() -> np.ndarray:
    """G, uint16 [K, 4073] (read-only; column t + 2036)."""
    return _tables()[0]


def level_thresholds() -> np.ndarray:
    """tau_j, j = 1..K-1: the geometric midpoints 2^((j - 22.5) / 5) of the levels, float32 [K - 1] (read-only)."""
    return _tables()[1]


def table_crc() -> int:
    """CRC32 of G's little-endian bytes followed by the thresholds' -- the header field."""
    return _tables()[2]


def quantize_params(mu_norm, sigma_norm) -> Tuple[np.ndarray, np.ndarray]:
    """float32 mean / standard deviation in symbol units -> (mu_q int16, k uint8) of the same shape.  mu_q = 0 where
    ``not (mu_norm > 0)`` (NaN included), 2040 where ``mu_norm >= 255``, else ``rint(mu_norm * 8)``; k = the number of
    thresholds ``tau_j <= sigma_norm`` in float32 (NaN: 0)."""
    mu = np.asarray(mu_norm, np.float32)
    sg = np.asarray(sigma_norm, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        pos = mu > 0
        top = mu >= np.float32(255)
        mid = np.rint(np.where(pos & ~top, mu, np.float32(0)) * np.float32(MEAN_STEPS))
        mu_q = np.where(top, MU_Q_MAX, np.where(pos, mid, 0)).astype(np.int16)
        k = np.zeros(sg.shape, np.uint8)
        for tau in level_thresholds():
            k += (tau <= sg).astype(np.uint8)
    return mu_q, k


def regress_params(features, w1, b1, w2, b2, mins, maxs, return_float: bool = False):
    """features float32 [N, 48] (the hash-grid encoder's output), W1 [5C, 48], b1 [5C], W2 [2C, 5C], b2 [2C], mins / maxs [C]
    -> (mu_q int16 [N, C], k uint8 [N, C]).  Everything is float32 and every operation is rounded on its own (no fma):

        h_j = b1_j;  for i = 0..47:  h_j = h_j + x_i * W1[j, i];   h_j = h_j if h_j > 0 else 0
        o_m = b2_m;  for j = 0..5C-1: o_m = o_m + h_j * W2[m, j]
        miu_c = o_c;  sigma_c = 1e-9 if o_{C+c} < 1e-9 else o_{C+c}
        mu_norm = (miu - mins) / (maxs - mins) * 255;   sigma_norm = sigma / (maxs - mins) * 255

    then ``quantize_params``.  ``return_float`` appends the float32 miu and sigma."""
    x = np.ascontiguousarray(features, np.float32)
    w1, b1, w2, b2 = (np.asarray(a, np.float32) for a in (w1, b1, w2, b2))
    mins, maxs = np.asarray(mins, np.float32).reshape(-1), np.asarray(maxs, np.float32).reshape(-1)
    c = mins.size
    hid = HIDDEN_PER_CHANNEL * c
    if x.ndim != 2 or x.shape[1] != N_FEATURES or w1.shape != (hid, N_FEATURES) or b1.shape != (hid,) or w2.shape != (2 * c, hid) \
            or b2.shape != (2 * c,) or maxs.size != c or c < 1:
        raise ValueError(f"regress_params: features {x.shape}, W1 {w1.shape}, b1 {b1.shape}, W2 {w2.shape}, b2 {b2.shape} for "
                         f"{c} channels; expected [N, {N_FEATURES}], [{hid}, {N_FEATURES}], [{hid}], [{2 * c}, {hid}], [{2 * c}]")
    with np.errstate(all="ignore"):
        h = np.broadcast_to(b1, (x.shape[0], hid)).copy()
        for i in range(N_FEATURES):
            h = h + x[:, i:i + 1] * w1[None, :, i]
        h = np.where(h > 0, h, np.float32(0))
        o = np.broadcast_to(b2, (x.shape[0], 2 * c)).copy()
        for j in range(hid):
            o = o + h[:, j:j + 1] * w2[None, :, j]
        miu = o[:, :c]
        sigma = np.where(o[:, c:] < SCALE_MIN, SCALE_MIN, o[:, c:])
        d = maxs - mins
        mu_norm = (miu - mins) / d * np.float32(255)
        sigma_norm = sigma / d * np.float32(255)
    assert mu_norm.dtype == np.float32 and sigma_norm.dtype == np.float32
    mu_q, k = quantize_params(mu_norm, sigma_norm)
    if return_float:
        return mu_q, k, np.ascontiguousarray(miu), np.ascontiguousarray(sigma)
    return mu_q, k


def slot_bytes(stream_len: int) -> int:
    """Worst-case renormalisation bytes of one stream at P = 16, with 8 bytes of slack: 2 S + S // 512 + 8 (module docstring)."""
    return 2 * stream_len + stream_len // 512 + 8


def cum_at(mu_q: np.ndarray, k: np.ndarray, s: np.ndarray) -> np.ndarray:
    """cum(s) for s in 0..256, elementwise (int64)."""
    s = np.asarray(s, np.int64)
    t = np.clip(MEAN_STEPS * s - MEAN_STEPS // 2 - np.asarray(mu_q, np.int64), -T_MAX, T_MAX) + T_MAX
    mid = gaussian_table()[np.asarray(k, np.int64), t].astype(np.int64) + s
    return np.where(s <= 0, 0, np.where(s >= 256, 1 << BITS, mid))


def frequencies(mu_q, k) -> np.ndarray:
    """All 256 frequencies of every (mu_q, k) pair: int64 [..., 256], each row sums to 2^16 (tests, size estimates)."""
    mu_q, k = np.asarray(mu_q)[..., None], np.asarray(k)[..., None]
    s = np.arange(257)
    return np.diff(cum_at(mu_q, k, s), axis=-1)


def build_container(n_channels: int, stream_len: int, n: int, offsets: np.ndarray, payload: np.ndarray) -> np.ndarray:
    """Header + offset table + payload -> the file's bytes (uint8 array)."""
    head = _HEADER.pack(MAGIC, VERSION, BITS, n_channels, stream_len, n, N_LEVELS, MEAN_STEPS, table_crc())
    return S._container(head, offsets, payload)


def parse_container(blob, what: str = "the buffer") -> Tuple[int, int, int, np.ndarray, np.ndarray]:
    """Validate a container and split it: (C, S, N, offsets int64 [C * n_streams + 1], payload uint8).  Raises ValueError for
    anything a decoder must not be started on: a foreign or short file, an unknown version, P / K / F other than 16 / 64 / 8, a
    table CRC that is not this host's, offsets that decrease, point outside the file or leave a stream fewer than its 4 state
    bytes."""
    buf = S._as_bytes(blob)
    if buf.size < len(MAGIC) or buf[:len(MAGIC)].tobytes() != MAGIC:
        raise ValueError(NOT_OURS.format(what=what))
    if buf.size < _HEADER.size:
        raise ValueError(f"{what}: truncated Gaussian ANS header")
    _, version, bits, n_channels, stream_len, n, levels, steps, crc = _HEADER.unpack(buf[:_HEADER.size].tobytes())
    if version != VERSION:
        raise ValueError(f"{what}: Gaussian ANS container version {version}, this reader knows version {VERSION}")
    if (bits, levels, steps) != (BITS, N_LEVELS, MEAN_STEPS) or n_channels < 1 or stream_len < 1 or n < 1:
        raise ValueError(f"{what}: bad Gaussian ANS header (P = {bits}, K = {levels}, F = {steps}, C = {n_channels}, "
                         f"S = {stream_len}, N = {n}); this reader knows P = {BITS}, K = {N_LEVELS}, F = {MEAN_STEPS}")
    if crc != table_crc():
        raise ValueError(f"{what}: the file was written against frequency tables with CRC32 {crc:08x}, this host builds "
                         f"{table_crc():08x} (its erf or pow rounds differently): decoding would give noise")
    return (n_channels, stream_len, n) + S._split_container(buf, _HEADER.size, n_channels * (-(-n // stream_len)), what)


def check_model(mu_q, k, n: int, n_channels: int) -> Tuple[np.ndarray, np.ndarray]:
    """The model arrays of one call, [N, C]: integer, mu_q in 0..2040, k in 0..63 -- ValueError otherwise."""
    mu_q, k = np.asarray(mu_q), np.asarray(k)
    if mu_q.shape != (n, n_channels) or k.shape != (n, n_channels):
        raise ValueError(f"the model must be [N, C] = [{n}, {n_channels}], got mu_q {mu_q.shape} and k {k.shape}")
    if mu_q.dtype.kind not in "iu" or k.dtype.kind not in "iu":
        raise ValueError("mu_q and k must be integer arrays")
    if mu_q.min() < 0 or mu_q.max() > MU_Q_MAX or k.min() < 0 or k.max() >= N_LEVELS:
        raise ValueError(f"model out of range: mu_q must lie in 0..{MU_Q_MAX} and k in 0..{N_LEVELS - 1}")
    return mu_q.astype(np.int64), k.astype(np.int64)


def encode(symbols: np.ndarray, mu_q, k, stream_len: int = DEFAULT_STREAM_LEN) -> np.ndarray:
    """symbols uint8 [N, C], mu_q / k integer [N, C] -> container bytes."""
    sym = np.asarray(symbols)
    if sym.dtype != np.uint8 or sym.ndim != 2 or sym.shape[0] < 1 or sym.shape[1] < 1 or stream_len < 1:
        raise ValueError("symbols must be a non-empty uint8 [N, C] array and stream_len positive")
    n, n_channels = sym.shape
    mu_q, k = check_model(mu_q, k, n, n_channels)
    p_sym, p_mu, p_k = (S._pad(a, stream_len) for a in (sym.astype(np.int64), mu_q, k))

    def model(j):
        lo = cum_at(p_mu[:, j], p_k[:, j], p_sym[:, j])
        return cum_at(p_mu[:, j], p_k[:, j], p_sym[:, j] + 1) - lo, lo

    offsets, payload = S._encode_streams(n, n_channels, stream_len, BITS, slot_bytes(stream_len), model)
    return build_container(n_channels, stream_len, n, offsets, payload)


def decode(blob, mu_q, k) -> np.ndarray:
    """container bytes, mu_q / k integer [N, C] -> symbols uint8 [N, C].  Reads are bounded to each stream's byte range; a byte
    beyond it is 0 (a damaged stream gives wrong symbols, nothing else)."""
    n_channels, stream_len, n, offsets, payload = parse_container(blob)
    mu_q, k = check_model(mu_q, k, n, n_channels)
    p_mu, p_k = S._pad(mu_q, stream_len), S._pad(k, stream_len)

    def lookup(j, slot):
        s = np.zeros(slot.size, np.int64)
        step = 128
        while step >= 1:  # the last s with cum(s) <= slot: 8 steps, always
            s = np.where(cum_at(p_mu[:, j], p_k[:, j], s + step) <= slot, s + step, s)
            step >>= 1
        lo = cum_at(p_mu[:, j], p_k[:, j], s)
        return s, cum_at(p_mu[:, j], p_k[:, j], s + 1) - lo, lo

    return S._decode_streams(offsets, payload, n, n_channels, stream_len, BITS, lookup)


def pack_signs(signed: np.ndarray) -> np.ndarray:
    """+-1 (as ``STE_binary`` leaves a table) -> one bit per entry, LSB first: the bytes of the reference's ``to_bin_stream``
    (``(v + 1) // 2`` is the bit)."""
    v = np.asarray(signed).reshape(-1)
    return np.packbits(((v + 1) // 2).astype(np.int32) != 0, bitorder="little")


def unpack_signs(data, length: int) -> np.ndarray:
    """The reference's ``from_bin_stream``: ``length`` entries of +-1 float32; a bit behind the end of the data is 0 (-1)."""
    raw = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel()
    need = (length + 7) // 8
    if raw.size < need:
        raw = np.concatenate([raw, np.zeros(need - raw.size, np.uint8)])
    bits = np.unpackbits(raw[:need], bitorder="little")[:length]
    return (bits.astype(np.float32) * 2 - 1).astype(np.float32)
