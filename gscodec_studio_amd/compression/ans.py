"""The entropy coder of ``EntropyCodingCompression`` on the GPU: 8-bit symbols [N, C] <-> the ``<name>.bin`` container of
``ans_reference`` (which defines the format; the kernels of csrc/ans.hip write the same bytes).

    symbol_histogram(symbols)                 -> counts [C, 256]   (LDS histograms, one flush of atomics per workgroup)
    normalize_frequencies(prob, bits=14)      -> integer frequencies, the one host function both sides use
    ans_encode(symbols, prob, stream_len)     -> container bytes   (histogram / transpose, encode, scan, pack)
    ans_decode(blob, prob, device)            -> symbols [N, C]    (container validated on the host before any launch)

One lane owns one stream of ``stream_len`` symbols of one channel; ``stream_len`` is part of the file header."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _backend as B
from . import ans_reference as R
from ._ans_streams import _stream, check_symbols, decode_buffers, encode_streams
from .ans_reference import normalize_frequencies

MAX_CHANNELS = 16  # of one call: the histogram kernel keeps C x 256 counters in LDS


def _histogram(symbols: Tensor, channel_major: bool) -> Tuple[Tensor, Optional[Tensor]]:
    n, c = symbols.shape
    counts = torch.zeros((c, 256), dtype=torch.int32, device=symbols.device)  # uint32 on the device; N < 2^31 here
    cm = torch.empty((c, n), dtype=torch.uint8, device=symbols.device) if channel_major else None
    with torch.cuda.device(symbols.device):
        B.call("gs_ans_histogram", n, c, B.ptr(symbols), B.ptr(counts), B.ptr(cm), _stream(symbols))
    return counts, cm


@torch.no_grad()
def symbol_histogram(symbols: Tensor) -> Tensor:
    """Occurrences of every byte value per channel: uint8 [N, C] device tensor -> int32 [C, 256]."""
    return _histogram(check_symbols(symbols, MAX_CHANNELS, "ANS coder"), channel_major=False)[0]


def probabilities(counts: Tensor) -> np.ndarray:
    """The reference's ``_get_prob`` on the counts: count / total in float64, stored as float32 [C, 256]."""
    cnt = counts.cpu().numpy().astype(np.int64)
    return np.stack([(row / row.sum()).astype(np.float32) for row in cnt], axis=0)


@torch.no_grad()
def ans_encode(symbols: Tensor, prob: np.ndarray, stream_len: int = R.DEFAULT_STREAM_LEN, bits: int = R.DEFAULT_BITS) -> np.ndarray:
    """Encode device symbols uint8 [N, C] against the float32 table ``prob`` [C, 256] -> the container as a numpy uint8 array,
    byte-identical to ``ans_reference.encode``.  A symbol whose probability is 0 raises ValueError."""
    symbols = check_symbols(symbols, MAX_CHANNELS, "ANS coder", stream_len)
    n, c = symbols.shape
    freq = normalize_frequencies(prob, bits)
    if freq.shape[0] != c:
        raise ValueError(f"{c} channels of symbols, {freq.shape[0]} rows of probabilities")
    counts, cm = _histogram(symbols, channel_major=True)
    if np.any((counts.cpu().numpy() != 0) & (freq == 0)):
        raise ValueError("a symbol occurs whose probability is 0")
    d_freq = torch.from_numpy(freq.view(np.int32)).to(symbols.device)
    d_cum = torch.from_numpy(R.cumulative(freq).view(np.int32)).to(symbols.device)

    def launch(scratch, lengths, states, status, stream):
        B.call("gs_ans_encode", n, c, stream_len, bits, B.ptr(cm), B.ptr(d_freq), B.ptr(d_cum), B.ptr(scratch), scratch.numel(),
               B.ptr(lengths), B.ptr(states), B.ptr(status), stream)

    offsets, payload = encode_streams(symbols, stream_len, int(B.query("gs_ans_slot_bytes", stream_len, bits)), launch,
                                      "gs_ans_encode", "1: symbol without frequency, 2: slot too small")
    return R.build_container(bits, c, stream_len, n, offsets, payload)


@torch.no_grad()
def ans_decode(blob, prob: np.ndarray, device="cuda", what: str = "the buffer") -> Tensor:
    """Decode a container (bytes or uint8 array) against ``prob`` -> uint8 [N, C] on ``device``, the layout ``dequantize_grid``
    reads.  The container is validated on the host first (ValueError; nothing is launched on a file that is not this project's,
    or whose offsets decrease, leave the file or leave a stream fewer than 4 bytes); the kernel also bounds its own reads."""
    bits, c, stream_len, n, offsets, payload = R.parse_container(blob, what)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("the ANS coder runs on the GPU (no CPU fallback); ans_reference.decode is the numpy form")
    freq = normalize_frequencies(prob, bits)
    if freq.shape[0] != c:
        raise ValueError(f"{what}: the container has {c} channels, the probability table {freq.shape[0]}")
    d_off, d_payload, out = decode_buffers(n, c, stream_len, MAX_CHANNELS, offsets, payload, dev, what)
    d_freq = torch.from_numpy(freq.view(np.int32)).to(dev)
    d_cum = torch.from_numpy(R.cumulative(freq).view(np.int32)).to(dev)
    with torch.cuda.device(dev):
        B.call("gs_ans_decode", n, c, stream_len, bits, B.ptr(d_payload), d_payload.numel(), B.ptr(d_off), B.ptr(d_freq), B.ptr(d_cum),
               B.ptr(out), _stream(out))
    return out
