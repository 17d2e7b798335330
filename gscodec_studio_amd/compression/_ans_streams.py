"""What the GPU coders (``ans.py``: a table per channel; ``gauss_ans.py``: a Gaussian per symbol; ``plane_codec.py``: a table per
scan diagonal of a transform-coded plane, its flat symbols as ``[N, 1]``) do around their kernels, once:
the check of the symbol tensor, the encoder's tail (private slots -> lengths -> scan -> one read-back -> dense payload) and the
decoder's head (limits, uploads, output).  A route brings its model, its encode / decode launch and its slot size; the stream layer
under the kernels is csrc/ans_stream_dev.h."""
from __future__ import annotations

from typing import Callable, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _backend as B

MAX_STREAM_LEN = 1 << 24


def _stream(t: Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def check_symbols(symbols: Tensor, max_channels: int, who: str, stream_len: int = 1) -> Tensor:
    """-> the contiguous symbols; ``who`` names the route in the refusal."""
    if not symbols.is_cuda:
        raise RuntimeError(f"the {who} runs on the GPU: the symbols must be a device tensor (no CPU fallback)")
    if symbols.dtype != torch.uint8 or symbols.dim() != 2 or not 1 <= symbols.shape[0] < 1 << 31 or not 1 <= symbols.shape[1] <= max_channels:
        raise ValueError(f"symbols must be a non-empty uint8 [N, C] tensor with C <= {max_channels}, got {symbols.dtype} {tuple(symbols.shape)}")
    if not 1 <= stream_len <= MAX_STREAM_LEN:
        raise ValueError(f"stream_len = {stream_len}")
    return symbols.contiguous()


def encode_streams(symbols: Tensor, stream_len: int, slot: int, launch: Callable[..., None], entry: str,
                   legend: str) -> Tuple[np.ndarray, np.ndarray]:
    """The encoder behind the model: ``launch(scratch, lengths, states, status, stream)`` runs the route's kernel ``entry``, one
    lane per stream, each into its slot of ``slot`` bytes (the route's ``*_slot_bytes`` query); then the scan of the lengths, the
    one read-back (the payload's size and the status word, ``legend`` naming its bits) and the pack.  -> (offsets int64
    [C n_streams + 1], payload uint8), both numpy: what the route's ``build_container`` takes."""
    n, c = symbols.shape
    dev = symbols.device
    n_total = c * (-(-n // stream_len))
    scratch = torch.empty(n_total * slot, dtype=torch.uint8, device=dev)
    lengths = torch.empty(n_total, dtype=torch.int32, device=dev)
    states = torch.empty(n_total, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        launch(scratch, lengths, states, status, _stream(symbols))
        offsets = torch.zeros(n_total + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lengths.long() + 4, dim=0, out=offsets[1:])
        total, bad = int(offsets[-1]), int(status)  # the one read-back: the payload's size
        if bad:
            raise RuntimeError(f"{entry} reported status {bad} ({legend})")
        payload = torch.empty(total, dtype=torch.uint8, device=dev)
        B.call("gs_ans_pack_slots", n_total, slot, B.ptr(scratch), B.ptr(lengths), B.ptr(states), B.ptr(offsets), B.ptr(payload),
               total, _stream(symbols))
    return offsets.cpu().numpy(), payload.cpu().numpy()


def decode_buffers(n: int, c: int, stream_len: int, max_channels: int, offsets: np.ndarray, payload: np.ndarray, dev: torch.device,
                   what: str) -> Tuple[Tensor, Tensor, Tensor]:
    """The decoder before the model: a parsed container's limits against the kernels', then (offsets, payload, the output uint8
    [N, C]) on ``dev``."""
    if c > max_channels or n >= 1 << 31 or stream_len > MAX_STREAM_LEN:
        raise ValueError(f"{what}: C = {c}, N = {n}, S = {stream_len} is outside what the kernels take")
    return (torch.from_numpy(offsets).to(dev), torch.from_numpy(np.array(payload, copy=True)).to(dev),
            torch.empty((n, c), dtype=torch.uint8, device=dev))
