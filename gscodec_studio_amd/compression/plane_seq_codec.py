"""The transform-coded plane sequences of ``SeqHevcCompression`` on the GPU: 8-bit frames ``[T, H, W, ch]``, HEVC's quantisation
parameter and a GOP length  <->  the ``<name>.bin`` container of ``plane_seq_codec_reference`` (which defines the format; the
sequence kernels of csrc/plane_codec.hip compute the same levels, frames and bytes).

    plane_seq_encode(planes, qp, gop, stream_len=4096) -> container bytes       (closed loop, symbols, histograms, rANS, pack)
    plane_seq_decode(blob, device)                      -> uint8 [T, H, W, ch]   (container validated on the host before any launch)
    seq_transform_levels(planes, qp, gop, recon=False)  -> int16 [T, ch, n_blocks, 64] (and the decoder's frames)   gs_plane_seq_fwd alone
    seq_inverse_transform(levels, qp, gop, H, W)        -> uint8 [T, H, W, ch]                                      gs_plane_seq_inv alone

ONE launch runs the whole closed loop of a direction: a lane owns an 8 x 8 block through all T frames with the reconstruction in
registers.  Between the kernels sit the whole-array steps of ``plane_codec.py``, once per group of frames (I frames, P frames): the
DC differences (I group only), the fold, the escapes, the ``bincount`` and the host-side tables; the coding itself is the plane
codec's ``gs_plane_ans_encode`` / ``gs_plane_ans_decode``, unchanged -- the context of flat symbol i is still ``CTX[i % 64]``."""
from __future__ import annotations

from typing import Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import _backend as B
from . import plane_seq_codec_reference as R
from ._ans_streams import _stream
from .plane_codec import _check_qp, decode_levels, encode_levels

P = R.P


def _check_planes(planes: Tensor, qp, gop) -> Tensor:
    """-> the contiguous uint8 [T, H, W, ch] device sequence; ValueError for a wrong dtype, rank, channel count, qp or gop,
    RuntimeError for a host tensor."""
    if not isinstance(planes, Tensor):
        raise ValueError(f"the sequence must be a uint8 device tensor, got {type(planes).__name__}")
    if planes.dtype != torch.uint8 or planes.dim() not in (3, 4):
        raise ValueError(f"the sequence must be a uint8 [T, H, W] or [T, H, W, ch] tensor, got {planes.dtype} {tuple(planes.shape)}")
    if planes.dim() == 3:
        planes = planes[..., None]
    t, h, w, ch = planes.shape
    if not 1 <= ch <= P.MAX_CHANNELS or t < 1 or h < 1 or w < 1 or 64 * ch * P.n_blocks(h, w) * t >= 1 << 31:
        raise ValueError(f"the sequence must be non-empty with 1..{P.MAX_CHANNELS} channels and fewer than 2^31 coefficients, got {tuple(planes.shape)}")
    _check_qp(qp)
    R.check_gop(gop)
    if not planes.is_cuda:
        raise RuntimeError("the plane-sequence codec runs on the GPU: the sequence must be a device tensor (no CPU fallback); "
                           "plane_seq_codec_reference.encode is the numpy form")
    return planes.contiguous()


@torch.no_grad()
def seq_transform_levels(planes: Tensor, qp: int, gop: int, recon: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """uint8 device frames -> int16 levels [T, ch, n_blocks, 64] in scan order, equal to ``plane_seq_codec_reference.forward_levels``;
    with ``recon`` also the frames a decoder will see, uint8 [T, H, W, ch], equal to ``reconstruct``."""
    planes = _check_planes(planes, qp, gop)
    t, h, w, ch = planes.shape
    levels = torch.empty((t, ch, P.n_blocks(h, w), 64), dtype=torch.int16, device=planes.device)
    out = torch.empty_like(planes) if recon else None
    with torch.cuda.device(planes.device):
        B.call("gs_plane_seq_fwd", t, int(gop), h, w, ch, int(qp), B.ptr(planes), B.ptr(levels), B.ptr(out), _stream(planes))
    return (levels, out) if recon else levels


@torch.no_grad()
def seq_inverse_transform(levels: Tensor, qp: int, gop: int, height: int, width: int) -> Tensor:
    """int16 device levels [T, ch, n_blocks, 64] (any values) -> uint8 [T, H, W, ch], equal to
    ``plane_seq_codec_reference.inverse_levels``."""
    if not isinstance(levels, Tensor) or not levels.is_cuda:
        raise RuntimeError("the plane-sequence codec runs on the GPU: the levels must be a device tensor (no CPU fallback)")
    _check_qp(qp)
    R.check_gop(gop)
    if (levels.dtype != torch.int16 or levels.dim() != 4 or height < 1 or width < 1 or levels.shape[0] < 1
            or not 1 <= levels.shape[1] <= P.MAX_CHANNELS or tuple(levels.shape[2:]) != (P.n_blocks(height, width), 64)
            or levels.numel() >= 1 << 31):
        raise ValueError(f"levels {levels.dtype} {tuple(levels.shape)} do not belong to a sequence of {height} x {width} planes of "
                         f"1..{P.MAX_CHANNELS} channels")
    levels = levels.contiguous()
    t, ch = levels.shape[:2]
    planes = torch.empty((t, height, width, ch), dtype=torch.uint8, device=levels.device)
    with torch.cuda.device(levels.device):
        B.call("gs_plane_seq_inv", t, int(gop), height, width, ch, int(qp), B.ptr(levels), B.ptr(planes), _stream(levels))
    return planes


@torch.no_grad()
def plane_seq_encode(planes: Tensor, qp: int, gop: int, stream_len: int = R.DEFAULT_STREAM_LEN, bits: int = R.DEFAULT_BITS,
                     return_recon: bool = False):
    """Encode uint8 device frames [T, H, W] or [T, H, W, ch] (ch = 1..4) at ``qp`` (0..51) with an I frame every ``gop`` frames ->
    the container as a numpy uint8 array, byte-identical to ``plane_seq_codec_reference.encode``; with ``return_recon`` also the
    decoder's frames (device uint8 [T, H, W, ch]), which the closed loop has anyway.  Refused before any launch: a host tensor
    (RuntimeError), a wrong dtype, rank, channel count, qp, gop, stream length or resolution (ValueError)."""
    planes = _check_planes(planes, qp, gop)
    if isinstance(stream_len, bool) or not isinstance(stream_len, (int, np.integer)) or not 1 <= stream_len <= P.MAX_STREAM_LEN:
        raise ValueError(f"stream_len = {stream_len!r}")
    if not R.A.MIN_BITS <= bits <= R.A.MAX_BITS:
        raise ValueError(f"probability resolution of {bits} bits, supported: {R.A.MIN_BITS}..{R.A.MAX_BITS}")
    t, h, w, ch = planes.shape
    got = seq_transform_levels(planes, qp, gop, recon=return_recon)
    levels, recon = got if return_recon else (got, None)
    intra = R.is_intra(t, int(gop))
    d_intra, d_inter = torch.from_numpy(np.flatnonzero(intra)).to(planes.device), torch.from_numpy(np.flatnonzero(~intra)).to(planes.device)
    group_i = R.Group(*encode_levels(levels[d_intra].reshape(-1, levels.shape[2], 64), True, int(stream_len), bits))
    group_p = None if intra.all() else R.Group(*encode_levels(levels[d_inter].reshape(-1, 1, 64), False, int(stream_len), bits))
    head = R.Header(bits, int(stream_len), int(qp), h, w, ch, t, int(gop), group_i.escapes.size, 0 if group_p is None else group_p.escapes.size)
    blob = R.build_container(head, group_i, group_p)
    return (blob, recon) if return_recon else blob


@torch.no_grad()
def plane_seq_decode(blob, device="cuda", what: str = "the buffer") -> Tensor:
    """Decode a container (bytes or uint8 array) -> uint8 [T, H, W, ch] on ``device``, equal to ``plane_seq_codec_reference.decode``.
    The container is validated on the host first (ValueError naming ``what``; nothing is launched on a file ``parse_container``
    refuses); the kernels also bound their own reads and clamp the levels."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("the plane-sequence codec runs on the GPU (no CPU fallback); plane_seq_codec_reference.decode is the numpy form")
    head, group_i, group_p = R.parse_container(blob, what)
    n_blocks = P.n_blocks(head.height, head.width)
    if 64 * head.channels * n_blocks * head.frames >= 1 << 31:  # the parser bounds each group; the kernels take the sequence whole
        raise ValueError(f"{what}: {head.frames} frames of {head.height} x {head.width} x {head.channels} are 2^31 coefficients or more, "
                         "outside what the kernels take")
    intra = R.is_intra(head.frames, head.gop)
    n_i = int(intra.sum())
    per_frame = 64 * head.channels * n_blocks
    levels = torch.empty((head.frames, head.channels, n_blocks, 64), dtype=torch.int16, device=dev)
    d_intra, d_inter = torch.from_numpy(np.flatnonzero(intra)).to(dev), torch.from_numpy(np.flatnonzero(~intra)).to(dev)
    levels[d_intra] = decode_levels(*group_i, per_frame * n_i, n_i * head.channels, True, head.stream_len, head.bits, dev,
                                    what).reshape(n_i, head.channels, n_blocks, 64)
    if group_p is not None:
        n_p = head.frames - n_i
        levels[d_inter] = decode_levels(*group_p, per_frame * n_p, 1, False, head.stream_len, head.bits, dev,
                                        what).reshape(n_p, head.channels, n_blocks, 64)
    return seq_inverse_transform(levels, head.qp, head.gop, head.height, head.width)
