"""The evaluation-time colour matching of the reference's ``examples/lib_bilagrid.py`` on HIP (``csrc/color_correct.hip``):
``color_correct(img, ref)`` warps the colours of a render onto those of its ground truth before ``cc_psnr`` and the metrics
beside it are taken (``simple_trainer.py:1266``).

* ``color_correct(img, ref, num_iters=5, eps=0.5 / 255, per_image=False)`` -- the reference's name, argument order and defaults.
  ``img`` and ``ref`` are float32 GPU tensors of one shape ``[..., n]`` with ``n`` in 1..3; the result is a new, detached float32
  tensor of that shape.  ``per_image=True`` is an extension: every entry of dimension 0 is fitted on its own, in the same launches.

The arithmetic is the reference's, statement for statement.  The features of a pixel are ``x_c * x_c'`` for ``c' >= c``, then
``x``, then 1 (3, 6 or 10 columns); the rows of channel ``c`` are those whose input value, current value and ``ref`` value of
that channel are all unclipped (``eps <= z <= 1 - eps``); each iteration solves the masked least-squares problem per channel and
replaces the image by ``clip(A w, 0, 1)``, stored as float32.  What differs is how it is evaluated:

* one pass over the pixels per iteration forms the features in float64 and accumulates the normal equations (``A^T A``, ``A^T b``)
  in float64 registers, one record per workgroup, no atomics; one small kernel sums the records in a fixed order and solves each
  system through a symmetric eigen-decomposition (Jacobi sweeps on at most 10 x 10), cutting the eigenvalues at ``EIG_RCOND`` times
  the largest.  A full-rank system gets the least-squares solution; a rank-deficient one (an empty mask, a constant channel, fewer
  unmasked rows than columns) gets the minimum-norm solution, and no input can produce a non-finite warp (a system whose sums are
  not finite -- a NaN in another channel of an unmasked row -- gets the zero warp where the reference's assertion fires).  The
  reference passes ``rcond=-1`` to ``torch.linalg.lstsq``, which makes LAPACK treat every system as full rank: its result for a
  rank-deficient system depends on the driver and is not reproduced.
* applying the warp of iteration ``k`` and accumulating for iteration ``k + 1`` are one pass, so a call makes
  ``2 * num_iters + 1`` launches; nothing synchronises with the host or is read back (the reference's ``assert torch.all(...)``
  is a host wait), and results are bit-identical from run to run.
* the thresholds are compared in float32 (``float32(eps)``, ``float32(1 - eps)``), as torch compares a float32 tensor with a
  Python number.

``img`` may be a channel slice of a wider contiguous tensor (``renders[..., 0:3]`` of a 4-channel render): it is read in place
through its constant pixel stride.  Anything else non-contiguous is copied once.  Inputs the kernels do not cover raise
``ValueError`` before any launch; there is no CPU path and no backward.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _backend as B

__all__ = ["color_correct", "EIG_RCOND", "DEFAULT_WORKGROUPS"]

# eigenvalues of A^T A at or below EIG_RCOND times the largest one are treated as zero: the kernels' constant
# (gs_color_correct_rcond_log2; tests/test_color_correct_cpu.py holds the two together)
EIG_RCOND = 2.0 ** -40
# most workgroups per (group, channel) of a pass: 3 channels of one image then fill the 256 compute units three times over
DEFAULT_WORKGROUPS = 256
_PIXELS_PER_WORKGROUP = 1024  # below DEFAULT_WORKGROUPS of them, a lane of the 256 walks four pixels
_MAX_PIXELS = 2 ** 31 - 1


def num_columns(n: int) -> int:
    """Columns of the quadratic expansion of an ``n``-channel pixel: 3, 6, 10."""
    return n * (n + 1) // 2 + n + 1


def _pixel_stride(t: Tensor) -> Optional[int]:
    """The constant element stride between consecutive pixels of ``t`` ``[..., n]`` (``n`` for a contiguous tensor, the width of
    the parent for a channel slice), or None where there is none."""
    n = t.shape[-1]
    if t.stride(-1) != 1 and n > 1:
        return None
    dims = [(s, st) for s, st in zip(t.shape[:-1], t.stride()[:-1]) if s != 1]
    if not dims:
        return n
    step = dims[-1][1]
    if step < n:
        return None
    for (_, outer), (size, inner) in zip(dims[:-1], dims[1:]):
        if outer != inner * size:
            return None
    return step


def _check(img, ref, num_iters, eps, workgroups) -> None:
    for t, name in ((img, "img"), (ref, "ref")):
        if not isinstance(t, Tensor):
            raise ValueError(f"color_correct: {name} must be a tensor (got {type(t).__name__})")
        if t.dtype != torch.float32:
            raise ValueError(f"color_correct: {name} must be float32 (got {t.dtype})")
    if img.dim() < 1 or img.shape[-1] not in (1, 2, 3):
        raise ValueError(f"color_correct: img must be [..., n] with n = 1, 2 or 3 channels (got shape {tuple(img.shape)})")
    if img.shape != ref.shape:
        raise ValueError(f"color_correct: img {tuple(img.shape)} and ref {tuple(ref.shape)} must have the same shape")
    if img.numel() == 0:
        raise ValueError(f"color_correct: empty input {tuple(img.shape)}")
    if img.numel() // img.shape[-1] > _MAX_PIXELS:
        raise ValueError(f"color_correct: {tuple(img.shape)} has more than 2^31 - 1 pixels")
    if int(num_iters) != num_iters or num_iters < 0:
        raise ValueError(f"color_correct: num_iters must be a non-negative integer (got {num_iters!r})")
    if not 0.0 <= float(eps) < 0.5:
        raise ValueError(f"color_correct: eps must be in [0, 0.5) (got {eps!r})")
    if workgroups is not None and not 1 <= int(workgroups) <= 65535:
        raise ValueError(f"color_correct: workgroups must be between 1 and 65535 (got {workgroups!r})")
    for t, name in ((img, "img"), (ref, "ref")):  # last, so that a wrong dtype or shape is named as such whatever the device
        if not t.is_cuda:
            raise ValueError(f"color_correct: {name} must be on a GPU (got device {t.device}); there is no CPU path")
    if img.device != ref.device:
        raise ValueError(f"color_correct: img and ref are on different devices ({img.device}, {ref.device})")


def color_correct(img: Tensor, ref: Tensor, num_iters: int = 5, eps: float = 0.5 / 255, per_image: bool = False, *,
                  workgroups: Optional[int] = None) -> Tensor:
    """Warps the colours of ``img`` onto those of ``ref`` (both ``[..., n]`` in [0, 1]) by ``num_iters`` rounds of masked least
    squares on the quadratic expansion of the pixels; returns the corrected image, float32, detached.  ``per_image=True`` fits
    every ``img[i]`` to ``ref[i]`` on its own.  ``workgroups`` overrides the number of workgroups (and partial records) per
    system of a pass; the result does not depend on the run, but its last bits depend on this number."""
    _check(img, ref, num_iters, eps, workgroups)
    img, ref = img.detach(), ref.detach()
    n = int(img.shape[-1])
    if num_iters == 0:
        return img.clone(memory_format=torch.contiguous_format)
    stride = _pixel_stride(img)
    if stride is None:
        img, stride = img.contiguous(), n
    ref = ref.contiguous()
    groups = int(img.shape[0]) if per_image and img.dim() >= 2 else 1
    pixels = img.numel() // n // groups
    blocks = int(workgroups) if workgroups is not None else max(1, min(DEFAULT_WORKGROUPS, -(-pixels // _PIXELS_PER_WORKGROUP)))
    lo, hi = float(eps), 1.0 - float(eps)  # rounded to float32 on their way into the call
    dev = img.device
    record = int(B.query("gs_color_correct_record_doubles", n))
    partials = torch.empty((groups, n, blocks, record), dtype=torch.float64, device=dev)
    warp = torch.empty((groups, num_columns(n), n), dtype=torch.float64, device=dev)
    # pass i reads image i - 1 and writes image i: two buffers in turn, the last write into the one that is returned
    bufs = [torch.empty(img.shape, dtype=torch.float32, device=dev), torch.empty(img.shape, dtype=torch.float32, device=dev) if num_iters > 1 else None]
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        cur, cur_stride = img, stride
        for i in range(num_iters + 1):
            out = bufs[(num_iters - i) % 2] if i > 0 else None
            B.call("gs_color_correct_pass", cur.data_ptr(), cur_stride, img.data_ptr(), stride, ref.data_ptr(), groups, pixels, n, lo, hi,
                   warp.data_ptr() if i > 0 else None, B.ptr(out), partials.data_ptr() if i < num_iters else None, blocks, st)
            if i < num_iters:
                B.call("gs_color_correct_solve", partials.data_ptr(), groups, n, blocks, warp.data_ptr(), st)
            if i > 0:
                cur, cur_stride = out, n
    return bufs[0]
