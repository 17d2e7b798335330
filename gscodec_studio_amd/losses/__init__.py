"""The trainers' photometric loss on HIP (``csrc/loss.hip``): a drop-in for the ``fused_ssim`` package and the fused L1 + SSIM loss.

* ``fused_ssim(img1, img2, padding="same", train=True)`` -- the ``fused_ssim`` package's function: the 3DGS SSIM (11-tap Gaussian
  window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2) of two float32 ``[B, C, H, W]`` GPU tensors of any strides, averaged
  over every position (``"same"``) or over ``[5:-5, 5:-5]`` (``"valid"``).  Only ``img1`` gets a gradient.  ``train=False``
  returns the same value without keeping anything for a backward.
* ``photometric_loss(colors, pixels, ssim_lambda=0.2, padding="valid")`` -- the trainers' whole loss
  ``(1 - lambda) * mean|colors - pixels| + lambda * (1 - ssim)`` on their own ``[B, H, W, C]`` tensors (no permute), one forward
  pass and one backward pass; returns ``(loss, l1, ssim)`` with ``l1`` and ``ssim`` detached 0-d device tensors for logging.

A trainer switches with one import line: ``from gscodec_studio_amd.losses import fused_ssim``.  Neither function synchronises with
the host; inputs the kernels do not cover raise ``ValueError``.
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from .. import _wrapper as W

__all__ = ["fused_ssim", "photometric_loss"]

_MAX_ELEMENTS = 2 ** 31 - 1


def _check(fn: str, a: Tensor, b: Tensor, padding: str, hw=(2, 3), names=("img1", "img2"), layout="[B, C, H, W]") -> None:
    for t, name in zip((a, b), names):
        if not isinstance(t, Tensor):
            raise ValueError(f"{fn}: {name} must be a tensor (got {type(t).__name__})")
        if t.dtype != torch.float32:
            raise ValueError(f"{fn}: {name} must be float32 (got {t.dtype})")
        if t.dim() != 4:
            raise ValueError(f"{fn}: {name} must be 4-D {layout} (got {t.dim()}-D, shape {tuple(t.shape)})")
    if a.shape != b.shape:
        raise ValueError(f"{fn}: {names[0]} and {names[1]} must have the same shape (got {tuple(a.shape)} and {tuple(b.shape)})")
    if padding not in W.SSIM_PADDING:
        raise ValueError(f"{fn}: unknown padding {padding!r} (expected 'same' or 'valid')")
    if a.numel() > _MAX_ELEMENTS:
        raise ValueError(f"{fn}: {tuple(a.shape)} has {a.numel()} elements, more than 2^31 - 1")
    if a.numel() == 0:
        raise ValueError(f"{fn}: empty input {tuple(a.shape)}")
    h, w = a.shape[hw[0]], a.shape[hw[1]]
    if padding == "valid" and (h <= 10 or w <= 10):
        raise ValueError(f"{fn}: padding='valid' needs H > 10 and W > 10 (got H = {h}, W = {w})")
    for t, name in zip((a, b), names):
        if not t.is_cuda:
            raise ValueError(f"{fn}: {name} must be on a GPU (got device {t.device}); there is no CPU path")
    if a.device != b.device:
        raise ValueError(f"{fn}: {names[0]} and {names[1]} are on different devices ({a.device}, {b.device})")


def _grad_scalar(g: Tensor) -> Tensor:
    return g.to(torch.float32).contiguous()


class _FusedSSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1: Tensor, img2: Tensor, padding: str):
        ssim, _, _, work = W.ssim_fwd(img1, img1.stride(), img2, img2.stride(), img1.shape, padding, train=True)
        ctx.save_for_backward(img1, img2, work)
        ctx.padding = padding
        return ssim

    @staticmethod
    def backward(ctx, grad):
        img1, img2, work = ctx.saved_tensors
        dx = torch.empty_like(img1)  # img1's own strides when it is dense (a permuted NHWC view stays NHWC)
        W.ssim_bwd(img1, img1.stride(), img2, img2.stride(), img1.shape, ctx.padding, work, _grad_scalar(grad), 1.0, None, 0.0, dx,
                   dx.stride())
        return dx, None, None


def fused_ssim(img1: Tensor, img2: Tensor, padding: str = "same", train: bool = True) -> Tensor:
    """Mean 3DGS SSIM of ``img1`` against ``img2`` (float32 ``[B, C, H, W]`` on the GPU, any strides); a 0-d device tensor.
    ``padding="valid"`` averages over ``[:, :, 5:-5, 5:-5]`` only.  Gradient for ``img1`` only (``train=True``)."""
    _check("fused_ssim", img1, img2, padding)
    if train and torch.is_grad_enabled() and img1.requires_grad:
        return _FusedSSIM.apply(img1, img2, padding)
    ssim, _, _, _ = W.ssim_fwd(img1, img1.stride(), img2, img2.stride(), img1.shape, padding, train=False)
    return ssim


def _nchw(t: Tensor):
    """The logical [B, C, H, W] shape and element strides of a [B, H, W, C] tensor."""
    b, h, w, c = t.shape
    s = t.stride()
    return (b, c, h, w), (s[0], s[3], s[1], s[2])


class _PhotometricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colors: Tensor, pixels: Tensor, ssim_lambda: float, padding: str):
        shape, cs = _nchw(colors)
        _, ps = _nchw(pixels)
        ssim, l1, loss, work = W.ssim_fwd(colors, cs, pixels, ps, shape, padding, train=True, ssim_lambda=ssim_lambda, want_l1=True,
                                          want_loss=True)
        ctx.save_for_backward(colors, pixels, work)
        ctx.padding, ctx.ssim_lambda = padding, ssim_lambda
        ctx.mark_non_differentiable(l1, ssim)
        return loss, l1, ssim

    @staticmethod
    def backward(ctx, grad_loss, _grad_l1, _grad_ssim):
        colors, pixels, work = ctx.saved_tensors
        if grad_loss is None:
            return None, None, None, None
        shape, cs = _nchw(colors)
        _, ps = _nchw(pixels)
        dx = torch.empty_like(colors)
        _, ds = _nchw(dx)
        g = _grad_scalar(grad_loss)
        lam = ctx.ssim_lambda
        W.ssim_bwd(colors, cs, pixels, ps, shape, ctx.padding, work, g, -lam, g, 1.0 - lam, dx, ds)
        return dx, None, None, None


def photometric_loss(colors: Tensor, pixels: Tensor, ssim_lambda: float = 0.2, padding: str = "valid") -> Tuple[Tensor, Tensor, Tensor]:
    """The trainers' loss on their ``[B, H, W, C]`` tensors: ``(loss, l1, ssim)`` with
    ``loss = (1 - ssim_lambda) * mean|colors - pixels| + ssim_lambda * (1 - fused_ssim(colors, pixels, padding))`` (NCHW views),
    ``l1`` and ``ssim`` detached.  Gradient for ``colors`` only; the L1 gradient is 0 where colors == pixels."""
    _check("photometric_loss", colors, pixels, padding, hw=(1, 2), names=("colors", "pixels"), layout="[B, H, W, C]")
    lam = float(ssim_lambda)
    if torch.is_grad_enabled() and colors.requires_grad:
        return _PhotometricLoss.apply(colors, pixels, lam, padding)
    shape, cs = _nchw(colors)
    _, ps = _nchw(pixels)
    ssim, l1, loss, _ = W.ssim_fwd(colors, cs, pixels, ps, shape, padding, train=False, ssim_lambda=lam, want_l1=True, want_loss=True)
    return loss, l1, ssim
