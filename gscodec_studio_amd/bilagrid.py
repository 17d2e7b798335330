"""The trainers' bilateral-grid colour correction on HIP (``csrc/bilagrid.hip``): the counterpart of the reference's
``examples/lib_bilagrid.py`` for its per-step part (``--use_bilateral_grid``).

* ``BilateralGrid(num, grid_X=16, grid_Y=16, grid_W=8)`` -- the module with the reference's attributes (``grids`` parameter
  ``(num, 12, L, H, W)``, ``grid_width``, ``grid_height``, ``grid_guidance``, the ``rgb2gray_weight`` buffer, ``tv_loss()``),
  identity initialisation, and a ``state_dict`` interchangeable with the reference's.  ``forward(grid_xy, rgb, idx)`` returns the
  sliced ``(..., 3, 4)`` matrices for 2-D to 5-D inputs.
* ``slice(bil_grids, xy, rgb, grid_idx, affine_mats=True)`` -- ``{"rgb", "rgb_affine_mats"}`` for 2-D, 3-D and 4-D inputs with the
  reference's shapes, from one kernel: guidance, trilinear interpolation (``align_corners=True``, ``padding_mode="border"``) and
  the 3x4 affine product per point.  The grid of batch entry ``b`` is ``grid_idx[b, 0, ..., 0]``, read by the kernel: no
  ``torch.unique``, no host synchronisation; this is the reference's result in both of its branches.
* ``slice_image(bil_grids, colors, image_ids)`` -- the trainer's case: a ``[C, H, W, 3]`` image (a strided view such as
  ``renders[..., 0:3]`` is read in place) at its own pixel centres, with no coordinate tensor at all.
* ``total_variation_loss(x)`` -- the reference's function for a 5-D float32 GPU tensor, one pass, summed in double.
* ``color_affine_transform(affine_mats, rgb)`` -- plain torch.

Extensions over the reference, which fails on both for more than one batch entry: ``grid_idx`` may be a 1-D tensor of length B,
and ``xy`` may have a leading dimension of 1 that is broadcast over the batch (the trainer's ``[1, H, W, 2]``).

Gradients flow to ``grids`` and ``rgb``; ``xy`` gets none (an ``xy`` that requires one is refused).  ``rgb_affine_mats`` is
returned detached.  The grid gradient is summed per workgroup on chip and added to memory once per workgroup with float atomics,
so its last bits can differ from run to run; every other result is bit-identical from run to run.  Grid indices outside
``[0, num)`` are the caller's error: the kernels clamp them, they never read outside ``grids``.  Nothing here synchronises with
the host.  Inputs the kernels do not cover raise ``ValueError``; there is no CPU path.

Out of scope: ``BilateralGridCP4D`` and ``slice4d``.  ``color_correct`` (evaluation-time least squares) is in
``gscodec_studio_amd.color_correct``.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _wrapper as W

__all__ = ["BilateralGrid", "slice", "slice_image", "total_variation_loss", "color_affine_transform"]

_MAX_ELEMENTS = 2 ** 31 - 1


def color_affine_transform(affine_mats: Tensor, rgb: Tensor) -> Tensor:
    """Applies ``(..., 3, 4)`` colour affine transformations to ``(..., 3)`` colours."""
    return torch.matmul(affine_mats[..., :3], rgb.unsqueeze(-1)).squeeze(-1) + affine_mats[..., 3]


def _check_float(fn: str, t, name: str) -> None:
    if not isinstance(t, Tensor):
        raise ValueError(f"{fn}: {name} must be a tensor (got {type(t).__name__})")
    if t.dtype != torch.float32:
        raise ValueError(f"{fn}: {name} must be float32 (got {t.dtype})")


def _check_devices(fn: str, **tensors) -> None:
    """Last of the checks, so that a wrong dtype or rank is named as such whatever the device."""
    first = None
    for name, t in tensors.items():
        if not t.is_cuda:
            raise ValueError(f"{fn}: {name} must be on a GPU (got device {t.device}); there is no CPU path")
        if first is not None and t.device != first[1].device:
            raise ValueError(f"{fn}: {first[0]} and {name} are on different devices ({first[1].device}, {t.device})")
        first = first or (name, t)


def _check_grids(fn: str, grids) -> None:
    _check_float(fn, grids, "grids")
    if grids.dim() != 5 or grids.shape[1] != 12 or grids.numel() == 0:
        raise ValueError(f"{fn}: grids must be a non-empty 5-D (N, 12, L, H, W) tensor (got shape {tuple(grids.shape)})")


def _as4(t: Tensor) -> Tensor:
    """A 2-D, 3-D or 4-D (B, ..., c) tensor as a (B, D1, D2, c) view."""
    if t.dim() == 2:
        return t[:, None, None, :]
    if t.dim() == 3:
        return t[:, None, :, :]
    return t


class _Slice(torch.autograd.Function):
    """(rgb_out or None, matrices or None) of the logical [B, D1, D2] points; gradients for grids and rgb."""

    @staticmethod
    def forward(ctx, grids: Tensor, rgb4: Tensor, xy4: Optional[Tensor], xy_strides, idx: Optional[Tensor], idx_stride: int,
                want_rgb: bool, want_affine: bool):
        g = grids.contiguous()
        shape = tuple(rgb4.shape[:3])
        out_rgb, out_aff = W.bilagrid_slice_fwd(g, shape, xy4, xy_strides, rgb4, rgb4.stride(), idx, idx_stride, want_rgb, want_affine)
        ctx.save_for_backward(g, rgb4, xy4, idx)
        ctx.geo = (shape, xy_strides, idx_stride)
        return out_rgb, out_aff

    @staticmethod
    def backward(ctx, v_rgb_out, v_aff):
        g, rgb4, xy4, idx = ctx.saved_tensors
        shape, xy_strides, idx_stride = ctx.geo
        need_g, need_rgb = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (v_rgb_out is None and v_aff is None) or not (need_g or need_rgb):
            return (None,) * 8
        v_rgb_out = v_rgb_out.contiguous() if v_rgb_out is not None else None
        v_aff = v_aff.contiguous() if v_aff is not None else None
        v_grids, v_rgb = W.bilagrid_slice_bwd(g, shape, xy4, xy_strides, rgb4, rgb4.stride(), idx, idx_stride, v_rgb_out, v_aff,
                                              want_grids=need_g, want_rgb=need_rgb)
        return v_grids, v_rgb, None, None, None, None, None, None


def _run(fn: str, grids: Tensor, rgb4: Tensor, xy4: Optional[Tensor], idx: Optional[Tensor], idx_stride: int, want_rgb: bool,
         want_affine: bool) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    if rgb4.numel() == 0:
        raise ValueError(f"{fn}: empty input {tuple(rgb4.shape)}")
    if rgb4.numel() // 3 > _MAX_ELEMENTS:
        raise ValueError(f"{fn}: {tuple(rgb4.shape)} has more than 2^31 - 1 points")
    xy_strides = None
    if xy4 is not None:
        s = xy4.stride()
        xy_strides = (0 if xy4.shape[0] == 1 else s[0], s[1], s[2], s[3])
    return _Slice.apply(grids, rgb4, xy4, xy_strides, idx, idx_stride, want_rgb, want_affine)


def _check_points(fn: str, xy, rgb, dims) -> None:
    _check_float(fn, rgb, "rgb")
    _check_float(fn, xy, "xy")
    for t, name, c in ((xy, "xy", 2), (rgb, "rgb", 3)):
        if t.dim() not in dims:
            raise ValueError(f"{fn}: {name} must be {', '.join(f'{d}-D' for d in dims)} (got {t.dim()}-D, shape {tuple(t.shape)})")
        if t.shape[-1] != c:
            raise ValueError(f"{fn}: the last dimension of {name} must be {c} (got shape {tuple(t.shape)})")
    if xy.requires_grad:
        raise ValueError(f"{fn}: xy requires a gradient, but the slice has none for the coordinates (detach it)")
    if xy.dim() != rgb.dim() or xy.shape[1:-1] != rgb.shape[1:-1] or xy.shape[0] not in (1, rgb.shape[0]):
        raise ValueError(f"{fn}: xy {tuple(xy.shape)} does not match rgb {tuple(rgb.shape)} (same leading dimensions, or a leading 1)")


def _check_idx(fn: str, grid_idx, rgb: Tensor) -> Tuple[Tensor, int]:
    if not isinstance(grid_idx, Tensor) or grid_idx.dtype.is_floating_point or grid_idx.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError(f"{fn}: grid_idx must be an integer tensor (got {getattr(grid_idx, 'dtype', type(grid_idx).__name__)})")
    ok = grid_idx.dim() >= 1 and grid_idx.shape[0] == rgb.shape[0] and (grid_idx.dim() == 1 or grid_idx.dim() == rgb.dim())
    if not ok:
        raise ValueError(f"{fn}: grid_idx must be (B,) or (B, ..., 1) with rgb's rank and B = {rgb.shape[0]} (got shape {tuple(grid_idx.shape)})")
    if grid_idx.numel() == 0:
        raise ValueError(f"{fn}: empty grid_idx {tuple(grid_idx.shape)}")
    if grid_idx.dtype != torch.int64:
        grid_idx = grid_idx.to(torch.int64)
    return grid_idx, int(grid_idx.stride(0))  # entry b: grid_idx[b, 0, ..., 0]


def slice(bil_grids: "BilateralGrid", xy: Tensor, rgb: Tensor, grid_idx: Tensor, affine_mats: bool = True) -> Dict[str, Tensor]:  # noqa: A001
    """Slices the bilateral grids at ``xy`` (``(..., 2)`` in [0, 1]) and the gray-scale guidance of ``rgb`` (``(..., 3)``) and applies
    the sliced affine transformations: ``{"rgb": (..., 3), "rgb_affine_mats": (..., 3, 4)}`` for 2-D, 3-D and 4-D inputs.  Batch
    entry ``b`` uses grid ``grid_idx[b, 0, ..., 0]`` (clamped to the grids there are).  ``rgb_affine_mats`` is detached;
    ``affine_mats=False`` omits it."""
    grids = bil_grids.grids
    _check_grids("slice", grids)
    _check_points("slice", xy, rgb, (2, 3, 4))
    idx, idx_stride = _check_idx("slice", grid_idx, rgb)
    _check_devices("slice", rgb=rgb, xy=xy, grid_idx=idx, grids=grids)
    out_rgb, out_aff = _run("slice", grids, _as4(rgb), _as4(xy), idx, idx_stride, True, bool(affine_mats))
    out = {"rgb": out_rgb.reshape(rgb.shape)}
    if affine_mats:
        out["rgb_affine_mats"] = out_aff.detach().reshape(*rgb.shape[:-1], 3, 4)
    return out


def slice_image(bil_grids: "BilateralGrid", colors: Tensor, image_ids: Tensor) -> Tensor:
    """The trainer's colour correction: ``colors`` ``[C, H, W, 3]`` (any strides) sliced at its own pixel centres
    ``((j + 0.5) / W, (i + 0.5) / H)`` with grid ``image_ids[c]`` per image; returns the corrected ``[C, H, W, 3]``."""
    grids = bil_grids.grids
    _check_grids("slice_image", grids)
    _check_float("slice_image", colors, "colors")
    if colors.dim() != 4 or colors.shape[-1] != 3:
        raise ValueError(f"slice_image: colors must be 4-D [C, H, W, 3] (got {colors.dim()}-D, shape {tuple(colors.shape)})")
    if not isinstance(image_ids, Tensor) or image_ids.numel() != colors.shape[0]:
        raise ValueError(f"slice_image: image_ids must hold one index per image ({colors.shape[0]})")
    idx, idx_stride = _check_idx("slice_image", image_ids.reshape(-1), colors)
    _check_devices("slice_image", colors=colors, image_ids=idx, grids=grids)
    out_rgb, _ = _run("slice_image", grids, colors, None, idx, idx_stride, True, False)
    return out_rgb


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor):
        xc = x.contiguous()
        ctx.save_for_backward(xc)
        return W.bilagrid_tv_fwd(xc)

    @staticmethod
    def backward(ctx, grad):
        (xc,) = ctx.saved_tensors
        return W.bilagrid_tv_bwd(xc, grad.to(torch.float32).contiguous())


def total_variation_loss(x: Tensor) -> Tensor:
    """Total variation of a 5-D ``(B, C, L, H, W)`` float32 GPU tensor, as the reference's ``total_variation_loss``: the sum over the
    three spatial axes of the mean squared forward difference, divided by B.  A 0-d device tensor."""
    _check_float("total_variation_loss", x, "x")
    if x.dim() != 5:
        raise ValueError(f"total_variation_loss: x must be 5-D (B, C, L, H, W) (got {x.dim()}-D, shape {tuple(x.shape)})")
    if x.numel() == 0 or x.numel() > _MAX_ELEMENTS:
        raise ValueError(f"total_variation_loss: {tuple(x.shape)} must have between 1 and 2^31 - 1 elements")
    _check_devices("total_variation_loss", x=x)
    return _TotalVariation.apply(x)


class BilateralGrid(nn.Module):
    """``num`` 3-D bilateral grids of 3x4 colour affine transformations, initialised to the identity."""

    def __init__(self, num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8):
        super().__init__()
        self.grid_width = grid_X
        self.grid_height = grid_Y
        self.grid_guidance = grid_W
        eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=torch.float32)
        grid = eye.view(1, 12, 1, 1, 1).expand(num, 12, grid_W, grid_Y, grid_X)
        self.grids = nn.Parameter(grid.contiguous())  # (N, 12, L, H, W)
        self.register_buffer("rgb2gray_weight", torch.tensor([[0.299, 0.587, 0.114]], dtype=torch.float32))

    def rgb2gray(self, rgb: Tensor) -> Tensor:
        """RGB to the gray-scale guidance in [-1, 1] (plain torch; the kernels evaluate the same expression)."""
        return (rgb @ self.rgb2gray_weight.T) * 2.0 - 1.0

    def tv_loss(self) -> Tensor:
        return total_variation_loss(self.grids)

    def forward(self, grid_xy: Tensor, rgb: Tensor, idx: Optional[Tensor] = None) -> Tensor:
        """The sliced ``(..., 3, 4)`` matrices.  2-D, 3-D and 4-D inputs: entry ``b`` uses grid ``idx[b]`` (``idx`` of shape (B,));
        5-D inputs ``(N, m, h, w, .)``: entry ``n`` uses grid ``n`` and ``idx`` is unused, as in ``F.grid_sample``."""
        _check_grids("BilateralGrid.forward", self.grids)
        _check_points("BilateralGrid.forward", grid_xy, rgb, (2, 3, 4, 5))
        if rgb.dim() == 5:
            if rgb.shape[0] != self.grids.shape[0]:
                raise ValueError(f"BilateralGrid.forward: 5-D inputs need one entry per grid ({self.grids.shape[0]}), got {rgb.shape[0]}")
            n, m, h, w = rgb.shape[:4]
            rgb4, xy4 = rgb.reshape(n, m * h, w, 3), grid_xy.reshape(grid_xy.shape[0], m * h, w, 2)
            index, stride = None, 0
            _check_devices("BilateralGrid.forward", rgb=rgb, grid_xy=grid_xy, grids=self.grids)
        else:
            if idx is None:
                raise ValueError("BilateralGrid.forward: idx is required for 2-D, 3-D and 4-D inputs")
            index, stride = _check_idx("BilateralGrid.forward", idx.reshape(-1) if isinstance(idx, Tensor) else idx, rgb)
            _check_devices("BilateralGrid.forward", rgb=rgb, grid_xy=grid_xy, idx=index, grids=self.grids)
            rgb4, xy4 = _as4(rgb), _as4(grid_xy)
        _, aff = _run("BilateralGrid.forward", self.grids, rgb4, xy4, index, stride, False, True)
        return aff.reshape(*rgb.shape[:-1], 3, 4)
