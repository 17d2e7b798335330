"""2D Gaussian splatting (surfels) on HIP (``csrc/surfel.hip``): the operators behind ``rendering.rasterization_2dgs``, with
the names, parameters, defaults and return order of the reference's ``gsplat/cuda/_wrapper.py:1260-1361, 1626-1749``.

* ``fully_fused_projection_2dgs`` -- per (camera, splat): ``radii``, ``means2d``, ``depths``, the 3x3 ray transforms
  ``K [R q_x s_x | R q_y s_y | mean_c]`` (row-major) and the camera-space normals.  Gradients go to ``means``, ``quats``,
  ``scales`` (components 0 and 1; component 2 gets zero) and to ``viewmats`` when it requires one; ``Ks`` gets none, as in
  the reference.  The semantics are the reference KERNEL's (which its torch twin only approximates): the radius is
  ``ceil(3 sqrt(max(1e-4, .)))`` and splats whose ``M_w,x^2 + M_w,y^2 - M_w,z^2`` is zero are culled with ``radii = 0``.
  Outputs of culled splats are zeros (the reference leaves them uninitialised).
* ``rasterize_to_pixels_2dgs`` -- per-tile compositing: colours, alphas, camera-space normals, the distortion map (zeros
  unless ``distloss``) and the median depth.  Gradients go to ``means2d``, ``ray_transforms``, ``colors``, ``opacities``,
  ``normals``, ``densify`` and ``backgrounds``; with ``absgrad=True`` the backward sets ``means2d.absgrad``.
* ``depth_to_normal`` -- the fused kernel pair behind ``utils.depth_to_normal``.

One deliberate difference from the reference: it writes ``v_densify = v_ray_transforms[.., 2 or 5] * depth`` from inside the
compositing backward while other workgroups are still adding into ``v_ray_transforms`` -- a race whose result depends on
scheduling.  Here ``densify.grad[c, n] = (v_ray_transforms[c, n, 0, 2], v_ray_transforms[c, n, 1, 2]) * depth[c, n]`` (depth =
``ray_transforms[c, n, 2, 2]``) is computed from the FINAL sums, after the kernel.

Not in this version, each refused with ``NotImplementedError`` before any launch: ``packed=True`` (and ``sparse_grad=True``,
which needs it), more than 4 colour channels (the depth column included) and ``tile_size != 16``.  CPU tensors are refused with
``RuntimeError``: there is no CPU path.  Nothing here synchronises with the host; gradients are accumulated with float atomics,
so their last bits can differ from run to run.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _backend as B
from ._wrapper import _device_of, _f32c, _require_gpu, _stream

__all__ = ["fully_fused_projection_2dgs", "rasterize_to_pixels_2dgs", "depth_to_normal"]

MAX_CHANNELS = 4


def check_unpacked(fn: str, packed: bool, sparse_grad: bool = False) -> None:
    if sparse_grad:
        assert packed, "sparse_grad is only supported when packed is True"
    if packed:
        raise NotImplementedError(f"{fn}: packed=True (and sparse_grad=True, which needs it) is not built on the HIP backend yet; "
                                  "use packed=False, the 2DGS trainer's default")


def check_channels(fn: str, channels: int) -> None:
    if channels < 1:
        raise ValueError(f"Unsupported number of color channels: {channels}")
    if channels > MAX_CHANNELS:
        raise NotImplementedError(f"{fn}: {channels} colour channels (the depth column included) are not built on the HIP backend "
                                  f"yet; at most {MAX_CHANNELS}")


def check_tile_size(fn: str, tile_size: int) -> None:
    if tile_size != 16:
        raise NotImplementedError(f"{fn}: tile_size={tile_size} is not built on the HIP backend yet; the 2DGS kernels use 16")


def fully_fused_projection_2dgs(
    means: Tensor,  # [N, 3]
    quats: Tensor,  # [N, 4]
    scales: Tensor,  # [N, 3]
    viewmats: Tensor,  # [C, 4, 4]
    Ks: Tensor,  # [C, 3, 3]
    width: int,
    height: int,
    eps2d: float = 0.3,
    near_plane: float = 0.01,
    far_plane: float = 1e10,
    radius_clip: float = 0.0,
    packed: bool = False,
    sparse_grad: bool = False,
) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Ray-splat intersection matrices, screen-space centres and bounding radii of 2D Gaussians.

    Returns ``(radii int32 [C, N], means2d [C, N, 2], depths [C, N], ray_transforms [C, N, 3, 3], normals [C, N, 3])``.
    ``eps2d`` is accepted and unused, as in the reference."""
    C = viewmats.size(0)
    N = means.size(0)
    assert means.size() == (N, 3), means.size()
    assert viewmats.size() == (C, 4, 4), viewmats.size()
    assert Ks.size() == (C, 3, 3), Ks.size()
    assert quats is not None, "quats is required"
    assert scales is not None, "scales is required"
    assert quats.size() == (N, 4), quats.size()
    assert scales.size() == (N, 3), scales.size()
    check_unpacked("fully_fused_projection_2dgs", packed, sparse_grad)
    _require_gpu(means, "fully_fused_projection_2dgs")
    return _FullyFusedProjection2DGS.apply(means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane, radius_clip)


class _FullyFusedProjection2DGS(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane, radius_clip):
        means, quats, scales, viewmats, Ks = _f32c(means), _f32c(quats), _f32c(scales), _f32c(viewmats), _f32c(Ks)
        for t in (quats, scales, viewmats, Ks):
            _require_gpu(t, "fully_fused_projection_2dgs")
        C, N, dev = viewmats.shape[0], means.shape[0], means.device
        radii = torch.empty((C, N), dtype=torch.int32, device=dev)
        means2d = torch.empty((C, N, 2), dtype=torch.float32, device=dev)
        depths = torch.empty((C, N), dtype=torch.float32, device=dev)
        ray_transforms = torch.empty((C, N, 3, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((C, N, 3), dtype=torch.float32, device=dev)
        with _device_of(means):
            B.call("gs_projection_2dgs_fwd", C, N, B.ptr(means), B.ptr(quats), B.ptr(scales), B.ptr(viewmats), B.ptr(Ks), width, height,
                   eps2d, near_plane, far_plane, radius_clip, B.ptr(radii), B.ptr(means2d), B.ptr(depths), B.ptr(ray_transforms),
                   B.ptr(normals), _stream(means))
        ctx.save_for_backward(means, quats, scales, viewmats, Ks, radii, ray_transforms)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        return radii, means2d, depths, ray_transforms, normals

    @staticmethod
    def backward(ctx, v_radii, v_means2d, v_depths, v_ray_transforms, v_normals):
        means, quats, scales, viewmats, Ks, radii, ray_transforms = ctx.saved_tensors
        C, N = viewmats.shape[0], means.shape[0]
        # accumulated with atomics (a splat is seen by up to C cameras; the pose sums run over all splats): zero-filled here
        v_means, v_quats, v_scales = torch.zeros_like(means), torch.zeros_like(quats), torch.zeros_like(scales)
        v_viewmats = torch.zeros_like(viewmats) if ctx.needs_input_grad[3] else None
        grads = [_f32c(v) if v is not None else None for v in (v_means2d, v_depths, v_normals, v_ray_transforms)]
        if any(g is not None for g in grads):
            with _device_of(means):
                B.call("gs_projection_2dgs_bwd", C, N, B.ptr(means), B.ptr(quats), B.ptr(scales), B.ptr(viewmats), B.ptr(Ks), B.ptr(radii),
                       B.ptr(ray_transforms), *[B.ptr(g) for g in grads], B.ptr(v_means), B.ptr(v_quats), B.ptr(v_scales),
                       B.ptr(v_viewmats), _stream(means))
        need = ctx.needs_input_grad
        return (v_means if need[0] else None, v_quats if need[1] else None, v_scales if need[2] else None, v_viewmats,
                None, None, None, None, None, None, None)


def rasterize_to_pixels_2dgs(
    means2d: Tensor,  # [C, N, 2]
    ray_transforms: Tensor,  # [C, N, 3, 3]
    colors: Tensor,  # [C, N, channels]
    opacities: Tensor,  # [C, N]
    normals: Tensor,  # [C, N, 3]
    densify: Tensor,  # [C, N, 2]
    image_width: int,
    image_height: int,
    tile_size: int,
    isect_offsets: Tensor,  # [C, tile_height, tile_width]
    flatten_ids: Tensor,  # [n_isects]
    backgrounds: Optional[Tensor] = None,  # [C, channels]
    masks: Optional[Tensor] = None,  # [C, tile_height, tile_width] bool
    packed: bool = False,
    absgrad: bool = False,
    distloss: bool = False,
) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Rasterizes 2D Gaussians to pixels.

    Returns ``(render_colors [C, H, W, channels], render_alphas [C, H, W, 1], render_normals [C, H, W, 3] (camera space),
    render_distort [C, H, W, 1], render_median [C, H, W, 1])``.  The LAST colour channel is what the distortion and the median
    depth read (the renderer appends the depth there).  ``densify`` is the dummy input whose gradient the densification
    strategy reads (``key_for_gradient="gradient_2dgs"``): see the module docstring for how it is formed."""
    check_unpacked("rasterize_to_pixels_2dgs", packed)
    check_tile_size("rasterize_to_pixels_2dgs", tile_size)
    check_channels("rasterize_to_pixels_2dgs", colors.shape[-1])
    C = isect_offsets.size(0)
    N = means2d.size(1)
    assert means2d.shape == (C, N, 2), means2d.shape
    assert ray_transforms.shape == (C, N, 3, 3), ray_transforms.shape
    assert colors.shape[:2] == (C, N), colors.shape
    assert opacities.shape == (C, N), opacities.shape
    assert normals.shape == (C, N, 3), normals.shape
    assert densify.shape == (C, N, 2), densify.shape
    if backgrounds is not None:
        assert backgrounds.shape == (C, colors.shape[-1]), backgrounds.shape
    tile_height, tile_width = isect_offsets.shape[1:3]
    assert tile_height * tile_size >= image_height, f"Assert Failed: {tile_height} * {tile_size} >= {image_height}"
    assert tile_width * tile_size >= image_width, f"Assert Failed: {tile_width} * {tile_size} >= {image_width}"
    if masks is not None:
        assert masks.shape == isect_offsets.shape and masks.dtype == torch.bool, (masks.shape, masks.dtype)
    _require_gpu(means2d, "rasterize_to_pixels_2dgs")
    return _RasterizeToPixels2DGS.apply(means2d, ray_transforms, colors, opacities, normals, densify, backgrounds, masks, image_width,
                                        image_height, tile_size, isect_offsets, flatten_ids, absgrad, distloss)


class _RasterizeToPixels2DGS(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means2d, ray_transforms, colors, opacities, normals, densify, backgrounds, masks, width, height, tile_size,
                isect_offsets, flatten_ids, absgrad, distloss):
        means2d, ray_transforms, colors, opacities, normals = (_f32c(means2d), _f32c(ray_transforms), _f32c(colors), _f32c(opacities),
                                                               _f32c(normals))
        backgrounds = _f32c(backgrounds)
        isect_offsets, flatten_ids = isect_offsets.contiguous(), flatten_ids.contiguous()
        assert isect_offsets.dtype == torch.int32 and flatten_ids.dtype == torch.int32
        masks = masks.contiguous() if masks is not None else None
        for t in (ray_transforms, colors, opacities, normals, isect_offsets, flatten_ids, backgrounds, masks):
            if t is not None:
                _require_gpu(t, "rasterize_to_pixels_2dgs")
        C, tile_height, tile_width = isect_offsets.shape
        channels, n_elems, n_isects, dev = colors.shape[-1], opacities.numel(), flatten_ids.shape[0], means2d.device
        render_colors = torch.empty((C, height, width, channels), dtype=torch.float32, device=dev)
        render_alphas = torch.empty((C, height, width, 1), dtype=torch.float32, device=dev)
        render_normals = torch.empty((C, height, width, 3), dtype=torch.float32, device=dev)
        render_distort = torch.empty((C, height, width, 1), dtype=torch.float32, device=dev)
        render_median = torch.empty((C, height, width, 1), dtype=torch.float32, device=dev)
        last_ids = torch.empty((C, height, width), dtype=torch.int32, device=dev)
        median_ids = torch.empty((C, height, width), dtype=torch.int32, device=dev)
        m8 = masks.view(torch.uint8) if masks is not None else None
        with _device_of(means2d):
            B.call("gs_rasterize_2dgs_fwd", C, n_elems // max(C, 1), n_isects, channels, B.ptr(means2d), B.ptr(ray_transforms),
                   B.ptr(colors), B.ptr(opacities), B.ptr(normals), B.ptr(backgrounds), B.ptr(m8), width, height, tile_size, tile_width,
                   tile_height, B.ptr(isect_offsets), B.ptr(flatten_ids), int(bool(distloss)), B.ptr(render_colors),
                   B.ptr(render_alphas), B.ptr(render_normals), B.ptr(render_distort), B.ptr(render_median), B.ptr(last_ids),
                   B.ptr(median_ids), _stream(means2d))
        ctx.save_for_backward(means2d, ray_transforms, colors, opacities, normals, backgrounds, masks, isect_offsets, flatten_ids,
                              render_colors, render_alphas, last_ids, median_ids)
        ctx.geo = (width, height, tile_size, bool(absgrad), bool(distloss))
        ctx.set_materialize_grads(False)
        return render_colors, render_alphas, render_normals, render_distort, render_median

    @staticmethod
    def backward(ctx, v_render_colors, v_render_alphas, v_render_normals, v_render_distort, v_render_median):
        (means2d, ray_transforms, colors, opacities, normals, backgrounds, masks, isect_offsets, flatten_ids, render_colors, render_alphas,
         last_ids, median_ids) = ctx.saved_tensors
        width, height, tile_size, absgrad, distloss = ctx.geo
        C, tile_height, tile_width = isect_offsets.shape
        channels, n_elems, n_isects, dev = colors.shape[-1], opacities.numel(), flatten_ids.shape[0], means2d.device
        v_rc, v_ra, v_rn, v_rd, v_rm = (_f32c(v) if v is not None else None
                                        for v in (v_render_colors, v_render_alphas, v_render_normals, v_render_distort, v_render_median))
        # accumulated with atomics: ONE zero-filled buffer, carved into the contiguous gradient tensors
        widths = (2, 9, channels, 1, 3) + ((2,) if absgrad else ())
        flat = torch.zeros(n_elems * sum(widths), dtype=torch.float32, device=dev)
        parts, at = [], 0
        for w in widths:
            parts.append(flat[at:at + n_elems * w])
            at += n_elems * w
        v_means2d, v_ray_transforms, v_colors = parts[0].view(means2d.shape), parts[1].view(ray_transforms.shape), parts[2].view(colors.shape)
        v_opacities, v_normals = parts[3].view(opacities.shape), parts[4].view(normals.shape)
        v_means2d_abs = parts[5].view(means2d.shape) if absgrad else None
        m8 = masks.view(torch.uint8) if masks is not None else None
        with _device_of(means2d):
            B.call("gs_rasterize_2dgs_bwd", C, n_elems // max(C, 1), n_isects, channels, B.ptr(means2d), B.ptr(ray_transforms),
                   B.ptr(colors), B.ptr(opacities), B.ptr(normals), B.ptr(backgrounds), B.ptr(m8), width, height, tile_size, tile_width,
                   tile_height, B.ptr(isect_offsets), B.ptr(flatten_ids), int(distloss), B.ptr(render_colors), B.ptr(render_alphas),
                   B.ptr(last_ids), B.ptr(median_ids), B.ptr(v_rc), B.ptr(v_ra), B.ptr(v_rn), B.ptr(v_rd), B.ptr(v_rm),
                   B.ptr(v_means2d), B.ptr(v_means2d_abs), B.ptr(v_ray_transforms), B.ptr(v_colors), B.ptr(v_opacities),
                   B.ptr(v_normals), _stream(means2d))
        if absgrad:
            means2d.absgrad = v_means2d_abs
        need = ctx.needs_input_grad
        v_densify = None
        if need[5]:
            # from the FINAL sums (the reference reads them inside the kernel while other workgroups still add: module docstring)
            v_densify = v_ray_transforms[..., 0:2, 2] * ray_transforms[..., 2, 2].unsqueeze(-1)
        v_backgrounds = None
        if backgrounds is not None and need[6] and v_rc is not None:
            v_backgrounds = (v_rc * (1.0 - render_alphas)).sum(dim=(1, 2))
        return (v_means2d if need[0] else None, v_ray_transforms if need[1] else None, v_colors if need[2] else None,
                v_opacities if need[3] else None, v_normals if need[4] else None, v_densify, v_backgrounds,
                None, None, None, None, None, None, None, None)


def depth_to_normal(depths: Tensor, camtoworlds: Tensor, Ks: Tensor, z_depth: bool = True) -> Tensor:
    """Surface normals ``[..., H, W, 3]`` (world space) of depth maps ``[..., H, W, 1]``: one fused kernel each way.  The gradient
    goes to ``depths``; ``camtoworlds`` and ``Ks`` get none."""
    assert depths.shape[-1] == 1, f"Invalid depth shape: {depths.shape}"
    assert camtoworlds.shape[-2:] == (4, 4), f"Invalid viewmats shape: {camtoworlds.shape}"
    assert Ks.shape[-2:] == (3, 3), f"Invalid Ks shape: {Ks.shape}"
    assert depths.shape[:-3] == camtoworlds.shape[:-2] == Ks.shape[:-2], \
        f"Shape mismatch! depths: {depths.shape}, viewmats: {camtoworlds.shape}, Ks: {Ks.shape}"
    _require_gpu(depths, "depth_to_normal")
    H, W = depths.shape[-3:-1]
    out = _DepthToNormal.apply(depths.reshape(-1, H, W), camtoworlds.reshape(-1, 4, 4), Ks.reshape(-1, 3, 3), bool(z_depth))
    return out.reshape(*depths.shape[:-1], 3)


class _DepthToNormal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depths, camtoworlds, Ks, z_depth):
        depths, camtoworlds, Ks = _f32c(depths), _f32c(camtoworlds.detach()), _f32c(Ks.detach())
        _require_gpu(camtoworlds, "depth_to_normal")
        _require_gpu(Ks, "depth_to_normal")
        Bn, H, W = depths.shape
        normals = torch.empty((Bn, H, W, 3), dtype=torch.float32, device=depths.device)
        with _device_of(depths):
            B.call("gs_depth_to_normal_fwd", Bn, H, W, B.ptr(depths), B.ptr(camtoworlds), B.ptr(Ks), int(z_depth), B.ptr(normals),
                   _stream(depths))
        ctx.save_for_backward(depths, camtoworlds, Ks)
        ctx.z_depth = z_depth
        return normals

    @staticmethod
    def backward(ctx, v_normals):
        depths, camtoworlds, Ks = ctx.saved_tensors
        Bn, H, W = depths.shape
        v_depths = torch.empty_like(depths)
        with _device_of(depths):
            B.call("gs_depth_to_normal_bwd", Bn, H, W, B.ptr(depths), B.ptr(camtoworlds), B.ptr(Ks), int(ctx.z_depth),
                   B.ptr(_f32c(v_normals)), B.ptr(v_depths), _stream(depths))
        return v_depths, None, None, None
