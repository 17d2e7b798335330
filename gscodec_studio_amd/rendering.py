"""Render API: ``rasterization()`` with the reference's signature, defaults, return values
and ``meta`` dictionary (reference ``gsplat/rendering.py:28-582``), orchestrating the five
HIP stages  project -> SH colour -> tile-intersect + radix sort -> offset-encode ->
per-tile alpha compositing.

Drop-in contract kept from the reference:
* ``means2d`` stays an autograd intermediate between the projection Function and the
  rasterize Function, so ``meta["means2d"].retain_grad()`` / ``.absgrad`` work for the
  densification strategies (reference strategy/default.py:150, 221-226);
* ``meta`` keys and dtypes: camera_ids, gaussian_ids, radii, means2d, depths, conics,
  opacities, tile_width, tile_height, tiles_per_gauss, isect_ids, flatten_ids,
  isect_offsets, width, height, tile_size, n_cameras.

Differences by design: shared SH coefficients are not expanded to ``[C,N,K,3]`` and
channel padding is not needed (see _wrapper.py).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor
from typing_extensions import Literal

from . import _step
from ._readback import direct_block_sums
from ._route import Route, route
from .compression_simulation.ada_mask import MaskedShN
from ._wrapper import (
    ROW_COLOR,
    binning_meta,
    fully_fused_projection,
    project_rows,
    GradPrefill,
    gather_rows,
    isect_offset_encode,
    isect_tiles,
    isect_tiles_abandon,
    isect_tiles_begin,
    isect_tiles_finish,
    isect_tiles_start,
    rasterize_to_pixels,
    spherical_harmonics,
    spherical_harmonics_shared,
    spherical_harmonics_view,
    sh_bwd_fusable,
)


def _camera_centers(viewmats: Tensor) -> Tensor:
    """Camera positions in world space, ``inverse(viewmats)[:, :3, 3]``, in closed form.

    The reference calls ``torch.inverse(viewmats)`` (rendering.py:370); on ROCm that goes through
    a batched LU with a host-side status check, i.e. a device synchronisation of ~0.5 ms in the
    middle of every step (measured: tools/cpu_prof.py).  For an affine world->camera matrix
    [[A, t], [0, 1]] the inverse's translation is -A^-1 t, and A^-1 = adj(A) / det(A) is three
    cross products -- a handful of tiny asynchronous kernels, differentiable through autograd.
    """
    if viewmats.is_cuda and not viewmats.requires_grad:
        from . import _backend as B

        vm = viewmats.contiguous()
        out = torch.empty((vm.shape[0], 3), dtype=torch.float32, device=vm.device)
        with torch.cuda.device(vm.device):
            B.call("gs_camera_centers", vm.shape[0], B.ptr(vm), B.ptr(out), torch.cuda.current_stream(vm.device).cuda_stream)
        return out
    A = viewmats[:, :3, :3]
    t = viewmats[:, :3, 3]
    c0, c1, c2 = A[:, :, 0], A[:, :, 1], A[:, :, 2]
    r0 = torch.linalg.cross(c1, c2)
    r1 = torch.linalg.cross(c2, c0)
    r2 = torch.linalg.cross(c0, c1)
    det = (c0 * r0).sum(-1, keepdim=True)
    inv_t = torch.stack([(r0 * t).sum(-1), (r1 * t).sum(-1), (r2 * t).sum(-1)], dim=-1) / det
    return -inv_t


def _facts(means, colors, viewmats, Ks, covars, dynamic, sh_degree, packed, distributed, render_mode, rasterize_mode, channel_chunk,
           deterministic, tile_size) -> Route:
    """The one place that reads the routing facts off ``rasterization()``'s arguments; ``_route.route`` decides on them."""
    N, C = means.shape[0], viewmats.shape[0]
    pose_grads = viewmats.requires_grad
    pair = {}
    if isinstance(colors, (tuple, list)):
        assert sh_degree is not None and len(colors) == 2, "a (sh0, shN) pair needs sh_degree"
        sh0, shN = colors
        mask = shN if isinstance(shN, MaskedShN) else None  # shN + the mask to apply to it (compression_simulation.ada_mask)
        if mask is not None:
            shN = mask.shN
        assert sh0.shape == (N, 1, 3) and shN.dim() == 3 and shN.shape[0] == N and shN.shape[2] == 3, (sh0.shape, shN.shape)
        form, D, K = "pair", 3, 1 + shN.shape[1]
        pair = dict(mask=mask is not None, sh_bwd_fusable=sh_bwd_fusable(K, sh0, shN, pose_grads),
                    shN_aligned=shN.is_contiguous() and shN.data_ptr() % 16 == 0,
                    mask_n=mask is not None and mask.mask_logits.numel() == N)
    else:
        dim = colors.dim()
        form = ("ND" if dim == 2 else "CND") if sh_degree is None else ("NK3" if dim == 3 else "CNK3")
        D, K = (colors.shape[-1] if dim else 0), (colors.shape[-2] if dim >= 2 else 0)
    sparse_enabled = False
    if distributed:
        from . import distributed as dist

        sparse_enabled = dist.sparse_enabled(means, [C])  # (every rank renders the same number of cameras)
    return route(packed=packed, distributed=distributed, sparse_enabled=sparse_enabled, on_device=means.is_cuda and viewmats.is_cuda,
                 pose_grads=pose_grads, camera_grads=pose_grads or Ks.requires_grad, means_grad=means.requires_grad,
                 grad_enabled=torch.is_grad_enabled(), covars=covars is not None, sh_degree=sh_degree, form=form, D=D, K=K,
                 render_mode=render_mode, antialiased=rasterize_mode == "antialiased", channel_chunk=channel_chunk,
                 deterministic=deterministic, tile_size=tile_size, C=C, N=N, dynamic=dynamic is not None,
                 dyn_quantize=tuple(dynamic.quantize) if dynamic is not None else (), **pair)


class _RowsColorDepth(torch.autograd.Function):
    """``cat((colors, depths[..., None]), -1)`` when ``colors`` are columns 6:9 of the splat rows: column 9 of the same rows holds the
    depth (include/gsplat_hip.h "Splat rows"), so the four channels are the view ``rows[..., 6:10]`` -- nothing is copied, and on the
    way back the compositing backward's gradient rows stay the one buffer the projection backward reads in place."""

    @staticmethod
    def forward(ctx, colors, depths, hold):
        ctx.set_materialize_grads(False)
        return hold[0][..., ROW_COLOR:ROW_COLOR + 4]

    @staticmethod
    def backward(ctx, v):
        if v is None:
            return None, None, None
        return v[..., :3], v[..., 3], None


def _expected_depth(render_colors: Tensor, render_alphas: Tensor) -> Tensor:
    """accumulated depth -> expected depth (reference rendering.py:471-477: cat(rc[..., :-1], rc[..., -1:] / ra.clamp(min=1e-10)))"""
    if render_colors.is_cuda and render_colors.dtype == torch.float32 and render_alphas.dtype == torch.float32:
        return _ExpectedDepth.apply(render_colors, render_alphas)
    return torch.cat([render_colors[..., :-1], render_colors[..., -1:] / render_alphas.clamp(min=1e-10)], dim=-1)


class _ExpectedDepth(torch.autograd.Function):
    """The tail of the "ED" / "RGB+ED" modes in one kernel each way (``gs_expected_depth_fwd`` / ``_bwd``)."""

    @staticmethod
    def forward(ctx, renders, alphas):
        from . import _backend as B

        renders, alphas = renders.contiguous(), alphas.contiguous()
        out = torch.empty_like(renders)
        n_pix, ch = alphas.numel(), renders.shape[-1]
        with torch.cuda.device(renders.device):
            B.call("gs_expected_depth_fwd", n_pix, ch, B.ptr(renders), B.ptr(alphas), B.ptr(out), torch.cuda.current_stream(renders.device).cuda_stream)
        ctx.save_for_backward(renders, alphas)
        return out

    @staticmethod
    def backward(ctx, v_out):
        from . import _backend as B

        renders, alphas = ctx.saved_tensors
        v_out = v_out.contiguous().float()
        need = ctx.needs_input_grad
        v_r = torch.empty_like(renders) if need[0] else None
        v_a = torch.empty_like(alphas) if need[1] else None
        with torch.cuda.device(renders.device):
            B.call("gs_expected_depth_bwd", alphas.numel(), renders.shape[-1], B.ptr(renders), B.ptr(alphas), B.ptr(v_out), B.ptr(v_r), B.ptr(v_a),
                   torch.cuda.current_stream(renders.device).cuda_stream)
        return v_r, v_a


def rasterization(
    means: Tensor,  # [N, 3]
    quats: Tensor,  # [N, 4]
    scales: Tensor,  # [N, 3]
    opacities: Tensor,  # [N]
    colors,  # Tensor [(C,) N, D] or [(C,) N, K, 3]; or the pair (sh0 [N, 1, 3], shN [N, K-1, 3]) with sh_degree
    viewmats: Tensor,  # [C, 4, 4]
    Ks: Tensor,  # [C, 3, 3]
    width: int,
    height: int,
    near_plane: float = 0.01,
    far_plane: float = 1e10,
    radius_clip: float = 0.0,
    eps2d: float = 0.3,
    sh_degree: Optional[int] = None,
    packed: bool = True,
    tile_size: int = 16,
    backgrounds: Optional[Tensor] = None,
    render_mode: Literal["RGB", "D", "ED", "RGB+D", "RGB+ED"] = "RGB",
    sparse_grad: bool = False,
    absgrad: bool = False,
    rasterize_mode: Literal["classic", "antialiased"] = "classic",
    channel_chunk: int = 32,
    distributed: bool = False,
    camera_model: Literal["pinhole", "ortho", "fisheye"] = "pinhole",
    covars: Optional[Tensor] = None,
    deterministic: bool = False,
    dynamic=None,
) -> Tuple[Tensor, Tensor, Dict]:
    """Rasterize a set of 3D Gaussians (N) to a batch of image planes (C).

    Same semantics as the reference ``gsplat.rendering.rasterization``.

    Args:
        means: 3D centres [N,3].  quats: rotations wxyz [N,4] (need not be normalised).
        scales: [N,3].  opacities: [N].  colors: [(C,)N,D] post-activation features, or SH
        coefficients [(C,)N,K,3] when ``sh_degree`` is set.  viewmats: world->camera
        [C,4,4].  Ks: intrinsics [C,3,3].  covars: optional [N,3,3] replacing quats/scales.
        packed: COO intermediates (memory-efficient for many cameras).  sparse_grad: COO
        gradients (needs packed).  absgrad: also accumulate |d means2d| into
        ``meta["means2d"].absgrad``.  rasterize_mode "antialiased": opacity compensation.
        render_mode: RGB / D / ED / RGB+D / RGB+ED.  distributed: gaussian-sharded
        multi-GPU mode of the reference (see distributed.py; the camera-sharded data
        parallel wrapper is ``distributed.rasterization_camera_sharded``).
        deterministic (opt-in, beyond the reference's signature): bit-reproducible gradients -- the compositing
        backward accumulates in fixed point instead of with float atomics (up to 4 render channels).
        dynamic (opt-in, beyond the reference's signature): a ``dynamic.DynamicSlice`` or the tuple ``(motion [N,9], omega [N,4],
        trbf_center [N,1], trbf_scale [N,1], timestamp)`` -- the splats are DYNAMIC (spacetime) gaussians and ``means`` / ``quats`` /
        ``opacities`` their time-independent parameters: the temporal slice of the reference's dynamic trainer
        (examples/simple_trainer_dyngs.py:506-521) is evaluated inside the projection kernels, bit-identical to
        ``dynamic.temporal_slice`` followed by this call (csrc/projection_dyn.hip; routes the fused kernels do not cover take
        exactly that detour).

    Returns:
        render_colors [C,H,W,X], render_alphas [C,H,W,1], meta dict.
    """
    meta: Dict = {}

    N = means.shape[0]
    C = viewmats.shape[0]
    assert C > 0, "rasterization needs at least one camera (the reference fails on an empty batch too: log2(0) in isect_tiles)"
    device = means.device
    if dynamic is not None:
        from .dynamic import DynamicSlice

        dynamic = DynamicSlice.of(dynamic)
        dynamic.check(N)
        assert covars is None, "dynamic splats rotate their quaternions in time: pass quats + scales, not covars"
    R = _facts(means, colors, viewmats, Ks, covars, dynamic, sh_degree, packed, distributed, render_mode, rasterize_mode, channel_chunk,
               deterministic, tile_size)
    if dynamic is not None and not R.dyn_fused:  # the same chain through the stand-alone operators, then the plain call
        means, quats, scales, opacities, c_ = dynamic.apply_unfused(means, quats, scales, opacities,
                                                                     colors if torch.is_tensor(colors) else None)
        colors = c_ if c_ is not None else colors
        dynamic = None
    assert means.shape == (N, 3), means.shape
    if covars is None:
        assert quats.shape == (N, 4), quats.shape
        assert scales.shape == (N, 3), scales.shape
    else:
        assert covars.shape == (N, 3, 3), covars.shape
        quats, scales = None, None
        # 3x3 matrix -> upper-triangular 6-vector
        covars = covars[..., [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    assert opacities.shape == (N,), opacities.shape
    assert viewmats.shape == (C, 4, 4), viewmats.shape
    assert Ks.shape == (C, 3, 3), Ks.shape
    assert render_mode in ["RGB", "D", "ED", "RGB+D", "RGB+ED"], render_mode
    # Opt-in beyond the reference's signature: SH coefficients as the PAIR (sh0, shN) the trainers keep as separate parameters
    # (reference examples/simple_trainer.py:779-786 concatenates them before every render: 193 MB each way at 1 M splats, and
    # autograd splits the gradient again).  The fused route takes the two tensors as they are; every other route gets the cat.
    sh_rest = None
    sh_mask = None
    if isinstance(colors, (tuple, list)):
        sh0, shN = colors
        if isinstance(shN, MaskedShN):
            if R.fuse_mask:
                sh_mask, shN = (shN.mask_logits, shN.temperature, shN.binary), shN.shN
            else:
                shN = shN.materialize()
        if R.split_pair:
            colors, sh_rest = sh0, shN
        else:
            colors = torch.cat([sh0, shN], dim=1)
    # the compositing kernels map a tile onto wave64 quadrants of 8x8 pixels: tiles up to 16x16 (the reference launches
    # tile_size^2 threads per block, i.e. accepts up to 32; every caller in the reference uses 16).  Checked here, before
    # projection and binning run, instead of surfacing as a native error afterwards.
    assert 1 <= tile_size <= 32 and (tile_size < 17 or tile_size % 2 == 0), \
        f"tile_size must be in [1, 16] or an even size up to 32 on the HIP backend, got {tile_size}"

    if sh_degree is None:
        # post-activation values [N, D] or [C, N, D]
        assert (colors.dim() == 2 and colors.shape[0] == N) or (
            colors.dim() == 3 and colors.shape[:2] == (C, N)
        ), colors.shape
        if distributed:
            assert colors.dim() == 2, "Distributed mode only supports per-Gaussian colors."
    else:
        # SH coefficients [N, K, 3] or [C, N, K, 3]; partial bands allowed
        assert (colors.dim() == 3 and colors.shape[0] == N and colors.shape[2] == 3) or (
            colors.dim() == 4 and colors.shape[:2] == (C, N) and colors.shape[3] == 3
        ), colors.shape
        assert (sh_degree + 1) ** 2 <= colors.shape[-2] + (sh_rest.shape[1] if sh_rest is not None else 0), colors.shape
        if distributed:
            assert colors.dim() == 3, "Distributed mode only supports per-Gaussian colors."

    if absgrad:
        assert not distributed, "AbsGrad is not supported in distributed mode."

    if distributed:
        from . import distributed as D

        world_rank = torch.distributed.get_rank()
        world_size = torch.distributed.get_world_size()
        # gaussians are sharded over ranks; gather #gaussians and all cameras
        C_world = [C] * world_size
        cap_world = None  # chunk capacities of the sparse exchange (None: every row travels)
        if R.gather_autograd:  # (pose or intrinsics gradients travel back through the gather)
            N_world = D.all_gather_int32(world_size, N, device=device)
            viewmats, Ks = D.all_gather_tensor_list(world_size, [viewmats, Ks])
        else:
            # (the shard sizes travel over the host group while the projection is queued: resolved at the exchange)
            shard_sizes, viewmats, Ks = D.gather_shard_meta(world_size, N, viewmats, Ks, D.sparse_capacity(C, N) if R.sparse else 0)
            N_world = None
            cap_world = () if R.sparse else None  # chunk capacities: known to be in use, values still in flight
        C = len(viewmats)

    # Unpacked batches on one GPU go through SPLAT ROWS: the projection writes one 64-byte row per (camera, gaussian) --
    # mean2d, conic, opacity (x antialias compensation), colour, depth, radius -- that the compositing kernels fetch whole;
    # means2d / conics / opacities (/ colours) below are column views of that buffer (same shapes and dtypes as the
    # reference's separate tensors; like its means2d / conics they are only defined where radii > 0).
    # (gaussian-sharded: when the colours sit in the rows and the sparse exchange is on, the rows themselves travel --
    # distributed._ExchangeRows; otherwise the separate arrays of the reference's layout do)
    row_colors = colors if R.row_colors else None
    # shared SH coefficients and fixed poses: the colours are evaluated by the projection pass itself
    sh_coeffs, sh_deg = (colors, sh_degree) if R.fuse_sh else (None, None)
    antialiased = rasterize_mode == "antialiased"
    if R.step_driver:
        # the common training call: the whole forward as two native calls around the one host read-back (_step.py)
        return _step.rasterize_step(
            means, covars, quats, scales, opacities, viewmats, Ks, width, height, eps2d, near_plane, far_plane, radius_clip,
            antialiased, camera_model, row_colors, sh_coeffs, sh_rest, sh_deg, tile_size, backgrounds, absgrad, sh_mask=sh_mask,
            dynamic=dynamic)
    rows = None
    prefill = None
    if R.use_rows:
        # the dense per-gaussian gradients of the projection node are allocated and zero-filled by the compositing
        # forward's side job; its backward then writes the visible gaussians' rows only (_wrapper.GradPrefill)
        prefill = GradPrefill() if R.prefill else None
        radii, means2d, depths, conics, opacities, colors_rows, rows = project_rows(
            means, covars, quats, scales, viewmats, Ks, width, height, opacities, row_colors,
            eps2d=eps2d, near_plane=near_plane, far_plane=far_plane, radius_clip=radius_clip,
            antialiased=antialiased, camera_model=camera_model, sh_coeffs=sh_coeffs, sh_degree=sh_deg, sh_rest=sh_rest,
            prefill=prefill, sh_mask=sh_mask, dynamic=dynamic,
        )
        camera_ids, gaussian_ids = None, None
        if R.row_colors or R.fuse_sh:
            colors = colors_rows  # [C, N, 3]: columns 6:9 of the rows
    else:
        # the fused SH route reads the means a second time (view directions): with means_alias it gets them back FROM the
        # projection, so that its contribution to d/d means is added inside the projection's backward kernel
        proj_results = fully_fused_projection(
            means, covars, quats, scales, viewmats, Ks, width, height,
            eps2d=eps2d, packed=packed, near_plane=near_plane, far_plane=far_plane,
            radius_clip=radius_clip, sparse_grad=sparse_grad,
            calc_compensations=antialiased, camera_model=camera_model, _means_alias=R.means_alias,
        )
        means_sh = means
        if R.means_alias:
            means_sh, proj_results = proj_results[5], proj_results[:5]

        if packed:
            camera_ids, gaussian_ids, radii, means2d, depths, conics, compensations = proj_results
            opacities = gather_rows(opacities, gaussian_ids)  # [nnz] = opacities[gaussian_ids], one-pass atomic backward
        else:
            radii, means2d, depths, conics, compensations = proj_results
            camera_ids, gaussian_ids = None, None
            # classic mode + shared SH on the fused route: the per-view opacities ride along with the colour kernels
            # (written by the SH forward, summed over cameras by its backward) instead of `.repeat` + autograd's sum
            opacities_n = opacities
            if not R.opacity_rider:
                opacities = opacities.repeat(C, 1)  # [C, N]

        if compensations is not None:
            opacities = opacities * compensations

    meta.update(
        {
            "camera_ids": camera_ids,
            "gaussian_ids": gaussian_ids,
            "radii": radii,
            "means2d": means2d,
            "depths": depths,
            "conics": conics,
            "opacities": opacities,
        }
    )

    tile_width = math.ceil(width / float(tile_size))
    tile_height = math.ceil(height / float(tile_size))
    # Tile binning is split around its one host sync (the intersection count): the first half is queued here, the
    # colour evaluation below then runs on the GPU while the host waits for the count.
    isect_state = None
    if not distributed:
        n_elems = int(radii.numel())
        isect_state = isect_tiles_begin(means2d, radii, depths, tile_size, tile_width, tile_height, True, C,
                                        0 if packed else N, n_elems, camera_ids.contiguous() if packed else None)

    # colours -> [C, N, D] or [nnz, D]
    if R.sh_op is None:
        if packed:
            colors = gather_rows(colors, gaussian_ids) if colors.dim() == 2 else colors[camera_ids, gaussian_ids]
        elif colors.dim() == 2:
            # (one camera: a view -- autograd's expand backward is a sum over the camera axis, a 35 us reduce kernel at 2 M x 9
            # floats even when that axis has one entry)
            colors = colors[None] if C == 1 else colors.expand(C, -1, -1)
    elif R.sh_op == "view":
        # fused: camera centres, dirs, mask, SH and clamp_min(. + 0.5, 0) in one kernel each way
        if R.opacity_rider:
            colors, opacities = spherical_harmonics_view(sh_degree, means_sh, viewmats, colors, radii, opacities=opacities_n)
            meta["opacities"] = opacities
        else:
            colors = spherical_harmonics_view(sh_degree, means_sh, viewmats, colors, radii)  # [C, N, 3]
    elif R.sh_op != "projection":  # ("projection": evaluated by the projection pass, columns 6:9 of the splat rows)
        campos = _camera_centers(viewmats)  # [C, 3] == inverse(viewmats)[:, :3, 3]
        masks = radii > 0
        if R.sh_op == "packed":
            dirs = gather_rows(means, gaussian_ids) - campos[camera_ids]  # [nnz, 3]
            shs = gather_rows(colors, gaussian_ids) if colors.dim() == 3 else colors[camera_ids, gaussian_ids, :, :]
            colors = spherical_harmonics(sh_degree, dirs, shs, masks=masks)  # [nnz, 3]
        else:
            dirs = means[None, :, :] - campos[:, None, :]  # [C, N, 3]
            sh_fn = spherical_harmonics_shared if R.sh_op == "shared" else spherical_harmonics
            colors = sh_fn(sh_degree, dirs, colors, masks=masks)  # [C, N, 3]
        # same convention as the reference (rendering.py:392)
        colors = torch.clamp_min(colors + 0.5, 0.0)

    if distributed:
        from . import distributed as D

        # redistribute, then bin.  The sparse exchange sizes its chunks from earlier steps without a read-back; should a
        # chunk have been too small (every rank learns it at the tile-count read-back), repeat once at full capacity.
        pre = (radii, means2d, depths, conics, opacities, colors, camera_ids, gaussian_ids)
        pre_rows = rows
        if N_world is None:
            N_world, caps = shard_sizes()
            cap_world = caps if cap_world is not None else None
        for attempt in range(2):
            if R.use_rows:
                C, radii, means2d, depths, conics, opacities, colors, rows = D.exchange_rows(
                    world_rank, N, N_world, C_world, cap_world, *pre[:6], pre_rows)
            else:
                (C, radii, means2d, depths, conics, opacities, colors, camera_ids, gaussian_ids) = D.exchange_projected(
                    world_rank, world_size, N, N_world, C_world, packed, *pre, cap_world=cap_world,
                )
            # binning up to its read-back; the depth pre-sort queued behind the count keeps the GPU busy while the host
            # looks at the overflow flags (stored to pinned memory before the count) and comes back for the rest
            rows_state = None
            if R.rows_begin and direct_block_sums(radii.numel()):
                # (received rows: binning + compositing as native calls around the read-back, like the one-GPU fast path)
                rows_state = _step.rows_begin(radii, depths, rows, tile_size, tile_width, tile_height)
            else:
                isect_state = isect_tiles_start(
                    means2d, radii, depths, tile_size, tile_width, tile_height,
                    packed=packed, n_cameras=C, camera_ids=camera_ids, gaussian_ids=gaussian_ids,
                )
            if cap_world is None or not D.exchange_overflowed():
                break
            # (the count kernel may still be storing into the state's pinned buffer: handed back here, not left to the collector)
            _step.rows_abandon(rows_state)
            isect_tiles_abandon(isect_state)
            isect_state = rows_state = None
            cap_world = [C_world[r] * N_world[r] for r in range(world_size)]
        if rows_state is not None:
            render_colors, render_alphas, tiles_per_gauss, isect_ids, flatten_ids, isect_offsets = _step.rows_composite(
                rows_state, means2d, conics, colors, opacities, backgrounds, width, height, absgrad, prefill)
            meta.update(binning_meta(tile_size, tile_width, tile_height, tiles_per_gauss, isect_ids, flatten_ids, isect_offsets, width, height, C))
            return render_colors, render_alphas, meta

    if render_mode in ["RGB+D", "RGB+ED"]:
        if R.depth_view:
            # the colours ride in the splat rows, whose next column IS the depth: the four channels are a view (no cat, and the
            # compositing backward's gradient rows reach the projection backward in place instead of through autograd's split)
            colors = _RowsColorDepth.apply(colors, depths, (rows,))
        else:
            colors = torch.cat((colors, depths[..., None]), dim=-1)
        if backgrounds is not None:
            backgrounds = torch.cat([backgrounds, torch.zeros(C, 1, device=backgrounds.device)], dim=-1)
    elif render_mode in ["D", "ED"]:
        colors = depths[..., None]
        if backgrounds is not None:
            backgrounds = torch.zeros(C, 1, device=backgrounds.device)

    if isect_state is not None:  # (emit + pair sort + offsets: one native call on the sorted path)
        tiles_per_gauss, isect_ids, flatten_ids, isect_offsets = isect_tiles_finish(isect_state, offsets_for=C)
    else:
        tiles_per_gauss, isect_ids, flatten_ids = isect_tiles(
            means2d, radii, depths, tile_size, tile_width, tile_height,
            packed=packed, n_cameras=C, camera_ids=camera_ids, gaussian_ids=gaussian_ids,
        )
        isect_offsets = isect_offset_encode(isect_ids, C, tile_width, tile_height)

    meta.update(binning_meta(tile_size, tile_width, tile_height, tiles_per_gauss, isect_ids, flatten_ids, isect_offsets, width, height, C))

    if colors.shape[-1] > channel_chunk:
        n_chunks = (colors.shape[-1] + channel_chunk - 1) // channel_chunk
        render_colors, render_alphas = [], []
        for i in range(n_chunks):
            colors_chunk = colors[..., i * channel_chunk : (i + 1) * channel_chunk]
            backgrounds_chunk = (
                backgrounds[..., i * channel_chunk : (i + 1) * channel_chunk] if backgrounds is not None else None
            )
            rc_, ra_ = rasterize_to_pixels(
                means2d, conics, colors_chunk, opacities, width, height, tile_size, isect_offsets, flatten_ids,
                backgrounds=backgrounds_chunk, packed=packed, absgrad=absgrad, deterministic=deterministic,
            )
            render_colors.append(rc_)
            render_alphas.append(ra_)
        render_colors = torch.cat(render_colors, dim=-1)
        render_alphas = render_alphas[0]  # discard the rest
    else:
        render_colors, render_alphas = rasterize_to_pixels(
            means2d, conics, colors, opacities, width, height, tile_size, isect_offsets, flatten_ids,
            backgrounds=backgrounds, packed=packed, absgrad=absgrad, deterministic=deterministic, prefill=prefill,
        )
    if render_mode in ["ED", "RGB+ED"]:
        render_colors = _expected_depth(render_colors, render_alphas)

    return render_colors, render_alphas, meta


###### 2DGS ######
def _affine_inverse(viewmats: Tensor) -> Tensor:
    """``inverse(viewmats)`` for affine ``[[A, t], [0, 1]]`` matrices in closed form (adjugate / determinant): a few tiny
    asynchronous kernels, differentiable, instead of ``torch.linalg.inv``'s batched LU with its host-side status check."""
    A, t = viewmats[..., :3, :3], viewmats[..., :3, 3]
    c0, c1, c2 = A[..., :, 0], A[..., :, 1], A[..., :, 2]
    inv = torch.stack([torch.linalg.cross(c1, c2), torch.linalg.cross(c2, c0), torch.linalg.cross(c0, c1)], dim=-2)
    inv = inv / (c0 * inv[..., 0, :]).sum(-1)[..., None, None]
    out = torch.zeros_like(viewmats)
    out[..., :3, :3] = inv
    out[..., :3, 3] = -(inv @ t[..., None])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def rasterization_2dgs(
    means: Tensor,  # [N, 3]
    quats: Tensor,  # [N, 4]
    scales: Tensor,  # [N, 3]
    opacities: Tensor,  # [N]
    colors: Tensor,  # [(C,) N, D] or [N, K, 3]
    viewmats: Tensor,  # [C, 4, 4]
    Ks: Tensor,  # [C, 3, 3]
    width: int,
    height: int,
    near_plane: float = 0.01,
    far_plane: float = 1e10,
    radius_clip: float = 0.0,
    eps2d: float = 0.3,
    sh_degree: Optional[int] = None,
    packed: bool = False,
    tile_size: int = 16,
    backgrounds: Optional[Tensor] = None,
    render_mode: Literal["RGB", "D", "ED", "RGB+D", "RGB+ED"] = "RGB",
    sparse_grad: bool = False,
    absgrad: bool = False,
    distloss: bool = False,
    depth_mode: Literal["expected", "median"] = "expected",
) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Dict]:
    """Rasterize a set of 2D Gaussians (N) to a batch of image planes (C): the reference's
    ``gsplat.rendering.rasterization_2dgs`` (rendering.py:1002-1321) -- same parameters, defaults, asserts and return order --
    on the HIP operators of ``surfel.py``: project -> tile-intersect + radix sort -> offset-encode -> SH colour -> per-tile
    compositing -> (expected depth) -> normals from depth.

    Returns ``(render_colors [C,H,W,X], render_alphas [C,H,W,1], render_normals [C,H,W,3] (rotated to world space),
    render_normals_from_depth [C,H,W,3] (``None`` unless the mode is "RGB+D" or "RGB+ED"), render_distort [C,H,W,1],
    render_median [C,H,W,1], meta)``.  ``meta`` has the reference's keys, ``ray_transforms``, ``normals``, ``render_distort`` and
    ``gradient_2dgs`` included; ``meta["gradient_2dgs"]`` is what ``DefaultStrategy(key_for_gradient="gradient_2dgs")`` reads, and
    ``meta["means2d"].absgrad`` is set by the backward with ``absgrad=True`` (``gradient_2dgs`` gets no ``.absgrad``, as in the
    reference).  "ED" normalises the accumulated depth by ``alphas.clamp(min=1e-10)``.  ``distloss`` needs a depth mode.

    ``backgrounds`` is ``[C, D]`` for the colour channels; in the depth modes the depth channel's background is zero (a
    ``[C, X]`` tensor that already covers every rendered channel is taken as it is).

    One deliberate difference: ``gradient_2dgs.grad[c, n] = (v_ray_transforms[c, n, 0, 2], v_ray_transforms[c, n, 1, 2]) *
    depths[c, n]`` is formed from the FINAL gradient sums; the reference reads them inside its backward kernel while other
    workgroups are still adding (a race).  The normals from depth get their gradient through the depth map only.

    Not in this version (``NotImplementedError`` before any launch): ``packed=True`` and ``sparse_grad=True``, more than 4
    channels after the depth column is appended, ``tile_size != 16``.  There is no CPU path.
    """
    from . import surfel
    from ._wrapper import _require_gpu

    N = means.shape[0]
    C = viewmats.shape[0]
    assert means.shape == (N, 3), means.shape
    assert quats.shape == (N, 4), quats.shape
    assert scales.shape == (N, 3), scales.shape
    assert opacities.shape == (N,), opacities.shape
    assert viewmats.shape == (C, 4, 4), viewmats.shape
    assert Ks.shape == (C, 3, 3), Ks.shape
    assert render_mode in ["RGB", "D", "ED", "RGB+D", "RGB+ED"], render_mode
    assert depth_mode in ["expected", "median"], depth_mode
    if distloss:
        assert render_mode in ["D", "ED", "RGB+D", "RGB+ED"], \
            f"distloss requires depth rendering, render_mode should be D, ED, RGB+D, RGB+ED, but got {render_mode}"
    if sh_degree is None:
        # post-activation values [N, D] or [C, N, D]
        assert (colors.dim() == 2 and colors.shape[0] == N) or (colors.dim() == 3 and colors.shape[:2] == (C, N)), colors.shape
        D = colors.shape[-1]
    else:
        # SH coefficients [N, K, 3]; partial bands allowed
        assert colors.dim() == 3 and colors.shape[0] == N and colors.shape[2] == 3, colors.shape
        assert (sh_degree + 1) ** 2 <= colors.shape[1], colors.shape
        D = 3
    channels = {"RGB": D, "D": 1, "ED": 1}.get(render_mode, D + 1)
    surfel.check_unpacked("rasterization_2dgs", packed, sparse_grad)
    surfel.check_tile_size("rasterization_2dgs", tile_size)
    surfel.check_channels("rasterization_2dgs", channels)
    assert C > 0, "rasterization_2dgs needs at least one camera"
    for t in (means, quats, scales, opacities, colors, viewmats, Ks):
        _require_gpu(t, "rasterization_2dgs")

    if backgrounds is not None and backgrounds.shape[-1] != channels:
        assert render_mode != "RGB" and backgrounds.shape == (C, channels - 1), backgrounds.shape
        backgrounds = torch.cat([backgrounds, torch.zeros(C, 1, dtype=backgrounds.dtype, device=backgrounds.device)], dim=-1)

    radii, means2d, depths, ray_transforms, normals = surfel.fully_fused_projection_2dgs(
        means, quats, scales, viewmats, Ks, width, height, eps2d, near_plane, far_plane, radius_clip, packed, sparse_grad)
    opacities = opacities.repeat(C, 1)  # [C, N]
    densify = torch.zeros_like(means2d, requires_grad=True)

    tile_width = math.ceil(width / float(tile_size))
    tile_height = math.ceil(height / float(tile_size))
    # binning is split around its one host wait (the intersection count): the colour evaluation is queued in between
    isect_state = isect_tiles_begin(means2d, radii, depths, tile_size, tile_width, tile_height, True, C, N, int(radii.numel()), None)

    if sh_degree is not None:
        if viewmats.requires_grad:  # (the fused colour kernel has no gradient for the camera centres)
            dirs = means[None, :, :] - _camera_centers(viewmats)[:, None, :]
            colors = torch.clamp_min(spherical_harmonics_shared(sh_degree, dirs, colors, masks=radii > 0) + 0.5, 0.0)
        else:
            colors = spherical_harmonics_view(sh_degree, means, viewmats, colors, radii)  # [C, N, 3], clamp_min(. + 0.5, 0) included
    elif colors.dim() == 2:
        colors = colors.expand(C, -1, -1)

    if render_mode in ["RGB+D", "RGB+ED"]:
        colors = torch.cat((colors, depths[..., None]), dim=-1)
    elif render_mode in ["D", "ED"]:
        colors = depths[..., None]

    tiles_per_gauss, isect_ids, flatten_ids, isect_offsets = isect_tiles_finish(isect_state, offsets_for=C)

    render_colors, render_alphas, render_normals, render_distort, render_median = surfel.rasterize_to_pixels_2dgs(
        means2d, ray_transforms, colors, opacities, normals, densify, width, height, tile_size, isect_offsets, flatten_ids,
        backgrounds=backgrounds, packed=packed, absgrad=absgrad, distloss=distloss)

    if render_mode in ["ED", "RGB+ED"]:
        render_colors = _expected_depth(render_colors, render_alphas)
    camtoworlds = _affine_inverse(viewmats)
    render_normals_from_depth = None
    if render_mode in ["RGB+ED", "RGB+D"]:
        depth_for_normal = render_colors[..., -1:] if depth_mode == "expected" else render_median
        render_normals_from_depth = surfel.depth_to_normal(depth_for_normal, camtoworlds, Ks)

    meta = {"camera_ids": None, "gaussian_ids": None, "radii": radii, "means2d": means2d, "depths": depths,
            "ray_transforms": ray_transforms, "opacities": opacities, "normals": normals}
    meta.update(binning_meta(tile_size, tile_width, tile_height, tiles_per_gauss, isect_ids, flatten_ids, isect_offsets, width, height, C))
    meta.update({"render_distort": render_distort, "gradient_2dgs": densify})

    render_normals = torch.einsum("...ij,...hwj->...hwi", camtoworlds[..., :3, :3], render_normals)
    return render_colors, render_alphas, render_normals, render_normals_from_depth, render_distort, render_median, meta
