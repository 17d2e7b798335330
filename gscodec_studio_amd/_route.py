"""Which way one ``rasterization()`` call goes: ONE decision, taken from plain facts about the call (no tensors), as an
immutable record every later branch reads.  ``rendering._facts`` reads the facts off the tensors; nothing else in the
package asks again whether the batch is unpacked, on one GPU, on the device, with fixed poses.

The A/B switches are module attributes read at call time (tests flip them): ``_step.ENABLED`` (GS_STEP_DRIVER),
``_wrapper.PREFILL_ENABLED`` (GS_GRAD_PREFILL), ``_readback._PINNED_DIRECT_MAX``; ``_wrapper._FUSE_SH_BWD`` (GS_FUSE_SH_BWD)
and ``distributed.sparse_enabled`` (GS_DIST_SPARSE) reach this module as the facts ``sh_bwd_fusable`` and ``sparse_enabled``."""
from __future__ import annotations

from typing import NamedTuple, Optional

from . import _step, _wrapper
from ._readback import direct_block_sums


class Route(NamedTuple):
    dyn_fused: bool  # dynamic splats: the temporal slice inside the projection kernels (else DynamicSlice.apply_unfused first)
    split_pair: bool  # the (sh0, shN) pair stays two tensors (else concatenated)
    fuse_mask: bool  # a MaskedShN is applied by the projection pass (else materialised up front)
    fuse_sh: bool  # shared SH coefficients, fixed poses: the fused SH kernels (view directions, mask, SH, clamp in one)
    gather_autograd: bool  # gaussian-sharded: the cameras are gathered through autograd (pose / intrinsics gradients)
    sparse: bool  # gaussian-sharded: the sparse exchange is in use (only the visible rows travel)
    dist_rows: bool  # gaussian-sharded: the splat rows themselves travel (distributed._ExchangeRows)
    use_rows: bool  # projection into splat rows (project_rows) instead of separate arrays (fully_fused_projection)
    step_driver: bool  # the whole forward as two native calls (_step.rasterize_step)
    prefill: bool  # the projection's dense gradients are zero-filled by the compositing forward (_wrapper.GradPrefill)
    row_colors: bool  # [N, 3] colours are written into the rows by the projection
    means_alias: bool  # the array projection hands the means back, so that the SH backward's d/d means is added in its kernel
    opacity_rider: bool  # the per-view opacities are written by the fused SH kernel instead of `.repeat` + autograd's sum
    sh_op: Optional[str]  # who evaluates SH colours: None | "projection" | "view" | "shared" | "per_view" | "packed"
    depth_view: bool  # RGB+D / RGB+ED: colour + depth are the view rows[..., 6:10] (else a cat)
    rows_begin: bool  # receiver side of the row exchange: binning + compositing by _step.rows_begin (else isect_tiles_start)


def route(*, packed: bool, distributed: bool, sparse_enabled: bool, on_device: bool, pose_grads: bool, camera_grads: bool, means_grad: bool,
          grad_enabled: bool,
          covars: bool, sh_degree: Optional[int], form: str, D: int, K: int, render_mode: str, antialiased: bool, channel_chunk: int,
          deterministic: bool, tile_size: int, C: int, N: int, dynamic: bool = False, dyn_quantize=(), mask: bool = False,
          sh_bwd_fusable: bool = False, shN_aligned: bool = False, mask_n: bool = False) -> Route:
    """``form``: "ND" | "CND" post-activation colours, "NK3" | "CNK3" SH coefficients, "pair" = (sh0, shN); ``D`` their last
    dimension, ``K`` the number of SH coefficients.  ``sparse_enabled``: ``distributed.sparse_enabled`` of the call; ``camera_grads``: poses or
    intrinsics require gradients.
    ``dyn_quantize``: the attributes a dynamic slice quantizes.  ``sh_bwd_fusable``: ``_wrapper.sh_bwd_fusable`` of the
    coefficients; ``shN_aligned``: shN contiguous and 16-byte aligned; ``mask_n``: the mask has N logits."""
    sh = sh_degree is not None
    unpacked_fixed = not packed and on_device and not pose_grads  # unpacked, on the device, fixed poses
    local = unpacked_fixed and not distributed  # ... and on one GPU
    # what the step driver bins and composites: three colour channels in one chunk, float atomics, tiles of wave64 quadrants
    step_ok = _step.ENABLED and not deterministic and render_mode == "RGB" and channel_chunk >= 3 and tile_size <= 16

    dyn_fused = dynamic and local and not covars and not sh and form == "ND" and ("colors" not in dyn_quantize or D == 3)
    split_pair = form == "pair" and local and K >= 2
    # the fused mask rides on the fused SH backward: everything that backward's fused route checks must be known to hold
    # before the forward runs, or training would die in loss.backward()
    fuse_mask = mask and split_pair and sh_bwd_fusable and shN_aligned and mask_n
    shared_sh = sh and form in ("NK3", "pair")
    fuse_sh = shared_sh and unpacked_fixed
    colors3 = not sh and form == "ND" and D == 3
    sparse = distributed and not packed and not camera_grads and sparse_enabled
    dist_rows = sparse and on_device and (fuse_sh or colors3)
    use_rows = not packed and on_device and (not distributed or dist_rows)
    row_colors = use_rows and colors3
    in_rows = use_rows and (row_colors or fuse_sh)  # the colours are columns 6:9 of the splat rows
    step_driver = step_ok and local and in_rows and direct_block_sums(C * N)
    if not sh:
        sh_op = None
    elif in_rows:
        sh_op = "projection"
    elif packed:
        sh_op = "packed"
    else:
        sh_op = "view" if fuse_sh else "shared" if shared_sh else "per_view"
    return Route(
        dyn_fused=dyn_fused, split_pair=split_pair, fuse_mask=fuse_mask, fuse_sh=fuse_sh,
        gather_autograd=distributed and camera_grads, sparse=sparse, dist_rows=dist_rows, use_rows=use_rows,
        step_driver=step_driver, prefill=use_rows and not step_driver and grad_enabled and _wrapper.PREFILL_ENABLED,
        row_colors=row_colors, means_alias=fuse_sh and means_grad and not use_rows,
        opacity_rider=fuse_sh and not use_rows and not antialiased, sh_op=sh_op,
        depth_view=in_rows and not distributed and render_mode in ("RGB+D", "RGB+ED"),
        rows_begin=step_ok and distributed and use_rows)
