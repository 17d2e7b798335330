"""Depth-map helpers of the 2DGS trainer (reference ``gsplat/utils.py:44-131``).

* ``depth_to_points(depths, camtoworlds, Ks, z_depth=True)`` -- world-space points of depth maps; plain torch (a handful of
  elementwise operations, differentiable through autograd, any device).
* ``depth_to_normal(depths, camtoworlds, Ks, z_depth=True)`` -- world-space surface normals from the central differences of those
  points.  The reference builds them from ~15 torch launches over ``[C, H, W, 3]`` temporaries; here it is ONE kernel each way
  (``csrc/surfel.hip``: ``gs_depth_to_normal_fwd`` / ``_bwd``), GPU only, with the gradient going to ``depths``.

and the trainers' neighbour search (reference ``examples/utils.py:142``), re-exported from ``knn``: ``knn(x, K=4)``,
``knn_search``, ``init_scales`` (exact grid k-NN on the GPU, ``csrc/knn.hip``), and the other names the trainers import from
``examples/utils.py``: ``rgb_to_sh``, ``set_random_seed`` (plain restatements, lines 149-157) and ``load_ply`` with ``save_ply``
and ``load_ply_to_rasterizer_inputs`` beside it, re-exported from ``ply`` (``.ply`` files without plyfile, ``csrc/ply.hip``) -- so
``from utils import knn, rgb_to_sh, set_random_seed, load_ply`` becomes ``from gscodec_studio_amd.utils import ...``.
"""
from __future__ import annotations

import random

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

from .knn import init_scales, knn, knn_search
from .ply import load_ply, load_ply_to_rasterizer_inputs, read_ply_header, save_ply
from .surfel import depth_to_normal

__all__ = ["depth_to_points", "depth_to_normal", "knn", "knn_search", "init_scales", "rgb_to_sh", "set_random_seed", "load_ply",
           "save_ply", "load_ply_to_rasterizer_inputs", "read_ply_header"]


def rgb_to_sh(rgb: Tensor) -> Tensor:
    """Colours in [0, 1] to the degree-0 SH coefficient that renders them (reference ``examples/utils.py:149-151``)."""
    C0 = 0.28209479177387814
    return (rgb - 0.5) / C0


def set_random_seed(seed: int) -> None:
    """Seed ``random``, numpy and torch (reference ``examples/utils.py:154-157``)."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def depth_to_points(depths: Tensor, camtoworlds: Tensor, Ks: Tensor, z_depth: bool = True) -> Tensor:
    """Depth maps ``[..., H, W, 1]`` to world-space points ``[..., H, W, 3]``.  ``z_depth``: the depth is measured along the
    camera's z axis (True) or along the ray (False)."""
    assert depths.shape[-1] == 1, f"Invalid depth shape: {depths.shape}"
    assert camtoworlds.shape[-2:] == (4, 4), f"Invalid viewmats shape: {camtoworlds.shape}"
    assert Ks.shape[-2:] == (3, 3), f"Invalid Ks shape: {Ks.shape}"
    assert depths.shape[:-3] == camtoworlds.shape[:-2] == Ks.shape[:-2], \
        f"Shape mismatch! depths: {depths.shape}, viewmats: {camtoworlds.shape}, Ks: {Ks.shape}"
    height, width = depths.shape[-3:-1]
    x = torch.arange(width, device=depths.device, dtype=depths.dtype)  # [W]
    y = torch.arange(height, device=depths.device, dtype=depths.dtype)  # [H]
    fx, fy = Ks[..., 0, 0, None, None], Ks[..., 1, 1, None, None]
    cx, cy = Ks[..., 0, 2, None, None], Ks[..., 1, 2, None, None]
    dir_x = ((x[None, :] - cx + 0.5) / fx).expand(*depths.shape[:-1])  # [..., H, W]
    dir_y = ((y[:, None] - cy + 0.5) / fy).expand(*depths.shape[:-1])
    camera_dirs = torch.stack([dir_x, dir_y, torch.ones_like(dir_x)], dim=-1)  # [..., H, W, 3]
    directions = torch.einsum("...ij,...hwj->...hwi", camtoworlds[..., :3, :3], camera_dirs)
    if not z_depth:
        directions = F.normalize(directions, dim=-1)
    return camtoworlds[..., None, None, :3, 3] + depths * directions
