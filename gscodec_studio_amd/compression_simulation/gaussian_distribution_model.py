"""Multi-resolution hash-grid encoder and the position-conditioned parameter regressor of the Gaussian entropy model.

Counterpart of the reference's ``gsplat/compression_simulation/gaussian_distribution_model.py``: ``STE_binary``,
``STE_multistep``, ``GridEncoder``, ``mix_3D2D_encoding`` and ``hash_based_estimator`` keep the reference's constructors,
defaults, attribute names and registration order, so state dicts load both ways with ``strict=True``.  The reference's
encoder is the CUDA-only ``_gridencoder`` extension; here it is ``csrc/hashgrid.hip`` (``gs_hashgrid_encode_fwd/bwd``):

* ``GridEncoder.forward`` is one launch, ``mix_3D2D_encoding.forward`` is one launch for all four grids (no ``chunk`` /
  ``cat`` of the positions or of the outputs), and the output arrives in its final ``[N, levels * F]`` layout.
* ``STE_binary`` is evaluated inside the kernels on the raw parameter; ``add_noise`` and ``ste_multistep`` are applied in
  torch before the call.
* A coordinate outside ``[0, 1]`` -- or NaN, which the reference lets through into an undefined conversion -- gives zero
  features and no gradient.
* Construction does not call ``.cuda()``: modules are built on the CPU and moved; a forward on CPU tensors raises.

``binary_vxl``, a per-point ``min_level_id``, ``PV``, ``num_dim=1`` and half precision are not built (no caller in the
reference uses them).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor

from .. import _backend as B

use_clamp = True  # STE_multistep clamps to mean +- 15000 Q before rounding (the reference's module-level switch)

_AXES = {"xyz": 0, "xy": 1, "xz": 2, "yz": 3}  # the axis selectors of gs_hashgrid_encode_*
_MAX_LEVELS = 32  # levels per launch


class STE_binary(torch.autograd.Function):
    """sign with sign(0) = +1 (NaN -> 0); the gradient passes where -1 <= input <= 1."""

    @staticmethod
    def forward(ctx, input):
        ctx.save_for_backward(input)
        return (input >= 0).to(input.dtype) - (input < 0).to(input.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        (input,) = ctx.saved_tensors
        return grad_output * ((input >= -1) & (input <= 1)).to(grad_output.dtype)


class STE_multistep(torch.autograd.Function):
    """round(input / Q) * Q inside mean +- 15000 Q, identity gradient."""

    @staticmethod
    def forward(ctx, input, Q, input_mean=None):
        if use_clamp:
            if input_mean is None:
                input_mean = input.mean()
            input_min = input_mean - 15_000 * Q
            input_max = input_mean + 15_000 * Q
            input = torch.clamp(input, min=input_min.detach(), max=input_max.detach())
        return torch.round(input / Q) * Q

    @staticmethod
    def backward(ctx, grad_output):
        return grad_output, None, None


class _Level_table:
    """Host side of one launch: the per-grid lists ``gs_hashgrid_encode_*`` reads (ctypes arrays, built once)."""

    def __init__(self, n_features: int, grids: Sequence[tuple]):
        # grids: (num_dim, axes code, [resolutions], [offsets], rows)
        n = len(grids)
        self.n_grids, self.n_features = n, int(n_features)
        self.num_dim = (ctypes.c_uint32 * n)(*[g[0] for g in grids])
        self.axes = (ctypes.c_uint32 * n)(*[g[1] for g in grids])
        self.n_levels = (ctypes.c_uint32 * n)(*[len(g[2]) for g in grids])
        res = [r for g in grids for r in g[2]]
        off = [o for g in grids for o in g[3]]
        self.resolutions = (ctypes.c_int32 * len(res))(*res)
        self.offsets = (ctypes.c_int32 * len(off))(*off)
        self.rows = (ctypes.c_uint64 * n)(*[g[4] for g in grids])
        self.total_levels = len(res)
        self.output_dim = self.total_levels * self.n_features

    def pointers(self, tensors: Sequence[Optional[Tensor]]):
        return (ctypes.c_void_p * self.n_grids)(*[None if t is None else t.data_ptr() for t in tensors])


def _stream(t: Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


class _grid_encode(torch.autograd.Function):
    """features [N, levels * F] of positions [N, pos_dim] through 1..4 tables (one launch each way)."""

    @staticmethod
    def forward(ctx, pos: Tensor, table: _Level_table, ste_binary: bool, *params: Tensor) -> Tensor:
        if not pos.is_cuda or not all(p.is_cuda for p in params):
            raise RuntimeError("hash-grid encoder: the HIP path needs device tensors (no CPU fallback)")
        if pos.dtype != torch.float32 or any(p.dtype != torch.float32 for p in params):
            raise NotImplementedError("hash-grid encoder: float32 only")
        pos = pos.contiguous()
        params = tuple(p.contiguous() for p in params)
        out = torch.empty((pos.shape[0], table.output_dim), dtype=torch.float32, device=pos.device)
        with torch.cuda.device(pos.device):
            B.call("gs_hashgrid_encode_fwd", pos.shape[0], pos.shape[1], table.n_grids, table.n_features, int(ste_binary),
                   B.ptr(pos), table.pointers(params), table.rows, table.num_dim, table.axes, table.n_levels,
                   table.resolutions, table.offsets, B.ptr(out), _stream(pos))
        ctx.save_for_backward(pos, *params)
        ctx.table, ctx.ste_binary = table, bool(ste_binary)
        return out

    @staticmethod
    def backward(ctx, v_out: Tensor):
        pos, *params = ctx.saved_tensors
        table = ctx.table
        v_out = v_out.contiguous()
        v_pos = torch.empty_like(pos) if ctx.needs_input_grad[0] else None
        v_params = [torch.zeros_like(p) if ctx.needs_input_grad[3 + i] else None for i, p in enumerate(params)]
        with torch.cuda.device(pos.device):
            B.call("gs_hashgrid_encode_bwd", pos.shape[0], pos.shape[1], table.n_grids, table.n_features, int(ctx.ste_binary),
                   B.ptr(pos), table.pointers(params), table.rows, table.num_dim, table.axes, table.n_levels,
                   table.resolutions, table.offsets, B.ptr(v_out), table.pointers(v_params), B.ptr(v_pos), _stream(pos))
        return (v_pos, None, None) + tuple(v_params)


class GridEncoder(nn.Module):
    def __init__(self, num_dim=3, n_features=2, resolutions_list=(16, 23, 32, 46, 64, 92, 128, 184, 256, 368, 512, 736),
                 log2_hashmap_size=19, ste_binary=True, ste_multistep=False, add_noise=False, Q=1):
        super().__init__()
        if num_dim not in (2, 3):
            raise NotImplementedError("GridEncoder: num_dim must be 2 or 3")
        if n_features not in (1, 2, 4):
            raise NotImplementedError("GridEncoder: n_features must be 1, 2 or 4")
        resolutions_list = torch.tensor(resolutions_list).to(torch.int)
        n_levels = resolutions_list.numel()
        if not 1 <= n_levels <= _MAX_LEVELS:
            raise NotImplementedError("GridEncoder: 1..32 levels")

        self.num_dim = num_dim
        self.n_levels = n_levels
        self.n_features = n_features
        self.log2_hashmap_size = log2_hashmap_size
        self.output_dim = n_levels * n_features
        self.ste_binary = ste_binary
        self.ste_multistep = ste_multistep
        self.add_noise = add_noise
        self.Q = Q

        offsets_list = []
        offset = 0
        self.max_params = 2 ** log2_hashmap_size
        for i in range(n_levels):
            resolution = resolutions_list[i].item()
            params_in_level = min(self.max_params, resolution ** num_dim)
            params_in_level = int(np.ceil(params_in_level / 8) * 8)  # rows per level: a multiple of 8
            offsets_list.append(offset)
            offset += params_in_level
        offsets_list.append(offset)
        offsets_list = torch.from_numpy(np.array(offsets_list, dtype=np.int32))
        self.register_buffer("offsets_list", offsets_list)
        self.register_buffer("resolutions_list", resolutions_list)

        self.n_params = offsets_list[-1] * n_features
        self.params = nn.Parameter(torch.empty(offset, n_features))
        self.reset_parameters()
        self.n_output_dims = n_levels * n_features
        self._host = None  # (key, resolutions, offsets): host copies of the two buffers
        self._tables = {}  # (first level, last level + 1) -> _Level_table of this grid alone

    def reset_parameters(self):
        std = 1e-4
        self.params.data.uniform_(-std, std)

    def __repr__(self):
        return (f"GridEncoder: num_dim={self.num_dim} n_levels={self.n_levels} n_features={self.n_features} "
                f"log2_hashmap_size={self.log2_hashmap_size} params={tuple(self.params.shape)} ste_binary={self.ste_binary}")

    def host_lists(self):
        """([resolutions], [offsets]) as Python ints; read back from the buffers once per change (load_state_dict, .to())."""
        key = (self.offsets_list._version, self.offsets_list.data_ptr(), self.resolutions_list._version,
               self.resolutions_list.data_ptr())
        if self._host is None or self._host[0] != key:
            self._host = (key, [int(r) for r in self.resolutions_list.tolist()], [int(o) for o in self.offsets_list.tolist()])
            self._tables = {}
        return self._host[1], self._host[2]

    def host_key(self) -> tuple:
        self.host_lists()
        return self._host[0]

    def grid_spec(self, axes: str, lo: int = 0, hi: Optional[int] = None) -> tuple:
        res, off = self.host_lists()
        hi = self.n_levels if hi is None else hi
        return (self.num_dim, _AXES[axes], res[lo:hi], off[lo:hi + 1], self.params.shape[0])

    def embeddings(self, test_phase: bool = False, outspace_params: Optional[Tensor] = None):
        """-> (table handed to the kernel, whether the kernel applies STE_binary to it)."""
        params = self.params if outspace_params is None else outspace_params
        if self.ste_binary:
            return params, True
        if self.add_noise and not test_phase:
            return params + (torch.rand_like(params) - 0.5) * (1 / self.Q), False
        if self.ste_multistep or (self.add_noise and test_phase):
            return STE_multistep.apply(params, self.Q), False
        return params, False

    def forward(self, inputs, min_level_id=None, max_level_id=None, test_phase=False, outspace_params=None, binary_vxl=None,
                PV=0):
        # inputs: [..., num_dim] in [0, 1]; return: [..., n_levels * n_features]
        if binary_vxl is not None:
            raise NotImplementedError("GridEncoder: binary_vxl is not built")
        if isinstance(min_level_id, Tensor):
            raise NotImplementedError("GridEncoder: a per-point min_level_id is not built")
        prefix_shape = list(inputs.shape[:-1])
        inputs = inputs.reshape(-1, self.num_dim)
        lo = 0 if min_level_id is None else max(int(min_level_id), 0)
        hi = self.n_levels if max_level_id is None else min(int(max_level_id), self.n_levels)
        self.host_lists()
        table = self._tables.get((lo, hi))
        if table is None:
            table = self._tables[(lo, hi)] = _Level_table(self.n_features, [self.grid_spec("xyz" if self.num_dim == 3 else "xy", lo, hi)])
        emb, ste = self.embeddings(test_phase, outspace_params)
        outputs = _grid_encode.apply(inputs, table, ste, emb)
        return outputs.view(prefix_shape + [(hi - lo) * self.n_features])


class mix_3D2D_encoding(nn.Module):
    def __init__(self, n_features, resolutions_list, log2_hashmap_size, resolutions_list_2D, log2_hashmap_size_2D,
                 ste_binary, ste_multistep, add_noise, Q):
        super().__init__()
        kw = dict(n_features=n_features, ste_binary=ste_binary, ste_multistep=ste_multistep, add_noise=add_noise, Q=Q)
        self.encoding_xyz = GridEncoder(num_dim=3, resolutions_list=resolutions_list, log2_hashmap_size=log2_hashmap_size, **kw)
        self.encoding_xy = GridEncoder(num_dim=2, resolutions_list=resolutions_list_2D, log2_hashmap_size=log2_hashmap_size_2D, **kw)
        self.encoding_xz = GridEncoder(num_dim=2, resolutions_list=resolutions_list_2D, log2_hashmap_size=log2_hashmap_size_2D, **kw)
        self.encoding_yz = GridEncoder(num_dim=2, resolutions_list=resolutions_list_2D, log2_hashmap_size=log2_hashmap_size_2D, **kw)
        self.output_dim = (self.encoding_xyz.output_dim + self.encoding_xy.output_dim + self.encoding_xz.output_dim
                           + self.encoding_yz.output_dim)
        if self.output_dim // n_features > _MAX_LEVELS:
            raise NotImplementedError("mix_3D2D_encoding: at most 32 levels in total")
        self._table = None

    def _encoders(self) -> List[tuple]:
        return [("xyz", self.encoding_xyz), ("xy", self.encoding_xy), ("xz", self.encoding_xz), ("yz", self.encoding_yz)]

    def forward(self, x):
        # x: [..., 3] in [0, 1] -> [..., output_dim] = [xyz | xy | xz | yz] features, all four grids in one launch
        prefix_shape = list(x.shape[:-1])
        x = x.reshape(-1, 3)
        encoders = self._encoders()
        key = tuple(e.host_key() for _, e in encoders)
        if self._table is None or self._table[0] != key:
            self._table = (key, _Level_table(self.encoding_xyz.n_features, [e.grid_spec(a) for a, e in encoders]))
        tables = [e.embeddings() for _, e in encoders]
        out = _grid_encode.apply(x, self._table[1], tables[0][1], *[t[0] for t in tables])
        return out.view(prefix_shape + [self.output_dim])


class hash_based_estimator(nn.Module):
    def __init__(self, channel=4):
        super().__init__()
        self.channel = channel
        self.hash_grid = mix_3D2D_encoding(
            n_features=2,
            resolutions_list=(18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514),
            log2_hashmap_size=13,
            resolutions_list_2D=(130, 258, 514, 1026),
            log2_hashmap_size_2D=15,
            ste_binary=True,
            ste_multistep=False,
            add_noise=False,
            Q=1,
        )
        self.mlp_regressor = nn.Sequential(
            nn.Linear(self.hash_grid.output_dim, channel * 5),
            nn.ReLU(True),
            nn.Linear(channel * 5, channel * 2),
        )
        # plain tensors in the reference (not in its state dict): non-persistent buffers, so that they follow .to(device)
        self.register_buffer("bound_min", -100 * torch.ones((1, 3)), persistent=False)
        self.register_buffer("bound_max", 100 * torch.ones((1, 3)), persistent=False)

    def regress(self, x: Tensor) -> Tensor:
        """[N, 3] positions -> the regressor's raw output [N, 2 channel] = [means | scales]."""
        assert len(x.shape) == 2 and x.shape[1] == 3
        x = (x - self.bound_min) / (self.bound_max - self.bound_min)
        return self.mlp_regressor(self.hash_grid(x))

    def forward(self, x):
        out_net = self.regress(x)
        return out_net[:, 0:self.channel], out_net[:, self.channel:2 * self.channel]
