"""The grid sort on the GPU: the splat order in front of the image-grid codecs that makes every attribute image smooth (what
the reference takes from the external ``plas`` package), through the kernels of csrc/grid_sort.hip.

    grid_sort_order(features)    -> order int64 [N]: order[p] = the splat at grid position p
    sort_splats_grid(splats)     -> the splats in that order (the signature of ``sort_splats``, plus ``seed``)

``grid_sort_reference`` defines the algorithm in numpy; the kernels return the same permutation element for element.  The
12-bit normalisation of the features is that module's host function ``quantize_features`` (float64, once per call: one copy
of the features to the host and of the integers back, and the place where a non-finite feature is refused); after it the whole
schedule -- per round the blur, the keys, the radix sort and the assignment -- is queued on the current stream without a host
synchronisation."""
from __future__ import annotations

from typing import Dict

import torch
from torch import Tensor

from .. import _backend as B
from . import grid_sort_reference as R


def _stream(t: Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _check_features(features: Tensor) -> int:
    """ValueError for what the kernels do not take, before anything is launched; returns the side length."""
    if not isinstance(features, Tensor) or not features.is_cuda:
        raise ValueError("grid_sort_order: the features must be a device tensor (the grid sort runs on the GPU, no CPU fallback; "
                         "grid_sort_reference.grid_sort_order is the numpy form)")
    if features.dim() != 2 or not features.is_floating_point():
        raise ValueError(f"grid_sort_order: the features must be a floating-point [N, C] tensor, got {features.dtype} {tuple(features.shape)}")
    n, c = features.shape
    if not 1 <= c <= R.MAX_CHANNELS:
        raise ValueError(f"grid_sort_order: 1 <= C <= {R.MAX_CHANNELS} channels, got {c}")
    if n < 1 or n >= 1 << 31:
        raise ValueError(f"grid_sort_order: 1 <= N < 2^31 splats, got {n}")
    return R.side_of(n)  # ValueError when N is not a square


class _Rounds:
    """The device buffers of one sort and the four calls of a round; every stage is reachable on its own for the tests."""

    def __init__(self, q: Tensor, side: int, seed: int):
        n, c = q.shape
        dev = q.device
        self.q, self.side, self.n, self.c, self.seed, self.dev = q, side, n, c, int(seed) & 0xFFFFFFFF, dev
        self.order = torch.empty(n, dtype=torch.int32, device=dev)
        self.order_next = torch.empty(n, dtype=torch.int32, device=dev)
        self.tmp = torch.empty_like(q)
        self.target = torch.empty_like(q)
        self.keys = torch.empty(n, dtype=torch.int64, device=dev)
        self.pos = torch.empty(n, dtype=torch.int32, device=dev)
        self.sorted_keys = torch.empty(n, dtype=torch.int64, device=dev)
        self.sorted_pos = torch.empty(n, dtype=torch.int32, device=dev)
        self.temp = torch.empty(int(B.query("gs_sort_temp_bytes", n)), dtype=torch.uint8, device=dev)  # reused by every round
        self.stream = _stream(q)

    def blur(self, r: int) -> Tensor:
        B.call("gs_gridsort_blur", self.side, self.c, r, B.ptr(self.q), B.ptr(self.order), B.ptr(self.tmp), B.ptr(self.target), self.stream)
        return self.target

    def make_keys(self, b: int, k: int) -> Tensor:
        B.call("gs_gridsort_keys", self.side, b, self.seed, k, B.ptr(self.keys), B.ptr(self.pos), self.stream)
        return self.keys

    def sort(self, bits: int) -> Tensor:
        B.call("gs_sort_pairs_u64_i32", self.n, B.ptr(self.keys), B.ptr(self.pos), B.ptr(self.sorted_keys), B.ptr(self.sorted_pos), 0, bits,
               B.ptr(self.temp), self.temp.numel(), self.stream)
        return self.sorted_pos

    def assign(self) -> Tensor:
        B.call("gs_gridsort_assign", self.side, self.c, B.ptr(self.q), B.ptr(self.target), B.ptr(self.sorted_keys), B.ptr(self.sorted_pos),
               B.ptr(self.order), B.ptr(self.order_next), self.stream)
        self.order, self.order_next = self.order_next, self.order
        return self.order

    def start(self) -> Tensor:
        """order = the stable argsort of hash(seed, 0, p): the keys without blocks, sorted on their 32 bits."""
        self.make_keys(0, 0)
        self.sort(32)
        self.order.copy_(self.sorted_pos)
        return self.order

    def round(self, r: int, k: int) -> Tensor:
        self.blur(r)
        self.make_keys(R.block_side(r), k)
        self.sort(R.key_bits(self.side, r))
        return self.assign()


def _quantize(features: Tensor) -> Tensor:
    """The 12-bit features [N, C] on the features' device (int16 storage: the values are below 4096), through the reference's
    host function (ValueError for a non-finite feature)."""
    f = features.detach()
    q = R.quantize_features((f if f.dtype in (torch.float32, torch.float64) else f.float()).cpu().numpy())
    return torch.from_numpy(q.view("int16")).to(features.device).contiguous()


@torch.no_grad()
def grid_sort_order(features: Tensor, seed: int = 0, decay: float = 0.95, reps: int = 8) -> Tensor:
    """order int64 [N] of the grid sort of ``features`` (device tensor, float [N, C], N a square, C <= 64, finite); equal to
    ``grid_sort_reference.grid_sort_order`` on the same input.  ValueError for anything else, before any launch."""
    side = _check_features(features)
    radii = R.schedule(side, decay, reps)
    q = _quantize(features)
    with torch.cuda.device(features.device):
        rounds = _Rounds(q, side, seed)
        rounds.start()
        for k, r in enumerate(radii, start=1):
            rounds.round(r, k)
        return rounds.order.long()


def sort_splats_grid(splats: Dict[str, Tensor], verbose: bool = True, return_indices: bool = False, sort_with_shN: bool = False,
                     seed: int = 0):
    """``sort_splats`` with the grid sort in the place of PLAS: every attribute except ``shN`` (or every one, with
    ``sort_with_shN``) is flattened to [N, -1] and concatenated, and the splats are returned in the order that makes those
    channels smooth on the square grid (with the indices, on request).  Deterministic for a given ``seed``."""
    n_gs = len(splats["means"])
    keys = [k for k in splats if (sort_with_shN or k != "shN") and splats[k].numel() > 0]
    params = torch.cat([splats[k].detach().reshape(n_gs, -1).float() for k in keys], dim=-1)
    idx = grid_sort_order(params, seed=seed)
    if verbose:
        print(f"Grid sort: {n_gs} splats, {params.shape[1]} channels, {len(R.schedule(R.side_of(n_gs)))} rounds.")
    out = {k: v[idx] for k, v in splats.items()}
    return (out, idx) if return_indices else out
