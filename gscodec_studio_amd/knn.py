"""Exact k nearest neighbours of 3-D points on the GPU, through the kernels of csrc/knn.hip: what the reference's trainers take
from ``examples/utils.py:knn`` (a copy to the host, sklearn's ``NearestNeighbors`` on one core, a copy back) to size their
initial splats.

    knn(x, K=4)                           -> distances [N, K], the drop-in (``from gscodec_studio_amd.utils import knn``)
    knn_search(points, K, queries=None)   -> (dist float32 [M, K], idx int64 [M, K]), rows ordered by (distance^2, index)
    init_scales(points, init_scale, K=4)  -> [N, 3] log scales: trainer lines 356-358 in one call, no [N, K] tensor
    knn_grid(points)                      -> (lo, h, R, cell_ids, order, cell_starts), the built grid

``knn_reference`` defines the algorithm in numpy; the kernels return its rows.  One host wait per call: the read-back of the
box (two order statistics per axis from a device sort) together with the extremes that show a non-finite coordinate; the cell
size is formed on the host from those values by the reference's own ``cell_size``.  Everything after it -- cell ids, the
library's radix sort, the sorted copy, ``cell_starts``, the search -- is queued on the current stream."""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _backend as B
from . import knn_reference as R

__all__ = ["knn", "knn_search", "init_scales", "knn_grid"]


def _check_xyz(who: str, x, name: str = "points") -> int:
    if not isinstance(x, Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{who}: the {name} must be a float32 [n, 3] tensor, got "
                         f"{(x.dtype, tuple(x.shape)) if isinstance(x, Tensor) else type(x).__name__}")
    if x.shape[0] >= 1 << 31:
        raise ValueError(f"{who}: fewer than 2^31 {name}, got {x.shape[0]}")
    return int(x.shape[0])


def _check_device(who: str, x: Tensor) -> None:
    if not x.is_cuda:
        raise RuntimeError(f"{who}: device tensors only (the search runs on the GPU, no CPU fallback; knn_reference.search is "
                           "the numpy form)")


def _check_host_values(who: str, x: Tensor, name: str) -> None:
    """A host tensor's non-finite coordinate is refused at once (a device tensor's: with the box, in ``_Grid``)."""
    if not x.is_cuda and not bool(torch.isfinite(x).all()):
        raise ValueError(f"{who}: the {name} must be finite")


class _Grid:
    """The grid of one point set on its device and the calls that build and search it; every stage is reachable on its own for
    the tests.  ``lo`` / ``h`` / ``R`` host values; ``cell_ids`` int64 [n]; ``order`` int32 [n]; ``sorted`` float32 [n, 4];
    ``cell_starts`` int32 [cells + 1]."""

    def __init__(self, who: str, points: Tensor, queries: Optional[Tensor] = None):
        pts = points.detach().contiguous()
        self.n, self.dev, self.pts = int(pts.shape[0]), pts.device, pts
        self.stream = B.current_stream(self.dev)
        # the box and the finite check in ONE read-back: a NaN sorts last and an infinity to an end, so the ends of the sorted
        # columns show either
        s = pts.t().contiguous().sort(dim=1).values
        i0, i1 = R.box_ranks(self.n)
        look = [s[:, [0, self.n - 1, i0, i1]].t()]
        if queries is not None and queries.shape[0]:
            look.append(torch.stack([queries.min(dim=0).values, queries.max(dim=0).values]))
        v = torch.cat(look).cpu()
        if not bool(torch.isfinite(v[:2]).all()):
            raise ValueError(f"{who}: the points must be finite")
        if not bool(torch.isfinite(v[4:]).all()):
            raise ValueError(f"{who}: the queries must be finite")
        self.lo = v[2].numpy().copy()
        self.h, self.R = R.cell_size(self.lo, v[3].numpy(), self.n)
        self.ncells = self.R[0] * self.R[1] * self.R[2]
        # the grid as the entry points take it: lo and h as four float64 in host memory, then the three counts
        self._box = ((ctypes.c_double * 4)(*(float(a) for a in self.lo), float(self.h)),) + tuple(int(r) for r in self.R)
        self.cell_ids, self.order, sorted_ids = self._sorted_by_cell(pts)
        self.sorted = torch.empty((self.n, 4), dtype=torch.float32, device=self.dev)
        self.cell_starts = torch.empty(self.ncells + 1, dtype=torch.int32, device=self.dev)
        B.call("gs_knn_finish_grid", self.n, self.ncells, B.ptr(pts), B.ptr(sorted_ids), B.ptr(self.order), B.ptr(self.sorted),
               B.ptr(self.cell_starts), self.stream)

    def _sorted_by_cell(self, xyz: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        """(cell ids int64 [m], the stable order by id int32 [m], the ids in that order) of any points in this grid."""
        m = int(xyz.shape[0])
        ids = torch.empty(m, dtype=torch.int64, device=self.dev)
        iota = torch.empty(m, dtype=torch.int32, device=self.dev)
        B.call("gs_knn_cells", m, B.ptr(xyz), *self._box, B.ptr(ids), B.ptr(iota), self.stream)
        bits = (self.ncells - 1).bit_length()
        if bits == 0:  # one cell: the pairs are in order
            return ids, iota, ids
        sorted_ids, order = torch.empty_like(ids), torch.empty_like(iota)
        temp = torch.empty(int(B.query("gs_sort_temp_bytes", m)), dtype=torch.uint8, device=self.dev)
        B.call("gs_sort_pairs_u64_i32", m, B.ptr(ids), B.ptr(iota), B.ptr(sorted_ids), B.ptr(order), 0, bits, B.ptr(temp), temp.numel(),
               self.stream)
        return ids, order, sorted_ids

    def sorted_queries(self, queries: Tensor) -> Tensor:
        """float32 [m, 4]: the queries in the order of their cells, each with its row in w."""
        q = queries.detach().contiguous()
        _, order, _ = self._sorted_by_cell(q)
        out = torch.empty((q.shape[0], 4), dtype=torch.float32, device=self.dev)
        B.call("gs_knn_finish_grid", int(q.shape[0]), 0, B.ptr(q), None, B.ptr(order), B.ptr(out), None, self.stream)
        return out

    def search(self, K: int, sorted_queries: Optional[Tensor] = None, rows: bool = True, init_scale: Optional[float] = None):
        """(dist, idx, log_scales): the rows and / or the log scales of the sorted queries (default: the points themselves)."""
        q = self.sorted if sorted_queries is None else sorted_queries
        m = int(q.shape[0])
        dist = torch.empty((m, K), dtype=torch.float32, device=self.dev) if rows else None
        idx = torch.empty((m, K), dtype=torch.int64, device=self.dev) if rows else None
        scales = torch.empty((m, 3), dtype=torch.float32, device=self.dev) if init_scale is not None else None
        B.call("gs_knn_search", self.n, m, K, B.ptr(self.sorted), B.ptr(self.cell_starts), B.ptr(q), *self._box, B.ptr(dist), B.ptr(idx),
               B.ptr(scales), float(init_scale or 0.0), self.stream)
        return dist, idx, scales


def _check_k(who: str, K, n: int) -> int:
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= R.MAX_K:
        raise ValueError(f"{who}: 1 <= K <= {R.MAX_K}, got {K!r}")
    if n < K:
        raise ValueError(f"{who}: {n} points are fewer than K = {K}")
    return K


def _check(who: str, points: Tensor, K: int, queries: Optional[Tensor] = None) -> None:
    """Every refusal but one, in the order ValueError (shapes, K, a host tensor's values), RuntimeError (a host tensor); a device
    tensor's non-finite value is the ValueError of ``_Grid``'s one read-back, before any launch of this library."""
    n = _check_xyz(who, points)
    if queries is not None:
        _check_xyz(who, queries, "queries")
    _check_k(who, K, n)
    _check_host_values(who, points, "points")
    if queries is not None:
        _check_host_values(who, queries, "queries")
    _check_device(who, points)
    if queries is not None:
        _check_device(who, queries)
        if queries.device != points.device:
            raise ValueError(f"{who}: points on {points.device}, queries on {queries.device}")


@torch.no_grad()
def knn_search(points: Tensor, K: int, queries: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(dist float32 [M, K], idx int64 [M, K]): the K nearest of ``points`` (device tensor, float32 [N, 3], finite, N >= K,
    1 <= K <= 16) to every query (default: the points themselves, each its own first neighbour unless a duplicate with a lower
    index ties).  Rows ascend by (float32 squared distance, index); bit-identical from run to run.  ValueError for anything
    refused, RuntimeError for host tensors, before any launch."""
    _check("knn_search", points, K, queries)
    with torch.cuda.device(points.device):
        g = _Grid("knn_search", points, queries)
        if queries is not None and queries.shape[0] == 0:
            return (torch.empty((0, K), dtype=torch.float32, device=g.dev), torch.empty((0, K), dtype=torch.int64, device=g.dev))
        dist, idx, _ = g.search(K, None if queries is None else g.sorted_queries(queries))
        return dist, idx


@torch.no_grad()
def knn(x: Tensor, K: int = 4) -> Tensor:
    """Drop-in for the trainers' ``knn`` (reference examples/utils.py:142): euclidean distances [N, K] from every point to its K
    nearest points of the same set, itself included, ascending, with the dtype and device of ``x`` (float32 [N, 3]).  A host
    tensor is copied to the current GPU and the result back -- the mirror image of the reference's round trip; without a GPU
    that is a RuntimeError."""
    n = _check_xyz("knn", x)
    _check_k("knn", K, n)
    if x.is_cuda:
        return knn_search(x, K)[0]
    _check_host_values("knn", x, "points")
    if not torch.cuda.is_available():
        raise RuntimeError("knn: no GPU (the search runs on the GPU, no CPU fallback; knn_reference.search is the numpy form)")
    return knn_search(x.cuda(), K)[0].to(x.device)


@torch.no_grad()
def init_scales(points: Tensor, init_scale: float = 1.0, K: int = 4) -> Tensor:
    """float32 [N, 3]: ``log(sqrt(mean(knn(points, K)[:, 1:] ** 2)) * init_scale)`` in every column -- the log scales the
    trainers start from -- out of the search kernel's epilogue, from the squared distances.  ``points`` as for ``knn_search``,
    2 <= K <= 16.  A point with K - 1 exact duplicates gets -inf, as in the reference: there is no clamp."""
    if isinstance(K, int) and not isinstance(K, bool) and K == 1:
        raise ValueError("init_scales: K >= 2 (the mean is over the K - 1 neighbours)")
    if isinstance(init_scale, bool) or not isinstance(init_scale, (int, float)) or not math.isfinite(init_scale):
        raise ValueError(f"init_scales: init_scale must be a finite number, got {init_scale!r}")
    _check("init_scales", points, K)
    with torch.cuda.device(points.device):
        return _Grid("init_scales", points).search(K, rows=False, init_scale=float(init_scale))[2]


@torch.no_grad()
def knn_grid(points: Tensor):
    """(lo float32 [3] host array, h float, R (rx, ry, rz), cell_ids int64 [N], order int64 [N], cell_starts int64 [cells + 1]):
    the grid the search walks, as ``knn_reference.build_grid`` returns it (the last three on the points' device)."""
    _check("knn_grid", points, 1)
    with torch.cuda.device(points.device):
        g = _Grid("knn_grid", points)
        return g.lo, g.h, g.R, g.cell_ids, g.order.long(), g.cell_starts.long()
