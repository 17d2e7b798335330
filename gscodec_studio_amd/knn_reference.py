"""The exact grid k-NN as numpy code: the definition that csrc/knn.hip executes (``knn.knn_search`` returns the same rows).

    build_grid(points)              -> (lo, h, R, cell_ids, order, cell_starts)
    search(points, K, queries=None) -> (dist float32 [M, K], idx int64 [M, K]), rows ordered by (distance^2, index)

1. Box: per axis the order statistics sorted[floor(0.01 (N - 1))] and sorted[ceil(0.99 (N - 1))] of the float32 coordinates
   (no interpolation: SfM clouds have far outliers, and a bounding box would put almost every point into a few cells).
2. Cell side h (float64) and counts R_a = clamp(ceil(e_a / h), 1, 1024) of the extents e = hi - lo: h is the least side at
   which the cells number at most N / 2 + 8 (found by bisection; never below max(e) / 1024).  The count then is at least
   N / 8 unless an axis sits at 1024 or every extent is zero: one step of h changes it by a factor of at most 4.5, and
   where that exceeds the window's 4 the ``+ 8`` covers it.  An axis thinner than h has one layer, whatever the others need.
3. Cell of a point: c_a = clamp(floor((double(p_a) - lo_a) / h), 0, R_a - 1), id (c_z R_y + c_y) R_x + c_x: border cells
   reach to infinity on their outer side.  ``order`` is the stable sort by id, ``cell_starts`` has one entry per cell + 1.
4. Search, per query in cell c, r = 0, 1, ...: scan the cells at Chebyshev distance exactly r (clipped), keep the K best by
   (d^2, index) with d^2 = (dx dx + dy dy) + dz dz in float32; then b = the least distance from the query to a face of the
   block [c - r, c + r] that is no grid border, from the float64 faces lo + k h, less an absolute slack (the faces are
   exact to 2^-52 of the coordinates; the slack is 2^-40 of them), squared and shrunk by 1 - 2^-20 (float32 d^2 of a point
   beyond the face is at least b^2 (1 - 2^-22)).  Stop when no such face is left, or when the K-th d^2 is BELOW that
   bound: strictly, so that no point outside the block can tie with the K-th and win on its index.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

MAX_K = 16
MAX_CELLS_PER_AXIS = 1024
NO_INDEX = np.iinfo(np.int32).max
SLACK = 2.0 ** -40
SHRINK = 1.0 - 2.0 ** -20


def check_points(who: str, x, name: str = "points") -> np.ndarray:
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 2 or x.shape[1] != 3:
        raise ValueError(f"{who}: the {name} must be a float32 [n, 3] array, got {x.dtype} {x.shape}")
    if x.shape[0] >= 1 << 31:
        raise ValueError(f"{who}: fewer than 2^31 {name}, got {x.shape[0]}")
    if not np.isfinite(x).all():
        raise ValueError(f"{who}: the {name} must be finite")
    return x


def check_k(who: str, K: int, n: int) -> int:
    if not isinstance(K, (int, np.integer)) or not 1 <= K <= MAX_K:
        raise ValueError(f"{who}: 1 <= K <= {MAX_K}, got {K!r}")
    if n < K:
        raise ValueError(f"{who}: {n} points are fewer than K = {K}")
    return int(K)


def box_ranks(n: int) -> Tuple[int, int]:
    """The ranks of the two order statistics that span the box."""
    return math.floor(0.01 * (n - 1)), math.ceil(0.99 * (n - 1))


def box(points: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(lo, hi) float32 [3]."""
    s = np.sort(points, axis=0)
    i0, i1 = box_ranks(len(points))
    return s[i0].copy(), s[i1].copy()


def _counts(e, h: float) -> Tuple[int, int, int]:
    return tuple(min(max(math.ceil(x / h), 1), MAX_CELLS_PER_AXIS) for x in e)


def cell_size(lo, hi, n: int) -> Tuple[float, Tuple[int, int, int]]:
    """(h, (R_x, R_y, R_z)) from the box, in float64 (step 2)."""
    e = [float(np.float64(b) - np.float64(a)) for a, b in zip(lo, hi)]
    top = max(e)
    if not top > 0.0:
        return 1.0, (1, 1, 1)
    most = n // 2 + 8
    fits = lambda h: math.prod(_counts(e, h)) <= most
    a, b = top / MAX_CELLS_PER_AXIS, top  # one cell at h = top
    if fits(a):
        return a, _counts(e, a)
    for _ in range(80):  # to neighbouring doubles: a does not fit, b does
        mid = 0.5 * (a + b)
        if not a < mid < b:
            break
        a, b = (a, mid) if fits(mid) else (mid, b)
    return b, _counts(e, b)


def cell_coords(x: np.ndarray, lo, h: float, R) -> np.ndarray:
    """int64 [n, 3] (step 3)."""
    v = np.floor((x.astype(np.float64) - np.asarray(lo, np.float64)) / np.float64(h))
    return np.clip(v, 0, np.asarray(R, np.float64) - 1).astype(np.int64)


def cell_ids(x: np.ndarray, lo, h: float, R) -> np.ndarray:
    c = cell_coords(x, lo, h, R)
    return (c[:, 2] * R[1] + c[:, 1]) * R[0] + c[:, 0]


def build_grid(points: np.ndarray):
    """(lo float32 [3], h, R, cell_ids int64 [n], order int64 [n], cell_starts int64 [cells + 1])."""
    points = check_points("build_grid", points)
    if len(points) < 1:
        raise ValueError("build_grid: no points")
    lo, hi = box(points)
    h, R = cell_size(lo, hi, len(points))
    ids = cell_ids(points, lo, h, R)
    order = np.argsort(ids, kind="stable")
    starts = np.searchsorted(ids[order], np.arange(R[0] * R[1] * R[2] + 1), side="left")
    return lo, h, R, ids, order, starts


def _ring_runs(c: np.ndarray, r: int, R, starts: np.ndarray):
    """The runs of sorted positions that hold the cells at Chebyshev distance exactly r of the cells ``c`` [a, 3]:
    (owner, first, end) with one entry per non-empty run.  The cells of one x-row are neighbours in the sorted order."""
    owner, first, end = [], [], []
    rows = np.arange(len(c))
    for dz in range(-r, r + 1):
        for dy in range(-r, r + 1):
            z, y = c[:, 2] + dz, c[:, 1] + dy
            ok = (z >= 0) & (z < R[2]) & (y >= 0) & (y < R[1])
            base = (z * R[1] + y) * R[0]
            if max(abs(dz), abs(dy)) == r:
                spans = [(np.maximum(c[:, 0] - r, 0), np.minimum(c[:, 0] + r, R[0] - 1), ok)]
            else:
                spans = [(x, x, ok & (x >= 0) & (x < R[0])) for x in (c[:, 0] - r, c[:, 0] + r)]
            for x0, x1, good in spans:
                a, b = starts[(base + x0)[good]], starts[(base + x1)[good] + 1]
                owner.append(rows[good][b > a]), first.append(a[b > a]), end.append(b[b > a])
    return np.concatenate(owner), np.concatenate(first), np.concatenate(end)


def face_bound(q: np.ndarray, c: np.ndarray, r: int, lo, h: float, R) -> np.ndarray:
    """float64 [a]: the bound of step 4 on the squared distance to anything outside the block; inf where the block is the grid."""
    b = np.full(len(q), np.inf)
    for a in range(3):
        qa, la = q[:, a].astype(np.float64), float(lo[a])
        slack = SLACK * (np.abs(qa) + (abs(la) + R[a] * h))
        k = c[:, a] - r
        b = np.where(k > 0, np.minimum(b, qa - (la + k * h) - slack), b)
        k = c[:, a] + r + 1
        b = np.where(k < R[a], np.minimum(b, (la + k * h) - qa - slack), b)
    b = np.maximum(b, 0.0)
    return b * b * SHRINK


def search(points: np.ndarray, K: int, queries: Optional[np.ndarray] = None, grid=None):
    points = check_points("search", points)
    K = check_k("search", K, len(points))
    q = points if queries is None else check_points("search", queries, "queries")
    lo, h, R, _, order, starts = build_grid(points) if grid is None else grid
    sorted_pts = points[order]
    qc = cell_coords(q, lo, h, R)
    best_d = np.full((len(q), K), np.inf, np.float32)
    best_i = np.full((len(q), K), NO_INDEX, np.int64)
    active, r = np.arange(len(q)), 0
    while active.size:
        owner, first, end = _ring_runs(qc[active], r, R, starts)
        length = end - first
        pos = np.repeat(first - (np.cumsum(length) - length), length) + np.arange(length.sum())
        who = active[np.repeat(owner, length)]
        d = q[who] - sorted_pts[pos]  # float32
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        # the K best of (held, new) per query: every active query holds K entries, so each group has K at least
        who = np.concatenate([np.repeat(active, K), who])
        d2 = np.concatenate([best_d[active].ravel(), d2])
        idx = np.concatenate([best_i[active].ravel(), order[pos]])
        by = np.lexsort((idx, d2, who))
        who, d2, idx = who[by], d2[by], idx[by]
        rank = np.arange(len(who)) - np.searchsorted(who, who, side="left")
        keep = rank < K
        best_d[who[keep], rank[keep]], best_i[who[keep], rank[keep]] = d2[keep], idx[keep]
        bound = face_bound(q[active], qc[active], r, lo, h, R)
        active = active[~(np.isinf(bound) | (best_d[active, K - 1].astype(np.float64) < bound))]
        r += 1
    return np.sqrt(best_d), best_i


def init_scales(points: np.ndarray, init_scale: float = 1.0, K: int = 4) -> np.ndarray:
    """float32 [n, 3]: log(sqrt(mean(d[:, 1:]^2)) * init_scale) per point, the mean and what follows in float64."""
    if K < 2:
        raise ValueError(f"init_scales: K >= 2 (the mean is over the K - 1 neighbours), got {K}")
    d, _ = search(points, K)
    with np.errstate(divide="ignore"):
        s = np.log(np.sqrt((d[:, 1:].astype(np.float64) ** 2).mean(axis=1)) * float(init_scale))
    return np.repeat(s.astype(np.float32)[:, None], 3, axis=1)
