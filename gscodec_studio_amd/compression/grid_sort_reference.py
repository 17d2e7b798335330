"""The definition of the grid sort: the order of the splats on the S x S image grid of ``PngCompression`` that makes EVERY
attribute image smooth (the role of the external ``plas`` package, "Self-Organizing Gaussian Grids"), as this project's own
algorithm.  Numpy only, integers only: the kernels of csrc/grid_sort.hip must return the same permutation element for element.

    features float32 [N = S*S, C]  --quantize_features-->  q uint16 [N, C]   (12 bits per channel, float64 on the host, once)
    order[p] = the splat at grid position p = y*S + x;  start order = stable argsort of hash32(seed, 0, p)
    radius r = S//2 - 1, then min(r - 1, floor(r * decay)) after every ``reps`` rounds, while r >= 1   (``schedule``)
    one round (radius r, counter k = 1, 2, ...):
      target  t = box blur of q[order] of width 2r + 1, reflect borders, rows then columns, each pass (2 s + w) // (2 w)
      blocks  side b = max(4, r + 1), shifted by (hash32(seed, k, N) % b, hash32(seed, k, N + 1) % b)
      groups  positions sorted (stable) by block << 32 | hash32(seed, k, p); runs of four inside one block
      assign  the first of the 24 permutations (itertools order, identity first) with the least sum of squared distances
              between the four items and the four targets

Everything random is the counter-based ``hash32``; there is no RNG state."""
from __future__ import annotations

import itertools
from typing import Iterator, List, Tuple

import numpy as np

BITS = 12
QMAX = (1 << BITS) - 1
MAX_CHANNELS = 64
PERMUTATIONS = np.array(list(itertools.permutations(range(4))), dtype=np.int64)  # [24, 4], identity first

GOLD = np.uint32(0x9E3779B9)
MIX1 = np.uint32(0x85EBCA6B)
MIX2 = np.uint32(0xC2B2AE35)
ONE = np.uint32(1)


def hash32(seed, k, p) -> np.ndarray:
    """murmur3's 32-bit finaliser, twice: over seed + (k + 1) * GOLD, then over that ^ p * MIX1.  uint32 arithmetic (wrapping).
    The body is the text of ``gridsort_hash`` in csrc/grid_sort.hip."""
    seed, k, p = (np.atleast_1d(np.asarray(v, dtype=np.uint32)) for v in (seed, k, p))
    x = seed + (k + ONE) * GOLD
    x ^= x >> 16
    x *= MIX1
    x ^= x >> 13
    x *= MIX2
    x ^= x >> 16
    x = x ^ (p * MIX1)
    x ^= x >> 16
    x *= MIX1
    x ^= x >> 13
    x *= MIX2
    x ^= x >> 16
    return x


def quantize_features(features: np.ndarray) -> np.ndarray:
    """float [N, C] -> uint16 [N, C]: round((f - lo) / (hi - lo) * 4095) per channel in float64 (half to even); a constant
    channel gives 0.  The one host function both sides start from."""
    f = np.asarray(features, dtype=np.float64)
    if f.ndim != 2 or not 1 <= f.shape[1] <= MAX_CHANNELS or f.shape[0] < 1:
        raise ValueError(f"features must be [N, C] with 1 <= C <= {MAX_CHANNELS} and N >= 1, got {f.shape}")
    if not np.isfinite(f).all():
        raise ValueError("features must be finite")
    lo, hi = f.min(axis=0), f.max(axis=0)
    span = np.where(hi > lo, hi - lo, 1.0)
    return np.where(hi > lo, np.rint((f - lo) / span * QMAX), 0.0).astype(np.uint16)


def side_of(n: int) -> int:
    s = int(np.sqrt(n))
    s += (s + 1) * (s + 1) <= n
    s -= s * s > n
    if s * s != n:
        raise ValueError(f"{n} splats are not a square grid")
    return s


def schedule(side: int, decay: float = 0.95, reps: int = 8) -> List[int]:
    """The radius of every round, in order."""
    if not (0.0 <= decay < 1.0 and reps >= 1):
        raise ValueError(f"need 0 <= decay < 1 and reps >= 1, got {decay}, {reps}")
    radii, r = [], side // 2 - 1
    while r >= 1:
        radii += [r] * reps
        r = min(r - 1, int(np.floor(r * decay)))
    return radii


def start_order(n: int, seed: int) -> np.ndarray:
    return np.argsort(hash32(seed, 0, np.arange(n)), kind="stable").astype(np.int64)


def _box(g: np.ndarray, r: int, axis: int) -> np.ndarray:
    w = 2 * r + 1
    pad = [(0, 0)] * g.ndim
    pad[axis] = (r, r)
    c = np.cumsum(np.pad(g, pad, mode="reflect"), axis=axis, dtype=np.int64)
    c = np.concatenate([np.zeros_like(np.take(c, [0], axis=axis)), c], axis=axis)
    n = g.shape[axis]
    s = np.take(c, np.arange(w, w + n), axis=axis) - np.take(c, np.arange(n), axis=axis)
    return (2 * s + w) // (2 * w)


def blur_target(q: np.ndarray, order: np.ndarray, side: int, r: int) -> np.ndarray:
    """t int64 [N, C]: the blurred grid of the current order, row pass (along x) first."""
    g = q[order].astype(np.int64).reshape(side, side, -1)
    return _box(_box(g, r, axis=1), r, axis=0).reshape(side * side, -1)


def block_side(r: int) -> int:
    return max(4, r + 1)


def round_keys(side: int, r: int, seed: int, k: int) -> np.ndarray:
    """uint64 [N]: block(p) << 32 | hash32(seed, k, p)."""
    n, b = side * side, block_side(r)
    ox, oy = int(hash32(seed, k, n)[0]) % b, int(hash32(seed, k, n + 1)[0]) % b
    p = np.arange(n, dtype=np.int64)
    block = ((p // side + oy) // b) * (side // b + 2) + ((p % side + ox) // b)
    return (block.astype(np.uint64) << np.uint64(32)) | hash32(seed, k, p).astype(np.uint64)


def key_bits(side: int, r: int) -> int:
    """Populated bits of the keys: 32 of the hash + those of the largest block id."""
    nb = side // block_side(r) + 2
    return 32 + max(1, int(nb * nb - 1).bit_length())


def round_groups(keys: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(positions sorted by key [N], groups [G, 4] of positions that share a block)."""
    pos = np.argsort(keys, kind="stable").astype(np.int64)
    n4 = len(pos) // 4 * 4
    grp = pos[:n4].reshape(-1, 4)
    blk = (keys[grp] >> np.uint64(32)).astype(np.int64)
    return pos, grp[(blk == blk[:, :1]).all(axis=1)]


def assign(q: np.ndarray, t: np.ndarray, order: np.ndarray, groups: np.ndarray) -> np.ndarray:
    """The order after the best-of-24 reassignment inside every group."""
    out = order.copy()
    if len(groups) == 0:
        return out
    a = q[order[groups]].astype(np.int64)  # [G, 4, C] items
    d = ((a[:, :, None, :] - t[groups].astype(np.int64)[:, None, :, :]) ** 2).sum(axis=-1)  # [G, 4 items, 4 targets]
    cost = d[:, np.arange(4)[None, :], PERMUTATIONS].sum(axis=-1)  # [G, 24]
    best = PERMUTATIONS[np.argmin(cost, axis=1)]  # first minimum; item i -> the group's position best[i]
    np.put_along_axis(out, np.take_along_axis(groups, best, axis=1).reshape(-1), order[groups].reshape(-1), axis=0)
    return out


def rounds(q: np.ndarray, seed: int = 0, decay: float = 0.95, reps: int = 8) -> Iterator[Tuple[int, int, np.ndarray, np.ndarray, np.ndarray]]:
    """Yields (k, r, t, order before, order after) for every round; the orders are fresh arrays."""
    side = side_of(len(q))
    order = start_order(len(q), seed)
    for k, r in enumerate(schedule(side, decay, reps), start=1):
        t = blur_target(q, order, side, r)
        _, groups = round_groups(round_keys(side, r, seed, k))
        new = assign(q, t, order, groups)
        yield k, r, t, order, new
        order = new


def grid_sort_order(features: np.ndarray, seed: int = 0, decay: float = 0.95, reps: int = 8) -> np.ndarray:
    """int64 [N]: order[p] = the splat at grid position p."""
    q = quantize_features(features)
    order = start_order(len(q), seed)
    side_of(len(q))
    for *_, order in rounds(q, seed, decay, reps):
        pass
    return order


def round_objective(q: np.ndarray, order: np.ndarray, t: np.ndarray) -> int:
    """sum_p |q[order[p]] - t[p]|^2 for a fixed target t, exact."""
    return int(((q[order].astype(np.int64) - t.astype(np.int64)) ** 2).sum())


def neighbour_metric(q: np.ndarray, order: np.ndarray) -> float:
    """Mean squared difference between 4-neighbours of the grid q[order] (per neighbouring pair, summed over channels)."""
    side = side_of(len(order))
    g = q[order].astype(np.int64).reshape(side, side, -1)
    if side < 2:
        return 0.0
    dx, dy = ((g[:, 1:] - g[:, :-1]) ** 2).sum(), ((g[1:] - g[:-1]) ** 2).sum()
    return float(dx + dy) / (2 * side * (side - 1))
