"""The definition of the K-means codebook of the higher SH bands: Lloyd iterations with the manhattan distance (the role of
``torchpq.clustering.KMeans`` in the reference's shN codec), as this project's own algorithm.  Numpy only, and after one float64
normalisation integers only: no result depends on a summation order, so the kernels of csrc/kmeans.hip must return the same
labels and centroids element for element.

    x float [n, w]  --quantize-->  q int32 [n, w] in [0, 2^24 - 1]   (lo, hi = the scalar min / max of all of x, float64)
    assign   d(i, j) = sum_c |q[i, c] - cent[j, c]|  (w <= 64: d < 2^30);  label[i] = the lowest j with the least d(i, j)
    update   cent[j, c] = (2 s + cnt) // (2 cnt), s = the int64 sum over the members, cnt their number (round half up);
             a cluster without members keeps its centroid
    fit      cent = q[init_indices]; ``iters`` x (assign, update); the labels of the last assign, the centroids of the last update
    dequantize  lo + cent * ((hi - lo) / (2^24 - 1)) in float64, then float32"""
from __future__ import annotations

from typing import Tuple

import numpy as np

BITS = 24
QMAX = (1 << BITS) - 1
MAX_CHANNELS = 64
MAX_CLUSTERS = 1 << 20


def quantize(x: np.ndarray) -> Tuple[np.ndarray, float, float]:
    """float [n, w] -> (q int32 [n, w], lo, hi): rint((x - lo) / (hi - lo) * QMAX) in float64; hi == lo gives zeros."""
    f = np.asarray(x, dtype=np.float64)
    if f.ndim != 2 or not 1 <= f.shape[1] <= MAX_CHANNELS or f.shape[0] < 1:
        raise ValueError(f"x must be [n, w] with 1 <= w <= {MAX_CHANNELS} and n >= 1, got {f.shape}")
    if not np.isfinite(f).all():
        raise ValueError("x must be finite")
    lo, hi = float(f.min()), float(f.max())
    if hi == lo:
        return np.zeros(f.shape, np.int32), lo, hi
    return np.rint((f - lo) / (hi - lo) * QMAX).astype(np.int32), lo, hi


def assign(q: np.ndarray, cent: np.ndarray, chunk_elements: int = 1 << 24) -> np.ndarray:
    """labels int32 [n]; chunked over the points so that the [chunk, k, w] differences stay small (argmin: the first minimum).
    32-bit integers hold everything: a difference is below 2^24 and a distance below 2^30."""
    q, cent = q.astype(np.int32), cent.astype(np.int32)
    labels = np.empty(q.shape[0], np.int32)
    chunk = max(1, chunk_elements // (cent.shape[0] * q.shape[1]))
    for s in range(0, q.shape[0], chunk):
        labels[s:s + chunk] = np.abs(q[s:s + chunk, None, :] - cent[None, :, :]).sum(axis=2, dtype=np.int32).argmin(axis=1)
    return labels


def update(q: np.ndarray, labels: np.ndarray, cent: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(the new centroids int32 [k, w], counts int64 [k])."""
    k = cent.shape[0]
    sums = np.zeros(cent.shape, np.int64)
    np.add.at(sums, labels, q.astype(np.int64))
    cnt = np.bincount(labels, minlength=k).astype(np.int64)
    full = cnt > 0
    out = cent.astype(np.int32).copy()
    out[full] = ((2 * sums[full] + cnt[full, None]) // (2 * cnt[full, None])).astype(np.int32)
    return out, cnt


def fit_quantized(q: np.ndarray, init_indices: np.ndarray, iters: int) -> Tuple[np.ndarray, np.ndarray]:
    """(cent int32 [k, w], labels int32 [n]) after max(iters, 1) rounds from cent = q[init_indices], none of them skipped."""
    cent = q[np.asarray(init_indices, dtype=np.int64)].astype(np.int32)
    for _ in range(max(int(iters), 1)):
        labels = assign(q, cent)
        cent, _ = update(q, labels, cent)
    return cent, labels


def dequantize(cent: np.ndarray, lo: float, hi: float) -> np.ndarray:
    return (lo + cent.astype(np.float64) * ((hi - lo) / QMAX)).astype(np.float32)


def kmeans_fit(x: np.ndarray, init_indices: np.ndarray, iters: int = 10) -> Tuple[np.ndarray, np.ndarray]:
    """(centroids float32 [k, w], labels int32 [n]): what ``compression.kmeans.kmeans_fit`` returns for the same start."""
    q, lo, hi = quantize(x)
    cent, labels = fit_quantized(q, init_indices, iters)
    return dequantize(cent, lo, hi), labels
