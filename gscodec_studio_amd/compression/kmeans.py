"""The K-means codebook on the GPU: Lloyd iterations with the manhattan distance in fixed point (what the reference takes from
``torchpq.clustering.KMeans``), through the kernels of csrc/kmeans.hip.

    kmeans_fit(x, n_clusters)   -> (centroids float32 [k, w], labels int32 [n])
    KMeans(n_clusters, distance="manhattan")   the class the reference's call sites use: fit(x [d, n]) -> labels, .centroids [d, k]

``kmeans_reference`` defines the algorithm in numpy; the kernels return the same labels and centroids element for element.  The
24-bit normalisation is three float64 operations on the data's device (IEEE subtract, divide, multiply and round-to-even give
the bits numpy gives); after it every launch is queued on the current stream, and the only host wait is the 4-byte count of
changed labels per iteration, which ends the loop at a fixed point (the result is the one of all ``iters`` rounds)."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _backend as B
from . import kmeans_reference as R


def _check_points(who: str, x: Tensor) -> Tuple[int, int]:
    """ValueError for what the kernels do not take (on whatever device the tensor lives); returns (n, w)."""
    if not isinstance(x, Tensor) or x.dim() != 2 or not x.is_floating_point():
        raise ValueError(f"{who}: the points must be a floating-point [n, w] tensor, got "
                         f"{(x.dtype, tuple(x.shape)) if isinstance(x, Tensor) else type(x).__name__}")
    n, w = x.shape
    if not 1 <= w <= R.MAX_CHANNELS:
        raise ValueError(f"{who}: 1 <= w <= {R.MAX_CHANNELS} channels, got {w}")
    if n < 1 or n >= 1 << 31:
        raise ValueError(f"{who}: 1 <= n < 2^31 points, got {n}")
    return n, w


def _check_device(who: str, x: Tensor) -> None:
    if not x.is_cuda:
        raise RuntimeError(f"{who}: the points must be a device tensor (the clustering runs on the GPU, no CPU fallback; "
                           "kmeans_reference.kmeans_fit is the numpy form)")


def _range_of(who: str, x: Tensor) -> Tuple[float, float]:
    """(lo, hi) of all of x in float64: one read-back, and the place where a non-finite value is refused (a NaN or an
    infinity anywhere shows in the minimum or the maximum)."""
    lo, hi = torch.stack([x.min(), x.max()]).double().tolist()
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"{who}: the points must be finite")
    return lo, hi


def _quantize(x: Tensor, lo: float, hi: float) -> Tensor:
    """int32 [w, n] (channel-major): rint((x - lo) / (hi - lo) * QMAX) in float64 on the device, zeros for hi == lo.  The
    divisor is a device tensor: a true division, not a product with the reciprocal.  Values outside [lo, hi] (``predict`` on
    other data) are clamped to the ends."""
    if hi == lo:
        return torch.zeros((x.shape[1], x.shape[0]), dtype=torch.int32, device=x.device)
    span = torch.tensor(hi - lo, dtype=torch.float64, device=x.device)
    q = torch.round((x.detach().double() - lo) / span * float(R.QMAX)).clamp_(0.0, float(R.QMAX))
    return q.to(torch.int32).t().contiguous()


def _check_slices(k_slices: Optional[int], k: int) -> None:
    if k_slices is not None and not 1 <= int(k_slices) <= min(k, 65535):
        raise ValueError(f"kmeans_fit: 1 <= k_slices <= min(k, 65535), got {k_slices} for k = {k}")


def _slices(k_slices: Optional[int], n: int, w: int, k: int) -> int:
    return int(B.query("gs_kmeans_default_slices", n, w, k)) if k_slices is None else int(k_slices)


class _Steps:
    """The device buffers of one clustering and its two calls; each is reachable on its own for the tests.  ``q_t`` int32
    [w, n]; ``cent`` int32 [k, wp], the padded channels zero; ``labels`` int32 [n], -1 before the first assign."""

    def __init__(self, q_t: Tensor, cent_rows: Tensor, k_slices: int):
        self.w, self.n = q_t.shape
        self.k = int(cent_rows.shape[0])
        dev = q_t.device
        self.q_t, self.k_slices = q_t, int(k_slices)
        self.wp = int(B.query("gs_kmeans_padded_width", self.w))
        self.cent = torch.zeros((self.k, self.wp), dtype=torch.int32, device=dev)
        self.cent[:, :self.w] = cent_rows
        self.labels = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        self.n_changed = torch.zeros(1, dtype=torch.int32, device=dev)
        self.keys = torch.empty(self.n if self.k_slices > 1 else 0, dtype=torch.int64, device=dev)
        self.sums = torch.empty((self.k, self.w), dtype=torch.int64, device=dev)
        self.counts = torch.empty(self.k, dtype=torch.int32, device=dev)
        self.stream = B.current_stream(dev)

    def assign(self) -> Tensor:
        B.call("gs_kmeans_assign", self.n, self.w, self.k, B.ptr(self.q_t), B.ptr(self.cent), self.k_slices,
               B.ptr(self.keys) if self.k_slices > 1 else None, B.ptr(self.labels), B.ptr(self.n_changed), self.stream)
        return self.labels

    def update(self) -> Tensor:
        B.call("gs_kmeans_update", self.n, self.w, self.k, B.ptr(self.q_t), B.ptr(self.labels), B.ptr(self.sums), B.ptr(self.counts),
               B.ptr(self.cent), self.stream)
        return self.cent[:, :self.w]

    def run(self, iters: int) -> int:
        """max(iters, 1) rounds of assign then update, ended early once an assign changed no label: the update that would
        follow recomputes the centroids it started from.  Returns the number of assigns."""
        for it in range(max(int(iters), 1)):
            self.assign()
            if it > 0 and int(self.n_changed.item()) == 0:
                return it + 1
            self.update()
        return max(int(iters), 1)


def _dequantize(cent: Tensor, lo: float, hi: float) -> Tensor:
    return (lo + cent.double() * ((hi - lo) / R.QMAX)).float()


def _check_init(init_indices, n: int, k: int) -> Optional[np.ndarray]:
    """The given start as int64 [k] on the host (ValueError unless k integers in [0, n)); None stays None."""
    if init_indices is None:
        return None
    idx = init_indices.detach().cpu().numpy() if isinstance(init_indices, Tensor) else np.asarray(init_indices)
    if idx.ndim != 1 or idx.shape[0] != k or idx.dtype.kind not in "iu":
        raise ValueError(f"kmeans_fit: init_indices must be {k} integers, got {idx.dtype} {idx.shape}")
    if int(idx.min()) < 0 or int(idx.max()) >= n:
        raise ValueError(f"kmeans_fit: init_indices must lie in [0, {n})")
    return idx.astype(np.int64)


def _start(init: Optional[np.ndarray], n: int, k: int, seed: int, device) -> Tensor:
    """int64 [k] on the device: the given start, or ``kmeans_encode``'s seeded one."""
    if init is not None:
        return torch.from_numpy(init).to(device)
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randperm(n, device=device, generator=g)[:k]


def _fit(x: Tensor, n_clusters: int, iters: int, seed: int, init_indices, k_slices: Optional[int]):
    n, w = _check_points("kmeans_fit", x)
    if int(n_clusters) < 1:
        raise ValueError(f"kmeans_fit: n_clusters >= 1, got {n_clusters}")
    k = min(int(n_clusters), n)
    if k > R.MAX_CLUSTERS:
        raise ValueError(f"kmeans_fit: at most 2^20 clusters, got {k}")
    _check_slices(k_slices, k)
    lo, hi = _range_of("kmeans_fit", x)
    init = _check_init(init_indices, n, k)
    _check_device("kmeans_fit", x)
    with torch.cuda.device(x.device):
        q_t = _quantize(x, lo, hi)
        steps = _Steps(q_t, q_t[:, _start(init, n, k, seed, x.device)].t(), _slices(k_slices, n, w, k))
        n_iter = steps.run(iters)
    return steps, lo, hi, n_iter


@torch.no_grad()
def kmeans_fit(x: Tensor, n_clusters: int, iters: int = 10, seed: int = 0, init_indices=None, k_slices: Optional[int] = None
               ) -> Tuple[Tensor, Tensor]:
    """(centroids float32 [k, w], labels int32 [n]) of ``x`` (device tensor, float [n, w], w <= 64, finite), k = min(n_clusters,
    n) <= 2^20; equal to ``kmeans_reference.kmeans_fit`` from the same start.  The default start is ``kmeans_encode``'s:
    ``randperm(n)[:k]`` of a device generator seeded with ``seed``.  ``k_slices`` forces the number of centroid slices of the
    assignment (default: chosen from the shape); the result does not depend on it.  ValueError for anything the kernels do not take, then
    RuntimeError for a host tensor, before any launch."""
    steps, lo, hi, _ = _fit(x, n_clusters, iters, seed, init_indices, k_slices)
    return _dequantize(steps.cent[:, :steps.w], lo, hi), steps.labels


class KMeans:
    """``torchpq.clustering.KMeans`` as the reference's codecs use it: ``KMeans(n_clusters, distance="manhattan", verbose=...)``,
    ``fit(x [d, n]) -> labels int64 [n]``, ``.centroids`` float32 [d, k]; ``predict(x [d, m])`` is one assignment against the
    stored centroids, on the grid of the fitted data (values outside its range are clamped).  Deterministic for a ``seed``."""

    def __init__(self, n_clusters: int, distance: str = "manhattan", max_iter: int = 10, seed: int = 0, verbose: bool = False):
        if distance != "manhattan":
            raise NotImplementedError(f"KMeans: distance {distance!r}; the kernels implement \"manhattan\"")
        self.n_clusters, self.distance, self.max_iter, self.seed, self.verbose = int(n_clusters), distance, int(max_iter), int(seed), verbose
        self.centroids: Optional[Tensor] = None
        self.n_iter_ = 0
        self._cent: Optional[Tensor] = None
        self._range = (0.0, 0.0)

    @torch.no_grad()
    def fit(self, x: Tensor) -> Tensor:
        if isinstance(x, Tensor) and x.dim() == 2:
            x = x.t()
        steps, lo, hi, self.n_iter_ = _fit(x, self.n_clusters, self.max_iter, self.seed, None, None)
        self._cent, self._range = steps.cent[:, :steps.w].clone(), (lo, hi)
        self.centroids = _dequantize(self._cent, lo, hi).t().contiguous()
        if self.verbose:
            print(f"KMeans: {steps.n} points, {steps.k} clusters, {self.n_iter_} assignment(s).")
        return steps.labels.long()

    @torch.no_grad()
    def predict(self, x: Tensor) -> Tensor:
        if self._cent is None:
            raise RuntimeError("KMeans.predict: call fit first")
        if isinstance(x, Tensor) and x.dim() == 2:
            x = x.t()
        n, w = _check_points("KMeans.predict", x)
        if w != self._cent.shape[1]:
            raise ValueError(f"KMeans.predict: {w} channels, fitted with {self._cent.shape[1]}")
        _range_of("KMeans.predict", x)
        _check_device("KMeans.predict", x)
        with torch.cuda.device(x.device):
            steps = _Steps(_quantize(x, *self._range), self._cent, _slices(None, n, w, int(self._cent.shape[0])))
            return steps.assign().long()
