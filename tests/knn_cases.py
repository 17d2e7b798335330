"""Inputs and row checks shared by tests/test_knn_cpu.py and tests/test_gpu_knn.py: seeded point sets (the smallest shapes at
which the grid k-NN can go wrong), the float64 brute force they are held against, and the bars.

Bars (derived, not measured): sqrt(dx^2 + dy^2 + dz^2) in float32 on float32 inputs has four roundings on d^2 and one on the
root, at most 3.5 unit roundoffs on d (4.5 with a 1-ulp sqrtf); the bar is 2^-21 relative (8 unit roundoffs).  For
``init_scales`` the distance error passes through the logarithm as an absolute error and the result is rounded twice:
|out - ref| <= 2^-21 + 2^-22 |ref|."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSET = os.path.join(ROOT, "gscodec_studio_amd", "assets", "garden_crop.npz")
GOLDEN = os.path.join(ROOT, "tests", "golden", "knn.npz")

KS = (1, 4, 10, 16)
DIST_BAR = 2.0 ** -21
CASES = ("uniform", "outliers", "dups", "plane", "slab", "line", "lattice", "offset_1000", "offset_30000", "tiny", "n_equals_k",
         "single", "same", "garden")


@functools.lru_cache(maxsize=None)
def _points(name):
    rng = np.random.default_rng(CASES.index(name))
    if name == "uniform":  # N not a multiple of the workgroup
        x = rng.uniform(-1.0, 1.0, (1500, 3))
    elif name == "outliers":  # border cells, infinite faces
        x = np.concatenate([rng.standard_normal((1400, 3)), 80.0 * rng.standard_normal((100, 3))])
    elif name == "dups":  # a cell longer than a workgroup, zero distances
        x = np.concatenate([rng.standard_normal((700, 3)), np.repeat(rng.standard_normal((8, 3)), 300, axis=0)])
        x = x[rng.permutation(len(x))]
    elif name == "plane":  # R_z = 1
        x = np.concatenate([rng.uniform(-2.0, 2.0, (1200, 2)), np.zeros((1200, 1))], axis=1)
    elif name == "slab":  # thin cloud
        x = rng.uniform(0.0, 1.0, (1000, 3)) * (10.0, 10.0, 0.001)
    elif name == "line":  # linear cloud
        x = np.concatenate([rng.uniform(-3.0, 3.0, (600, 1)), np.zeros((600, 2))], axis=1)
    elif name == "lattice":  # points on cell faces, exact ties
        g = np.arange(11) * 0.25
        x = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        x = x[rng.permutation(len(x))]
    elif name.startswith("offset_"):  # absolute slack on the face bound
        x = rng.uniform(0.0, 0.05, (800, 3)) + float(name.split("_")[1])
    elif name == "tiny":  # fewer points than a wave
        x = rng.standard_normal((5, 3))
    elif name == "n_equals_k":  # the first K rows are the case for K
        x = rng.standard_normal((16, 3))
    elif name == "single":
        x = rng.standard_normal((1, 3))
    elif name == "same":  # one cell, all distances zero
        x = np.repeat(rng.standard_normal((1, 3)), 40, axis=0)
    elif name == "garden":  # 64 workgroups
        x = np.load(ASSET)["means3d"][:16384]
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def points(name, K=None):
    """float32 [n, 3], read-only; ``n_equals_k`` is cut to its first K rows."""
    x = _points(name)
    return x[:K] if name == "n_equals_k" and K is not None else x


def case_ks(name):
    """The K of KS that the case admits (N >= K), and for ``n_equals_k`` all of them."""
    return [K for K in KS if name == "n_equals_k" or len(_points(name)) >= K]


CASE_KS = [(name, K) for name in CASES for K in case_ks(name)]


def queries_for_outliers():
    """777 queries against ``outliers``, a third of them far outside the box."""
    rng = np.random.default_rng(777)
    q = rng.standard_normal((777, 3))
    q[::3] *= 60.0
    return np.ascontiguousarray(q, dtype=np.float32)


def brute_force(points_, K, queries=None):
    """float64 (dist [m, K], idx [m, K]): the K nearest by direct differences, squared and summed per axis, in query chunks."""
    p = points_.astype(np.float64)
    q = p if queries is None else queries.astype(np.float64)
    dist, idx = np.empty((len(q), K)), np.empty((len(q), K), np.int64)
    for a in range(0, len(q), 256):
        d2 = sum((q[a:a + 256, None, c] - p[None, :, c]) ** 2 for c in range(3))
        near = np.argpartition(d2, K - 1, axis=1)[:, :K] if K < len(p) else np.broadcast_to(np.arange(len(p)), d2.shape)
        dk = np.take_along_axis(d2, near, axis=1)
        by = np.argsort(dk, axis=1, kind="stable")
        dist[a:a + 256], idx[a:a + 256] = np.sqrt(np.take_along_axis(dk, by, axis=1)), np.take_along_axis(near, by, axis=1)
    return dist, idx


@functools.lru_cache(maxsize=None)
def truth(name, K):
    """The brute force of a case, computed once per point set (K = 16, or N where that is less); the callers cut it to their K
    columns.  Call it with the K of the test: only ``n_equals_k`` depends on it."""
    p = points(name, K)
    return _truth(name, len(p))


@functools.lru_cache(maxsize=None)
def _truth(name, n):
    return brute_force(_points(name)[:n], min(16, n))


def check_rows(dist, idx, points_, K, want_dist, queries=None, what=""):
    """The checks on every row: ascending distances, distinct indices in range, each distance within the bar of the float64
    distance to the returned index and of the true j-th smallest distance (``want_dist``, K columns at least).  Returns the
    worst error as a share of the bar."""
    dist, idx = np.asarray(dist), np.asarray(idx)
    q = points_ if queries is None else queries
    m, n = len(q), len(points_)
    assert dist.shape == (m, K) and idx.shape == (m, K) and dist.dtype == np.float32, (what, dist.shape, idx.shape, dist.dtype)
    assert (np.diff(dist, axis=1) >= 0).all(), f"{what}: distances not ascending"
    assert (idx >= 0).all() and (idx < n).all(), f"{what}: index out of range"
    assert (np.diff(np.sort(idx, axis=1), axis=1) > 0).all(), f"{what}: repeated index in a row"
    d64 = dist.astype(np.float64)
    diff = q.astype(np.float64)[:, None, :] - points_.astype(np.float64)[idx]
    to_returned = np.sqrt((diff * diff).sum(axis=2))
    worst = 0.0
    for name, ref in (("distance to the returned index", to_returned), ("j-th smallest distance", want_dist[:, :K])):
        err = np.abs(d64 - ref)
        ratio = float((err[err > 0] / (DIST_BAR * ref[err > 0])).max()) if (err > 0).any() else 0.0
        assert (err <= DIST_BAR * ref).all(), f"{what}: {name}: worst error {ratio:.3f} of the bar"
        worst = max(worst, ratio)
    return worst


def trainer_scales(points_, init_scale, K=4):
    """float64 [n, 3]: the trainers' three lines on the float64 brute force."""
    d, _ = brute_force(points_, K)
    with np.errstate(divide="ignore"):
        s = np.log(np.sqrt((d[:, 1:] ** 2).mean(axis=1)) * init_scale)
    return np.repeat(s[:, None], 3, axis=1)


def case_scales(name, init_scale, K=4):
    """``trainer_scales`` of a whole case, from its cached brute force."""
    d = truth(name, None)[0][:, :K]
    assert d.shape[1] == K
    with np.errstate(divide="ignore"):
        s = np.log(np.sqrt((d[:, 1:] ** 2).mean(axis=1)) * init_scale)
    return np.repeat(s[:, None], 3, axis=1)


def check_scales(out, ref, what=""):
    """|out - ref| <= 2^-21 + 2^-22 |ref|, -inf where the reference has it.  Returns the worst error / bar."""
    out = np.asarray(out, dtype=np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    inf = np.isneginf(ref)
    assert np.array_equal(np.isneginf(out), inf), f"{what}: -inf in other rows than the reference's"
    assert np.isfinite(out[~inf]).all(), f"{what}: non-finite scale"
    err, bar = np.abs(out[~inf] - ref[~inf]), 2.0 ** -21 + 2.0 ** -22 * np.abs(ref[~inf])
    worst = float((err / bar).max()) if err.size else 0.0
    assert (err <= bar).all(), f"{what}: worst error {worst:.3f} of the bar"
    return worst
