"""Inputs shared by tests/test_kmeans_cpu.py and tests/test_gpu_kmeans.py, and the float64 Lloyd iteration the fixed-point
algorithm is held against."""
import functools

import numpy as np

ITERS = 6
# (n, w, k) whose fixed-point labels equal the float64 iteration's, six rounds each (seeds 0, 1, 2 in this order)
SEEDED = ((2000, 9, 32), (3000, 45, 64), (1500, 24, 100))

# name -> (n, w, k, k_slices): the smallest shapes at which a kernel can go wrong.  One width per padded width of the assign kernel
# (4, 8, 16, 32, 48, 64), a lane's second point missing (odd n), more than one workgroup (n > 512), k = 1, and slices that do
# not divide k (7 in 2 slices: 4 + 3; 300 in 7: six of 43 and one of 42); k_slices None = the library's choice.
SHAPES = {
    "one_point": (1, 1, 1, None),
    "w1_two_clusters": (63, 1, 2, None),
    "odd_n_k7": (257, 9, 7, None),
    "odd_n_k7_two_slices": (257, 9, 7, 2),
    "w45_k300": (1000, 45, 300, None),
    "w45_k300_one_slice": (1000, 45, 300, 1),
    "w45_k300_seven_slices": (1000, 45, 300, 7),
    "w24_k1024": (4096, 24, 1024, None),
    "w8": (300, 8, 5, None),
    "w64": (300, 64, 5, None),
    "w64_three_slices": (300, 64, 5, 3),
    "k1": (100, 8, 1, None),
}


def seeded(seed, n, w, k):
    """The issue's generator: per-channel scales between 0.02 and 0.5, a start of k distinct rows."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, w)) * rng.uniform(0.02, 0.5, w)).astype(np.float32)
    return x, rng.permutation(n)[:k]


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(x, init, k_slices); the entries of one (n, w, k) share their points and their start."""
    n, w, k, k_slices = SHAPES[name]
    x, init = seeded(n + w + k, n, w, k)
    return x, init, k_slices


def shape_key(name):
    """The first entry of SHAPES with the same (n, w, k): the one whose reference result the others use."""
    return next(other for other, v in SHAPES.items() if v[:3] == SHAPES[name][:3])


def few_distinct():
    """500 rows, only 10 distinct ones, k = 32 from the first 32 rows: equal centroids (the lower index wins) and clusters
    that stay empty."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((10, 9)).astype(np.float32)[rng.integers(0, 10, 500)]
    return x, np.arange(32)


def extremes():
    """Rows of all zeros and of all ones in 64 channels (0 and 2^24 - 1 after the normalisation): the largest distance,
    64 * (2^24 - 1); the third centroid repeats the first."""
    x = np.zeros((130, 64), np.float32)
    x[1::2] = 1.0
    return x, np.array([0, 1, 2])


def constant():
    return np.full((100, 5), 0.7, np.float32), np.array([3, 1, 4, 1])


def blobs(n=600, w=3, k=5, seed=3):
    """k overlapping groups: from this start the eighth assign is the first that changes no label."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-10.0, 10.0, (k, w))
    x = (centres[rng.integers(0, k, n)] + 2.0 * rng.standard_normal((n, w))).astype(np.float32)
    return x, rng.permutation(n)[:k]


def float64_lloyd(x, init, iters):
    """Labels of the last assign and means of the last update of a float64 Lloyd iteration (manhattan distance, first minimum,
    an empty cluster keeps its centroid) from the rows ``init``."""
    x = x.astype(np.float64)
    cent = x[init].copy()
    for _ in range(iters):
        labels = np.abs(x[:, None, :] - cent[None, :, :]).sum(axis=2).argmin(axis=1)
        for j in np.unique(labels):
            cent[j] = x[labels == j].mean(axis=0)
    return cent, labels
