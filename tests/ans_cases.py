"""Inputs and the size bound shared by tests/test_ans_cpu.py and tests/test_gpu_ans.py."""
import numpy as np

DISTRIBUTIONS = ("gaussian", "peaked", "uniform")


def draw(kind, n, channels=1, seed=0):
    """uint8 [n, channels] symbols: a rounded Gaussian with sigma = 12, 90 % one symbol over a uniform rest, uniform."""
    rng = np.random.default_rng([seed, DISTRIBUTIONS.index(kind), n, channels])
    if kind == "gaussian":
        return np.clip(np.rint(rng.normal(128.0, 12.0, (n, channels))), 0, 255).astype(np.uint8)
    if kind == "peaked":
        return np.where(rng.random((n, channels)) < 0.9, 7, rng.integers(0, 256, (n, channels))).astype(np.uint8)
    return rng.integers(0, 256, (n, channels)).astype(np.uint8)


def probabilities(symbols):
    """The reference's _get_prob: bincount / count in float64, stored as float32 [C, 256]."""
    return np.stack([(np.bincount(symbols[:, c], minlength=256) / symbols.shape[0]).astype(np.float32)
                     for c in range(symbols.shape[1])])


def entropy_bytes(symbols):
    """Empirical zeroth-order entropy of every channel, summed, in bytes."""
    total = 0.0
    for c in range(symbols.shape[1]):
        cnt = np.bincount(symbols[:, c], minlength=256)
        cnt = cnt[cnt > 0].astype(np.float64)
        total -= float((cnt * np.log2(cnt / symbols.shape[0])).sum())
    return total / 8.0


def size_bound(symbols, stream_len):
    """file bytes <= 1.01 x the empirical entropy + 8 bytes per stream (state and offset) + 64."""
    n, channels = symbols.shape
    return 1.01 * entropy_bytes(symbols) + 8 * channels * (-(-n // stream_len)) + 64
