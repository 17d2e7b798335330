"""Inputs shared by the CPU and the GPU tests of the Gaussian ANS coder."""
import numpy as np

from gscodec_studio_amd.compression import gauss_ans_reference as R


def model_case(n, c, seed):
    """Symbols and a model that visit the corners of the format: every k, mu_q in {0, 1, 2040} next to arbitrary ones, symbols 0
    and 255 under a far-away mean at the narrowest level (frequency 1: the most expensive symbol there is), and otherwise symbols
    drawn near the mean."""
    rng = np.random.default_rng(seed)
    k = (np.arange(n * c).reshape(n, c) % R.N_LEVELS).astype(np.uint8)  # every level, from N * C >= 64 on
    mu_q = rng.integers(0, R.MU_Q_MAX + 1, (n, c)).astype(np.int16)
    mu_q[rng.random((n, c)) < 0.3] = 0
    mu_q[rng.random((n, c)) < 0.1] = 1
    mu_q[rng.random((n, c)) < 0.2] = R.MU_Q_MAX
    sigma = R.level_sigmas()[k]
    sym = np.clip(np.rint(mu_q / 8.0 + sigma * rng.standard_normal((n, c))), 0, 255).astype(np.uint8)
    far = rng.random((n, c)) < 0.1
    sym[far] = np.where(mu_q[far] > 1020, 0, 255)
    k[far & (rng.random((n, c)) < 0.5)] = 0
    return sym, mu_q, k
