"""A numpy float64 restatement of exactly what csrc/color_correct.hip computes (the oracle of tests/test_gpu_color_correct.py, held
to the reference's own output by tests/test_color_correct_cpu.py): the reference's color_correct in its normal-equation form, with
the image stored as float32 between iterations, the thresholds compared in float32, and each system solved through the
eigen-decomposition of A^T A with the eigenvalues cut at ``rcond`` times the largest.

It also reports how close any value that decides a mask bit -- an input, a ``ref`` value or an iterate -- comes to a clipping
threshold: two implementations can disagree on a mask bit only where a value lies within their rounding of a threshold, and one
flipped row moves the fit far more than rounding does, so the tests use inputs that keep this distance large."""
import numpy as np

EIG_RCOND = 2.0 ** -40  # the module's constant; test_color_correct_cpu.py holds the two together


def features(x):
    """[P, K] float64 quadratic expansion of float32 pixels [P, n]: x_c x_c' for c' >= c, then x, then 1."""
    x = np.asarray(x, np.float64)
    n = x.shape[1]
    cols = [x[:, c:c + 1] * x[:, c:] for c in range(n)]
    return np.concatenate(cols + [x, np.ones_like(x[:, :1])], axis=1)


def solve(m, r, rcond=EIG_RCOND):
    """The minimum-norm least-squares solution of the normal equations m w = r (m symmetric positive semi-definite)."""
    if not (np.isfinite(m).all() and np.isfinite(r).all()):
        return np.zeros_like(r)
    lam, v = np.linalg.eigh(m)
    keep = (lam > rcond * max(lam.max(), 0.0)) & (lam > 0.0)
    inv = np.zeros_like(lam)
    inv[keep] = 1.0 / lam[keep]
    return v @ (inv * (v.T @ r))


def _threshold_distance(z, lo, hi):
    z = np.asarray(z, np.float64)
    z = z[np.isfinite(z)]
    if z.size == 0:
        return np.inf
    return float(min(np.abs(z - float(lo)).min(), np.abs(z - float(hi)).min()))


def color_correct(img, ref, num_iters=5, eps=0.5 / 255, per_image=False, rcond=EIG_RCOND):
    """(corrected image float32 of img's shape, the smallest distance of an input, a ref value or an iterate that decides a mask
    bit to a threshold).  per_image: every img[i] against ref[i] on its own."""
    img, ref = np.asarray(img, np.float32), np.asarray(ref, np.float32)
    if per_image:
        parts = [color_correct(a, b, num_iters, eps, False, rcond) for a, b in zip(img, ref)]
        return np.stack([p[0] for p in parts]), min(p[1] for p in parts)
    n = img.shape[-1]
    x0, b = img.reshape(-1, n), ref.reshape(-1, n)
    lo, hi = np.float32(eps), np.float32(1.0 - eps)
    unclipped = lambda z: (z >= lo) & (z <= hi)  # noqa: E731
    base = unclipped(x0) & unclipped(b)
    dist = min(_threshold_distance(x0, lo, hi), _threshold_distance(b, lo, hi))
    x = x0
    for it in range(num_iters):
        if it:
            dist = min(dist, _threshold_distance(x, lo, hi))
        a = features(x)
        warp = np.zeros((a.shape[1], n), np.float64)
        for c in range(n):
            rows = base[:, c] & unclipped(x[:, c])
            am = a[rows]
            warp[:, c] = solve(am.T @ am, am.T @ b[rows, c].astype(np.float64), rcond)
        x = np.clip(a @ warp, 0.0, 1.0).astype(np.float32)
    return x.reshape(img.shape), dist
