"""The nearest-neighbour kernels (csrc/knn.hip behind gscodec_studio_amd.knn) against their numpy definition (knn_reference) and
a float64 brute force: the built grid element for element, every row of every case of knn_cases within the derived bar, exact
equality where the arithmetic is exact, run-to-run identity, separate queries, the trainers' drop-in and ``init_scales``."""
import functools

import numpy as np
import pytest
import torch

import knn_cases as C
from util import N
from util import T as _T

pytestmark = pytest.mark.gpu


def T(a):
    """A device copy (the cases' arrays are shared and read-only)."""
    return _T(np.array(a))


@functools.lru_cache(maxsize=None)
def _reference_grid(name, K):
    from gscodec_studio_amd import knn_reference as R

    return R.build_grid(C.points(name, K))


@pytest.mark.parametrize("name", C.CASES)
def test_grid_equals_the_numpy_reference(name):
    from gscodec_studio_amd.knn import knn_grid

    for K in ((1, 4, 10, 16) if name == "n_equals_k" else (None,)):
        p = C.points(name, K)
        lo, h, counts, ids, order, starts = _reference_grid(name, K)
        g_lo, g_h, g_counts, g_ids, g_order, g_starts = knn_grid(T(p))
        assert np.array_equal(g_lo, lo) and g_h == h and tuple(g_counts) == tuple(counts), (name, g_lo, lo, g_h, h, g_counts, counts)
        assert g_ids.dtype == g_order.dtype == g_starts.dtype == torch.int64
        assert np.array_equal(N(g_ids), ids), name
        assert np.array_equal(N(g_order), order), name
        assert np.array_equal(N(g_starts), starts), name


@pytest.mark.parametrize("name,K", C.CASE_KS)
def test_rows_against_float64_brute_force(name, K):
    from gscodec_studio_amd.knn import knn_search

    p = C.points(name, K)
    dist, idx = knn_search(T(p), K)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.is_cuda and idx.is_cuda
    worst = C.check_rows(N(dist), N(idx), p, K, C.truth(name, K)[0], what=f"{name} K={K}")
    print(f"{name} K={K}: worst distance error {worst:.3f} of the bar 2^-21")
    if name == "same":
        assert np.array_equal(N(idx), np.broadcast_to(np.arange(K), (len(p), K)))


@pytest.mark.parametrize("K", C.KS)
def test_lattice_equals_the_numpy_reference(K):
    """Coordinates k / 4 with k <= 10: differences, squares and sums are exact in float32 in either rounding order, so the rows --
    with their many exact ties -- are the definition's element for element."""
    from gscodec_studio_amd import knn_reference as R
    from gscodec_studio_amd.knn import knn_search

    p = C.points("lattice")
    want_d, want_i = R.search(p, K, grid=_reference_grid("lattice", None))
    dist, idx = knn_search(T(p), K)
    assert np.array_equal(N(idx), want_i) and np.array_equal(N(dist), want_d)


@pytest.mark.parametrize("name", ["dups", "garden"])
def test_two_calls_are_bit_identical(name):
    from gscodec_studio_amd.knn import init_scales, knn_search

    x = T(C.points(name))
    a, b = knn_search(x, 10), knn_search(x, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    s, t = init_scales(x, 0.3), init_scales(x, 0.3)
    assert torch.equal(s.view(torch.int32), t.view(torch.int32))


@pytest.mark.parametrize("K", [1, 4, 16])
def test_separate_queries(K):
    """777 queries, a third of them outside the box, against ``outliers``."""
    from gscodec_studio_amd.knn import knn_search

    p, q = C.points("outliers"), C.queries_for_outliers()
    dist, idx = knn_search(T(p), K, T(q))
    worst = C.check_rows(N(dist), N(idx), p, K, C.brute_force(p, K, q)[0], queries=q, what=f"queries K={K}")
    print(f"queries K={K}: worst distance error {worst:.3f} of the bar 2^-21")
    none = knn_search(T(p), K, T(q[:0]))
    assert tuple(none[0].shape) == tuple(none[1].shape) == (0, K)


def test_knn_of_a_host_tensor_against_the_golden():
    """The trainers' call: a host tensor in, a host tensor out, within the bar of what the reference's own knn returned."""
    from gscodec_studio_amd.utils import knn

    g = np.load(C.GOLDEN)
    x = torch.from_numpy(g["points"])
    for K in (4, 16):
        out = knn(x, K)
        assert out.device == x.device and out.dtype == x.dtype and tuple(out.shape) == (4096, K)
        want = g[f"dist{K}"].astype(np.float64)
        err = np.abs(out.numpy().astype(np.float64) - want)
        print(f"golden K={K}: worst distance error {(err / (C.DIST_BAR * np.maximum(want, 1e-300))).max():.3f} of the bar")
        assert (err <= C.DIST_BAR * want).all()
    on_device = knn(T(g["points"]))  # a device tensor stays where it is; K defaults to the trainers' 4
    assert on_device.is_cuda and torch.equal(on_device.cpu(), knn(x, 4))


@pytest.mark.parametrize("name,init_scale,K", [("dups", 1.0, 4), ("garden", 0.1, 4), ("uniform", 2.5, 16), ("offset_30000", 1.0, 2),
                                               ("outliers", 1.0, 4), ("tiny", 1.0, 5)])
def test_init_scales_against_the_trainer_lines_in_float64(name, init_scale, K):
    from gscodec_studio_amd.knn import init_scales

    p = C.points(name)
    out = init_scales(T(p), init_scale=init_scale, K=K)
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(p), 3) and out.is_cuda
    ref = C.case_scales(name, init_scale, K)
    if name == "dups":
        assert np.isneginf(ref).sum() == 3 * 8 * 300  # every copy of the eight repeated points: no clamp
    worst = C.check_scales(N(out), ref, f"{name} init_scale={init_scale} K={K}")
    print(f"init_scales {name} K={K}: worst error {worst:.3f} of the bar 2^-21 + 2^-22 |ref|")


def test_a_side_stream_is_honoured():
    """Everything is queued on the caller's stream: launched on a side stream behind a long fill of the input and waited for on
    that stream only, the rows are those of the filled input."""
    from gscodec_studio_amd.knn import init_scales, knn_search

    p = C.points("garden")
    src = T(p)
    x = torch.zeros_like(src)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(20):  # work in front of the copy, on the side stream only
            x.add_(1.0)
        x.copy_(src)
        dist, idx = knn_search(x, 4)
        scales = init_scales(x, 0.5)
    side.synchronize()
    worst = C.check_rows(N(dist), N(idx), p, 4, C.truth("garden", 4)[0], what="side stream")
    assert worst <= 1.0
    C.check_scales(N(scales), C.case_scales("garden", 0.5), "side stream")


def test_device_values_are_refused():
    from gscodec_studio_amd.knn import knn_search

    good = C.points("uniform").copy()
    for row, col, v in ((3, 1, np.nan), (1499, 0, np.inf), (0, 2, -np.inf)):
        bad = good.copy()
        bad[row, col] = v
        with pytest.raises(ValueError, match="finite"):
            knn_search(T(bad), 4)
        with pytest.raises(ValueError, match="queries must be finite"):
            knn_search(T(good), 4, T(bad))
