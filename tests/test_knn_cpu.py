"""The grid k-NN as its numpy definition states it (gscodec_studio_amd.knn_reference): exact rows against a float64 brute force on
every case of knn_cases, the cell-count property, the golden recorded from the reference's own ``knn``, and what the GPU driver
refuses before it launches anything."""
import numpy as np
import pytest
import torch

import knn_cases as C

from gscodec_studio_amd import knn_reference as R


@pytest.mark.parametrize("name,K", C.CASE_KS)
def test_reference_rows_against_float64_brute_force(name, K):
    p = C.points(name, K)
    dist, idx = R.search(p, K)
    worst = C.check_rows(dist, idx, p, K, C.truth(name, K)[0], what=f"{name} K={K}")
    print(f"{name} K={K}: worst distance error {worst:.3f} of the bar 2^-21")
    if name == "same":
        assert np.array_equal(idx, np.broadcast_to(np.arange(K), idx.shape))


def test_reference_separate_queries():
    p, q = C.points("outliers"), C.queries_for_outliers()
    for K in (4, 16):
        dist, idx = R.search(p, K, q)
        C.check_rows(dist, idx, p, K, C.brute_force(p, K, q)[0], queries=q, what=f"queries K={K}")


@pytest.mark.parametrize("name", C.CASES)
def test_cell_count_stays_in_its_window(name):
    """N / 8 <= cells <= N / 2 + 8 whatever the aspect ratio.  The lower end needs something to divide: a box without any extent
    (``same``, ``single``, one point of ``n_equals_k``) is one cell, as the case table says of ``same``; no case reaches the
    1024 cells per axis that would cap it from above."""
    for K in C.case_ks(name):
        p = C.points(name, K)
        lo, hi = R.box(p)
        h, counts = R.cell_size(lo, hi, len(p))
        cells = counts[0] * counts[1] * counts[2]
        assert all(1 <= r <= R.MAX_CELLS_PER_AXIS for r in counts) and h > 0
        assert cells <= len(p) // 2 + 8, (name, counts)
        if (hi > lo).any():
            assert cells >= len(p) / 8, (name, counts)
            assert max(counts) < R.MAX_CELLS_PER_AXIS
        else:
            assert counts == (1, 1, 1)
        for a in range(3):  # a degenerate axis has one layer
            if hi[a] == lo[a]:
                assert counts[a] == 1


def test_thin_and_flat_clouds_collapse_their_axes():
    for name in ("plane", "slab", "line"):
        counts = R.build_grid(C.points(name))[2]
        assert counts[2] == 1 and (counts[1] == 1) == (name == "line"), (name, counts)


def test_box_is_two_order_statistics():
    p = C.points("outliers")
    lo, hi = R.box(p)
    s = np.sort(p, axis=0)
    assert R.box_ranks(1500) == (14, 1485) and np.array_equal(lo, s[14]) and np.array_equal(hi, s[1485])
    assert R.box_ranks(1) == (0, 0) and R.box_ranks(2) == (0, 1)
    assert (np.abs(p) > np.abs(np.stack([lo, hi])).max()).any()  # the far points are outside it


def test_grid_arrays_are_consistent():
    p = C.points("dups")
    lo, h, counts, ids, order, starts = R.build_grid(p)
    cells = counts[0] * counts[1] * counts[2]
    assert starts.shape == (cells + 1,) and starts[0] == 0 and starts[-1] == len(p) and (np.diff(starts) >= 0).all()
    assert np.array_equal(np.sort(order), np.arange(len(p))) and (np.diff(ids[order]) >= 0).all()
    assert np.array_equal(np.bincount(ids, minlength=cells), np.diff(starts))
    assert np.diff(starts).max() > 256  # 300 copies of a point share a cell: longer than a workgroup


def test_golden_from_the_reference_knn():
    """4,096 garden points and what the reference's examples/utils.py:knn (sklearn) returns for them."""
    g = np.load(C.GOLDEN)
    p = g["points"]
    assert p.shape == (4096, 3) and p.dtype == np.float32
    for K in (4, 16):
        want = g[f"dist{K}"].astype(np.float64)
        dist, _ = R.search(p, K)
        err = np.abs(dist.astype(np.float64) - want)
        print(f"golden K={K}: worst distance error {(err / (C.DIST_BAR * np.maximum(want, 1e-300))).max():.3f} of the bar")
        assert (err <= C.DIST_BAR * want).all()
    for init_scale in (1.0, 0.37):
        ref = np.log(np.sqrt((g["dist4"].astype(np.float64)[:, 1:] ** 2).mean(axis=1)) * init_scale)
        worst = C.check_scales(R.init_scales(p, init_scale), np.repeat(ref[:, None], 3, axis=1), f"golden init_scale={init_scale}")
        print(f"golden init_scales({init_scale}): worst error {worst:.3f} of the bar")


def test_init_scales_has_minus_infinity_on_duplicates():
    p = C.points("dups")
    out = R.init_scales(p, 0.5)
    ref = C.case_scales("dups", 0.5)
    assert np.isneginf(ref).sum() == 3 * 8 * 300 and out.dtype == np.float32
    C.check_scales(out, ref, "dups")


def test_reference_refuses_what_it_does_not_define():
    good = C.points("tiny")
    nan, inf = good.copy(), good.copy()
    nan[2, 1], inf[4, 0] = np.nan, -np.inf
    for bad in (good.astype(np.float64), good[:, :2], good[:, 0], nan, inf):
        with pytest.raises(ValueError):
            R.search(bad, 1)
        with pytest.raises(ValueError):
            R.search(good, 1, bad)
    for K in (0, 17, -1, 2.0, 6):  # 6 > N = 5
        with pytest.raises(ValueError):
            R.search(good, K)
    with pytest.raises(ValueError):
        R.init_scales(good, 1.0, K=1)


def test_refused_inputs_raise_before_any_launch(monkeypatch):
    from gscodec_studio_amd import knn as M

    calls = []
    monkeypatch.setattr(M.B, "call", lambda *a: calls.append(a[0]))
    good = torch.from_numpy(C.points("uniform").copy())
    nan, inf = good.clone(), good.clone()
    nan[3, 1], inf[1499, 0] = float("nan"), float("inf")
    bad_points = (good.double(), good.to(torch.int32), good[:, :2], good[:, 0], good.reshape(500, 3, 3), good.numpy(), nan, inf)
    for fn in (lambda x: M.knn(x, 4), lambda x: M.knn_search(x, 4), lambda x: M.init_scales(x), lambda x: M.knn_grid(x),
               lambda x: M.knn_search(good, 4, queries=x)):
        for x in bad_points:
            with pytest.raises(ValueError):
                fn(x)
    for K in (0, 17, -2, 4.0, True, None):
        for fn in (lambda: M.knn(good, K), lambda: M.knn_search(good, K), lambda: M.init_scales(good, K=K)):
            with pytest.raises(ValueError):
                fn()
    for fn in (lambda: M.knn(good[:3], 4), lambda: M.knn_search(good[:9], 10), lambda: M.init_scales(good[:3]),
               lambda: M.knn_search(good[:0], 1), lambda: M.init_scales(good, K=1), lambda: M.init_scales(good, init_scale=float("nan")),
               lambda: M.init_scales(good, init_scale="1")):
        with pytest.raises(ValueError):
            fn()
    for fn in (lambda: M.knn_search(good, 4), lambda: M.knn_search(good, 4, queries=good[:7]), lambda: M.init_scales(good),
               lambda: M.knn_grid(good)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # host tensors: nothing is computed on the CPU instead
            fn()
    assert calls == []


def test_knn_on_a_host_tensor_without_a_gpu_is_a_runtime_error(monkeypatch):
    from gscodec_studio_amd.knn import knn

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no GPU"):
        knn(torch.from_numpy(C.points("tiny").copy()), 4)


def test_header_lists_the_knn_entries():
    from gscodec_studio_amd import _backend as B

    protos = B.parse_header()
    assert sorted(n for n in protos if n.startswith("gs_knn_")) == ["gs_knn_cells", "gs_knn_finish_grid", "gs_knn_search"]
    _, argtypes, argnames = protos["gs_knn_search"]
    assert argnames[:3] == ["n", "m", "K"] and argnames[-1] == "stream" and argnames[6] == "box" and len(argtypes) == len(argnames) == 15


def test_utils_reexports_the_drop_in():
    import gscodec_studio_amd.knn as M
    import gscodec_studio_amd.utils as U

    assert U.knn is M.knn and U.knn_search is M.knn_search and U.init_scales is M.init_scales
    assert {"knn", "knn_search", "init_scales"} <= set(U.__all__)
