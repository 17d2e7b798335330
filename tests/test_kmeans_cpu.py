"""The fixed-point K-means as its numpy definition states it (gscodec_studio_amd.compression.kmeans_reference): the rules on
hand-made inputs, the agreement with a float64 Lloyd iteration, and what the GPU driver refuses before it launches anything."""
import functools
import inspect

import numpy as np
import pytest
import torch

from kmeans_cases import ITERS, SEEDED, float64_lloyd, seeded

from gscodec_studio_amd.compression import kmeans_reference as R


def test_range_ends_map_to_the_ends_of_the_grid():
    q, lo, hi = R.quantize(np.array([[-2.0, 6.0], [2.0, 0.0]], np.float32))
    assert (lo, hi) == (-2.0, 6.0) and q.dtype == np.int32
    assert q.tolist() == [[0, R.QMAX], [(R.QMAX + 1) // 2, R.QMAX // 4 + 1]]  # 8388607.5 -> 8388608 (even), 4194303.75 -> 4194304


def test_constant_input_maps_to_zeros():
    q, lo, hi = R.quantize(np.full((7, 3), 0.25, np.float32))
    assert lo == hi == 0.25 and not q.any()
    cent, labels = R.kmeans_fit(np.full((7, 3), 0.25, np.float32), np.array([2, 5]), iters=3)
    assert not labels.any() and np.array_equal(cent, np.full((2, 3), 0.25, np.float32))


def test_duplicate_centroids_the_lower_index_wins_and_the_other_stays():
    q = np.array([[5, 5], [5, 5], [90, 90], [7, 5]], np.int32)
    cent = q[[0, 1, 2]]
    labels = R.assign(q, cent)
    assert labels.tolist() == [0, 0, 2, 0]
    new, cnt = R.update(q, labels, cent)
    assert cnt.tolist() == [3, 0, 1] and new[1].tolist() == [5, 5] and new[2].tolist() == [90, 90]
    assert new[0].tolist() == [(2 * 17 + 3) // 6, 5]  # 17 / 3 = 5.67 -> 6


def test_mean_rounds_half_up():
    q = np.array([[0], [1]], np.int32)
    new, _ = R.update(q, np.zeros(2, np.int32), q[[0]])
    assert new.tolist() == [[1]]
    new, _ = R.update(np.array([[1], [2], [2], [2]], np.int32), np.zeros(4, np.int32), q[[0]])
    assert new.tolist() == [[2]]  # 1.75


def test_largest_distance_is_exact():
    q = np.array([[0] * 64, [R.QMAX] * 64], np.int32)
    assert R.assign(q, q).tolist() == [0, 1]
    assert int(np.abs(q[0].astype(np.int64) - q[1]).sum()) == 64 * R.QMAX < 1 << 30


@functools.lru_cache(maxsize=None)
def _seeded_fit(seed):
    x, init = seeded(seed, *SEEDED[seed])
    q, lo, hi = R.quantize(x)
    cent, labels = R.fit_quantized(q, init, ITERS)
    return x, init, cent, labels, lo, hi


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_labels_equal_a_float64_lloyd_iteration(seed):
    x, init, _, labels, _, _ = _seeded_fit(seed)
    _, want = float64_lloyd(x, init, ITERS)
    assert np.array_equal(labels, want), int((labels != want).sum())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_centroids_within_one_step_of_the_member_mean(seed):
    x, _, cent, labels, lo, hi = _seeded_fit(seed)
    step = (hi - lo) / R.QMAX
    got = R.dequantize(cent, lo, hi).astype(np.float64)
    worst = 0.0
    for j in np.unique(labels):
        worst = max(worst, float(np.abs(got[j] - x[labels == j].astype(np.float64).mean(axis=0)).max()))
    print(f"seed {seed}: worst |centroid - member mean| = {worst:.3e}, one step = {step:.3e}")
    assert worst <= step


def test_kmeans_fit_is_quantize_fit_dequantize():
    x, init, cent, labels, lo, hi = _seeded_fit(0)
    c, l = R.kmeans_fit(x, init, ITERS)
    assert c.dtype == np.float32 and l.dtype == np.int32 and np.array_equal(l, labels) and np.array_equal(c, R.dequantize(cent, lo, hi))


def test_reference_refuses_what_it_does_not_define():
    for bad in (np.zeros((0, 3), np.float32), np.zeros((4, 65), np.float32), np.zeros(4, np.float32),
                np.array([[np.nan, 1.0]], np.float32), np.array([[np.inf, 1.0]], np.float32)):
        with pytest.raises(ValueError):
            R.quantize(bad)


def test_refused_inputs_raise_before_any_launch(monkeypatch):
    from gscodec_studio_amd.compression import KMeans, kmeans as K, kmeans_encode

    calls = []
    monkeypatch.setattr(K.B, "call", lambda *a: calls.append(a[0]))
    good = torch.randn(40, 5, generator=torch.Generator().manual_seed(0))
    nan, inf = good.clone(), good.clone()
    nan[3, 1], inf[39, 0] = float("nan"), float("-inf")
    for x, kw in ((good.to(torch.int32), {}), (nan, {}), (inf, {}), (torch.zeros(40, 65), {}), (torch.zeros(40, 0), {}),
                  (torch.zeros(0, 5), {}), (good[:, 0], {}), (good.numpy(), {}), (good, {"n_clusters": 0}), (good, {"n_clusters": -3}),
                  (torch.zeros((1 << 20) + 1, 1), {"n_clusters": (1 << 20) + 1}),
                  (good, {"init_indices": np.arange(7)}), (good, {"init_indices": np.arange(8, dtype=np.float32)}),
                  (good, {"init_indices": np.array([0, 1, 2, 3, 4, 5, 6, 40])}), (good, {"init_indices": torch.tensor([-1, 1, 2, 3, 4, 5, 6, 7])}),
                  (good, {"init_indices": np.arange(8).reshape(2, 4)}), (good, {"k_slices": 0}), (good, {"k_slices": 9})):
        with pytest.raises(ValueError):
            K.kmeans_fit(x, **{"n_clusters": 8, **kw})
    for call in (lambda: K.kmeans_fit(good, 8), lambda: K.kmeans_fit(good, 8, init_indices=np.arange(8)),
                 lambda: KMeans(8).fit(good.t()), lambda: kmeans_encode(good.reshape(40, 5, 1), n_clusters=8, method="fixed")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # a host tensor: nothing is computed on the CPU instead
            call()
    with pytest.raises(NotImplementedError):
        KMeans(8, distance="euclidean")
    with pytest.raises(RuntimeError):
        KMeans(8).predict(good.t())
    with pytest.raises(ValueError):
        kmeans_encode(good.reshape(40, 5, 1), n_clusters=8, method="fast")
    assert calls == []


def test_the_default_method_is_the_torch_path():
    from gscodec_studio_amd.compression import EntropyCodingCompression, PngCompression, kmeans_encode
    from gscodec_studio_amd.compression._container import compress_masked_kmeans

    assert inspect.signature(kmeans_encode).parameters["method"].default == "torch"
    assert inspect.signature(compress_masked_kmeans).parameters["method"].default == "torch"
    assert list(inspect.signature(compress_masked_kmeans).parameters)[-1] == "method"
    assert PngCompression().kmeans_method == "torch" and EntropyCodingCompression().kmeans_method == "torch"
    assert PngCompression(kmeans_method="fixed").kmeans_method == "fixed"
    # and it still takes host tensors, with today's results: a seeded Lloyd iteration in torch
    x = torch.randn(60, 2, 3, generator=torch.Generator().manual_seed(1))
    cq, labels, meta = kmeans_encode(x, n_clusters=4, iters=3)
    cq2, labels2, meta2 = kmeans_encode(x, n_clusters=4, iters=3, method="torch")
    assert cq.dtype == torch.uint8 and tuple(cq.shape) == (4, 6) and labels.dtype == torch.int32 and int(labels.max()) < 4
    assert torch.equal(cq, cq2) and torch.equal(labels, labels2) and meta == meta2
