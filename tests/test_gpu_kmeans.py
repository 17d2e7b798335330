"""The K-means kernels (csrc/kmeans.hip behind gscodec_studio_amd.compression.kmeans) against their numpy definition
(kmeans_reference): every comparison is exact equality -- the assign alone, the update alone, then the whole fit from float
points, ``KMeans``, ``kmeans_encode(method="fixed")`` and ``kmeans_method="fixed"`` of the two codec classes."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from grid_sort_cases import asset_splats
from kmeans_cases import SHAPES, blobs, constant, extremes, few_distinct, shape_case, shape_key
from util import N, T

pytestmark = pytest.mark.gpu

ROUNDS = 3  # of every whole fit below: the second assign is the first against centroids that are no rows of q
# name -> (inputs, k_slices).  The forced slices put what each case is for through the sliced route (packed keys, atomic minimum,
# labels kernel): few_distinct's equal centroids into different slices of 8, extremes' repeated centroid 2 into another slice than
# centroid 0 with d = 64 * (2^24 - 1) in the key's upper word, constant's four equal centroids into two slices.  With k_slices
# None these k (32, 3, 4) are below the 64 centroids a slice has at least, so the library takes the one-slice route.
HAND_MADE = {"few_distinct": (few_distinct, None), "few_distinct_four_slices": (few_distinct, 4), "extremes": (extremes, None),
             "extremes_three_slices": (extremes, 3), "constant": (constant, None), "constant_two_slices": (constant, 2)}


def _case(name):
    """(x float32 [n, w], init [k], k_slices) of a named case of either table."""
    if name in SHAPES:
        return shape_case(name)
    make, k_slices = HAND_MADE[name]
    return (*make(), k_slices)


@functools.lru_cache(maxsize=None)
def _reference_of(name):
    from gscodec_studio_amd.compression import kmeans_reference as R

    x, init, _ = _case(name)
    q, lo, hi = R.quantize(x)
    cent, rounds = q[init].astype(np.int32), []
    for _ in range(ROUNDS):
        labels = R.assign(q, cent)
        cent, cnt = R.update(q, labels, cent)
        rounds.append((cent, labels, cnt))
    return q, lo, hi, rounds


def _reference(name):
    """(q, lo, hi, the centroids, labels and counts after every round) of the numpy definition: computed once per set of
    points, whatever the number of slices."""
    return _reference_of(shape_key(name) if name in SHAPES else next(o for o, v in HAND_MADE.items() if v[0] is HAND_MADE[name][0]))


def _steps(q, cent, k_slices):
    from gscodec_studio_amd.compression import kmeans as K

    n, w = q.shape
    slices = K._slices(k_slices, n, w, cent.shape[0])
    return K._Steps(T(np.ascontiguousarray(q.T)), T(cent), slices), slices


ALL_CASES = list(SHAPES) + list(HAND_MADE)


@pytest.mark.parametrize("name", ALL_CASES)
def test_assign_alone(name):
    """From the start and from the centroids after the first round (no longer rows of q), against previous labels of -1 and
    then the first round's: labels and the count of changed ones."""
    _, init, k_slices = _case(name)
    q, _, _, rounds = _reference(name)
    steps, slices = _steps(q, q[init], k_slices)
    assert np.array_equal(N(steps.assign()), rounds[0][1]), ("first assign", name, slices)
    assert int(steps.n_changed.item()) == q.shape[0]
    steps.cent[:, :q.shape[1]] = T(rounds[0][0])
    assert np.array_equal(N(steps.assign()), rounds[1][1]), ("second assign", name, slices)
    assert int(steps.n_changed.item()) == int((rounds[0][1] != rounds[1][1]).sum())
    assert not N(steps.cent[:, q.shape[1]:]).any(), "the padded channels stay zero"


@pytest.mark.parametrize("name", ALL_CASES)
def test_update_alone(name):
    """From the reference's first labels, and from labels that leave the upper half of the clusters empty."""
    from gscodec_studio_amd.compression import kmeans_reference as R

    _, init, k_slices = _case(name)
    q, _, _, rounds = _reference(name)
    k = len(init)
    steps, _ = _steps(q, q[init], k_slices)
    steps.labels.copy_(T(rounds[0][1]))
    assert np.array_equal(N(steps.update()), rounds[0][0]), ("update", name)
    assert np.array_equal(N(steps.counts).astype(np.int64), rounds[0][2])
    lower = (np.arange(q.shape[0]) % max(k // 2, 1)).astype(np.int32)
    want, cnt = R.update(q, lower, rounds[0][0])
    steps.labels.copy_(T(lower))
    assert np.array_equal(N(steps.update()), want), ("update with empty clusters", name)
    assert np.array_equal(N(steps.counts).astype(np.int64), cnt) and (k == 1 or (cnt == 0).any())


@pytest.mark.parametrize("name", ALL_CASES)
def test_whole_fit(name):
    """From the float points: the normalisation on the device, ROUNDS rounds, the centroids back in float32."""
    from gscodec_studio_amd.compression import kmeans_fit, kmeans_reference as R

    x, init, k_slices = _case(name)
    _, lo, hi, rounds = _reference(name)
    cent, labels = kmeans_fit(T(x), len(init), iters=ROUNDS, init_indices=init, k_slices=k_slices)
    assert cent.dtype == torch.float32 and labels.dtype == torch.int32 and cent.is_cuda and labels.is_cuda
    assert tuple(cent.shape) == (len(init), x.shape[1]) and tuple(labels.shape) == (x.shape[0],)
    assert np.array_equal(N(labels), rounds[-1][1]), name
    assert np.array_equal(N(cent), R.dequantize(rounds[-1][0], lo, hi)), name


def test_hand_made_cases_hold_what_they_are_for():
    """The case table's claims about its own inputs, on the reference's results."""
    from gscodec_studio_amd.compression import kmeans_reference as R

    q, _, _, rounds = _reference("few_distinct")
    assert len(np.unique(q, axis=0)) == 10 and (rounds[-1][2] == 0).sum() >= 22  # at most 10 of the 32 clusters have members
    twins = [(i, j) for i in range(32) for j in range(i + 1, 32) if np.array_equal(q[i], q[j])]
    assert any(i // 8 != j // 8 for i, j in twins), "equal centroids in different slices of 8"
    assert all(rounds[0][2][j] == 0 for _, j in twins), "the later of two equal centroids gets no member"
    q, _, _, rounds = _reference("extremes")
    assert set(np.unique(q)) == {0, R.QMAX} and int(np.abs(q[0].astype(np.int64) - q[1]).sum()) == 64 * R.QMAX
    assert rounds[-1][1][:4].tolist() == [0, 1, 0, 1] and rounds[-1][2].tolist() == [65, 65, 0]
    q, lo, hi, rounds = _reference("constant")
    assert lo == hi and not q.any() and not rounds[-1][1].any()


def test_two_runs_are_bit_equal():
    """Through the atomic minimum over the slices and the atomic sums of the update."""
    from gscodec_studio_amd.compression import kmeans_fit

    x, init, _ = _case("w45_k300_seven_slices")
    a = kmeans_fit(T(x), 300, iters=4, init_indices=init, k_slices=7)
    b = kmeans_fit(T(x), 300, iters=4, init_indices=init, k_slices=7)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_fit_that_stops_early_equals_all_rounds():
    from gscodec_studio_amd.compression import kmeans as K, kmeans_reference as R

    x, init = blobs()
    q = R.quantize(x)[0]
    cent, history = q[init].astype(np.int32), []
    for _ in range(40):
        history.append(R.assign(q, cent))
        cent, _ = R.update(q, history[-1], cent)
    first_still = next(i for i in range(1, 40) if np.array_equal(history[i], history[i - 1]))
    assert first_still == 7  # the eighth assign
    steps, _, _, n_assigns = K._fit(T(x), len(init), 40, 0, init, None)
    assert n_assigns == first_still + 1
    assert np.array_equal(N(steps.labels), history[-1]) and np.array_equal(N(steps.cent[:, :x.shape[1]]), cent)


def test_kmeans_class_fit_then_predict():
    """The shape of torchpq's class: [d, n] in, int64 labels out, centroids [d, k]; at a fixed point predict() on the training
    data returns the labels, and the default start is kmeans_encode's."""
    from gscodec_studio_amd.compression import KMeans, kmeans_fit

    x, _ = blobs()
    xt = T(np.ascontiguousarray(x.T))
    km = KMeans(n_clusters=5, distance="manhattan", max_iter=100, verbose=False)
    labels = km.fit(xt)
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (600,) and tuple(km.centroids.shape) == (3, 5)
    assert km.centroids.dtype == torch.float32 and 1 < km.n_iter_ < 100
    assert torch.equal(km.predict(xt), labels)
    cent, lab = kmeans_fit(T(x), 5, iters=100, seed=0)
    assert torch.equal(cent, km.centroids.t()) and torch.equal(lab.long(), labels)
    g = torch.Generator(device=xt.device).manual_seed(0)
    start = torch.randperm(600, device=xt.device, generator=g)[:5]
    cent2, lab2 = kmeans_fit(T(x), 5, iters=100, init_indices=start)
    assert torch.equal(cent2, cent) and torch.equal(lab2, lab)
    far = km.predict(T(np.array([[1e6], [-1e6], [0.0]], np.float32)))  # outside the fitted range: clamped, still a cluster
    assert far.dtype == torch.int64 and 0 <= int(far[0]) < 5


def test_kmeans_encode_fixed_round_trip():
    """The invariants of the existing round trip (tests/test_gpu_codec.py) with method="fixed": shapes, dtypes, labels < k,
    equal labels decode equally, a decoded centroid is its members' mean within half an 8-bit step."""
    from gscodec_studio_amd.compression import kmeans_decode, kmeans_encode

    rng = np.random.default_rng(5)
    shn = T((0.05 * rng.standard_normal((5000, 15, 3))).astype(np.float32))
    cq, labels, m = kmeans_encode(shn, n_clusters=64, iters=4, method="fixed")
    assert cq.dtype == torch.uint8 and tuple(cq.shape) == (64, 45) and labels.dtype == torch.int32 and tuple(labels.shape) == (5000,)
    assert 0 <= int(labels.min()) and int(labels.max()) < 64 and m["shape"] == [5000, 15, 3] and m["quantization"] == 8
    back = kmeans_decode(cq, labels, m)
    assert back.shape == shn.shape and back.dtype == shn.dtype
    step = (m["maxs"] - m["mins"]) / 255
    rows, flat = back.reshape(5000, -1), shn.reshape(5000, -1)
    for j in (int(labels[0]), int(labels[4999]), int(labels[1234])):
        same = labels == j
        assert bool((rows[same] == rows[same][0]).all())
        assert float((rows[same][0] - flat[same].mean(0)).abs().max()) <= 0.5 * step * 1.01 + 1e-6
    again = kmeans_encode(shn, n_clusters=64, iters=4, method="fixed")
    assert torch.equal(again[0], cq) and torch.equal(again[1], labels) and again[2] == m


def _splats_with_mask():
    sp = asset_splats()
    shn = sp["shN"].copy()
    shn[::5] = -np.abs(shn[::5])  # no positive coefficient: outside the mask
    return {**{k: T(v) for k, v in sp.items()}, "shN": T(shn)}, (shn > 0).any(axis=(1, 2))


@pytest.mark.parametrize("codec_name", ["PngCompression", "EntropyCodingCompression"])
def test_codec_classes_take_the_fixed_method(codec_name, tmp_path):
    from gscodec_studio_amd import compression as C

    splats, mask = _splats_with_mask()
    assert 0 < mask.sum() < 4096
    codec = getattr(C, codec_name)(use_sort=False, verbose=False, n_clusters=64, kmeans_method="fixed")
    d = str(tmp_path)
    codec.compress(d, splats, **({"entropy_models": {}} if codec_name == "EntropyCodingCompression" else {}))
    out = codec.decompress(d)
    shn = N(out["shN"])
    assert shn.shape == (4096, 3, 3) and not shn[~mask].any()
    with open(os.path.join(d, "meta.json")) as f:
        m = json.load(f)["shN"]
    z = np.load(os.path.join(d, "shN.npz"))
    assert z["centroids"].shape == (64, 9) and z["labels"].shape == (int(mask.sum()),) and int(z["labels"].max()) < 64
    book = N(C.kmeans_decode(torch.from_numpy(z["centroids"]), torch.arange(64, dtype=torch.int32), {**m, "shape": [64, 3, 3]}))
    assert np.array_equal(shn[mask], book[z["labels"].astype(np.int64)])
    # the file is the clustering of the masked rows by kmeans_fit from the default start
    _, labels = C.kmeans_fit(splats["shN"][T(mask)].reshape(-1, 9), 64)
    assert np.array_equal(N(labels), z["labels"].astype(np.int32))


def test_refused_inputs_on_the_device_raise_before_any_launch(monkeypatch):
    from gscodec_studio_amd.compression import kmeans as K

    calls = []
    monkeypatch.setattr(K.B, "call", lambda *a: calls.append(a[0]))
    good = T(blobs()[0])
    nan = good.clone()
    nan[5, 1] = float("nan")
    for x, kw in ((nan, {}), (good.long(), {}), (good, {"n_clusters": 0}), (good, {"init_indices": np.arange(4)}), (good, {"k_slices": 6})):
        with pytest.raises(ValueError):
            K.kmeans_fit(x, **{"n_clusters": 5, **kw})
    assert calls == []
