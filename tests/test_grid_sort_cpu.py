"""The grid sort's definition (gscodec_studio_amd/compression/grid_sort_reference.py, numpy): it is a permutation, deterministic
per seed, every round lowers (never raises) its own objective, it beats the Morton order on the bundled asset, and the edge
sizes work.  The kernels are held to this code in tests/test_gpu_grid_sort.py."""
import numpy as np
import pytest
import torch

from grid_sort_cases import asset_sample, extreme_case, features

from gscodec_studio_amd.compression import grid_sort_reference as R


def _is_permutation(order, n):
    return order.dtype == np.int64 and order.shape == (n,) and np.array_equal(np.sort(order), np.arange(n))


def test_hash_is_the_written_out_murmur_finaliser():
    def fmix(x):
        x ^= x >> 16
        x = x * 0x85EBCA6B & 0xFFFFFFFF
        x ^= x >> 13
        x = x * 0xC2B2AE35 & 0xFFFFFFFF
        return x ^ x >> 16

    for seed, k, p in [(0, 0, 0), (1, 2, 3), (0xFFFFFFFF, 700, 1006008), (12345, 0xFFFFFFFF, 0x7FFFFFFF)]:
        want = fmix(fmix((seed + (k + 1) * 0x9E3779B9) & 0xFFFFFFFF) ^ (p * 0x85EBCA6B & 0xFFFFFFFF))
        assert int(R.hash32(seed, k, p)[0]) == want
    h = R.hash32(0, 1, np.arange(1 << 16))
    assert h.dtype == np.uint32 and len(np.unique(h)) == 1 << 16  # a bijection of p for fixed (seed, k)


def test_quantize_features():
    f = np.array([[0.0, 5.0, -1.0], [1.0, 5.0, 1.0], [0.5, 5.0, 0.0], [0.25, 5.0, -0.99993]], np.float32)
    q = R.quantize_features(f)
    assert q.dtype == np.uint16 and q[:, 0].tolist() == [0, 4095, 2048, 1024] and not q[:, 1].any()  # 2047.5 -> 2048 (half to even)
    assert q[:, 2].tolist() == [0, 4095, 2048, 0]
    for bad in (np.full((4, 65), 1.0), np.array([[np.nan], [0], [0], [0]]), np.array([[np.inf], [0], [0], [0]]), np.zeros(4)):
        with pytest.raises(ValueError):
            R.quantize_features(bad)
    with pytest.raises(ValueError, match="square"):
        R.grid_sort_order(np.zeros((15, 2), np.float32))


def test_schedule():
    assert R.schedule(3) == [] and R.schedule(4) == [1] * 8 and R.schedule(8, reps=1) == [3, 2, 1]
    s = R.schedule(1003)
    assert s[0] == 500 and s[8] == 475 and s[-1] == 1 and all(a >= b for a, b in zip(s, s[1:])) and len(s) % 8 == 0
    assert R.schedule(64, decay=0.5, reps=2) == [31, 31, 15, 15, 7, 7, 3, 3, 1, 1]


def test_bijection_and_determinism():
    f = features(16, 5)
    a, b, c = R.grid_sort_order(f, seed=0), R.grid_sort_order(f, seed=0), R.grid_sort_order(f, seed=1)
    assert _is_permutation(a, 256) and _is_permutation(c, 256)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert not np.array_equal(R.start_order(256, 0), R.start_order(256, 1))


def test_objective_never_rises():
    """Exact in integers: the identity is one of the 24 candidates and a tie keeps it."""
    q = R.quantize_features(features(16, 5))
    n_rounds = fell = 0
    for k, r, t, before, after in R.rounds(q, seed=3):
        o0, o1 = R.round_objective(q, before, t), R.round_objective(q, after, t)
        assert o1 <= o0, (k, r, o0, o1)
        assert _is_permutation(after, 256)
        n_rounds += 1
        fell += o1 < o0
    assert n_rounds == len(R.schedule(16)) and fell > n_rounds // 2


def test_blur_is_the_padded_box_filter():
    """Against the direct sum over numpy's reflect padding, rows first: S = 9 with r = 1 and the widest r = 3."""
    q = R.quantize_features(features(9, 2))
    order = R.start_order(81, 0)
    g = q[order].astype(np.int64).reshape(9, 9, 2)
    for r in (1, 3):
        w = 2 * r + 1
        pad = np.pad(g, ((0, 0), (r, r), (0, 0)), mode="reflect")
        rows = np.stack([(2 * pad[:, x:x + w].sum(axis=1) + w) // (2 * w) for x in range(9)], axis=1)
        pad = np.pad(rows, ((r, r), (0, 0), (0, 0)), mode="reflect")
        want = np.stack([(2 * pad[y:y + w].sum(axis=0) + w) // (2 * w) for y in range(9)], axis=0)
        assert np.array_equal(R.blur_target(q, order, 9, r).reshape(9, 9, 2), want)


def test_quality_on_the_bundled_asset():
    """4096 splats of the garden crop, means and colours (six channels) on a 64 x 64 grid: the grid order is smoother than the
    Morton order (measured: shuffled 8.52e6, Morton 4.18e6, grid 3.55e5 -- README, "Grid sort")."""
    from gscodec_studio_amd.compression import morton_order

    means, colours = asset_sample()
    q = R.quantize_features(np.concatenate([means, colours], axis=1))
    shuffled = R.neighbour_metric(q, np.arange(4096))
    morton = R.neighbour_metric(q, morton_order(torch.from_numpy(means)).numpy())
    order = R.grid_sort_order(np.concatenate([means, colours], axis=1))
    grid = R.neighbour_metric(q, order)
    print(f"neighbour metric: shuffled {shuffled:.4g}, Morton {morton:.4g}, grid {grid:.4g}")
    assert _is_permutation(order, 4096)
    assert grid < morton < shuffled


@pytest.mark.parametrize("side", [1, 2, 3])
def test_tiny_grids_return_the_start_order(side):
    n = side * side
    assert np.array_equal(R.grid_sort_order(features(side, 4), seed=7), R.start_order(n, 7))
    assert _is_permutation(R.start_order(n, 7), n)


@pytest.mark.parametrize("channels", [1, 64])
def test_channel_extremes(channels):
    f = features(8, channels)
    order = R.grid_sort_order(f)
    q = R.quantize_features(f)
    assert _is_permutation(order, 64) and R.neighbour_metric(q, order) < R.neighbour_metric(q, R.start_order(64, 0))


def test_constant_channel():
    f = features(8, 3)
    f[:, 1] = 2.5
    assert not R.quantize_features(f)[:, 1].any()
    g = np.delete(f, 1, axis=1)
    assert np.array_equal(R.grid_sort_order(f), R.grid_sort_order(g))  # a constant channel adds nothing to any distance
    assert _is_permutation(R.grid_sort_order(np.zeros((64, 2), np.float32)), 64)  # nothing but constant channels


def test_odd_side_groups_cover_every_position_once():
    """S = 33: N % 4 = 1.  Per round: every position is in at most one group, and the positions in no group are exactly the
    tail of one and the runs of four that straddle two blocks."""
    side, n, n_straddling = 33, 33 * 33, 0
    for k, r in [(1, 15), (40, 6), (90, 1)]:
        keys = R.round_keys(side, r, seed=0, k=k)
        pos, groups = R.round_groups(keys)
        assert np.array_equal(np.sort(pos), np.arange(n))
        assert len(np.unique(groups)) == groups.size
        runs = pos[: n - 1].reshape(-1, 4)
        blocks = (keys[runs] >> np.uint64(32)).astype(np.int64)
        straddling = runs[(blocks != blocks[:, :1]).any(axis=1)]
        assert len(straddling) + len(groups) == len(runs)
        n_straddling += len(straddling)
        left_out = np.setdiff1d(np.arange(n), groups.reshape(-1))
        assert np.array_equal(left_out, np.sort(np.concatenate([straddling.reshape(-1), pos[n - 1:]])))
        assert int(keys.max()).bit_length() <= R.key_bits(side, r)
    assert n_straddling > 0
    order = R.grid_sort_order(features(33, 14))
    assert _is_permutation(order, n)


def test_extreme_distances_are_reached():
    """The case the GPU test uses for the accumulator bound: some item-to-target distance is 4095^2 * 64."""
    f, order, r = extreme_case()
    q = R.quantize_features(f)
    t = R.blur_target(q, order, 40, r)
    _, groups = R.round_groups(R.round_keys(40, r, seed=0, k=1))
    a = q[order[groups]].astype(np.int64)
    d = ((a[:, :, None, :] - t[groups][:, None, :, :]) ** 2).sum(axis=-1)
    assert d.max() == 4095 * 4095 * 64
    assert _is_permutation(R.assign(q, t, order, groups), 1600)


def test_entry_points_validate_their_arguments():
    """Status and message for bad arguments, without a GPU: the checks precede the launch."""
    from gscodec_studio_amd import _backend as B

    for args, msg in (((0, 3, 1, 1, 1, 1, 1, None), "1 <= S"), ((8, 65, 1, 1, 1, 1, 1, None), "C <= 64"), ((8, 3, 8, 1, 1, 1, 1, None), "r < S"),
                      ((8, 3, 0, 1, 1, 1, 1, None), "r < S"), ((8, 3, 1, None, 1, 1, 1, None), "null pointer"),
                      ((8, 3, 1, 8, 8, 16, 16, None), "three buffers")):
        with pytest.raises(RuntimeError, match=msg):
            B.call("gs_gridsort_blur", *args)
    with pytest.raises(RuntimeError, match="null pointer"):
        B.call("gs_gridsort_keys", 8, 4, 0, 1, None, 1, None)
    with pytest.raises(RuntimeError, match="46340"):
        B.call("gs_gridsort_keys", 46341, 4, 0, 1, 1, 1, None)
    with pytest.raises(RuntimeError, match="must not alias"):
        B.call("gs_gridsort_assign", 8, 3, 4, 4, 8, 8, 16, 16, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        B.call("gs_gridsort_assign", 8, 3, 4, 4, None, 8, 16, 24, None)
