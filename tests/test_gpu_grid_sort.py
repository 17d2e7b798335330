"""The grid sort on the GPU (csrc/grid_sort.hip behind gscodec_studio_amd.compression.grid_sort) against its numpy definition
(grid_sort_reference): every comparison is exact equality -- stage by stage, so that a mismatch names one kernel, then the whole
schedule, ``sort_splats_grid``, ``use_sort="grid"`` of PngCompression, and the rejected inputs."""
import functools
import os

import numpy as np
import pytest
import torch

from grid_sort_cases import STAGE_SHAPES, asset_splats, extreme_case, features
from util import N, T

pytestmark = pytest.mark.gpu


def _rounds(q, side, seed):
    from gscodec_studio_amd.compression import grid_sort as G

    return G._Rounds(T(q.view(np.int16)), side, seed)


def _check_round(rounds, q, order, side, r, seed, k):
    """One round on the GPU from ``order`` (already in rounds.order), each stage against the reference."""
    from gscodec_studio_amd.compression import grid_sort_reference as R

    t = R.blur_target(q, order, side, r)
    got_t = N(rounds.blur(r)).view(np.uint16)
    assert np.array_equal(got_t, t), ("blur", side, q.shape[1], r, int(np.abs(got_t.astype(np.int64) - t).max()))
    keys = R.round_keys(side, r, seed, k)
    assert np.array_equal(N(rounds.make_keys(R.block_side(r), k)).view(np.uint64), keys), ("keys", side, r)
    pos, groups = R.round_groups(keys)
    assert np.array_equal(N(rounds.sort(R.key_bits(side, r))), pos), ("sorted positions", side, r)
    want = R.assign(q, t, order, groups)
    assert np.array_equal(N(rounds.assign()), want), ("assign", side, q.shape[1], r)
    return want, t, groups


@pytest.mark.parametrize("side,channels", STAGE_SHAPES)
def test_stage_by_stage(side, channels):
    """The start order, then the first round (the widest radius, S // 2 - 1) and a round at radius 1 (4 x 4 blocks, the most
    groups), each from the reference's order: blur, keys, sorted positions, order after the assignment."""
    from gscodec_studio_amd.compression import grid_sort_reference as R

    seed = 3
    q = R.quantize_features(features(side, channels))
    rounds = _rounds(q, side, seed)
    order = R.start_order(side * side, seed)
    assert np.array_equal(N(rounds.start()), order), "start order"
    order, _, _ = _check_round(rounds, q, order, side, side // 2 - 1, seed, 1)
    _check_round(rounds, q, order, side, 1, seed, 2)


def test_largest_distances():
    """(40, 64) with items at every channel's minimum next to targets at every channel's maximum: a distance of 4095^2 * 64,
    the most a 32-bit accumulator has to hold."""
    from gscodec_studio_amd.compression import grid_sort_reference as R

    f, order, r = extreme_case()
    q = R.quantize_features(f)
    rounds = _rounds(q, 40, 0)
    rounds.order.copy_(T(order.astype(np.int32)))
    _, t, groups = _check_round(rounds, q, order, 40, r, 0, 1)
    d = ((q[order[groups]].astype(np.int64)[:, :, None, :] - t[groups][:, None, :, :]) ** 2).sum(axis=-1)
    assert d.max() == 4095 * 4095 * 64


@functools.lru_cache(maxsize=None)
def _reference_order(side, channels, seed):
    from gscodec_studio_amd.compression import grid_sort_reference as R

    return R.grid_sort_order(features(side, channels), seed=seed)


@pytest.mark.parametrize("side,channels", [(33, 14), (96, 14)])
def test_whole_schedule(side, channels):
    from gscodec_studio_amd.compression import grid_sort_order

    got = grid_sort_order(T(features(side, channels)), seed=11)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (side * side,)
    assert np.array_equal(N(got), _reference_order(side, channels, 11))


@pytest.mark.parametrize("side", [1, 2, 3])
def test_tiny_grids(side):
    from gscodec_studio_amd.compression import grid_sort_order, grid_sort_reference as R

    assert np.array_equal(N(grid_sort_order(T(features(side, 4)), seed=7)), R.start_order(side * side, 7))


def _splats(n=4096):
    return {k: T(v[:n]) for k, v in asset_splats().items()}


def test_sort_splats_grid():
    from gscodec_studio_amd.compression import grid_sort_reference as R, sort_splats_grid

    sp = _splats(1089)  # S = 33
    flat = {k: N(v).reshape(1089, -1) for k, v in sp.items()}
    want = R.grid_sort_order(np.concatenate([flat[k] for k in sp if k != "shN"], axis=1), seed=0)
    out = sort_splats_grid(sp, verbose=False)
    assert isinstance(out, dict) and list(out) == list(sp)
    for k in sp:
        assert out[k].shape == sp[k].shape and np.array_equal(N(out[k]), N(sp[k])[want]), k
    out2, idx = sort_splats_grid(sp, verbose=False, return_indices=True)
    assert idx.dtype == torch.int64 and np.array_equal(N(idx), want) and all(torch.equal(out2[k], out[k]) for k in sp)
    want_n = R.grid_sort_order(np.concatenate([flat[k] for k in sp], axis=1), seed=5)  # 14 + 9 channels
    _, idx_n = sort_splats_grid(sp, verbose=False, return_indices=True, sort_with_shN=True, seed=5)
    assert np.array_equal(N(idx_n), want_n) and not np.array_equal(want_n, want)


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


@functools.lru_cache(maxsize=None)
def _compressed(use_sort, root):
    from gscodec_studio_amd.compression import PngCompression

    d = os.path.join(root, str(use_sort))
    codec = PngCompression(use_sort=use_sort, verbose=False, n_clusters=64)
    codec.compress(d, _splats())
    return d, codec.decompress(d)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("grid_sort"))


def test_round_trip_is_the_unsorted_result_permuted(root):
    from gscodec_studio_amd.compression import sort_splats_grid
    from gscodec_studio_amd.compression._container import prepare_splats

    _, plain = _compressed(False, root)
    _, grid = _compressed("grid", root)
    prepared, side = prepare_splats(_splats(), 0.005, False, False)
    assert side == 64
    _, idx = sort_splats_grid(prepared, verbose=False, return_indices=True)
    assert np.array_equal(np.sort(N(idx)), np.arange(4096)) and not np.array_equal(N(idx), np.arange(4096))
    for name in ("means", "scales", "quats", "opacities", "sh0"):
        assert grid[name].shape == plain[name].shape and torch.equal(grid[name], plain[name][idx]), name


def test_directory_is_smaller_than_unsorted(root):
    sizes = {u: _dir_bytes(_compressed(u, root)[0]) for u in (False, "morton", "grid")}
    print(f"directory bytes, 4096 splats of the asset: unsorted {sizes[False]}, Morton {sizes['morton']}, grid {sizes['grid']}")
    assert sizes["grid"] < sizes[False]


def test_entropy_coding_compression_takes_it(tmp_path):
    from gscodec_studio_amd.compression import EntropyCodingCompression

    codec = EntropyCodingCompression(use_sort="grid", verbose=False, n_clusters=64)
    codec.compress(str(tmp_path), _splats(1024), entropy_models={})
    out = codec.decompress(str(tmp_path))
    assert tuple(out["means"].shape) == (1024, 3) and torch.isfinite(out["scales"]).all()


def test_rejected_inputs_raise_before_any_launch(monkeypatch):
    from gscodec_studio_amd.compression import grid_sort as G

    calls = []
    monkeypatch.setattr(G.B, "call", lambda *a: calls.append(a[0]))
    good = features(8, 3)
    nan, inf = good.copy(), good.copy()
    nan[5, 1], inf[63, 0] = np.nan, -np.inf
    for bad in (T(features(8, 65)), T(good[:63]), torch.from_numpy(good), T(nan), T(inf)):
        with pytest.raises(ValueError):
            G.grid_sort_order(bad)
    with pytest.raises(ValueError):
        G.sort_splats_grid({"means": T(good[:60]), "scales": T(good[:60])}, verbose=False)
    assert calls == []
