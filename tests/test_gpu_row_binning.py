"""Row binning, the third route of gs_isect_finish_presorted (tile rows by one counting pass over the (splat, row) entries, every
row list expanded into its columns), against the packed / pair routes it stands in for and against the oracle: isect_ids,
flatten_ids and the tile offsets must be IDENTICAL, ties in position order included.  gs_isect_last_route() tells a fallback from
the real thing.  The route ranks the items of a workgroup in wave slots of 64, two per thread: 512 positions per block and 512
entries per chunk of a row list, staged in LDS up to 4096 pairs per chunk: the shapes sit on both sides of 64, 256, 512 and 1024,
of the staging limit, of the width and row limits (256), and of empty / full grids."""
import numpy as np
import pytest
import torch

from util import N, T, dev, garden, garden_sh

pytestmark = pytest.mark.gpu

TS = 16
LIMIT_W = LIMIT_R = 256


def _begin(m2, radii, d, tw, th):
    from gscodec_studio_amd import _wrapper as W

    C, n = radii.shape
    return W.isect_tiles_begin(T(m2), T(radii), T(d), TS, tw, th, True, C, n, C * n, None)


def _finish(m2, radii, d, tw, th, on):
    from gscodec_studio_amd import _wrapper as W

    prev = W.set_row_binning(on)
    try:
        out = W.isect_tiles_finish(_begin(m2, radii, d, tw, th), offsets_for=radii.shape[0])
        torch.cuda.synchronize()
        return [N(x) for x in out], W.isect_last_route()
    finally:
        W.set_row_binning(prev)


def _check(m2, radii, d, tw, th, expect="rows", oracle=True):
    """Route on against off (and the oracle); -> the outputs.  expect: the route the switched-on call must report
    (None: the call has no pairs, the route query is not touched)."""
    m2, radii, d = np.asarray(m2, np.float32), np.asarray(radii, np.int32), np.asarray(d, np.float32)
    a, route_a = _finish(m2, radii, d, tw, th, True)
    b, route_b = _finish(m2, radii, d, tw, th, False)
    if expect is not None:
        assert route_a == expect, (route_a, expect)
        assert route_b in ("packed", "pairs")
    for name, x, y in zip(("tiles_per_gauss", "isect_ids", "flatten_ids", "offsets"), a, b):
        assert x.shape == y.shape and np.array_equal(x, y), name
    if oracle:
        from oracle import gs_oracle as O

        tpg, ids, flat = O.isect_tiles(m2, radii, d, TS, tw, th, sort=True)
        assert np.array_equal(a[0], tpg) and np.array_equal(a[1], ids) and np.array_equal(a[2], flat)
        assert np.array_equal(a[3], O.isect_offset_encode(ids, radii.shape[0], tw, th))
    return a


def _random(n, tw, th, seed, C=1, vis=0.8, rmax=None):
    rs = np.random.RandomState(seed)
    w, h = tw * TS, th * TS
    m2 = np.stack([rs.uniform(-0.3 * w - 20, 1.3 * w + 20, (C, n)), rs.uniform(-0.3 * h - 20, 1.3 * h + 20, (C, n))], -1)
    rmax = rmax or 2 * max(w, h)
    radii = np.exp(rs.uniform(0.0, np.log(rmax), (C, n))).astype(np.int32)  # 1 pixel ... larger than the image
    radii[rs.rand(C, n) > vis] = 0
    d = rs.uniform(0.2, 9.0, (C, n))
    return m2, radii, d


@pytest.mark.parametrize("tw,th,n", [(1, 1, 300), (7, 5, 3000), (64, 2, 1500), (65, 2, 1500), (LIMIT_W, 1, 2500)])
def test_random_splats_on_small_grids(tw, th, n):
    m2, radii, d = _random(n, tw, th, seed=tw * 31 + th, rmax=max(40, (tw * TS) // 3) if tw > 7 else None)
    a = _check(m2, radii, d, tw, th)
    assert (radii == 0).any() and (a[0] == 0)[radii > 0].any()  # radius 0 and off-screen splats are both in the mix
    assert a[1].size > n // 10


def _one_row(k, tw, th, row, seed=0, n_total=None):
    """k splats whose boxes lie inside tile row `row` (each 1 to 3 tiles wide); with n_total, further culled splats around them."""
    rs = np.random.RandomState(seed + k)
    n = n_total or k
    m2 = np.zeros((1, n, 2))
    radii = np.zeros((1, n), np.int32)
    at = np.sort(rs.choice(n, k, replace=False))
    m2[0, at, 0] = rs.uniform(0, tw * TS, k)
    m2[0, at, 1] = row * TS + 8.0
    radii[0, at] = rs.choice([3, 7, 20], k)  # y: [row*16 + 8 - r, row*16 + 8 + r] stays in the row for r <= 7; 20 covers 3 rows
    d = rs.uniform(0.5, 5.0, (1, n))
    return m2, radii, d


@pytest.mark.parametrize("k", [255, 256, 257, 512, 513, 1023, 1024, 1025, 2049])
def test_entry_counts_around_wave_round_and_chunk_boundaries(k):
    """k entries in ONE tile row, every other row empty (the splats are 7 pixels at most: they stay in their row): the chunk
    kernels at the ends of a thread round (256) and of one and two chunks (512, 1024); the same k kept positions for the block
    kernels."""
    m2, radii, d = _one_row(k, 9, 5, row=3)
    radii = np.minimum(radii, 7)
    a = _check(m2, radii, d, 9, 5)
    assert a[3][0, :3].max() == 0 and (a[3][0, 4] == a[1].size).all()  # rows 0-2 in front, row 4 behind every pair


@pytest.mark.parametrize("wider", [0, 1, 40])
def test_chunk_at_the_staging_limit(wider):
    """One chunk of 512 entries, eight columns each = exactly the 4096 pairs the expansion stages in LDS; with one (or 40) of the
    splats a column wider the chunk writes its pairs unstaged."""
    n, tw, th = 512, 16, 1
    m2 = np.tile(np.array([64.0, 8.0]), (1, n, 1))   # columns [floor(1 / 16), ceil(127 / 16)) = [0, 8)
    radii = np.full((1, n), 63, np.int32)
    radii[0, 100:100 + wider] = 79                   # ... [0, ceil(143 / 16)) = [0, 9)
    d = np.random.RandomState(wider).uniform(0.5, 5.0, (1, n))
    a = _check(m2, radii, d, tw, th)
    assert a[1].size == 4096 + wider


@pytest.mark.parametrize("k", [255, 257, 1024, 1025])
def test_kept_positions_around_block_boundaries_with_tall_splats(k):
    """k kept positions among 3 k elements, a third of them three rows tall: ranks across rows, rounds and blocks."""
    m2, radii, d = _one_row(k, 9, 5, row=2, seed=7, n_total=3 * k)
    _check(m2, radii, d, 9, 5)


@pytest.mark.parametrize("tw,expect", [(1, "rows"), (63, "rows"), (64, "rows"), (65, "rows"), (LIMIT_W, "rows"), (LIMIT_W + 1, "packed")])
def test_full_width_splats(tw, expect):
    """Every splat covers ALL columns (of one or two rows); one column past the limit the call takes the old route."""
    n, th = 200, 3
    rs = np.random.RandomState(tw)
    m2 = np.stack([np.full((1, n), tw * TS / 2.0), rs.uniform(0, th * TS, (1, n))], -1)
    radii = np.full((1, n), tw * TS, np.int32)
    d = rs.uniform(0.5, 5.0, (1, n))
    a = _check(m2, radii, d, tw, th, expect=expect)
    assert a[1].size >= n * tw and a[1].size % tw == 0


@pytest.mark.parametrize("C,th,expect", [(1, 1, "rows"), (1, 65, "rows"), (1, LIMIT_R, "rows"), (1, LIMIT_R + 1, "packed"),
                                         (2, LIMIT_R // 2, "rows"), (2, LIMIT_R // 2 + 1, "packed")])
def test_full_height_splats_and_the_row_limit(C, th, expect):
    n, tw = 150, 2
    rs = np.random.RandomState(th + C)
    m2 = np.stack([rs.uniform(0, tw * TS, (C, n)), np.full((C, n), th * TS / 2.0)], -1)
    radii = np.full((C, n), th * TS, np.int32)
    radii[C - 1, ::3] = 0
    d = rs.uniform(0.5, 5.0, (C, n))
    _check(m2, radii, d, tw, th, expect=expect)


def test_ties_keep_position_order():
    """300 splats with the same depth bits and the same rectangle: inside every tile's list the flatten ids ascend (the
    pre-sort is stable); then two depths interleaved in memory: the nearer half first, each half in memory order."""
    n, tw, th = 300, 7, 5
    m2 = np.tile(np.array([40.0, 37.0]), (1, n, 1))
    radii = np.full((1, n), 30, np.int32)
    a = _check(m2, radii, np.full((1, n), 1.75), tw, th)
    off = np.append(a[3].reshape(-1), a[1].size)
    for t in range(tw * th):
        ids = a[2][off[t]:off[t + 1]]
        assert ids.size in (0, n) and np.array_equal(ids, np.arange(ids.size))
    d = np.where(np.arange(n) % 2 == 0, 2.5, 1.25)[None]
    a = _check(m2, radii, d, tw, th)
    off = np.append(a[3].reshape(-1), a[1].size)
    want = np.concatenate([np.arange(1, n, 2), np.arange(0, n, 2)])
    for t in range(tw * th):
        ids = a[2][off[t]:off[t + 1]]
        assert ids.size == 0 or np.array_equal(ids, want)


def test_degenerate_counts():
    tw, th = 7, 5
    # no visible splat: offsets all zero, and the route query is not touched
    m2, radii, d = _random(200, tw, th, seed=1)
    a = _check(m2, np.zeros_like(radii), d, tw, th, expect=None)
    assert a[1].size == 0 and not a[3].any()
    # one splat in one tile
    one = lambda x, y: (np.array([[[x * TS + 8.0, y * TS + 8.0]]]), np.array([[2]], np.int32), np.array([[1.0]]))
    a = _check(*one(3, 2), tw, th)
    assert a[1].size == 1 and np.array_equal(a[3].reshape(-1), (np.arange(tw * th) > 2 * tw + 3).astype(np.int32))
    a = _check(*one(0, 0), 1, 1)
    assert a[1].size == 1 and a[3].reshape(-1).tolist() == [0]
    # splats only in the last tile: every tile in front of it has offset 0; only in the first: every later tile n_isects
    n = 70
    m2 = np.tile(np.array([(tw - 1) * TS + 8.0, (th - 1) * TS + 8.0]), (1, n, 1))
    radii, d = np.full((1, n), 3, np.int32), np.linspace(1, 2, n)[None]
    a = _check(m2, radii, d, tw, th)
    assert a[1].size == n and not a[3].any()
    a = _check(np.tile(np.array([8.0, 8.0]), (1, n, 1)), radii, d, tw, th)
    assert a[1].size == n and a[3].reshape(-1)[0] == 0 and (a[3].reshape(-1)[1:] == n).all()


@pytest.mark.parametrize("C", [2, 3])
def test_cameras_with_very_different_visible_sets(C):
    tw, th, n = 12, 9, 1500
    m2, radii, d = _random(n, tw, th, seed=C, C=C, rmax=60)
    radii[0, 5:] = 0                 # five splats in the first camera
    radii[C - 1, : n // 2] = 0       # half of them in the last
    if C == 3:
        radii[1] = 0                 # none in the middle one
    _check(m2, radii, d, tw, th)


def _direct(st, n_isects, n_kept, ids, flat, offsets, work, C):
    from gscodec_studio_amd import _backend as B

    B.call("gs_isect_finish_presorted", st["n_elems"], max(st["N"], 1), n_isects, B.ptr(st["perm"]), B.ptr(st["n_kept"]), None,
           B.ptr(st["means2d"]), st["s_m2"], B.ptr(st["radii"]), B.ptr(st["depths"]), B.ptr(st["tiles_per_gauss"]), B.ptr(st["gsums"]),
           B.ptr(st["gpre"]), TS, st["tile_width"], st["tile_height"], st["tile_n_bits"], st["cam_n_bits"], C, B.ptr(ids), B.ptr(flat),
           B.ptr(offsets), B.ptr(work), work.numel(), n_kept, B.ptr(st.get("sorted_keys")), torch.cuda.current_stream().cuda_stream)


def test_buffers_sized_for_a_capacity_and_reused_for_a_smaller_call():
    """The step driver's case: work buffer and outputs allocated for a capacity well above n_isects (the call fills a prefix),
    and the same buffers serve a second, smaller call; both with the pre-sort's keys and with perm + depths for the ids."""
    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd import _wrapper as W

    tw, th, cap = 20, 12, 60_000
    work = torch.empty(int(B.query("gs_isect_finish_work_bytes", cap)), dtype=torch.uint8, device=dev())
    ids = torch.full((cap,), -1, dtype=torch.int64, device=dev())
    flat = torch.full((cap,), -1, dtype=torch.int32, device=dev())
    offsets = torch.empty((1, th, tw), dtype=torch.int32, device=dev())
    for n, seed in ((2500, 3), (700, 4)):
        m2, radii, d = _random(n, tw, th, seed=seed, rmax=80)
        m2, radii, d = m2.astype(np.float32), radii.astype(np.int32), d.astype(np.float32)
        want, route = _finish(m2, radii, d, tw, th, False)
        k = want[1].size
        assert 0 < k < cap // 2
        for keys in (True, False):
            st = _begin(m2, radii, d, tw, th)
            n_isects, n_kept = st["sums"].wait()
            st["sums"].release()
            assert n_isects == k
            if not keys:
                st["sorted_keys"] = None
            ids.fill_(-1)
            flat.fill_(-1)
            prev = W.set_row_binning(True)
            try:
                _direct(st, n_isects, n_kept, ids, flat, offsets, work, 1)
            finally:
                W.set_row_binning(prev)
            assert W.isect_last_route() == "rows"
            assert np.array_equal(N(ids[:k]), want[1]) and np.array_equal(N(flat[:k]), want[2]) and np.array_equal(N(offsets), want[3])
            assert (N(ids[k:]) == -1).all() and (N(flat[k:]) == -1).all()  # nothing behind the prefix is written


def test_a_work_buffer_too_small_for_the_route_falls_back():
    """Thousands of kept splats that reach no tile need row counters the buffer for a handful of pairs does not hold: the call
    takes the old route, with the same outputs."""
    tw, th, n = 7, 250, 40_000
    rs = np.random.RandomState(5)
    m2 = np.stack([rs.uniform(-900, -500, (1, n)), rs.uniform(0, th * TS, (1, n))], -1)
    m2[0, :3] = [20.0, 30.0]
    radii = np.full((1, n), 4, np.int32)
    _check(m2, radii, rs.uniform(1, 2, (1, n)), tw, th, expect="packed")


def test_rasterization_is_bit_identical_with_the_route_on_and_off():
    from gscodec_studio_amd import _wrapper as W
    from gscodec_studio_amd import rasterization

    fx = garden(4000, scale_mult=3.0)
    Wd, Hd = 208, 120
    Ks = fx["Ks"][:1].copy()
    Ks[:, 0] *= Wd / fx["width"]
    Ks[:, 1] *= Hd / fx["height"]
    names = ("means", "quats", "scales", "opacities", "sh")
    res = {}
    for on in (True, False):
        prev = W.set_row_binning(on)
        try:
            P = {"means": T(fx["means"], True), "quats": T(fx["quats"], True), "scales": T(fx["scales"], True),
                 "opacities": T(fx["opacities"], True), "sh": T(garden_sh(fx["rgb"]), True)}
            rc, ra, meta = rasterization(P["means"], P["quats"], P["scales"], P["opacities"], P["sh"], T(fx["viewmats"][:1]), T(Ks), Wd, Hd,
                                         sh_degree=3, packed=False, deterministic=True)
            (rc * T(np.linspace(0.5, 1.5, 3, dtype=np.float32))).sum().add(ra.sum()).backward()
            torch.cuda.synchronize()
            res[on] = ([N(rc), N(ra)] + [N(meta[k]) for k in ("tiles_per_gauss", "isect_ids", "flatten_ids", "isect_offsets")]
                       + [N(P[k].grad) for k in names], W.isect_last_route())
        finally:
            W.set_row_binning(prev)
    assert res[True][1] == "rows" and res[False][1] in ("packed", "pairs")
    assert res[True][0][3].size > 4000
    for x, y in zip(res[True][0], res[False][0]):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
