"""The unsorted emission called directly: gs_isect_emit (64-bit ids) and gs_isect_emit_compact (32-bit keys) over an identity
order and over a permutation of the visible elements with a device-side count (perm / n_valid), fed like the chain feeds
them -- tiles_per_gauss from gs_isect_count, cum_tiles from gs_cumsum_i32 or gs_cumsum_gather_i32 -- against the oracle's
unsorted emission.  Bit-exact.  A wave owns 16 positions and walks its pairs 64 slots at a time: the sizes are one partial
group, a full one, one over and several workgroups, and one splat covers the whole grid (144 pairs: more than one walk)."""
import numpy as np
import pytest
import torch

from util import N, T

pytestmark = pytest.mark.gpu

from oracle import gs_oracle as O  # noqa: E402

TS, TW, TH = 16, 12, 12


def _scene(n, seed):
    rs = np.random.RandomState(seed)
    w, h = TW * TS, TH * TS
    m2 = np.stack([rs.uniform(-20, w + 20, n), rs.uniform(-20, h + 20, n)], -1).astype(np.float32)
    radii = rs.randint(1, 41, size=n).astype(np.int32)
    radii[rs.rand(n) < 1.0 / 3.0] = 0  # culled
    d = rs.choice(np.linspace(0.5, 8.0, 12), size=n).astype(np.float32)  # a dozen distinct depths: ties
    big = rs.randint(n)
    m2[big], radii[big] = (w / 2, h / 2), 2 * w  # covers all 144 tiles
    if np.count_nonzero(radii) % 16 == 0 and n > 16:  # the permuted run wants a count that is no multiple of a wave's 16
        radii[(big + 1) % n] = 0 if radii[(big + 1) % n] > 0 else 7
    return m2, radii, d


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("n", [1, 16, 17, 300])
def test_isect_emit_unsorted(n, permuted):
    from gscodec_studio_amd import _backend as B

    m2, radii, d = _scene(n, 11 + n)
    st = torch.cuda.current_stream().cuda_stream
    m2_t, r_t, d_t = T(m2), T(radii), T(d)
    tpg = torch.full((n,), -1, dtype=torch.int32, device=r_t.device)
    B.call("gs_isect_count", n, B.ptr(m2_t), 2, B.ptr(r_t), TS, TW, TH, B.ptr(tpg), st)
    cum = torch.empty(n, dtype=torch.int64, device=r_t.device)
    sb = B.query("gs_cumsum_scratch_bytes", n)
    scratch = torch.empty(sb, dtype=torch.uint8, device=r_t.device)
    if permuted:
        vis = np.nonzero(radii > 0)[0]
        order = np.random.RandomState(n).permutation(vis).astype(np.int32)
        if n > 16:
            assert len(order) % 16 != 0
        # behind the count perm is undefined: in-bounds entries of visible elements that must never show up
        perm = np.concatenate([order, np.full(n - len(order), order[0], np.int32)])
        perm_t, nv_t = T(perm), T(np.array([len(order)], np.int32))
        B.call("gs_cumsum_gather_i32", n, B.ptr(tpg), B.ptr(perm_t), B.ptr(nv_t), B.ptr(cum), B.ptr(scratch), sb, st)
        perm_p, nv_p = B.ptr(perm_t), B.ptr(nv_t)
    else:
        order = np.arange(n, dtype=np.int32)
        B.call("gs_cumsum_i32", n, B.ptr(tpg), B.ptr(cum), B.ptr(scratch), sb, st)
        perm_p, nv_p = None, None
    # the oracle on the inputs in emission order; its flatten ids are positions
    e_tpg, e_ids, e_pos = O.isect_tiles(m2[order][None], radii[order][None], d[order][None], TS, TW, TH, sort=False)
    e_flat = order[e_pos]
    n_isects = len(e_ids)
    assert n_isects >= TW * TH
    assert np.array_equal(N(tpg), O.isect_tiles(m2[None], radii[None], d[None], TS, TW, TH, sort=False)[0][0])
    assert np.array_equal(N(cum)[: len(order)], np.cumsum(e_tpg[0].astype(np.int64)))
    tb, _ = O.tile_bits(TW * TH, 1)

    ids = torch.full((n_isects,), -1, dtype=torch.int64, device=r_t.device)
    flat = torch.full((n_isects,), -1, dtype=torch.int32, device=r_t.device)
    B.call("gs_isect_emit", n, n, perm_p, nv_p, None, B.ptr(m2_t), 2, B.ptr(r_t), B.ptr(d_t), B.ptr(cum), TS, TW, TH, tb,
           B.ptr(ids), B.ptr(flat), st)
    assert np.array_equal(N(ids), e_ids)
    assert np.array_equal(N(flat), e_flat)

    keys32 = torch.full((n_isects,), -1, dtype=torch.int32, device=r_t.device)
    flat_c = torch.full((n_isects,), -1, dtype=torch.int32, device=r_t.device)
    B.call("gs_isect_emit_compact", n, n, perm_p, nv_p, None, B.ptr(m2_t), 2, B.ptr(r_t), B.ptr(d_t), B.ptr(cum), TS, TW, TH, tb,
           B.ptr(keys32), B.ptr(flat_c), st)
    assert np.array_equal(N(keys32).astype(np.int64), e_ids >> 32)
    assert np.array_equal(N(flat_c), e_flat)
