"""CPU: the numpy restatements of tests/exchange_reference.py, pinned before any kernel is compared with them.

plan / visibility / reduce_rows against the torch formulations distributed.py keeps as its CPU / gloo route, on every rank of
a world-2 and a world-3 gloo group (worker: tests/test_distributed_cpu.py::_exchange_restatements); rows_exchange against a
loop over single (sender, camera, gaussian) triples at toy size; and the conditions the GPU cases of
tests/test_gpu_exchange.py state about their inputs, on the same seeds, so they are known to hold before a GPU is touched."""
import numpy as np
import pytest

import exchange_reference as XR
from test_distributed_cpu import _run


def test_restatements_match_torch_formulations_world2():
    _run("_exchange_restatements", world=2)


def test_restatements_match_torch_formulations_world3():
    _run("_exchange_restatements", world=3)


def test_plan_by_hand():
    """W = 2, block = 3: every field of the plan written out."""
    m = np.array([[0, 1, 0, 0, 1, 1],
                  [0, 1, 1, 0, 0, 1]], dtype=np.uint8)
    p = XR.plan(m, 3)
    assert p.rows.tolist() == [[1, 2], [2, 1]] and p.urows.tolist() == [2, 2]
    assert p.counts.tolist() == [1, 2, 2, 1, 2, 2]
    assert p.send_idx[0].tolist() == [1, 4, 5] and p.send_idx[1].tolist() == [1, 2, 5]
    assert p.uidx.tolist() == [1, 2, 4, 5] and p.urank[p.union].tolist() == [0, 1, 2, 3]
    assert XR.visibility(np.array([[0, 3, -1], [0, 0, -1]]), 5).tolist() == [0, 1, 0, 0, 0]
    assert XR.visibility(np.zeros((0, 3), np.int32), 4).tolist() == [0, 0, 0, 0]


def test_reduce_rows_by_hand():
    """Owner 1 of the plan above (its block: splats 3..5, union rows 4 and 5): sender order, the -1 rows, scale and padding."""
    p = XR.plan(np.array([[0, 1, 0, 0, 1, 1], [0, 1, 1, 0, 0, 1]], dtype=np.uint8), 3)

    def row(i, *v):
        return [float(np.array(i, np.int32).view(np.float32))] + list(v)

    wire = np.array([row(4, 1.0, 2.0), row(5, 1e8, -0.0), row(-1, 9.0, 9.0), row(5, 1.0, -0.0)], dtype=np.float32)
    acc = XR.reduce_rows(wire, [0, 3, 4], p.urank, 2, p.uidx[2:4], 3, 0.5)
    assert acc[:, 0].copy().view(np.int32).tolist() == [4, 5, -1]
    assert acc[:, 1:].tolist() == [[0.5, 1.0], [0.5 * float(np.float32(1e8) + np.float32(1.0)), 0.0], [0.0, 0.0]]
    assert not np.signbit(acc[1, 2])  # +0.0f + -0.0f + -0.0f
    with pytest.raises(AssertionError):  # two rows of one sender for one splat
        XR.reduce_rows(np.array([row(4, 1.0), row(4, 1.0)], dtype=np.float32), [0, 2, 2], p.urank, 2, p.uidx[2:4], 3, 1.0)


@pytest.mark.parametrize("W, C_local", [(1, 2), (2, 1), (3, 2)])
def test_rows_exchange_against_triple_loop(W, C_local):
    rng = np.random.default_rng(W)
    N_world = [[4], [3, 0], [2, 5, 1]][W - 1]
    C_total, N_total = C_local * W, sum(N_world)
    radii_s = [rng.integers(-1, 2, size=(C_total, n)).astype(np.int32) * 3 for n in N_world]
    rows_s = [rng.standard_normal((C_total * n, XR.ROW)).astype(np.float32) if n else None for n in N_world]
    for s, n in enumerate(N_world):
        if n:
            rows_s[s][:, XR.ROW_RADIUS] = radii_s[s].reshape(-1).view(np.float32)
    cap_world = [2] * W
    ex = XR.rows_exchange(radii_s, rows_s, C_local, N_world, cap_world)
    want = [dict() for _ in range(W)]  # destination -> {destination row: source row}
    counts = np.zeros((W, W), dtype=np.int64)
    for s in range(W):
        for c in range(C_total):
            for n in range(N_world[s]):
                if radii_s[s][c, n] > 0:
                    d = c // C_local
                    want[d][(c % C_local) * N_total + sum(N_world[:s]) + n] = rows_s[s][c * N_world[s] + n]
                    counts[s, d] += 1
    assert np.array_equal(ex.counts, counts) and ex.max_count.tolist() == counts.max(1).tolist()
    assert ex.over.tolist() == [bool((counts[s] > 2).any()) for s in range(W)] and ex.overflow == bool((counts > 2).any())
    for d in range(W):
        radii, depths, rows = ex.radii[d].reshape(-1), ex.depths[d].reshape(-1), ex.rows[d].reshape(-1, XR.ROW)
        assert sorted(np.flatnonzero(radii > 0).tolist()) == sorted(want[d]) and (radii[radii <= 0] == 0).all()
        for dst, src in want[d].items():
            assert radii[dst] == 3 and depths[dst] == src[XR.ROW_DEPTH]
            keep = [k for k in range(XR.ROW) if k not in (XR.ROW_DST, XR.ROW_AUX)]
            assert np.array_equal(rows[dst][keep].view(np.int32), src[keep].view(np.int32))
            assert rows[dst][[XR.ROW_DST, XR.ROW_AUX]].view(np.int32).tolist() == [dst, 0]
        assert (depths[radii <= 0] == 0).all()


# --------------------------------------------------------------------------- the conditions the GPU cases state on their inputs
@pytest.mark.parametrize("variant", XR.PLAN_VARIANTS)
@pytest.mark.parametrize("W, block", XR.PLAN_CASES)
def test_plan_case_inputs(W, block, variant):
    m = XR.plan_masks(W, block, variant)
    f = XR.check_plan_masks(m, W, block, variant)
    tiles = -(-W * block // XR.PLAN_TILE)
    if (W, block) == (2, 1024):
        assert tiles == 1
    if (W, block) == (2, 1025):
        assert tiles == 2 and XR.PLAN_TILE // block == 1 and XR.PLAN_TILE % block != 0  # a tile edge inside owner block 1
    p = XR.plan(m, block)
    assert int(p.counts[:W * W].reshape(W, W).sum()) == int(m.sum()) and int(p.urows.sum()) == p.uidx.size

    def tile_has_rows(t):  # a tile whose count matters to its successors / a successor whose rows show a wrong offset
        return bool(p.union[t * XR.PLAN_TILE:(t + 1) * XR.PLAN_TILE].any())

    if (W, block) == (16, 8197):
        assert tiles == 65 and f["full_tile"] is not None     # the last tile has 64 predecessors: all 64 lanes of the first wave
        assert tile_has_rows(63) and tile_has_rows(64)
    if (W, block) == (16, 8401):
        assert tiles == 66 and f["full_tile"] is not None     # 65 predecessors: tile 64 is added by a lane of the SECOND wave
        assert tile_has_rows(64) and tile_has_rows(65)
    if (W, block) == (3, 176129):
        assert tiles == 259 and f["full_tile"] is not None    # threads 0 and 1 of the last tile add TWO predecessor tiles each
        assert tile_has_rows(0) and tile_has_rows(1) and tile_has_rows(256) and tile_has_rows(257) and tile_has_rows(258)


@pytest.mark.parametrize("umax", XR.REDUCE_UMAX)
@pytest.mark.parametrize("W, width", XR.REDUCE_CASES)
def test_reduce_case_inputs(W, width, umax):
    for owner in XR.reduce_owners(W):
        p, wire, starts, uoff, uidx_mine = XR.reduce_inputs(W, width, umax, owner)
        XR.check_reduce_inputs(W, owner, p, wire, starts, uoff, uidx_mine, umax)
        assert wire.shape[1] == 1 + width and wire.nbytes < 48 << 20


@pytest.mark.parametrize("C_local", [1, 2])
@pytest.mark.parametrize("W", sorted(XR.EXCHANGE_WORLDS))
def test_exchange_case_inputs(W, C_local):
    N_world, radii_s, rows_s = XR.exchange_inputs(W, C_local)
    counts = XR.check_exchange_inputs(W, C_local, N_world, radii_s)
    assert len(N_world) == W and (W in (1, 3) or 0 in N_world)  # an owner of nothing (a NULL rows pointer)
    assert all((rows is None) == (n == 0) for rows, n in zip(rows_s, N_world))
    for kind in XR.EXCHANGE_CAPS:
        caps = XR.exchange_caps(counts, kind)
        ex = XR.rows_exchange(radii_s, rows_s, C_local, N_world, caps)
        assert np.array_equal(ex.counts, counts)
        assert ex.overflow == (kind == "short")
        if kind == "short":  # exactly the senders with something to send overflow; some sender's chunks all fit (W > 1)
            assert ex.over.tolist() == [bool(c > 0) for c in counts.max(1)] and (W == 1 or not ex.over.all())
