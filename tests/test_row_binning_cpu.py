"""CPU: the sizes, limits and the switch of the row-binning route of gs_isect_finish_presorted (no launches).

The route lays its arrays out in the work buffer it is handed and is only taken when they fit, so gs_isect_finish_work_bytes
stays what it was: a function of n_isects alone that never decreases.  The route's own need changes form wherever one of its
arrays crosses a 256-byte boundary or gains a chunk: at multiples of 32 pairs (8-byte entries), of 512 (one more chunk of
column counters, one more block of row counters) and their neighbours."""
import pytest

CHUNK = 512  # entries per chunk of a row list = positions per block of the row histogram
BENCH = dict(n_isects=3_997_870, n_kept=292_931, rows=68, tw=120)  # config 2: one 1080p camera


def _lib():
    from gscodec_studio_amd import _backend as B

    return B.lib()


def _sweep():
    ns = set(range(0, 3 * CHUNK + 2))
    for k in (1, 2, 3, 7, 8, 64, 255, 256, 257, 1000, 4095, 4096, 7808, 8192):
        for d in (-33, -32, -31, -1, 0, 1, 31, 32, 33):
            ns.add(max(0, k * CHUNK + d))
    ns.update(int(round(2.0 ** (26.0 * i / 149.0))) for i in range(150))
    return sorted(ns)


def test_finish_work_bytes_never_decreases_where_the_route_changes_form():
    f = _lib().gs_isect_finish_work_bytes
    ns = _sweep()
    vals = [int(f(n)) for n in ns]
    bad = [(a, b, x, y) for a, b, x, y in zip(ns, ns[1:], vals, vals[1:]) if x > y]
    assert not bad, bad[:5]


@pytest.mark.parametrize("rows,tw,kept_per_pair", [(68, 120, 0.08), (1, 1, 1.0), (256, 256, 0.25), (5, 7, 1.0)])
def test_route_need_never_decreases_in_the_count(rows, tw, kept_per_pair):
    g = _lib().gs_isect_row_binning_work_bytes
    ns = _sweep()
    vals = [int(g(n, max(1, int(n * kept_per_pair)), rows, tw)) for n in ns]
    bad = [(a, b, x, y) for a, b, x, y in zip(ns, ns[1:], vals, vals[1:]) if x > y]
    assert not bad, bad[:5]
    # and in each of the other arguments
    n = 100_000
    assert int(g(n, 5000, rows, tw)) <= int(g(n, 5001, rows, tw)) <= int(g(n, 50_000, rows, tw))


def test_bench_frame_and_the_step_drivers_capacity_fit_the_work_buffer():
    """The headline frame takes the route with room to spare, also in a buffer the step driver kept from a larger count."""
    from gscodec_studio_amd import _step

    L = _lib()
    n, kept, rows, tw = BENCH["n_isects"], BENCH["n_kept"], BENCH["rows"], BENCH["tw"]
    have = int(L.gs_isect_finish_work_bytes(n))
    assert int(L.gs_isect_row_binning_work_bytes(n, kept, rows, tw)) <= have
    assert int(L.gs_isect_row_binning_work_bytes(n, n // 2, rows, tw)) <= have  # two tiles per kept splat still fit
    cap = _step._next_cap(n)
    assert int(L.gs_isect_row_binning_work_bytes(n, kept, rows, tw)) <= int(L.gs_isect_finish_work_bytes(cap))
    # a single pair on a small grid fits the smallest buffer there is
    assert int(L.gs_isect_row_binning_work_bytes(1, 1, 5, 7)) <= int(L.gs_isect_finish_work_bytes(1))


def test_limits_and_switch():
    from gscodec_studio_amd import _wrapper as W

    # the headline frame's row counters are well inside GS_ROW_BINNING_MAX_COUNTERS
    assert BENCH["rows"] * -(-BENCH["n_kept"] // CHUNK) <= 131072 // 3
    prev = W.set_row_binning(None)
    try:
        assert W.set_row_binning(False) == prev
        assert W.set_row_binning(None) is False
        assert W.set_row_binning(True) is False
        assert W.set_row_binning(None) is True
    finally:
        W.set_row_binning(prev)
    assert W.set_row_binning(None) == prev
    assert W.isect_last_route() in ("none", "pairs", "packed", "rows")
