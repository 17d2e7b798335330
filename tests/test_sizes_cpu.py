"""CPU: the size queries the callers allocate with, as functions of the element count.

Both radix sorts change their block from 1024 to 4096 keys above 2^21 keys, so the per-block histogram of their temp layout has
fewer rows just above the switch than just below it.  The step driver (_step._finish) allocates the binning's work buffer BEFORE
it knows the intersection count, for a capacity a little above the last count, and keeps it whenever the count fits: that is
only right if a buffer sized for n serves every smaller count, i.e. if the queries never decrease.  Checked here on the library
itself (no launches), together with the driver's own keep / grow rule; the values up to 2^21 are pinned to what the library
returned before the histogram region was sized for the larger of the two block layouts."""
import hashlib

import pytest

SWITCH = 1 << 21
QUERIES = ("gs_sort_temp_bytes", "gs_sort_isect_temp_bytes", "gs_presort_temp_bytes", "gs_isect_finish_work_bytes",
           "gs_cumsum_scratch_bytes")


def _sweep():
    ns = {0, 1}
    for c in (1024, 4096):
        ns.update((c - 1, c, c + 1))
    ns.update(range(SWITCH - 5000, SWITCH + 5001))
    for k in range(2, 9):
        ns.update((k * SWITCH - 1, k * SWITCH, k * SWITCH + 1))
    ns.update(int(round(2.0 ** (26.0 * i / 199.0))) for i in range(200))  # 1 ... 2^26, log-spaced
    return sorted(ns)


SWEEP = _sweep()


@pytest.fixture(scope="module")
def sizes():
    """name -> f(n), each value asked of the library once."""
    from gscodec_studio_amd import _backend as B

    cache = {}

    def make(name):
        fn = getattr(B.lib(), name)

        def f(n):
            v = cache.get((name, n))
            if v is None:
                v = cache[name, n] = int(fn(n))
            return v

        return f

    return {name: make(name) for name in QUERIES}


def _window(bad):
    return f"{len(bad)} violations, n in [{min(b[0] for b in bad):,}, {max(b[0] for b in bad):,}]; first {bad[0]}, last {bad[-1]}"


@pytest.mark.parametrize("name", QUERIES)
def test_size_query_is_non_decreasing(sizes, name):
    f = sizes[name]
    bad = [(a, b, f(a), f(b)) for a, b in zip(SWEEP, SWEEP[1:]) if f(a) > f(b)]
    if bad:
        print(f"{name} decreases: {_window(bad)}")
    assert not bad, f"{name}(a) > {name}(b) for a < b: {_window(bad)}"


@pytest.mark.parametrize("name", QUERIES)
def test_buffer_sized_for_the_next_capacity_serves_smaller_counts(sizes, name):
    """The reuse rule as the step driver applies it: a buffer of f(cap) bytes, cap = the capacity after a call with n, is handed
    to calls with any count up to cap -- n itself, cap, and the counts around the block switch when they lie below cap."""
    from gscodec_studio_amd import _step

    f = sizes[name]
    bad = []
    for n in SWEEP:
        cap = _step._next_cap(n)
        assert cap == n + (n >> 5) + 4096  # (what the sweep below was laid out for: 3 % + 4096 above the count)
        for m in (n, cap, SWITCH - 1, SWITCH, SWITCH + 1):
            if 0 <= m <= cap and f(cap) < f(m):
                bad.append((n, cap, m, f(cap), f(m)))
    if bad:
        print(f"{name}(cap) < {name}(m), m <= cap: {_window(bad)}")
    assert not bad, f"{name}: a buffer for cap is too small for m <= cap: {_window(bad)}"


def _replay(f, counts):
    """_step._finish's buffer decision over a sequence of intersection counts of one call shape -> [(n, cap, kept, shortfall)] of
    the calls whose work buffer gs_isect_finish_presorted would refuse."""
    from gscodec_studio_amd import _step

    cap, bad = 0, []
    for n in counts:
        work_bytes = f(cap) if cap else None  # allocated before the read-back, for the capacity of the last call
        kept = work_bytes is not None and _step._cap_serves(cap, n)
        if not kept:
            work_bytes = f(n)  # exact, after the read-back
        if n > 0 and work_bytes < f(n):
            bad.append((n, cap, kept, f(n) - work_bytes))
        cap = _step._next_cap(n)
    return bad


SEQUENCES = [
    [2_060_000, 2_060_000, 2_097_152, 2_097_153, 2_125_000, 2_600_000, 1_000, 0, 2_060_000],
    [2_040_000, 2_045_000, 2_107_846, 2_040_000, 2_107_846],  # small steps below the switch, their capacity above it
    [3_000_000, 2_950_000, 2_200_000, 2_150_000, 2_097_153, 2_097_152, 2_097_151, 2_050_000, 2_000_000],  # downwards
    [1_900_000, 1_950_000, 2_000_000, 2_050_000, 2_097_151, 2_097_152, 2_097_153, 2_150_000, 2_200_000],  # upwards
    [2_029_631, 2_029_631, 2_029_632, 2_029_632, 2_097_152, 2_097_152, 2_097_153, 2_097_153],  # the ends of the window
    [4_000_000, 0, 4_000_000, 1, 2_097_152, 2_097_152],
]


@pytest.mark.parametrize("counts", SEQUENCES, ids=lambda c: "-".join(str(n) for n in c[:3]))
def test_step_driver_keeps_only_buffers_that_are_large_enough(sizes, counts):
    bad = _replay(sizes["gs_isect_finish_work_bytes"], counts)
    if bad:
        print(f"work buffer too small at (n_isects, cap, kept, missing bytes): {bad}")
    assert not bad, f"kept work buffer smaller than gs_isect_finish_work_bytes(n_isects): {bad}"


def test_same_count_twice_never_outgrows_its_buffer(sizes):
    """The plainest sequence -- the same view rendered twice -- for EVERY count from 1.9 M to 2.2 M: the second call runs in the
    buffer sized for _next_cap(n).  (Prints the window of counts that fail, so a regression names its range.)"""
    from gscodec_studio_amd import _step

    f = sizes["gs_isect_finish_work_bytes"]
    at_cap = {}
    bad = []
    for n in range(1_900_000, 2_200_001):
        cap = _step._next_cap(n)
        have = at_cap.get(cap)
        if have is None:
            have = at_cap[cap] = f(cap)
        if _step._cap_serves(cap, n) and have < f(n):
            bad.append((n, cap, have, f(n)))
    if bad:
        print(f"second render of the same view fails: {_window(bad)}")
    assert not bad, f"work buffer too small on the second call: {_window(bad)}"


# What the library returned at these counts before the histogram region was sized for the larger block layout (recorded from a
# build of that commit): up to 2^21 nothing may move, offsets included -- gs_isect_count_keys writes the first pass's histogram
# where the sort expects it.  Columns as QUERIES.
RECORDED = {
    0: (1024, 1024, 1024, 1024, 8),
    1: (2560, 2560, 2568, 3072, 16),
    1023: (14336, 10240, 22520, 18432, 16),
    1024: (14336, 10240, 22528, 18432, 16),
    1025: (15872, 11776, 24072, 20480, 16),
    4095: (54272, 37888, 87032, 70656, 24),
    4096: (54272, 37888, 87040, 70656, 24),
    4097: (55808, 39424, 88584, 72704, 32),
    100000: (1301504, 901632, 2101504, 1701888, 400),
    1000000: (13001472, 9001472, 21001472, 17001472, 3920),
    2029632: (26387200, 18268672, 42624256, 34505728, 7944),
    2040000: (26521856, 18361856, 42841856, 34681856, 7984),
    2092152: (27200000, 18831360, 43937216, 35568640, 8184),
    2097151: (27264000, 18875392, 44041208, 35652608, 8200),
    2097152: (27264000, 18875392, 44041216, 35652608, 8200),
}
# sha256 over "name:n=value\n" for every query and every SWEEP count up to 2^21, in QUERIES / ascending order (same build)
RECORDED_DIGEST = "bd18002eacb275c8c8085153ddc5bb1430748ebe65a8ac85108598da894a3549"


def test_sizes_up_to_the_switch_are_unchanged(sizes):
    for n, want in RECORDED.items():
        assert n <= SWITCH
        got = tuple(sizes[name](n) for name in QUERIES)
        assert got == want, (n, got, want)
    h = hashlib.sha256()
    for name in QUERIES:
        for n in SWEEP:
            if n <= SWITCH:
                h.update(f"{name}:{n}={sizes[name](n)}\n".encode())
    assert h.hexdigest() == RECORDED_DIGEST


def test_extra_memory_above_the_switch_is_bounded(sizes):
    """Above the switch the histogram keeps at least the 2048 rows of blocks that 2^21 keys need: at most 256 digits * 2048 blocks
    * 4 bytes = 2 MiB minus the rows the count needs itself, and nothing once the count has 2048 blocks of its own (8 M keys)."""
    for name, per_key in (("gs_sort_temp_bytes", 12), ("gs_sort_isect_temp_bytes", 8), ("gs_presort_temp_bytes", 20),
                          ("gs_isect_finish_work_bytes", 16)):
        f = sizes[name]
        for n in SWEEP:
            if n > SWITCH:
                blocks = -(-n // 4096)
                rows = max(blocks, 2048)
                payload = per_key * n + 256 * rows * 4 + 1024
                assert payload <= f(n) <= payload + 6 * 256, (name, n, f(n), payload)
