"""The host's one wait per step (`_readback._SentinelEvent`: block sums appearing in pinned memory) must be BOUNDED: a kernel
that never stores, a stream that is stuck, or a device fault raise a RuntimeError instead of spinning a core for good
(round-4 verdict / advisor finding; the reference's blocking `.item()` of isect_tiles.cu:200 raises on a HIP error too)."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu


def _pinned(n=64):
    buf = torch.empty(n, dtype=torch.int32, pin_memory=True)
    buf.fill_(-1)
    return buf


def test_never_written_buffer_raises_instead_of_hanging():
    from gscodec_studio_amd import _readback as W

    torch.cuda.synchronize()
    ev = W._SentinelEvent(_pinned(), what="test sums")
    t0 = time.perf_counter()
    with pytest.raises(RuntimeError, match="never arrived"):
        W._wait_event(ev)
    assert time.perf_counter() - t0 < 2.0


def test_busy_stream_times_out():
    from gscodec_studio_amd import _readback as W

    ev = W._SentinelEvent(_pinned(), what="test sums")
    torch.cuda._sleep(int(2.4e9 * 1.5))  # ~1.5 s of GPU time queued in front
    t0 = time.perf_counter()
    with pytest.raises(RuntimeError, match="timed out"):
        ev.synchronize(timeout_s=0.2)
    assert 0.15 < time.perf_counter() - t0 < 1.0
    torch.cuda.synchronize()


def test_late_store_is_seen():
    from gscodec_studio_amd import _readback as W

    buf = _pinned()
    src = torch.arange(64, dtype=torch.int32, device="cuda")
    ev = W._SentinelEvent(buf, what="test sums")
    torch.cuda._sleep(int(2.4e9 * 0.05))  # the store comes ~50 ms late: past the spin phase, into the naps
    buf.copy_(src, non_blocking=True)
    W._wait_event(ev)
    assert ev.query() and int(buf[-1]) == 63
    torch.cuda.synchronize()


def test_partial_store_is_not_taken_for_complete():
    from gscodec_studio_amd import _readback as W

    buf = _pinned()
    buf[0] = 5
    buf[-1] = 7
    assert not W._SentinelEvent(buf).query()
    buf[1:-1] = 0
    assert W._SentinelEvent(buf).query()


# ---- `_readback.BlockSums`: the buffer's way from the take to the hand-back.  The stand-in for the count kernel's stores is a
# non-blocking copy into the buffer behind ~50 ms of GPU time, as in test_late_store_is_seen; 3 blocks (6 ints) is the smallest
# size with interior entries, which only the minimum scan of `query()` looks at.

def _stored(n_sums=3):
    from gscodec_studio_amd import _readback as RB

    return RB.BlockSums.stored(n_sums, torch.cuda.current_stream())


def _late_store(sums):
    src = torch.arange(sums.buf.numel(), dtype=torch.int32, device="cuda")
    torch.cuda._sleep(int(2.4e9 * 0.05))
    sums.buf.copy_(src, non_blocking=True)


def _settle(sums):
    """Hand a buffer no kernel writes back without the abandon watch: the host stores the sums itself."""
    sums.buf.fill_(0)
    sums.wait()
    sums.release()


def test_abandoned_buffer_is_not_reused_before_its_stores_land():
    sums = _stored()
    ptr = sums.buf.data_ptr()
    _late_store(sums)
    del sums  # (no release, no abandon: __del__ watches for the stores)
    nxt = _stored()
    assert nxt.buf.data_ptr() == ptr and nxt.buf.tolist() == [-1] * 6
    torch.cuda.synchronize()
    assert nxt.buf.tolist() == [-1] * 6  # ... and none of the stores was still under way
    _settle(nxt)


def test_buffer_whose_stores_are_late_is_parked(monkeypatch):
    from gscodec_studio_amd import _readback as RB

    monkeypatch.setattr(RB, "_ABANDON_S", 0.010)
    sums = _stored()
    buf, ptr = sums.buf, sums.buf.data_ptr()
    _late_store(sums)
    del sums
    nxt = _stored()
    assert nxt.buf.data_ptr() != ptr
    torch.cuda.synchronize()
    assert buf.tolist() == list(range(6))
    assert RB._PARKED[-1] is buf and all(b is not buf for b in RB._PINNED_FREE.get(6, []))
    _settle(nxt)


def test_abandon_never_raises(monkeypatch):
    from gscodec_studio_amd import _readback as RB

    monkeypatch.setattr(RB, "_ABANDON_S", 0.05)
    torch.cuda.synchronize()  # a drained stream and a buffer nothing writes: what makes the wait raise "never arrived"
    sums = _stored()
    buf = sums.buf
    t0 = time.perf_counter()
    sums.abandon()
    assert time.perf_counter() - t0 < 0.05 + 0.25
    assert RB._PARKED[-1] is buf and all(b is not buf for b in RB._PINNED_FREE.get(6, []))
    n_parked = len(RB._PARKED)
    sums.abandon()
    sums.release()
    assert len(RB._PARKED) == n_parked and all(b is not buf for b in RB._PINNED_FREE.get(6, []))


def test_wait_is_idempotent():
    from gscodec_studio_amd import _readback as RB

    sums = _stored()
    buf = sums.buf
    buf.copy_(torch.tensor([5, 1, 7, 0, 9, 2], dtype=torch.int32, device="cuda"), non_blocking=True)
    assert sums.wait() == (21, 3) and sums.wait() == (21, 3)
    sums.release()
    sums.release()
    assert sum(b is buf for b in RB._PINNED_FREE[6]) == 1
    nxt = _stored()
    assert nxt.buf is buf and buf.tolist() == [-1] * 6
    assert sums.wait() == (21, 3)
    sums.release()
    sums.abandon()
    assert all(b is not buf for b in RB._PINNED_FREE[6])  # (still nxt's)
    _settle(nxt)


@pytest.fixture(scope="module")
def binning_case():
    """C = 1, N = 3000 (3 count blocks) on a 128 x 128 image with 16-pixel tiles, and its ``isect_tiles``."""
    from gscodec_studio_amd import _wrapper as W

    g = torch.Generator(device="cpu").manual_seed(11)
    means2d = (torch.rand(1, 3000, 2, generator=g) * 128).cuda()
    radii = torch.randint(-2, 40, (1, 3000), generator=g, dtype=torch.int32).cuda()
    depths = (torch.rand(1, 3000, generator=g) * 10 + 0.1).cuda()
    args = (means2d, radii, depths, 16, 8, 8)
    return args, W.isect_tiles(*args)


def test_begin_without_finish(binning_case):
    from gscodec_studio_amd import _readback as RB
    from gscodec_studio_amd import _wrapper as W

    args, want = binning_case
    n_parked = len(RB._PARKED)
    st = W.isect_tiles_begin(*args, True, 1, 3000, 3000, None)
    assert st["sums"].sentinel is not None and st["sums"].buf.numel() == 6
    del st
    torch.cuda.synchronize()
    assert len(RB._PARKED) == n_parked
    got = W.isect_tiles(*args)
    assert want[1].numel() > 0
    for a, b in zip(want, got):
        assert torch.equal(a, b)


def test_both_read_back_forms_agree(binning_case, monkeypatch):
    from gscodec_studio_amd import _readback as RB
    from gscodec_studio_amd import _wrapper as W

    args, want = binning_case
    a = W.isect_tiles_begin(*args, True, 1, 3000, 3000, None)
    monkeypatch.setattr(RB, "_PINNED_DIRECT_MAX", 0)
    b = W.isect_tiles_begin(*args, True, 1, 3000, 3000, None)
    c = W.isect_tiles_begin(*args, False, 1, 3000, 3000, None)
    assert a["sums"].sentinel is not None and b["sums"].sentinel is None and c["sums"].sentinel is None
    totals = a["sums"].wait()
    assert totals == b["sums"].wait() == (want[1].numel(), int(a["n_kept"]))
    assert c["sums"].wait() == (int(c["tiles_per_gauss"].sum()), 0) and c["sums"].wait()[0] == totals[0]
    for st in (a, b, c):
        st["sums"].release()
