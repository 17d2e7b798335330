"""The one host read-back of every ``rasterization()`` call: the count kernel's per-block (intersections, visible) sums, which the host
adds up to ``n_isects`` / ``n_kept``.  ``BlockSums`` owns the pinned buffer, the wait and the totals for every producer
(``_wrapper.isect_tiles_begin``, ``_step._phase1``).  Its rule: a buffer a kernel stores into is reused only once every entry has been
seen >= 0, and never goes back to torch's pinned allocator, which does not track kernel stores -- its next owner would get them."""
import os
import time
from typing import Optional, Tuple

import torch
from torch import Tensor

_PINNED_FREE: dict = {}  # size -> stored buffers ready for reuse (the steady state makes no pinned allocation)
_PARKED: list = []  # stored buffers a kernel may still write to: kept alive for good, never handed out again
_ABANDON_S = 1.0  # how long abandon() watches for the stores of a kernel that is still queued
# A few thousand blocks -- 983 at 1 M splats -- store straight into pinned memory (4-byte PCIe writes); beyond that the sums are added
# up on the device and 8 bytes are copied, as in round 1: with 48 K block sums per step at 49 M splats, stored directly OR copied as
# one 192 KB block, every third or fourth forward stalled the GPU for ~85 ms
_PINNED_DIRECT_MAX = 2048


def direct_block_sums(n_elems: int) -> bool:
    """The same bound in elements (one count block per 1024): what both uses of the step driver need."""
    return 0 < n_elems <= _PINNED_DIRECT_MAX * 1024


def block_sum_totals(a) -> Tuple[int, int]:
    """(sum of the even entries, sum of the odd entries) of the pinned int32 block-sum array [(intersections, visible)] -- exact, and
    ~10 us instead of the ~50 of ``a.reshape(-1, 2).sum(0)`` (a strided reduction with a dtype conversion), which sat between the
    host's read-back and the binning launch with the GPU waiting (round 6, tools/host_timeline.py).  The non-negative pairs are read as
    int64 words (little endian: even entry = low half, odd entry = high half) and the halves summed separately."""
    w = a.view("int64")
    return int((w & 0xFFFFFFFF).sum()), int((w >> 32).sum())


def _pinned_take(n: int) -> Tensor:
    """A pinned int32 buffer the count kernel stores its block sums into, PRE-SET to -1: every sum is >= 0, so the host sees
    the kernel's progress in the buffer itself (``_SentinelEvent``) and no event has to be recorded behind the kernel -- a
    recorded event is a barrier packet in the queue, ~6 us of idle GPU between the count kernel and the pre-sort."""
    free = _PINNED_FREE.get(n)
    buf = free.pop() if free else torch.empty(n, dtype=torch.int32, pin_memory=True)
    buf.fill_(-1)
    return buf


_WAIT_TIMEOUT_S = float(os.environ.get("GS_WAIT_TIMEOUT_S", "600"))  # backstop of any host wait on a BUSY stream (<= 0: none)
_WAIT_WARNED = [False]


class _SentinelEvent:
    """``query`` / ``synchronize`` of an event over a pinned buffer whose entries go from -1 to >= 0 as the kernel stores them
    (posted 4-byte writes of independent workgroups into host-coherent memory: each becomes visible on its own -- the
    mechanism needs fine-grained coherent pinned memory, HIP's default for ``hipHostMalloc``; with HIP_HOST_COHERENT=0 the
    stores only show at a synchronisation point, which the stream check below turns into a late but correct result).

    The wait is BOUNDED and notices a dead GPU: round 4's query / yield loop for the first few hundred polls, then a yielding spin up to 20 ms, naps after that; every ~2 ms the launch stream is queried -- a
    device fault raises there, and a stream that has drained while the sentinel is still unset means the kernel never stored
    (failed launch, lost write): RuntimeError instead of a core spinning for good.  A stream that is still busy is waited for (one
    warning after 30 s); ``GS_WAIT_TIMEOUT_S`` (600; <= 0: none) is only the backstop behind that."""

    __slots__ = ("buf", "np", "stream", "what")

    def __init__(self, buf: Tensor, stream=None, what: str = "the count kernel's block sums (isect_count_keys_kernel / projection_fwd_kernel)"):
        self.buf = buf
        self.np = buf.numpy()  # (a view of the pinned memory: numpy's min over ~1 K ints is a microsecond, torch's op is ~5)
        self.stream = stream  # the stream the storing kernel was launched on (None: the current one at wait time)
        self.what = what

    def query(self) -> bool:
        a = self.np
        return a[-1] >= 0 and a[0] >= 0 and int(a.min()) >= 0  # (two cache lines while the kernel is far from done)

    def synchronize(self, timeout_s: Optional[float] = None) -> None:
        query, nap0 = self.query, time.sleep
        # fast phase: exactly round 4's wait (query, yield) for the first few hundred polls -- the usual wait is tens to hundreds of
        # microseconds, up to a step's length when the host runs ahead of the GPU; no clock reads in here (an A/B on one box read
        # 0.744 against 0.738 ms per step with a perf_counter() per poll)
        for _ in range(400 if timeout_s is None else 1):
            if query():
                return
            nap0(0)
        t0 = time.perf_counter()
        limit = _WAIT_TIMEOUT_S if timeout_s is None else timeout_s
        next_check = t0
        while not query():
            now = time.perf_counter()
            if now >= next_check:
                next_check = now + 2e-3
                st = self.stream if self.stream is not None else torch.cuda.current_stream()
                try:
                    drained = st.query()  # raises on a device fault / an earlier HIP error on the stream
                except Exception as e:
                    raise RuntimeError(f"GPU error while waiting for {self.what}: {e}") from e
                if drained:
                    # everything queued has run: stores of a finished kernel are visible now or never
                    if query():
                        return
                    raise RuntimeError(f"the stream drained but {self.what} never arrived in pinned memory "
                                       f"(kernel not launched, faulted, or its stores were lost)")
                # a stream that is still BUSY is not an error: a long evaluation queued ahead, a shared GPU or a profiler serialising
                # kernels can legitimately put many seconds of work in front of the count kernel.  Warn once and keep waiting; the
                # bound (GS_WAIT_TIMEOUT_S, default 600 s; <= 0: none) is a backstop for a hung device whose stream query still answers
                if now - t0 > 30.0 and not _WAIT_WARNED[0]:
                    _WAIT_WARNED[0] = True
                    import warnings

                    warnings.warn(f"gscodec_studio_amd: waited {now - t0:.0f} s for {self.what}; the launch stream is still busy -- waiting on")
                if limit > 0 and now - t0 > limit:
                    raise RuntimeError(f"timed out after {limit:.1f} s (GS_WAIT_TIMEOUT_S) waiting for {self.what}")
            # yielding spin for 20 ms (a thread that napped comes back late: a 50 us time.sleep takes ~100 us on the test hosts, and
            # with naps from 1 ms on a 2-camera step read 2.63 ms instead of 1.37, tools/bench_multicam.py), naps after that: a wait
            # this long is not a step's own
            nap0(0 if now - t0 < 20e-3 else 200e-6)


def _wait_event(ev) -> None:
    """Wait for a CUDA event by POLLING it.  ``Event.synchronize()`` spins only briefly and then sleeps; when the GPU needs a
    few milliseconds to get there (49 M splats: 3 ms per forward) the wake-up came ~17 ms late on the bench host -- the
    forward ran at 42 FPS instead of 300.  A few milliseconds of host polling cost nothing here.  Past 0.25 s the wait is
    handed to the event's own ``synchronize`` (a real event sleeps and raises HIP errors; a ``_SentinelEvent`` naps, watches
    the stream for faults and gives up after ``GS_WAIT_TIMEOUT_S``): never an unbounded spin."""
    if isinstance(ev, _SentinelEvent):
        ev.synchronize()
        return
    deadline = time.perf_counter() + 0.25
    while not ev.query():
        if time.perf_counter() > deadline:  # something long is queued in front: stop burning the core
            ev.synchronize()
            return


class BlockSums:
    """One read-back in flight: ``wait()`` -> ``(n_isects, n_kept)``, then ``release()``; or ``abandon()``; or just drop the object.
    ``stored(n_sums, stream)``: the kernel queued on ``stream`` stores every block's (intersections, visible elements) pair STRAIGHT into
    ``buf``, pinned int32 [n_sums][2] (device-visible under HIP's unified addressing): no device-to-host copy command in the stream.
    ``copied(totals)``: a device int64 tensor (the two totals summed there, or ``cum[-1:]`` of the unsorted path) copied into a pinned
    buffer of its own behind an event; torch's allocator tracks that copy, so it needs no abandon care."""

    __slots__ = ("buf", "sentinel", "event", "totals", "settled")

    def __init__(self, buf: Tensor, sentinel: Optional[_SentinelEvent], event):
        self.buf, self.sentinel, self.event, self.totals, self.settled = buf, sentinel, event, None, False  # (settled: handed back or parked)

    @classmethod
    def stored(cls, n_sums: int, stream) -> "BlockSums":
        buf = _pinned_take(2 * n_sums)
        return cls(buf, _SentinelEvent(buf, stream=stream), None)

    @classmethod
    def copied(cls, totals: Tensor) -> "BlockSums":
        buf = torch.empty(totals.numel(), dtype=torch.int64, pin_memory=True)
        buf.copy_(totals, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(totals.device))
        return cls(buf, None, ev)

    def wait(self) -> Tuple[int, int]:
        """The one host sync of the pipeline (the reference's blocking ``.item()``, isect_tiles.cu:200); the totals are cached."""
        if self.totals is None:
            if self.sentinel is not None:
                self.sentinel.synchronize()
                self.totals = block_sum_totals(self.sentinel.np)
            else:
                _wait_event(self.event)
                self.totals = tuple((self.buf.tolist() + [0])[:2])  # ([n_isects] of the unsorted path: no kept count)
        return self.totals

    def abandon(self) -> None:
        """Hand a stored buffer back.  After ``wait()`` (``release``): to the free list.  WITHOUT one (the sparse exchange's overflow retry, an
        error between begin and finish): bounded watch for the kernel's stores first; a buffer they never reached (a failed launch in
        front) is parked.  Idempotent, and never raises: no error on its way up is replaced."""
        if self.settled or self.sentinel is None:
            return
        self.settled = True
        if self.totals is None:
            deadline = time.perf_counter() + _ABANDON_S
            while not self.sentinel.query():
                if time.perf_counter() > deadline:
                    _PARKED.append(self.buf)
                    return
                time.sleep(0)
        _PINNED_FREE.setdefault(self.buf.numel(), []).append(self.buf)

    release = abandon

    def __del__(self):  # dropped without release or abandon (an exception in between): same care for the buffer
        try:
            self.abandon()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass
