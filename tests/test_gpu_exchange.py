"""GPU: the multi-GPU kernels of csrc/exchange.hip at operator level, every rank played in ONE process on one GPU.

None of these kernels communicates: gs_dp_plan takes the masks of all ranks as an input, a chunk is a slice of a buffer, and
the all-to-all / all-gather between the calls is slicing and torch.cat here.  Every result is an integer or a float32 sum in a
fixed order, so every comparison with the numpy restatements of tests/exchange_reference.py is BIT FOR BIT (their agreement
with the torch formulations of distributed.py, and the conditions on the inputs used here, are pinned on the CPU by
tests/test_exchange_cpu.py).  Every buffer a kernel writes sits between guard bands; entries the contract leaves undefined
(send_idx behind its count, uidx behind the union's size, urank off the union, rows where radii = 0) are not looked at.

  gs_dp_visibility                     against visibility()
  gs_dp_plan                           against plan(): 1, 2, 65, 66 and 259 tiles (a plan tile is 2048 splats), for every rank
  gs_dp_reduce_rows                    against reduce_rows(): widths on both sides of 64, one to 32768 + 5 accumulator rows
  the sparse reduction composed        gs_dp_plan + the library's _pack_rows / _reduce_received_rows / _unpack_rows, W ranks
  gs_exchange_rows_send / _recv /      against rows_exchange(): capacities above, at and below the largest count
  gs_exchange_flags

Measured on an MI355X: profiles/exchange_operator_tests.txt."""
import ctypes

import numpy as np
import pytest
import torch

import exchange_reference as XR
from gscodec_studio_amd import _backend as B

pytestmark = pytest.mark.gpu

GUARD = 4096            # elements on each side of a buffer the kernels write
SENTINEL = 0x7FC0BEEF   # int32 / float32 buffers: a NaN bit pattern no kernel produces, and no valid index or count
SENTINEL8 = 0xA5        # uint8 buffers
DTYPES = {torch.int32: SENTINEL, torch.float32: SENTINEL, torch.uint8: SENTINEL8}


def guarded(numel, dtype=torch.int32, fill=None):
    """(whole, inner): ``inner`` [numel] lies between two guard bands; everything holds the sentinel unless ``fill`` is given."""
    whole = torch.empty(numel + 2 * GUARD, dtype=dtype, device="cuda")
    bits(whole).fill_(DTYPES[dtype])
    inner = whole[GUARD:GUARD + numel]
    if fill is not None:
        inner.fill_(fill)
    return whole, inner


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def guards_intact(whole, numel):
    torch.cuda.synchronize()
    w, s = bits(whole), DTYPES[whole.dtype]
    return bool((w[:GUARD] == s).all()) and bool((w[GUARD + numel:] == s).all())


def untouched(*wholes):
    torch.cuda.synchronize()
    return all(bool((bits(w) == DTYPES[w.dtype]).all()) for w in wholes)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_bits(t):
    """A device tensor as int32 bit patterns on the host."""
    return bits(t.contiguous()).cpu().numpy()


def rejected(name, *args):
    with pytest.raises(RuntimeError, match=r"status 1"):
        B.call(name, *args)


# --------------------------------------------------------------------------- gs_dp_visibility
@pytest.mark.parametrize("C, N, n_pad", [(1, 1, 1), (3, 255, 256), (3, 257, 264), (2, 5000, 5008)])
def test_visibility(C, N, n_pad):
    rng = np.random.default_rng(C * 100000 + N)
    radii = rng.choice(np.array([-1, 0, 3], dtype=np.int32), size=(C, N))
    if N == 1:
        radii[:] = 3
    want = XR.visibility(radii, n_pad)
    assert want[:N].any() and (N < 64 or not want[:N].all()) and (radii < 0).any() == (N > 1)
    whole, vis = guarded(n_pad, torch.uint8)
    B.call("gs_dp_visibility", C, N, n_pad, B.ptr(dev(radii)), B.ptr(vis), stream())
    got = vis.cpu().numpy()
    assert np.array_equal(got, want)
    assert not got[N:].any()
    assert guards_intact(whole, n_pad)


def test_visibility_rejections():
    whole, vis = guarded(8, torch.uint8)
    radii = torch.full((2, 8), 3, dtype=torch.int32, device="cuda")
    rejected("gs_dp_visibility", 2, 8, 4, B.ptr(radii), B.ptr(vis), stream())      # n_pad < N
    rejected("gs_dp_visibility", 2, 8, 8, B.ptr(radii), None, stream())
    rejected("gs_dp_visibility", 2, 8, 8, None, B.ptr(vis), stream())
    B.call("gs_dp_visibility", 2, 8, 0, B.ptr(radii), B.ptr(vis), stream())       # nothing to do
    assert untouched(whole)
    B.call("gs_dp_visibility", 0, 8, 8, None, B.ptr(vis), stream())               # no camera: nobody sees anything
    assert not vis.cpu().numpy().any() and guards_intact(whole, 8)


# --------------------------------------------------------------------------- gs_dp_plan
class PlanBuffers:
    def __init__(self, W, n_pad):
        self.W, self.n_pad = W, n_pad
        self.tiles = int(B.query("gs_dp_plan_tiles", max(n_pad, 1)))
        self.sizes = {"tile_counts": 2 * self.tiles, "counts": W * W + W, "send_idx": max(n_pad, 1), "urank": max(n_pad, 1),
                      "uidx": max(n_pad, 1)}
        self.whole, self.inner = {}, {}
        for k, n in self.sizes.items():
            self.whole[k], self.inner[k] = guarded(n)

    def args(self, **null):
        return [None if k in null else B.ptr(self.inner[k]) for k in ("tile_counts", "counts", "send_idx", "urank", "uidx")]

    def intact(self):
        return all(guards_intact(self.whole[k], n) for k, n in self.sizes.items())

    def untouched(self):
        return untouched(*self.whole.values())


def run_plan(W, rank, block, masks_d):
    buf = PlanBuffers(W, W * block)
    buf.inner["counts"].zero_()  # (the contract: zero-filled by the caller)
    B.call("gs_dp_plan", W, rank, W * block, block, B.ptr(masks_d), *buf.args(), stream())
    assert buf.intact()
    return buf


@pytest.mark.parametrize("variant", XR.PLAN_VARIANTS)
@pytest.mark.parametrize("W, block", XR.PLAN_CASES)
def test_plan(W, block, variant):
    """counts whole, send_idx[:mine], uidx[:U] and urank on the union, from every rank of the world.  dp_plan_fill_kernel adds
    up a tile's predecessors with thread b % 256 taking tile b, reduces over 64 lanes and sums four wave partials: the last of
    65 tiles (W = 16, block 8197) fills the first wave's lanes, the last of 66 (block 8401) is the first to need the second
    wave's partial, and behind 257 tiles (W = 3, block 176129) a thread adds two."""
    m = XR.plan_masks(W, block, variant)
    XR.check_plan_masks(m, W, block, variant)
    ref = XR.plan(m, block)
    U = int(ref.uidx.size)
    masks_d = dev(m)
    first = None
    for rank in range(W):
        buf = run_plan(W, rank, block, masks_d)
        counts = buf.inner["counts"].cpu().numpy()
        assert np.array_equal(counts, ref.counts), (rank, counts, ref.counts)
        mine = int(ref.rows[rank].sum())
        assert np.array_equal(buf.inner["send_idx"][:mine].cpu().numpy(), ref.send_idx[rank]), rank
        uidx = buf.inner["uidx"][:U].cpu().numpy()
        urank = buf.inner["urank"].cpu().numpy()[ref.union]
        assert np.array_equal(uidx, ref.uidx), rank
        assert np.array_equal(urank, ref.urank[ref.union]), rank
        if first is None:
            first = (uidx, urank)
        assert np.array_equal(first[0], uidx) and np.array_equal(first[1], urank)  # every rank holds the same union lists


def test_plan_rejections():
    W, block = 2, 8
    n_pad = W * block
    masks_d = dev(XR.plan_masks(W, block, "full"))
    big = dev(np.ones((17, 17 * block), dtype=np.uint8))
    buf = PlanBuffers(17, 17 * block)
    rejected("gs_dp_plan", 0, 0, n_pad, block, B.ptr(masks_d), *buf.args(), stream())                 # world 0
    rejected("gs_dp_plan", 17, 0, 17 * block, block, B.ptr(big), *buf.args(), stream())               # world 17
    rejected("gs_dp_plan", W, W, n_pad, block, B.ptr(masks_d), *buf.args(), stream())                 # rank == world
    rejected("gs_dp_plan", W, 0, n_pad + 1, block, B.ptr(masks_d), *buf.args(), stream())             # block * world != n_pad
    rejected("gs_dp_plan", W, 0, n_pad, block + 1, B.ptr(masks_d), *buf.args(), stream())
    rejected("gs_dp_plan", W, 0, n_pad, block, None, *buf.args(), stream())                           # each null pointer
    for k in ("tile_counts", "counts", "send_idx", "urank", "uidx"):
        rejected("gs_dp_plan", W, 0, n_pad, block, B.ptr(masks_d), *buf.args(**{k: True}), stream())
    assert buf.untouched()
    B.call("gs_dp_plan", W, 0, 0, 0, B.ptr(masks_d), *buf.args(), stream())                           # n_pad = 0: nothing to do
    B.call("gs_dp_plan", W, 0, 0, 0, None, None, None, None, None, None, stream())
    assert buf.untouched()


# --------------------------------------------------------------------------- gs_dp_reduce_rows
def run_reduce(W, width, wire_d, starts, urank_d, uoff, uidx_d, n_valid, umax, scale, n_recv=None):
    """One call on guarded acc / inv; returns acc as int32 bit patterns [umax, 1 + width] on the host."""
    acc_w, acc = guarded(umax * (1 + width), torch.float32)
    inv_w, inv = guarded(W * umax)
    cs = (ctypes.c_int64 * (W + 1))(*[int(v) for v in starts])
    n_recv = int(starts[-1]) if n_recv is None else n_recv
    B.call("gs_dp_reduce_rows", n_recv, width, W, B.ptr(wire_d) if n_recv else None, ctypes.addressof(cs),
           B.ptr(urank_d) if n_recv else None, int(uoff), umax, n_valid, B.ptr(uidx_d) if n_valid else None, float(scale), B.ptr(inv),
           B.ptr(acc), stream())
    assert guards_intact(acc_w, umax * (1 + width)) and guards_intact(inv_w, W * umax)
    return host_bits(acc).reshape(umax, 1 + width)


@pytest.mark.parametrize("umax", XR.REDUCE_UMAX)
@pytest.mark.parametrize("W, width", XR.REDUCE_CASES)
def test_reduce_rows(W, width, umax):
    for owner in XR.reduce_owners(W):
        p, wire, starts, uoff, uidx_mine = XR.reduce_inputs(W, width, umax, owner)
        XR.check_reduce_inputs(W, owner, p, wire, starts, uoff, uidx_mine, umax)
        n_valid = len(uidx_mine)
        wire_d, urank_d, uidx_d = dev(wire), dev(p.urank), dev(uidx_mine)
        for scale in (1.0, 1.0 / W):
            want = XR.reduce_rows(wire, starts, p.urank, uoff, uidx_mine, umax, scale).view(np.int32)
            got = run_reduce(W, width, wire_d, starts, urank_d, uoff, uidx_d, n_valid, umax, scale)
            assert np.array_equal(got[:, 0], want[:, 0]), (owner, scale)
            assert (got[n_valid:, 0] == -1).all() and (got[n_valid:, 1:] == 0).all()   # the padding rows: index -1 and +0.0f
            bad = np.argwhere(got != want)
            assert bad.size == 0, (owner, scale, bad[:8].tolist())
            again = run_reduce(W, width, wire_d, starts, urank_d, uoff, uidx_d, n_valid, umax, scale)
            assert np.array_equal(got, again)                                          # no atomics on this path


@pytest.mark.parametrize("W, width, umax", [(1, 1, 1), (3, 59, 5), (16, 65, 70)])
def test_reduce_rows_nothing_received(W, width, umax):
    """n_recv = 0 with umax > 0: every row is (index or -1 | zeros); with n_valid = 0 the uidx pointer may be NULL."""
    uidx = np.arange(100, 100 + umax - 1, dtype=np.int32)
    for n_valid in sorted({0, umax - 1}):
        got = run_reduce(W, width, None, [0] * (W + 1), None, 3, dev(uidx) if n_valid else None, n_valid, umax, 0.5, n_recv=0)
        assert got[:n_valid, 0].tolist() == uidx[:n_valid].tolist() and (got[n_valid:, 0] == -1).all()
        assert (got[:, 1:] == 0).all()


def test_reduce_rows_rejections():
    W, width, umax = 2, 3, 4
    p, wire, starts, uoff, uidx_mine = XR.reduce_inputs(W, width, umax, 1)
    wire_d, urank_d, uidx_d = dev(wire), dev(p.urank), dev(uidx_mine)
    acc_w, acc = guarded(umax * (1 + width), torch.float32)
    inv_w, inv = guarded(17 * umax)
    cs = (ctypes.c_int64 * 18)(*([int(v) for v in starts] + [int(starts[-1])] * (18 - len(starts))))

    def call(world, w, acc_p, inv_p=B.ptr(inv), cs_p=ctypes.addressof(cs)):
        return ("gs_dp_reduce_rows", int(starts[-1]), w, world, B.ptr(wire_d), cs_p, B.ptr(urank_d), int(uoff), umax, len(uidx_mine),
                B.ptr(uidx_d), 1.0, inv_p, acc_p, stream())

    rejected(*call(0, width, B.ptr(acc)))        # world 0
    rejected(*call(17, width, B.ptr(acc)))       # world 17
    rejected(*call(W, 0, B.ptr(acc)))            # width 0
    rejected(*call(W, width, None))              # null acc
    rejected(*call(W, width, B.ptr(acc), inv_p=None))
    rejected(*call(W, width, B.ptr(acc), cs_p=None))
    assert untouched(acc_w, inv_w)
    B.call("gs_dp_reduce_rows", 0, width, W, None, ctypes.addressof(cs), None, 0, 0, 0, None, 1.0, None, None, stream())  # umax = 0
    assert untouched(acc_w, inv_w)


# --------------------------------------------------------------------------- the sparse reduction composed
@pytest.mark.parametrize("average", [False, True])
@pytest.mark.parametrize("W", [2, 3, 8])
def test_sparse_reduction_composed(W, average):
    """`distributed._sparse_all_reduce` step by step for all W ranks in one process, with the library's own helpers; the plans
    come from gs_dp_plan per rank, the all-to-all and the all-gather are slicing and torch.cat.  N = 6151: three full plan
    tiles and a short fourth, N % W != 0.  On every simulated rank and for every parameter: union rows = the float32 sum over ranks in ascending
    rank order (of the ranks that saw the splat) times scale, bit for bit; rows outside the union keep their sentinel."""
    from gscodec_studio_amd import distributed as D

    N, widths, OUTSIDE = 6151, [3, 4, 1, 48], 123.25
    assert N % W != 0
    block = -(-N // W)
    n_pad = W * block
    assert -(-n_pad // XR.PLAN_TILE) >= 3
    m = XR.plan_masks(W, block, "blind")
    m[:, N:] = 0
    XR.check_plan_masks(m, W, block, "blind")
    ref = XR.plan(m, block)
    union = ref.union[:N]
    assert 0 < union.sum() < N
    rng = np.random.default_rng(W)
    # gradients: random where the rank's mask is set, zero on the rest of the union, a sentinel outside the union
    grads = []
    for r in range(W):
        per = []
        for w in widths:
            g = rng.standard_normal((N, w)).astype(np.float32) * (m[r, :N, None] != 0)
            g[~union] = OUTSIDE
            per.append(g)
        grads.append(per)
    scale = np.float32(1.0 / W) if average else np.float32(1.0)
    want = []
    for k, w in enumerate(widths):
        acc = np.zeros((N, w), dtype=np.float32)
        for r in range(W):
            seen = m[r, :N] != 0
            acc[seen] = acc[seen] + grads[r][k][seen]
        acc = acc * scale
        acc[~union] = OUTSIDE
        want.append(acc)
    # ---- every rank's plan from the kernel
    masks_d = dev(m)
    plans = [run_plan(W, r, block, masks_d) for r in range(W)]
    counts = plans[0].inner["counts"].cpu().numpy()
    assert all(np.array_equal(p.inner["counts"].cpu().numpy(), counts) for p in plans) and np.array_equal(counts, ref.counts)
    rows, urows = counts[:W * W].reshape(W, W).tolist(), counts[W * W:].tolist()
    G = [[dev(g) for g in per] for per in grads]
    # ---- phase 1: pack, "all-to-all", gather-reduce on every owner
    send = []
    for r in range(W):
        n_mine = sum(rows[r])
        idx = plans[r].inner["send_idx"][:n_mine]
        parts = [(idx, 1, False)] + [(g, w, True) for g, w in zip(G[r], widths)]
        send.append(D._pack_rows(parts, n_mine, G[r][0], idx) if n_mine else torch.empty((0, sum(widths) + 1), device="cuda"))
    umax = max(urows)
    accs = []
    for o in range(W):
        out_splits = [rows[r][o] for r in range(W)]
        recv = torch.cat([send[r][sum(rows[r][:o]):sum(rows[r][:o + 1])] for r in range(W)], 0).contiguous()
        uoff, n_u = sum(urows[:o]), urows[o]
        accs.append(D._reduce_received_rows(recv, out_splits, plans[o].inner["urank"], uoff, plans[o].inner["uidx"][uoff:uoff + n_u], umax,
                                            float(scale)))
    # ---- phase 2: "all-gather", unpack on every rank
    allrows = torch.cat(accs, 0).contiguous()
    assert allrows.shape == (W * umax, sum(widths) + 1)
    for r in range(W):
        D._unpack_rows(allrows, [(None, 1, False)] + [(g, w, True) for g, w in zip(G[r], widths)], allrows.view(torch.int32)[:, 0])
    torch.cuda.synchronize()
    for r in range(W):
        for k, w in enumerate(widths):
            got = host_bits(G[r][k])
            bad = np.argwhere(got != want[k].view(np.int32))
            assert bad.size == 0, (r, w, bad[:8].tolist())


# --------------------------------------------------------------------------- gs_exchange_rows_send / _recv / gs_exchange_flags
OVER_BIT = 1 << 30


def exchange_send(W, C_local, N_world, radii_s, rows_s, caps, zero_radii):
    """gs_exchange_rows_send on every rank; zero_radii[s] (or None) is rank s's own receiver-side radii buffer."""
    C_total, N_total = C_local * W, sum(N_world)
    out = []
    for s in range(W):
        N, cap = N_world[s], caps[s]
        n_send = W * (cap + 1)
        src_w, src_index = guarded(n_send)
        hdr_w, hdr = guarded(2 * n_send)
        aux_w, aux = guarded(W + 2)              # counters [W] | stats [2]
        send_w, send = guarded(n_send * XR.ROW, torch.float32)
        radii_d = dev(radii_s[s]) if N else None
        rows_d = dev(rows_s[s]) if N else None   # (an owner of nothing passes NULL, as distributed.py does)
        z = zero_radii[s] if zero_radii is not None else None
        B.call("gs_exchange_rows_send", C_total, N, C_local, W, cap, N_total, sum(N_world[:s]), B.ptr(radii_d), B.ptr(rows_d),
               B.ptr(src_index), B.ptr(hdr), B.ptr(aux[:W]), B.ptr(aux[W:]), B.ptr(send), B.ptr(z), z.numel() if z is not None else 0,
               stream())
        assert guards_intact(src_w, n_send) and guards_intact(hdr_w, 2 * n_send) and guards_intact(aux_w, W + 2)
        assert guards_intact(send_w, n_send * XR.ROW)
        out.append(dict(send=send.view(n_send, XR.ROW), stats=aux[W:], counters=aux[:W], src_index=src_index, keep=(send_w, src_w, hdr_w, aux_w)))
    return out


def exchange_recv(W, C_local, N_world, caps, sent, d, radii_l, radii_zeroed):
    """gs_exchange_rows_recv on destination d: its chunk of every sender in ascending sender order."""
    n_dst = C_local * sum(N_world)
    recv = torch.cat([sent[s]["send"][d * (caps[s] + 1):(d + 1) * (caps[s] + 1)] for s in range(W)], 0).contiguous()
    hdr_rows = dev(np.cumsum([c + 1 for c in caps]).astype(np.int64) - 1)
    rows_w, rows_l = guarded(n_dst * XR.ROW, torch.float32)
    depths_w, depths_l = guarded(n_dst, torch.float32)
    out_w, out3 = guarded(3)
    radii_w, radii_i = radii_l
    B.call("gs_exchange_rows_recv", recv.shape[0], B.ptr(recv), n_dst, B.ptr(rows_l), B.ptr(radii_i), B.ptr(depths_l), W, B.ptr(hdr_rows),
           B.ptr(sent[d]["stats"]), B.ptr(out3), radii_zeroed, stream())
    assert guards_intact(rows_w, n_dst * XR.ROW) and guards_intact(depths_w, n_dst) and guards_intact(radii_w, n_dst)
    assert guards_intact(out_w, 3)
    return (radii_i.cpu().numpy(), host_bits(depths_l), host_bits(rows_l).reshape(n_dst, XR.ROW), out3.cpu().numpy().tolist(),
            host_bits(recv))


@pytest.mark.parametrize("kind", XR.EXCHANGE_CAPS)
@pytest.mark.parametrize("C_local", [1, 2])
@pytest.mark.parametrize("W", sorted(XR.EXCHANGE_WORLDS))
def test_exchange_rows(W, C_local, kind):
    N_world, radii_s, rows_s = XR.exchange_inputs(W, C_local)
    counts = XR.check_exchange_inputs(W, C_local, N_world, radii_s)
    caps = XR.exchange_caps(counts, kind)
    ex = XR.rows_exchange(radii_s, rows_s, C_local, N_world, caps)
    assert ex.overflow == (kind == "short") and np.array_equal(ex.counts, counts)
    n_dst = C_local * sum(N_world)
    # radii_zeroed = 1: the send call of rank d zero-fills d's receiver-side radii (as _ExchangeRows.forward does);
    # radii_zeroed = 0: the recv call does
    zeroed = [guarded(n_dst) for _ in range(W)]
    sent = exchange_send(W, C_local, N_world, radii_s, rows_s, caps, [z[1] for z in zeroed])
    for s in range(W):
        assert guards_intact(zeroed[s][0], n_dst)
        # every chunk header carries its count (capped) and the sender's overflow flag; stats = (largest count, overflowed)
        wire = host_bits(sent[s]["send"])
        for d in range(W):
            h = wire[d * (caps[s] + 1) + caps[s]]
            assert h[XR.ROW_DST] == -1 and h[XR.ROW_AUX] == (min(int(counts[s, d]), caps[s]) | (OVER_BIT if ex.over[s] else 0)), (s, d)
        assert sent[s]["counters"].cpu().numpy().tolist() == counts[s].tolist()
        assert sent[s]["stats"].cpu().numpy().tolist() == [int(ex.max_count[s]), int(ex.over[s])]
    for d in range(W):
        want_radii, want_depths = ex.radii[d].reshape(-1), ex.depths[d].reshape(-1).view(np.int32)
        want_rows = ex.rows[d].reshape(-1, XR.ROW).view(np.int32)
        results = [exchange_recv(W, C_local, N_world, caps, sent, d, zeroed[d], 1),
                   exchange_recv(W, C_local, N_world, caps, sent, d, guarded(n_dst), 0)]
        assert np.array_equal(results[0][0], results[1][0])        # both ways of zero-filling give the same radii
        for radii, depths, rows, out3, recv in results:
            assert out3 == [int(ex.overflow), int(ex.max_count[d]), int(ex.over[d])], (d, out3)
            arrived = radii > 0
            assert (radii[~arrived] == 0).all()
            # what arrived is right; nothing else was written (depths and rows keep their sentinel where nothing arrived)
            assert not (arrived & ~(want_radii > 0)).any()
            assert np.array_equal(radii[arrived], want_radii[arrived])
            assert np.array_equal(depths[arrived], want_depths[arrived]) and (depths[~arrived] == SENTINEL).all()
            assert np.array_equal(rows[arrived], want_rows[arrived]) and (rows[~arrived] == SENTINEL).all()
            # the chunks: min(count, cap) distinct valid rows in front, -1 behind them
            off = 0
            for s in range(W):
                k = min(int(counts[s, d]), caps[s])
                dst = recv[off:off + caps[s], XR.ROW_DST]
                lo = sum(N_world[:s])
                assert (dst[k:] == -1).all() and (dst[:k] >= 0).all() and np.unique(dst[:k]).size == k, (s, d)
                col = dst[:k] % sum(N_world)
                assert ((col >= lo) & (col < lo + N_world[s])).all() and (want_radii[dst[:k]] > 0).all(), (s, d)
                off += caps[s] + 1
            assert int(arrived.sum()) == sum(min(int(counts[s, d]), caps[s]) for s in range(W))
            if not ex.overflow:  # everything arrived: radii and depths equal the restatement everywhere
                assert np.array_equal(radii, want_radii)
                assert np.array_equal(np.where(arrived, depths, 0), want_depths)


def test_exchange_flags():
    """gs_exchange_flags alone: the overflow bit of ANY received chunk header sets out3[0]; out3[1:] are this rank's stats."""
    W, width = 8, 16
    caps = [3, 0, 5, 1, 0, 2, 7, 4]
    hdr_rows = np.cumsum([c + 1 for c in caps]).astype(np.int64) - 1
    stats = dev(np.array([41, 1], dtype=np.uint32).view(np.int32))
    for flagged in (None, 0, 4, 7):
        recv = np.full((int(hdr_rows[-1]) + 1, width), OVER_BIT | 5, dtype=np.int32)  # (the bit in rows that are no header: ignored)
        recv[hdr_rows, 1] = [c for c in caps]
        if flagged is not None:
            recv[hdr_rows[flagged], 1] |= OVER_BIT
        out_w, out3 = guarded(3)
        B.call("gs_exchange_flags", W, B.ptr(dev(recv)), width, B.ptr(dev(hdr_rows)), B.ptr(stats), B.ptr(out3), stream())
        assert guards_intact(out_w, 3)
        assert out3.cpu().numpy().tolist() == [int(flagged is not None), 41, 1]
    out_w, out3 = guarded(3)
    r, h = dev(recv), dev(hdr_rows)
    rejected("gs_exchange_flags", 0, B.ptr(r), width, B.ptr(h), B.ptr(stats), B.ptr(out3), stream())
    rejected("gs_exchange_flags", W, B.ptr(r), 1, B.ptr(h), B.ptr(stats), B.ptr(out3), stream())
    rejected("gs_exchange_flags", W, None, width, B.ptr(h), B.ptr(stats), B.ptr(out3), stream())
    rejected("gs_exchange_flags", W, B.ptr(r), width, B.ptr(h), B.ptr(stats), None, stream())
    assert untouched(out_w)
