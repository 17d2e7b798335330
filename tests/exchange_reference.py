"""Plain numpy restatements of what csrc/exchange.hip computes for the two multi-GPU modes: the plan and the owner-side
gather-reduce of the camera-sharded sparse gradient reduction, and the row exchange of the gaussian-sharded mode.  No torch,
no GPU.  Every result is an integer or a float32 sum in a fixed order, so the kernels are compared with these bit for bit
(tests/test_gpu_exchange.py); tests/test_exchange_cpu.py and the gloo workers of tests/test_distributed_cpu.py pin them to
the torch formulations of distributed.py and to loops over single elements.

All ranks are played at once: functions take the inputs of every rank and return what every rank must end up with."""
from types import SimpleNamespace

import numpy as np

ROW = 16          # floats per splat row
ROW_DEPTH = 9     # the depth of a (camera, gaussian) pair
ROW_RADIUS = 10   # its radius, int32 bit pattern
ROW_DST = 12      # padding columns: on the wire they carry the destination row ...
ROW_AUX = 13      # ... and 0 (the header row of a chunk: -1 and count | overflow << 30)


# --------------------------------------------------------------------------- camera-sharded: sparse gradient reduction
def visibility(radii, n_pad):
    """uint8 [n_pad]: splat n is seen by some camera of radii [C, N]; zeros behind N."""
    radii = np.asarray(radii)
    C, N = radii.shape
    assert n_pad >= N
    vis = np.zeros(n_pad, dtype=np.uint8)
    vis[:N] = (radii > 0).any(0) if C else False
    return vis


def plan(masks, block):
    """The plan of the reduction from the masks of all ranks, uint8 [W, n_pad = W * block]; splat n belongs to owner
    n // block.  Returns
      rows [W, W]     rows[r][o] = splats of owner o that rank r sees
      urows [W]       splats of owner o that any rank sees
      counts          the native layout [W * W + W]: rows rank-major, then urows
      send_idx        per rank, its visible splats in ascending order
      union, uidx     the union mask and its splats in ascending order
      urank [n_pad]   position of n in uidx -- defined on union splats only (-1 elsewhere HERE; callers must not look)."""
    m = np.asarray(masks) != 0
    W, n_pad = m.shape
    assert block >= 1 and n_pad == W * block
    union = m.any(0)
    rows = m.reshape(W, W, block).sum(-1).astype(np.int32)
    urows = union.reshape(W, block).sum(-1).astype(np.int32)
    send_idx = [np.flatnonzero(m[r]).astype(np.int32) for r in range(W)]
    uidx = np.flatnonzero(union).astype(np.int32)
    urank = np.full(n_pad, -1, dtype=np.int32)
    urank[uidx] = np.arange(uidx.size, dtype=np.int32)
    return SimpleNamespace(world=W, block=block, n_pad=n_pad, union=union, rows=rows, urows=urows,
                           counts=np.concatenate([rows.reshape(-1), urows]).astype(np.int32), send_idx=send_idx, uidx=uidx,
                           urank=urank)


def owner_inputs(p, owner, rng, width, extra_dead=0):
    """What owner ``owner`` receives in phase 1 of the reduction under plan ``p``: every sender's rows [index | values] of the
    splats it sees in the owner's block (values drawn from ``rng``, standard normal), one chunk per sender in ascending
    sender order.  ``extra_dead`` rows with index -1 (and non-zero values) are appended to every non-empty chunk.
    Returns (wire [n_recv, 1 + width], chunk_starts [W + 1], uoff, uidx_mine)."""
    W, block = p.world, p.block
    chunks, starts = [], [0]
    for s in range(W):
        idx = p.send_idx[s]
        idx = idx[(idx >= owner * block) & (idx < (owner + 1) * block)]
        n = idx.size + (extra_dead if idx.size else 0)
        c = np.full((n, 1 + width), 7.5, dtype=np.float32)
        c[:, 0] = np.full(n, -1, dtype=np.int32).view(np.float32)
        c[:idx.size, 0] = idx.view(np.float32)
        c[:idx.size, 1:] = rng.standard_normal((idx.size, width)).astype(np.float32)
        chunks.append(c)
        starts.append(starts[-1] + n)
    wire = np.concatenate(chunks, 0)
    uoff = int(p.urows[:owner].sum())
    return wire, np.asarray(starts, dtype=np.int64), uoff, p.uidx[uoff:uoff + int(p.urows[owner])]


def reduce_rows(wire, chunk_starts, urank, uoff, uidx_mine, umax, scale):
    """The owner's accumulator [umax, 1 + width], float32.  Column 0 of row u: uidx_mine[u] (int32 bit pattern) for
    u < len(uidx_mine), -1 behind.  The other columns: +0.0f, plus -- walking the senders in ascending order -- the one row
    of that sender whose index column maps to u = urank[index] - uoff (at most one per sender: asserted), then times
    ``scale``; all in float32.  Rows with a negative index column are skipped."""
    wire = np.ascontiguousarray(wire, dtype=np.float32)
    D1 = wire.shape[1]
    acc = np.zeros((umax, D1), dtype=np.float32)
    col0 = np.full(umax, -1, dtype=np.int32)
    col0[:len(uidx_mine)] = uidx_mine
    W = len(chunk_starts) - 1
    for s in range(W):
        chunk = wire[int(chunk_starts[s]):int(chunk_starts[s + 1])]
        idx = chunk[:, 0].copy().view(np.int32)
        ok = idx >= 0
        u = urank[idx[ok]].astype(np.int64) - uoff
        assert u.size == np.unique(u).size and (u.size == 0 or (u.min() >= 0 and u.max() < umax))
        acc[u, 1:] = acc[u, 1:] + chunk[ok, 1:]
    acc[:, 1:] = acc[:, 1:] * np.float32(scale)
    acc[:, 0] = col0.view(np.float32)
    return acc


# --------------------------------------------------------------------------- gaussian-sharded: row exchange
def rows_exchange(radii_s, rows_s, C_local, N_world, cap_world):
    """Every rank s owns N_world[s] gaussians and has projected them onto ALL C_total = C_local * W cameras: radii_s[s]
    int32 [C_total, N_s], rows_s[s] float32 [C_total * N_s, 16] (None for an owner of nothing).  Destination d renders
    cameras [d * C_local, (d + 1) * C_local).  Wherever radii_s[s][c, n] > 0 and c // C_local == d, destination row
    (c % C_local) * N_total + N_off_s + n holds source row c * N_s + n, its padding columns 12 / 13 replaced by that
    destination row (int32 bit pattern) and 0.  Returns
      radii  [d] int32 [C_local, N_total]       0 where nothing arrives
      depths [d] float32 [C_local, N_total]     column 9 of the arrived row, 0 where nothing arrives
      rows   [d] float32 [C_local, N_total, 16] only defined where radii > 0 (zeros elsewhere HERE)
      counts [s][d]                             rows sender s has for destination d
      max_count [s], over [s]                   max over d of counts[s][d]; any(counts[s][d] > cap_world[s])
      overflow                                  any(over)"""
    W = len(N_world)
    N_total = int(sum(N_world))
    radii = [np.zeros((C_local, N_total), np.int32) for _ in range(W)]
    depths = [np.zeros((C_local, N_total), np.float32) for _ in range(W)]
    rows = [np.zeros((C_local, N_total, ROW), np.float32) for _ in range(W)]
    counts = np.zeros((W, W), dtype=np.int64)
    for s in range(W):
        N_s, N_off = int(N_world[s]), int(sum(N_world[:s]))
        if N_s == 0:
            continue
        r = np.asarray(radii_s[s]).reshape(C_local * W, N_s)
        src = np.asarray(rows_s[s], dtype=np.float32).reshape(C_local * W, N_s, ROW)
        for d in range(W):
            rd = r[d * C_local:(d + 1) * C_local]                    # [C_local, N_s]
            vis = rd > 0
            counts[s, d] = int(vis.sum())
            cl, n = np.nonzero(vis)
            got = src[d * C_local + cl, n].copy()
            dst = (cl * N_total + N_off + n).astype(np.int32)
            got[:, ROW_DST] = dst.view(np.float32)
            got[:, ROW_AUX] = 0.0
            rows[d][cl, N_off + n] = got
            radii[d][cl, N_off + n] = rd[cl, n]
            depths[d][cl, N_off + n] = got[:, ROW_DEPTH]
    max_count = counts.max(1)
    over = np.array([bool((counts[s] > int(cap_world[s])).any()) for s in range(W)])
    return SimpleNamespace(radii=radii, depths=depths, rows=rows, counts=counts, max_count=max_count, over=over,
                           overflow=bool(over.any()))


# --------------------------------------------------------------------------- the inputs of the GPU cases (seeded)
# (world, block) of the plan cases; N where the block follows from a splat count
PLAN_TILE = 2048
# tiles: 1, 1, 2, 2, 2, 65, 66, 259.  A tile adds up its predecessors with thread b % 256 taking tile b, so the LAST of 65 tiles
# (64 predecessors) still keeps the whole sum in the first wave's 64 lanes; the last of 66 is the first to need a lane of the
# second wave, and tiles behind the 257th make a thread add two.
PLAN_CASES = [(1, 1), (2, 1024), (2, 1025), (3, -(-2999 // 3)), (8, -(-2999 // 8)), (16, 8197), (16, 8401), (3, 176129)]


PLAN_VARIANTS = ("blind", "full")


def plan_masks(W, block, variant):
    """uint8 [W, W * block] at density 0.3 per rank with fixed features (each only where the size leaves room for it; what
    holds is asserted by ``check_plan_masks``): splat 0 seen by nobody; the union of one owner block empty (W >= 2); one
    2048-splat tile fully set, off splat 0 and off the empty block (the sizes of 65 and 259 tiles).  A rank that sees nothing
    cannot have a full tile, so there are two variants of every size:
      "blind"  the last rank sees nothing at all (W >= 2); for W >= 3 rank 0 sees only splats of its own block (the full
               tile lies in that block); the tile is full on every rank but the blind one;
      "full"   every rank sees something, and the tile is full on EVERY rank."""
    assert variant in PLAN_VARIANTS
    n_pad = W * block
    rng = np.random.default_rng(1000 * W + block + PLAN_VARIANTS.index(variant))
    m = (rng.random((W, n_pad)) < 0.3).astype(np.uint8)
    f = plan_features(W, block, variant)
    if f["full_tile"] is not None:
        t = f["full_tile"]
        m[:, t * PLAN_TILE:(t + 1) * PLAN_TILE] = 1
    if f["own_only"] is not None:
        r = f["own_only"]
        m[r, :r * block] = 0
        m[r, (r + 1) * block:] = 0
    if f["empty_block"] is not None:
        o = f["empty_block"]
        m[:, o * block:(o + 1) * block] = 0
    if f["blind_rank"] is not None:
        m[f["blind_rank"]] = 0
    m[:, 0] = 0
    return m


def plan_features(W, block, variant):
    """Which fixed features the masks of (W, block, variant) carry, and where."""
    f = {"full_tile": None, "own_only": None, "empty_block": None, "blind_rank": None}
    if W >= 2:
        f["empty_block"] = 1
        if variant == "blind":
            f["blind_rank"] = W - 1
    if W >= 3 and variant == "blind":
        f["own_only"] = 0
    # a whole tile inside owner block 0 that does not hold splat 0: the last one that ends inside the block
    t = block // PLAN_TILE - 1
    if t >= 1:
        f["full_tile"] = t
    return f


def check_plan_masks(m, W, block, variant):
    """The structure the plan cases rely on, asserted on the masks themselves."""
    f = plan_features(W, block, variant)
    assert m.shape == (W, W * block) and m.dtype == np.uint8
    assert not m[:, 0].any()
    if W >= 2:
        assert f["empty_block"] is not None and (variant != "blind" or f["blind_rank"] is not None)
    if W >= 3 and variant == "blind":
        assert f["own_only"] is not None
    if -(-W * block // PLAN_TILE) >= 65:
        assert f["full_tile"] is not None
    if f["blind_rank"] is not None:
        assert not m[f["blind_rank"]].any()
    if f["empty_block"] is not None:
        o = f["empty_block"]
        assert not m[:, o * block:(o + 1) * block].any()
    seeing = [r for r in range(W) if r != f["blind_rank"]]
    if W * block > 1:
        assert all(m[r].any() for r in seeing)
    if f["full_tile"] is not None:
        t = f["full_tile"]
        assert t >= 1 and (t + 1) * PLAN_TILE <= block
        assert all(m[r, t * PLAN_TILE:(t + 1) * PLAN_TILE].all() for r in seeing)
    if f["own_only"] is not None:
        r = f["own_only"]
        assert m[r].any() and not m[r, :r * block].any() and not m[r, (r + 1) * block:].any()
    if W * block >= 64:  # neither empty nor everything
        assert 0 < int(m.any(0).sum()) < W * block
    return f


# (W, width) of the reduce cases (59 = the degree-3 gradient row; 64 / 65 / 129: one, two and three column trips of a wave),
# crossed with the accumulator rows: one to five (partial groups of four rows), and 32768 + 5: the grid covers 32768 rows
# per trip, so the last takes a second one
REDUCE_CASES = [(1, 1), (1, 59), (2, 59), (3, 64), (3, 65), (8, 129), (16, 59)]
REDUCE_UMAX = [1, 3, 4, 5, 32768 + 5]


def reduce_owners(W):
    """The owners the reduce cases play: one with a non-zero map offset where the world has one; both kinds at W = 3."""
    return [0] if W == 1 else [0, 1] if W == 3 else [1]


def reduce_empty_senders(W, owner):
    """Senders that see nothing of the owner's block: one chunk in the middle and the one at the end are empty (W = 3 has
    room for one of the two: the middle one for owner 0, the last one for owner 1)."""
    return () if W < 3 else ((1,) if owner == 0 else (2,)) if W == 3 else (W // 2, W - 1)


def reduce_inputs(W, width, umax, owner):
    """Inputs of one gs_dp_reduce_rows case built from ``plan``: the owner block holds n_valid < umax union splats (umax - 2;
    1 at umax = 1); the chunks of ``reduce_empty_senders`` are empty; every non-empty chunk ends with a row of index -1;
    owner block 0 has a union splat, so an owner > 0 has a non-zero map offset.
    Returns (plan, wire, chunk_starts, uoff, uidx_mine)."""
    n_valid = max(umax - 2, 0) if umax > 1 else umax
    block = max(int(n_valid * 1.5) + 3, 4)
    rng = np.random.default_rng(77 * W + 13 * width + umax + 1000 * owner)
    dens = 0.2 if W > 3 and n_valid > 1000 else 0.5  # (the wide worlds' wire stays at some 10 MB)
    m = (rng.random((W, W * block)) < dens).astype(np.uint8)
    if owner > 0:
        m[0, 0] = 1
    for s in reduce_empty_senders(W, owner):
        m[s, owner * block:(owner + 1) * block] = 0
    # exactly n_valid union splats in the owner's block: clear the surplus, give the missing ones to sender 0
    seg = m[:, owner * block:(owner + 1) * block]
    u = np.flatnonzero(seg.any(0))
    if u.size > n_valid:
        seg[:, u[n_valid:]] = 0
    elif u.size < n_valid:
        free = np.flatnonzero(~seg.any(0))[:n_valid - u.size]
        seg[0, free] = 1
    p = plan(m, block)
    assert int(p.urows[owner]) == n_valid
    wire, starts, uoff, uidx_mine = owner_inputs(p, owner, rng, width, extra_dead=1)
    return p, wire, starts, uoff, uidx_mine


def check_reduce_inputs(W, owner, p, wire, starts, uoff, uidx_mine, umax):
    """The conditions the reduce cases state on their inputs."""
    n_valid = len(uidx_mine)
    assert n_valid <= umax and len(starts) == W + 1 and starts[-1] == wire.shape[0]
    sizes = np.diff(starts)
    assert all(sizes[s] == 0 for s in reduce_empty_senders(W, owner)) and sizes.sum() > 0
    if W >= 8 and n_valid >= 100:  # rows still arrive behind the empty chunk in the middle
        assert sizes[W // 2 + 1:].sum() > 0
    assert n_valid < umax or umax == 1
    assert (uoff > 0) == (owner > 0) and uoff == int(p.urows[:owner].sum())
    idx = wire[:, 0].copy().view(np.int32)
    assert (idx < 0).any()
    assert set(idx[idx >= 0].tolist()) == set(np.asarray(uidx_mine).tolist())
    if W >= 2 and n_valid >= 100:  # some splat really gets rows of more than one sender
        assert np.unique(idx[idx >= 0], return_counts=True)[1].max() >= 2


# the gaussian-sharded worlds: shard sizes per world size
EXCHANGE_WORLDS = {1: [700], 2: [1500, 0], 3: [1025, 3000, 1], 8: [300, 1, 0, 1024, 777, 1025, 64, 2049]}
EXCHANGE_CAPS = ("roomy", "exact", "short")


def exchange_inputs(W, C_local):
    """radii_s / rows_s of every rank: radii > 0 on 30 % of the (camera, gaussian) pairs (3), the others 0 or -1; the first
    camera of the last rank sees nothing (where there is more than one camera), and nobody sees a shard of one gaussian (a
    sender with nothing to send next to the owner of nothing); random rows with the radius bits in column 10 and a depth in
    column 9."""
    N_world = EXCHANGE_WORLDS[W]
    C_total = C_local * W
    rng = np.random.default_rng(31 * W + C_local)
    radii_s, rows_s = [], []
    for s, N in enumerate(N_world):
        r = np.where(rng.random((C_total, N)) < 0.3, 3, rng.integers(-1, 1, size=(C_total, N))).astype(np.int32)
        if C_total > 1:
            r[C_total - C_local] = np.minimum(r[C_total - C_local], 0)
        if N <= 1:  # (a sender with nothing to send: its chunks fit whatever the capacity)
            r = np.minimum(r, 0)
        radii_s.append(r)
        if N == 0:
            rows_s.append(None)
            continue
        rows = rng.standard_normal((C_total * N, ROW)).astype(np.float32)
        rows[:, ROW_RADIUS] = r.reshape(-1).view(np.float32)
        rows[:, ROW_DEPTH] = rng.uniform(0.5, 9.0, size=C_total * N).astype(np.float32)
        rows_s.append(rows)
    return N_world, radii_s, rows_s


def exchange_caps(counts, kind):
    """Chunk capacity of every sender: the largest count of its chunks + 10 ("roomy"), exactly that ("exact": no overflow),
    or one less ("short": overflows; a sender with nothing to send keeps capacity 0 and cannot overflow)."""
    mx = counts.max(1)
    if kind == "roomy":
        return [int(c) + 10 for c in mx]
    if kind == "exact":
        return [int(c) for c in mx]
    assert kind == "short"
    return [max(int(c) - 1, 0) for c in mx]


def check_exchange_inputs(W, C_local, N_world, radii_s):
    C_total = C_local * W
    vis = sum(int((r > 0).sum()) for r in radii_s)
    pairs = (C_total - (1 if C_total > 1 else 0)) * sum(n for n in N_world if n > 1)  # (the blind camera and the unseen shards aside)
    assert 0.25 < vis / pairs < 0.35
    assert C_total == 1 or all(not (r[C_total - C_local] > 0).any() for r in radii_s)
    assert any((r < 0).any() for r in radii_s) and any((r == 0).any() for r in radii_s)
    counts = np.array([[int((radii_s[s][d * C_local:(d + 1) * C_local] > 0).sum()) for d in range(W)] for s in range(W)])
    assert counts.max() >= 2  # "short" really overflows somewhere
    if W > 1:
        assert (counts.max(1) == 0).any()  # a sender whose chunks always fit
    return counts
