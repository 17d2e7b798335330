"""Multi-GPU layer: one process per GPU, ``torch.distributed`` over RCCL (backend "nccl" on
ROCm) across the xGMI mesh of one MI355X node.

Two things live here:

1. The collectives API of the reference (``gsplat/distributed.py:10-257``:
   ``all_gather_int32``, ``all_to_all_int32``, ``all_gather_tensor_list``,
   ``all_to_all_tensor_list``) and the launcher ``cli`` (272-360), plus
   ``exchange_projected`` -- the gaussian-sharded exchange that the reference inlines in
   ``rendering.py:397-478`` -- so ``rasterization(distributed=True)`` is supported.
   Implementation differs: every exchange is ONE flat ``all_to_all_single`` on a fused
   [rows, features] buffer with an explicit autograd Function (the dual all-to-all in
   backward), rather than lists of per-rank tensors through ``torch.distributed.nn``.

2. The camera-sharded data-parallel path asked for by the north star: splats are
   replicated, the camera batch is sharded (rank r renders cameras r::world), forward
   needs no communication, and the only exchange is the sum of splat gradients
   (``all_reduce_splat_grads``).  Default on RCCL: every gradient tensor is reduced where it
   lies -- reduce_scatter_tensor + all_gather_into_tensor for the large ones (each of the 7
   xGMI peers carries 1/8 concurrently, no packing copies), an in-place all_reduce for the
   small ones.  With a ``SparseGradPlan`` (built in the forward from the visibility masks)
   only the rows of splats that SOME camera saw travel: ~30 % of the 236 B/splat at the bench
   workload (``plan_sparse_grad_exchange`` / ``all_reduce_splat_grads(..., plan=...)``).

On CPU (gloo; used by the world_size-2 tests) the same code paths run with point-to-point
fallbacks for the collectives gloo lacks.
"""
from __future__ import annotations

import os
import socket
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch
import torch.distributed as dist
from torch import Tensor


# ---------------------------------------------------------------------------
# low-level helpers
# ---------------------------------------------------------------------------
_BACKEND: dict = {"pg": None, "name": ""}


def _backend_name() -> str:
    # (cached per default process group -- the object itself is held, so a re-created group can never alias it: three
    # look-ups per step at ~3 us each on a path that is bound by host work)
    pg = dist.group.WORLD
    if _BACKEND["pg"] is not pg:
        _BACKEND["pg"], _BACKEND["name"] = pg, str(dist.get_backend()).lower()
    return _BACKEND["name"]


# bytes this rank puts on the wire (payload leaving the GPU, computed from the collective's shape: all-to-all = everything
# but the self chunk; all-gather = (world - 1) x input; reduce-scatter = (world - 1) / world x input; all-reduce counted as
# reduce-scatter + all-gather).  bench.py reads and resets it to report bytes per rank and step next to the xGMI floor.
WIRE = {"bytes": 0}


def _wire(nbytes: float) -> None:
    WIRE["bytes"] += int(nbytes)


def _single(world_size: int) -> bool:
    """World-1 short cut of every collective; GS_DIST_FORCE_COLLECTIVES=1 disables it so that a one-rank run
    still drives RCCL (used by the tests on single-GPU boxes)."""
    return world_size == 1 and os.environ.get("GS_DIST_FORCE_COLLECTIVES", "0") != "1"


def _staged(t: Tensor) -> bool:
    """Device tensors under a host-only backend (gloo) are exchanged through host memory.  This is what lets the
    world_size-2 tests run both ranks on the single GPU of a test box; RCCL never takes this route."""
    return t.is_cuda and "nccl" not in _backend_name()


def _all_gather_into(out: Tensor, inp: Tensor) -> None:
    _wire(inp.numel() * inp.element_size() * (dist.get_world_size() - 1))
    if _staged(inp):
        o = torch.empty(out.shape, dtype=out.dtype)
        dist.all_gather_into_tensor(o, inp.cpu())
        out.copy_(o)
    else:
        dist.all_gather_into_tensor(out, inp)


def _all_reduce_sum(t: Tensor) -> None:
    w = dist.get_world_size()
    _wire(2.0 * t.numel() * t.element_size() * (w - 1) / w)
    if _staged(t):
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)


def _all_to_all_single(out: Tensor, inp: Tensor, out_splits: List[int], in_splits: List[int]) -> None:
    """all_to_all_single with a P2P fallback for backends without it (gloo)."""
    if not _staged(inp):
        row = inp.element_size() * (inp.numel() // max(inp.shape[0], 1))
        _wire(row * (sum(in_splits) - in_splits[dist.get_rank()]))
    if "nccl" in _backend_name():
        dist.all_to_all_single(out, inp, out_splits, in_splits)
        return
    if _staged(inp):
        o = torch.empty(out.shape, dtype=out.dtype)
        _all_to_all_single(o, inp.cpu(), out_splits, in_splits)
        out.copy_(o)
        return
    rank, world = dist.get_rank(), dist.get_world_size()
    in_chunks = list(inp.split(in_splits, dim=0))
    out_chunks = list(out.split(out_splits, dim=0))
    out_chunks[rank].copy_(in_chunks[rank])
    ops = []
    for peer in range(world):
        if peer == rank:
            continue
        if in_splits[peer] > 0:
            ops.append(dist.P2POp(dist.isend, in_chunks[peer].contiguous(), peer))
        if out_splits[peer] > 0:
            ops.append(dist.P2POp(dist.irecv, out_chunks[peer], peer))
    if ops:
        for w in dist.batch_isend_irecv(ops):
            w.wait()


class _AllToAllRows(torch.autograd.Function):
    """Differentiable variable-split all-to-all over dim 0; backward is the dual exchange."""

    @staticmethod
    def forward(ctx, data: Tensor, in_splits: List[int], out_splits: List[int]) -> Tensor:
        ctx.in_splits, ctx.out_splits = in_splits, out_splits
        out = data.new_empty((sum(out_splits),) + tuple(data.shape[1:]))
        _all_to_all_single(out, data.contiguous(), out_splits, in_splits)
        return out

    @staticmethod
    def backward(ctx, v_out: Tensor):
        v_in = v_out.new_empty((sum(ctx.in_splits),) + tuple(v_out.shape[1:]))
        _all_to_all_single(v_in, v_out.contiguous(), ctx.in_splits, ctx.out_splits)
        return v_in, None, None


class _AllGatherRows(torch.autograd.Function):
    """Differentiable all_gather of equally-shaped tensors along a new leading dim."""

    @staticmethod
    def forward(ctx, data: Tensor) -> Tensor:
        world = dist.get_world_size()
        # concatenated form [world * N, ...] (accepted by both RCCL and gloo)
        out = data.new_empty((world * data.shape[0],) + tuple(data.shape[1:]))
        _all_gather_into(out, data.contiguous())
        ctx.rows = data.shape[0]
        return out

    @staticmethod
    def backward(ctx, v_out: Tensor):
        # d/d(local) = sum over ranks of their gradient for my slab
        v = v_out.contiguous().clone()
        _all_reduce_sum(v)
        r = dist.get_rank()
        return v[r * ctx.rows : (r + 1) * ctx.rows]


# ---------------------------------------------------------------------------
# reference collectives API
# ---------------------------------------------------------------------------
def all_gather_int32(
    world_size: int, value: Union[int, Tensor], device: Optional[torch.device] = None
) -> List[Union[int, Tensor]]:
    """Gather a 32-bit integer from all ranks (reference distributed.py:10-52)."""
    if _single(world_size):
        return [value]
    if isinstance(value, int):
        assert device is not None, "device is required for scalar input"
        t = torch.tensor([value], dtype=torch.int32, device=device)
    else:
        t = value.reshape(1)
    out = torch.empty(world_size, dtype=t.dtype, device=t.device)
    _all_gather_into(out, t)
    return out.tolist() if isinstance(value, int) else list(out.unbind())


_HOST_GROUP = {}


def _host_group():
    """A gloo group next to the RCCL one, for exchanging HOST integers (shard sizes) without touching the GPU queue:
    a device-side gather + read-back would make the host wait for the whole previous step before it can queue the
    next one.  None when it cannot be created (then the device path is used)."""
    world = dist.group.WORLD
    hit = _HOST_GROUP.get("world")
    if hit is None or hit[0] is not world:  # (the world object itself is held: a re-created default group can never alias it)
        g = None
        if "nccl" in _backend_name() and os.environ.get("GS_DIST_HOST_GROUP", "1") == "1":
            try:
                g = dist.new_group(backend="gloo")
            except Exception:  # noqa: BLE001 -- same outcome on every rank (same environment)
                g = None
        hit = _HOST_GROUP["world"] = (world, g)
    return hit[1]


def gather_shard_meta(world_size: int, N: int, viewmats: Tensor, Ks: Tensor, cap: int = 0):
    """What the gaussian-sharded mode needs from the other ranks before it can project (reference rendering.py:283-291:
    three collectives and a read-back): the shard sizes and ALL cameras -- plus, for the sparse exchange, the chunk
    capacity every rank is going to use (``cap``, see ``sparse_capacity``).  The integers are host values and travel over
    the host group (no GPU synchronisation), ASYNCHRONOUSLY: the all-gather is started here and only waited for when the
    sizes are first needed (``sizes()``, at the exchange -- the projection is queued in between); the cameras take ONE
    device all-gather of [viewmats | Ks] per rank.
    Returns (sizes, viewmats [C_total,4,4], Ks [C_total,3,3]) with ``sizes() -> (N_world, cap_world)``; cameras carry no
    gradient here."""
    C = viewmats.shape[0]
    hg = _host_group()
    cams = torch.cat([viewmats.detach().reshape(-1).float(), Ks.detach().reshape(-1).float()])
    work = ints = None
    if hg is not None:
        ints = torch.empty(2 * world_size, dtype=torch.int64)
        work = dist.all_gather_into_tensor(ints, torch.tensor([N, cap], dtype=torch.int64), group=hg, async_op=True)
        buf = cams
    else:
        n = torch.tensor([N, cap], dtype=torch.int32, device=viewmats.device).view(torch.float32)
        buf = torch.cat([cams, n])
    out = buf.new_empty((world_size, buf.numel()))
    _all_gather_into(out.view(-1), buf)
    cache: List[Any] = []

    def sizes() -> Tuple[List[int], List[int]]:
        if not cache:
            if work is not None:
                work.wait()
                t = ints.view(world_size, 2)
            else:
                t = out[:, 25 * C:25 * C + 2].contiguous().view(torch.int32)  # (device path: this read-back synchronises)
            cache.append((t[:, 0].tolist(), t[:, 1].tolist()))
        return cache[0]

    return (sizes, out[:, :16 * C].reshape(world_size * C, 4, 4).contiguous(),
            out[:, 16 * C:25 * C].reshape(world_size * C, 3, 3).contiguous())


def all_to_all_int32(
    world_size: int, values: List[Union[int, Tensor]], device: Optional[torch.device] = None
) -> List[Union[int, Tensor]]:
    """Exchange one 32-bit integer with every rank (reference distributed.py:55-99)."""
    if _single(world_size):
        return values
    assert len(values) == world_size, "The length of values should be equal to world_size"
    scalar = any(isinstance(v, int) for v in values)
    if scalar:
        assert device is not None, "device is required for scalar input"
        t = torch.tensor([int(v) for v in values], dtype=torch.int32, device=device)
    else:
        t = torch.stack([v.reshape(()) for v in values]).to(torch.int32)
    out = torch.empty_like(t)
    ones = [1] * world_size
    _all_to_all_single(out, t, ones, ones)
    return out.tolist() if scalar else list(out.unbind())


def all_gather_tensor_list(world_size: int, tensor_list: List[Tensor]) -> List[Tensor]:
    """Gather a list of same-shaped-across-ranks tensors (reference distributed.py:102-167).

    Returns, for every input tensor of shape [N, *], the concatenation over ranks
    [world_size * N, *].  Differentiable.
    """
    if _single(world_size):
        return tensor_list
    N = len(tensor_list[0])
    for t in tensor_list:
        assert len(t) == N, "All tensors should have the same first dimension size"
    data = torch.cat([t.reshape(N, -1) for t in tensor_list], dim=-1)
    sizes = [t.numel() // N for t in tensor_list]
    if data.requires_grad:
        gathered = _AllGatherRows.apply(data)
    else:
        gathered = data.new_empty((world_size * N,) + tuple(data.shape[1:]))
        _all_gather_into(gathered, data.contiguous())
    gathered = gathered.reshape(world_size * N, -1)
    outs = torch.split(gathered, sizes, dim=-1)
    return [o.reshape(-1, *t.shape[1:]) for o, t in zip(outs, tensor_list)]


def all_to_all_tensor_list(
    world_size: int,
    tensor_list: List[Tensor],
    splits: List[Union[int, Tensor]],
    output_splits: Optional[List[Union[int, Tensor]]] = None,
) -> List[Tensor]:
    """Split every tensor along dim 0 by ``splits`` and exchange (reference distributed.py:170-257)."""
    if _single(world_size):
        return tensor_list
    N = len(tensor_list[0])
    for t in tensor_list:
        assert len(t) == N, "All tensors should have the same first dimension size"
    assert len(splits) == world_size, "The length of splits should be equal to world_size"
    data = torch.cat([t.reshape(N, -1) for t in tensor_list], dim=-1)
    sizes = [t.numel() // N for t in tensor_list]
    if output_splits is None:
        output_splits = all_to_all_int32(world_size, splits, device=data.device)
    in_splits = [int(s.item()) if isinstance(s, Tensor) else int(s) for s in splits]
    out_splits = [int(s.item()) if isinstance(s, Tensor) else int(s) for s in output_splits]
    if data.requires_grad:
        collected = _AllToAllRows.apply(data, in_splits, out_splits)
    else:
        collected = data.new_empty((sum(out_splits),) + tuple(data.shape[1:]))
        _all_to_all_single(collected, data.contiguous(), out_splits, in_splits)
    outs = torch.split(collected, sizes, dim=-1)
    return [o.reshape(-1, *t.shape[1:]) for o, t in zip(outs, tensor_list)]


def exchange_projected(
    world_rank: int, world_size: int, N: int, N_world: List[int], C_world: List[int], packed: bool,
    radii: Tensor, means2d: Tensor, depths: Tensor, conics: Tensor, opacities: Tensor, colors: Tensor,
    camera_ids: Optional[Tensor], gaussian_ids: Optional[Tensor], cap_world: Optional[Sequence[int]] = None,
):
    """Gaussian-sharded -> camera-sharded redistribution (reference rendering.py:397-478).

    Every rank has projected ITS gaussians onto ALL cameras; afterwards every rank holds
    ALL gaussians projected onto ITS cameras.  Returns
    (C_local, radii, means2d, depths, conics, opacities, colors, camera_ids, gaussian_ids).
    """
    device = means2d.device
    C_local = C_world[world_rank]
    if packed:
        C_total = sum(C_world)
        cnts = torch.bincount(camera_ids, minlength=C_total).split(C_world, dim=0)
        cnts = [c.sum() for c in cnts]
        collected_splits = all_to_all_int32(world_size, cnts, device=device)
        (radii,) = all_to_all_tensor_list(world_size, [radii], cnts, output_splits=collected_splits)
        means2d, depths, conics, opacities, colors = all_to_all_tensor_list(
            world_size, [means2d, depths, conics, opacities, colors], cnts, output_splits=collected_splits
        )
        # global -> local camera ids, local -> global gaussian ids
        cnts_t = torch.stack(cnts)
        cam_off = torch.tensor([0] + C_world[:-1], device=device, dtype=camera_ids.dtype).cumsum(0)
        camera_ids = camera_ids - cam_off.repeat_interleave(cnts_t)
        # NOTE (deliberate fix): the reference adds the offset of the DESTINATION
        # rank here (rendering.py:428-436: offsets.repeat_interleave(cnts)), which makes ids of
        # different source ranks collide; a local id becomes global by adding the offset of the
        # rank that OWNS the gaussian, i.e. this (source) rank.
        gaussian_ids = gaussian_ids + int(sum(N_world[:world_rank]))
        camera_ids, gaussian_ids = all_to_all_tensor_list(
            world_size, [camera_ids, gaussian_ids], cnts, output_splits=collected_splits
        )
        return C_local, radii, means2d, depths, conics, opacities, colors, camera_ids, gaussian_ids

    if cap_world is not None and sparse_enabled(means2d, C_world):
        out = _ExchangeSparse.apply(radii, means2d, depths, conics, opacities, colors, N, tuple(N_world), tuple(C_world), world_rank,
                                    tuple(cap_world))
    else:
        out = _ExchangeDense.apply(radii, means2d, depths, conics, opacities, colors, N, tuple(N_world), tuple(C_world), world_rank)
    return (C_local,) + tuple(out) + (None, None)


def _pack_rows(parts, rows: int, like: Tensor, row_index: Optional[Tensor] = None) -> Tensor:
    """[rows, sum(widths)] fp32 wire rows from column blocks (None = zeros; int32 travels as its bit pattern; parts flagged
    ``indexed`` are read at row ``row_index[r]``)."""
    if like.is_cuda:
        from ._wrapper import rows_pack

        return rows_pack(parts, rows, like, row_index)
    cols = []
    for part in parts:
        t, w = part[0], part[1]
        if t is None:
            cols.append(like.new_zeros((rows, w), dtype=torch.float32))
            continue
        t = t.reshape(-1, w)
        if len(part) > 2 and part[2]:
            t = t[row_index.long()]
        cols.append(t.view(torch.float32) if t.dtype == torch.int32 else t)
    return torch.cat(cols, dim=1)


def _unpack_rows(wire: Tensor, parts, row_index: Optional[Tensor] = None) -> None:
    if wire.is_cuda:
        from ._wrapper import rows_unpack

        return rows_unpack(wire, parts, row_index)
    off = 0
    for part in parts:
        t, w = part[0], part[1]
        if t is not None:
            src = wire[:, off:off + w].contiguous()
            src = src.view(torch.int32) if t.dtype == torch.int32 else src
            if len(part) > 2 and part[2]:
                ri = row_index.long()
                keep = ri >= 0  # a negative index = no row (as in gs_rows_unpack_indexed)
                t.view(-1, w)[ri[keep]] = src[keep]
            else:
                t.copy_(src.reshape(t.shape))
        off += w


_DENSE_WIDTHS = (1, 2, 1, 3, 1)  # radii (int32 bits) | means2d | depths | conics | opacities | then D colour channels


class _ExchangeDense(torch.autograd.Function):
    """The unpacked gaussian-sharded -> camera-sharded redistribution as ONE exchange each way.

    Forward: the six per-(camera, gaussian) arrays [C_total, N_local, *] are packed into one [C_total * N_local, 8 + D]
    fp32 row buffer (radii travel as their bit pattern), one all-to-all moves the rows of camera c to the rank that
    renders it, and the rows come out as [C_local, N_total, *] (source ranks are gaussian-contiguous, so for one camera
    per rank the received order already is the final one).  Backward: the five gradients are packed the same way, the
    dual all-to-all returns them, and they are handed on as column views of the received buffer (the projection / SH
    backward kernels read strided rows; nothing is unpacked)."""

    @staticmethod
    def forward(ctx, radii, means2d, depths, conics, opacities, colors, N, N_world, C_world, rank):
        ctx.set_materialize_grads(False)
        C_total, C_local, D = sum(C_world), C_world[rank], colors.shape[-1]
        rows = C_total * N
        parts = [(radii, 1), (means2d, 2), (depths, 1), (conics, 3), (opacities, 1), (colors, D)]
        send = _pack_rows(parts, rows, means2d)
        in_splits = [c * N for c in C_world]
        out_splits = [C_local * n for n in N_world]
        recv = send.new_empty((sum(out_splits), send.shape[1]))
        _all_to_all_single(recv, send, out_splits, in_splits)
        N_total = sum(N_world)
        if C_local != 1:  # rank-major [(C_local, N_i) per source rank] -> [C_local, N_total]
            recv = torch.cat([p.view(C_local, n, -1) for p, n in zip(recv.split(out_splits, dim=0), N_world)], dim=1)
        recv = recv.view(C_local * N_total, -1)
        ctx.meta = (N, N_world, C_world, rank, D)
        outs = [recv.new_empty((C_local, N_total) + ((w,) if k in (1, 3, 5) else ()), dtype=torch.int32 if k == 0 else torch.float32)
                for k, w in enumerate(list(_DENSE_WIDTHS) + [D])]
        _unpack_rows(recv, list(zip(outs, list(_DENSE_WIDTHS) + [D])))
        radii_o = outs[0]
        ctx.mark_non_differentiable(radii_o)
        return tuple(outs)

    @staticmethod
    def backward(ctx, _v_radii, v_means2d, v_depths, v_conics, v_opacities, v_colors):
        N, N_world, C_world, rank, D = ctx.meta
        C_total, C_local, N_total = sum(C_world), C_world[rank], sum(N_world)
        ref = next(g for g in (v_means2d, v_conics, v_colors, v_opacities, v_depths) if g is not None)
        v_recv = _pack_rows([(v_means2d, 2), (v_depths, 1), (v_conics, 3), (v_opacities, 1), (v_colors, D)], C_local * N_total, ref)
        v_recv = v_recv.view(C_local, N_total, -1)  # [C_local, N_total, 7 + D]; absent gradients are zero columns
        W = v_recv.shape[-1]
        if C_local != 1:
            v_recv = torch.cat([p.reshape(-1, W) for p in v_recv.split(list(N_world), dim=1)], dim=0)
        v_recv = v_recv.view(C_local * N_total, W)
        v_send = v_recv.new_empty((C_total * N, W))
        _all_to_all_single(v_send, v_recv, [c * N for c in C_world], [C_local * n for n in N_world])
        v = v_send.view(C_total, N, W)
        g_m2, g_d, g_cn, g_op, g_col = v.split([2, 1, 3, 1, D], dim=-1)
        # every rank renders with the same mode, so an absent depth gradient here is absent everywhere (its column is zeros)
        return (None, g_m2, None if v_depths is None else g_d.squeeze(-1), g_cn, g_op.squeeze(-1), g_col, None, None, None, None)


# state of the sparse exchange: the visible fraction seen so far (drives the chunk capacity) and the read-backs in flight
_SPARSE: Dict[str, Any] = {"frac": 1.0, "stats": None, "overflow": None}
_SPARSE_HEADROOM, _SPARSE_QUANTUM = 1.25, 1024


def sparse_enabled(like: Tensor, C_world: Sequence[int]) -> bool:
    return like.is_cuda and os.environ.get("GS_DIST_SPARSE", "1") == "1" and len(set(C_world)) == 1


def sparse_capacity(C_local: int, N: int, full: bool = False) -> int:
    """Row slots per destination chunk for the next sparse exchange of [C_local * world, N] rows: the largest visible
    count of the previous exchange x 1.25 (everything on the first call).  No synchronisation: the previous step's
    statistics were copied to pinned memory before its tile-count read-back, so they are complete by now."""
    st = _SPARSE
    if st["stats"] is not None:
        pinned, ev, rows = st["stats"]
        ev.synchronize()
        if rows > 0:
            st["frac"] = min(1.0, float(pinned[1]) / rows * _SPARSE_HEADROOM + 0.01)  # (overflow, max count, own overflow)
        st["stats"] = None
    rows = C_local * N
    if full or st["frac"] >= 1.0:
        return rows
    cap = -(-int(st["frac"] * rows) // _SPARSE_QUANTUM) * _SPARSE_QUANTUM
    return max(min(cap, rows), min(rows, _SPARSE_QUANTUM))


def exchange_overflowed() -> bool:
    """True when some rank had more visible rows than its chunk capacity in the last sparse exchange (every rank sees the
    same answer: the flags travel in the chunk headers).  Call after a host synchronisation that follows the exchange
    (the tile-count read-back); the caller then repeats the exchange at full capacity."""
    st = _SPARSE
    if st["overflow"] is None:
        return False
    pinned, ev = st["overflow"]
    ev.synchronize()
    st["overflow"] = None
    over = int(pinned[0]) != 0
    if over:
        st["frac"], st["stats"] = 1.0, None
    return over


_HDR_ROWS: Dict[Any, Tensor] = {}


class _ExchangeSparse(torch.autograd.Function):
    """`_ExchangeDense` with only the VISIBLE (camera, gaussian) rows on the wire (29 % of them at bench config 2), and
    still no read-back: every rank sends one fixed-size chunk per destination, sized from the visible fraction of ITS
    previous exchanges (the sizes travel with the shard sizes over the host group), and `gs_exchange_compact` fills the
    chunk with the rows whose radii > 0.  A chunk ends with a header row carrying the real count and an overflow flag;
    every receiver reads the headers of all chunks, so all ranks agree when some chunk was too small and repeat the
    exchange at full capacity (`exchange_overflowed`).  The receiver still gets the reference's dense [C_local, N_total, *]
    arrays: radii are zero wherever nothing arrived, the others are only defined where radii > 0 (as the reference leaves
    them, SURVEY 8a' quirk 2).  Wire row: destination row | aux | radii | means2d | depths | conics | opacity | colours."""

    @staticmethod
    def forward(ctx, radii, means2d, depths, conics, opacities, colors, N, N_world, C_world, rank, cap_world):
        from ._wrapper import exchange_compact

        ctx.set_materialize_grads(False)
        world = len(C_world)
        C_total, C_local, D = sum(C_world), C_world[rank], colors.shape[-1]
        N_total, N_off, cap = sum(N_world), sum(N_world[:rank]), int(cap_world[rank])
        dev = means2d.device
        src_index, hdr, counters, stats = exchange_compact(radii.contiguous(), C_local, world, cap, N_total, N_off)
        rows = world * (cap + 1)
        send = _pack_rows([(hdr, 2), (radii, 1, True), (means2d, 2, True), (depths, 1, True), (conics, 3, True),
                           (opacities, 1, True), (colors, D, True)], rows, means2d, src_index)
        send_splits = [cap + 1] * world
        recv_splits = [int(c) + 1 for c in cap_world]
        recv = send.new_empty((sum(recv_splits), send.shape[1]))
        _all_to_all_single(recv, send, recv_splits, send_splits)
        recv_i = recv.view(torch.int32)
        dst_recv = recv_i[:, 0]  # a column of the wire: read in place, kept for the backward
        outs = [torch.zeros((C_local, N_total), dtype=torch.int32, device=dev)]
        outs += [torch.empty((C_local, N_total) + ((w,) if k in (0, 2, 4) else ()), dtype=torch.float32, device=dev)
                 for k, w in enumerate([2, 1, 3, 1, D])]
        _unpack_rows(recv, [(None, 2)] + [(o, w, True) for o, w in zip(outs, [1, 2, 1, 3, 1, D])], dst_recv)
        # overflow flags of ALL senders (header rows of the received chunks) and my own statistics -> pinned memory
        key = (tuple(recv_splits), dev)
        if key not in _HDR_ROWS:
            _HDR_ROWS[key] = (torch.tensor(recv_splits, dtype=torch.int64).cumsum(0) - 1).to(dev)
        # one small kernel stores (overflow, max count, own overflow) straight into pinned host memory: no torch indexing /
        # reduction kernels, no copy commands, and the host reads them after the tile-count event it waits for anyway
        from . import _backend as B

        # (one persistent buffer: both readers run on the host before the next exchange is queued)
        if _SPARSE.get("pinned") is None:
            _SPARSE["pinned"] = torch.empty(3, dtype=torch.int32).pin_memory()
        p3 = _SPARSE["pinned"]
        with torch.cuda.device(dev):
            B.call("gs_exchange_flags", world, B.ptr(recv_i), int(recv.shape[1]), B.ptr(_HDR_ROWS[key]), B.ptr(stats), B.ptr(p3),
                   torch.cuda.current_stream(dev).cuda_stream)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        _SPARSE["overflow"], _SPARSE["stats"] = (p3, ev), (p3, ev, C_local * N)
        ctx.meta = (N, C_total, D, send_splits, recv_splits)
        ctx.save_for_backward(src_index, dst_recv)
        ctx.mark_non_differentiable(outs[0])
        return tuple(outs)

    @staticmethod
    def backward(ctx, _v_radii, v_means2d, v_depths, v_conics, v_opacities, v_colors):
        N, C_total, D, send_splits, recv_splits = ctx.meta
        src_index, dst_recv = ctx.saved_tensors
        ref = next(g for g in (v_means2d, v_conics, v_colors, v_opacities, v_depths) if g is not None)
        v_wire = _pack_rows([(v_means2d, 2, True), (v_depths, 1, True), (v_conics, 3, True), (v_opacities, 1, True),
                             (v_colors, D, True)], int(dst_recv.numel()), ref, dst_recv)
        W = v_wire.shape[1]
        v_back = v_wire.new_empty((int(src_index.numel()), W))
        _all_to_all_single(v_back, v_wire, send_splits, recv_splits)
        v = v_back.new_zeros((C_total * N, W))  # rows that never left stay zero
        _unpack_rows(v_back, [(v, W, True)], src_index)
        g_m2, g_d, g_cn, g_op, g_col = v.view(C_total, N, W).split([2, 1, 3, 1, D], dim=-1)
        return (None, g_m2, None if v_depths is None else g_d.squeeze(-1), g_cn, g_op.squeeze(-1), g_col) + (None,) * 5


class _ExchangeRows(torch.autograd.Function):
    """`_ExchangeSparse` for SPLAT ROWS (``project_rows``): the 64-byte row of a visible (camera, gaussian) pair IS the wire
    row -- it already holds mean2d, conic, opacity, colour, depth and radius, and its padding columns 12 / 13 carry the
    destination row and the chunk header of ``gs_exchange_compact`` -- so nothing is packed or split on either side:
    ``gs_rows16_gather`` lists the visible rows into the send chunks, one all-to-all, ``gs_rows16_scatter`` puts them at
    their [C_local, N_total] places (and fills the dense radii / depths the binning streams through).  Backward: the
    gradient rows of ``gs_rasterize_bwd`` are gathered at the received rows' places, the dual all-to-all returns them, and
    they are scattered into a [C_total, N, 16] gradient-row buffer that ``gs_projection_rows_bwd`` / ``gs_sh_view_bwd`` read
    in place (rows that never travelled are never read: their radii are 0).  Capacity / overflow protocol as in
    `_ExchangeSparse`.  Inputs: the column views of ``rows`` [C_total, N, 16] (for autograd), depths, radii, rows."""

    @staticmethod
    def forward(ctx, means2d, conics, opacities, colors, depths, radii, rows, N, N_world, C_world, rank, cap_world):
        from ._wrapper import ROW, ROW_COLOR, ROW_CONIC, ROW_MEAN2D, ROW_OPACITY
        from . import _backend as B

        ctx.set_materialize_grads(False)
        world = len(C_world)
        C_total, C_local = sum(C_world), C_world[rank]
        N_total, N_off, cap = sum(N_world), sum(N_world[:rank]), int(cap_world[rank])
        dev = rows.device
        n_send = world * (cap + 1)
        st = torch.cuda.current_stream(dev).cuda_stream
        # compaction + gather of the visible rows into the send chunks: one native call (src_index stays for the backward)
        src_index = torch.empty(n_send, dtype=torch.int32, device=dev)
        aux = torch.empty(n_send * 2 + world + 2, dtype=torch.int32, device=dev)  # hdr [n_send, 2] | counters [world] | stats [2]
        hdr, counters, stats = aux[:n_send * 2], aux[n_send * 2:n_send * 2 + world], aux[n_send * 2 + world:]
        send = torch.empty((n_send, ROW), dtype=torch.float32, device=dev)
        radii = radii.contiguous()
        radii_l = torch.empty((C_local, N_total), dtype=torch.int32, device=dev)  # (zero-filled by the call's first launch)
        with torch.cuda.device(dev):
            B.call("gs_exchange_rows_send", C_total, N, C_local, world, cap, N_total, N_off, B.ptr(radii), B.ptr(rows), B.ptr(src_index),
                   B.ptr(hdr), B.ptr(counters), B.ptr(stats), B.ptr(send), B.ptr(radii_l), C_local * N_total, st)
        send_splits = [cap + 1] * world
        recv_splits = [int(c) + 1 for c in cap_world]
        n_recv = sum(recv_splits)
        recv = send.new_empty((n_recv, ROW))
        _all_to_all_single(recv, send, recv_splits, send_splits)
        depths_l = torch.empty((C_local, N_total), dtype=torch.float32, device=dev)
        rows_l = torch.empty((C_local, N_total, ROW), dtype=torch.float32, device=dev)
        key = (tuple(recv_splits), dev)
        if key not in _HDR_ROWS:
            _HDR_ROWS[key] = (torch.tensor(recv_splits, dtype=torch.int64).cumsum(0) - 1).to(dev)
        if _SPARSE.get("pinned") is None:
            _SPARSE["pinned"] = torch.empty(3, dtype=torch.int32).pin_memory()
        p3 = _SPARSE["pinned"]
        with torch.cuda.device(dev):  # scatter the rows to their places, collect the overflow flags: one call
            B.call("gs_exchange_rows_recv", n_recv, B.ptr(recv), C_local * N_total, B.ptr(rows_l), B.ptr(radii_l), B.ptr(depths_l), world,
                   B.ptr(_HDR_ROWS[key]), B.ptr(stats), B.ptr(p3), 1, st)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        _SPARSE["overflow"], _SPARSE["stats"] = (p3, ev), (p3, ev, C_local * N)
        ctx.meta = (N, C_total, C_local, N_total, send_splits, recv_splits, colors is not None)
        ctx.save_for_backward(src_index, recv)
        ctx.mark_non_differentiable(radii_l, rows_l)
        return (radii_l, rows_l[..., ROW_MEAN2D:ROW_MEAN2D + 2], depths_l, rows_l[..., ROW_CONIC:ROW_CONIC + 3], rows_l[..., ROW_OPACITY],
                rows_l[..., ROW_COLOR:ROW_COLOR + 3] if colors is not None else None, rows_l)

    @staticmethod
    def backward(ctx, _v_radii, v_means2d, v_depths, v_conics, v_opacities, v_colors, _v_rows):
        from ._wrapper import ROW, ROW_COLOR, ROW_CONIC, ROW_DEPTH, ROW_MEAN2D, ROW_OPACITY, _grad_rows_of, rows16_gather, rows16_scatter

        N, C_total, C_local, N_total, send_splits, recv_splits, has_colors = ctx.meta
        src_index, recv = ctx.saved_tensors
        dev = recv.device
        parts = [(v_means2d, ROW_MEAN2D, 2), (v_conics, ROW_CONIC, 3), (v_opacities, ROW_OPACITY, 1)]
        if has_colors:
            parts.append((v_colors, ROW_COLOR, 3))
        if v_depths is not None:
            parts.append((v_depths, ROW_DEPTH, 1))
        g_ptr, g_keep = _grad_rows_of(parts, (C_local, N_total), dev)
        n_recv, n_send = recv.shape[0], int(src_index.numel())
        v_wire = torch.empty((n_recv, ROW), dtype=torch.float32, device=dev)
        from . import _backend as B

        with torch.cuda.device(dev):  # (g_ptr: the gradient rows in place, or the buffer g_keep assembled from the parts)
            B.call("gs_rows16_gather", n_recv, recv.view(torch.int32)[:, 12].data_ptr(), ROW, g_ptr, None, B.ptr(v_wire),
                   torch.cuda.current_stream(dev).cuda_stream)
        del g_keep
        v_back = v_wire.new_empty((n_send, ROW))
        _all_to_all_single(v_back, v_wire, send_splits, recv_splits)
        g_src = torch.empty((C_total, N, ROW), dtype=torch.float32, device=dev)  # rows that never left are never read (radii 0)
        rows16_scatter(n_send, src_index, 1, v_back, g_src)
        return (g_src[..., ROW_MEAN2D:ROW_MEAN2D + 2], g_src[..., ROW_CONIC:ROW_CONIC + 3], g_src[..., ROW_OPACITY],
                g_src[..., ROW_COLOR:ROW_COLOR + 3] if has_colors else None,
                g_src[..., ROW_DEPTH] if v_depths is not None else None) + (None,) * 7


def exchange_rows(world_rank: int, N: int, N_world: Sequence[int], C_world: Sequence[int], cap_world: Sequence[int],
                  radii: Tensor, means2d: Tensor, depths: Tensor, conics: Tensor, opacities: Tensor, colors: Optional[Tensor], rows: Tensor):
    """Gaussian-sharded -> camera-sharded redistribution of splat rows (`_ExchangeRows`).  Returns
    (C_local, radii, means2d, depths, conics, opacities, colors, rows) in the receiver's [C_local, N_total] layout."""
    out = _ExchangeRows.apply(means2d, conics, opacities, colors, depths, radii, rows, N, tuple(N_world), tuple(C_world), world_rank,
                              tuple(cap_world))
    return (C_world[world_rank],) + tuple(out)


# ---------------------------------------------------------------------------
# camera-sharded data parallelism (north-star design)
# ---------------------------------------------------------------------------
def shard_cameras(n_cameras: int, rank: int, world_size: int) -> List[int]:
    """Camera indices rendered by ``rank``: r, r + world, r + 2 world, ..."""
    return list(range(rank, n_cameras, world_size))


def rasterization_camera_sharded(
    means: Tensor, quats: Tensor, scales: Tensor, opacities: Tensor, colors: Tensor,
    viewmats: Tensor, Ks: Tensor, width: int, height: int,
    rank: Optional[int] = None, world_size: Optional[int] = None, **kwargs,
):
    """Render this rank's share of a camera batch with replicated splats.

    ``viewmats`` / ``Ks`` hold the GLOBAL batch [C,...]; rank r renders cameras r::world.
    Returns (render_colors [C_local,H,W,X], render_alphas, meta, camera_indices).  No
    communication happens here; call ``all_reduce_splat_grads`` after ``backward()``.
    ``sparse_grads=True`` (unpacked mode) additionally gathers the ranks' visibility masks (1 byte per splat) and leaves
    a ``SparseGradPlan`` in ``meta["grad_plan"]``: pass it to ``all_reduce_splat_grads(..., plan=...)`` and only the
    rows some camera saw travel.
    """
    from .rendering import rasterization

    if rank is None:
        rank = dist.get_rank() if dist.is_initialized() else 0
    if world_size is None:
        world_size = dist.get_world_size() if dist.is_initialized() else 1
    idx = shard_cameras(viewmats.shape[0], rank, world_size)
    assert len(idx) > 0, "more ranks than cameras"
    sel = torch.as_tensor(idx, device=viewmats.device)
    if colors.dim() == (4 if kwargs.get("sh_degree") is not None else 3):
        colors = colors[sel]  # per-view colours follow their cameras
    kwargs.pop("distributed", None)
    sparse_grads = kwargs.pop("sparse_grads", False)
    if sparse_grads and kwargs.get("packed", True):
        # (packed COO intermediates carry no [C, N] visibility array to build the plan from; silently returning without a plan
        # would leave the caller reducing nothing)
        raise ValueError("rasterization_camera_sharded(sparse_grads=True) needs packed=False")
    rc, ra, meta = rasterization(means, quats, scales, opacities, colors, viewmats[sel], Ks[sel], width, height,
                                 distributed=False, **kwargs)
    if sparse_grads and not kwargs.get("packed", True):
        # visibility masks of all ranks + row counts, for all_reduce_splat_grads(..., plan=meta["grad_plan"])
        meta["grad_plan"] = plan_sparse_grad_exchange(meta["radii"], world_size)
    return rc, ra, meta, idx


def flatten_grads(params: Sequence[Tensor]) -> Tuple[Tensor, List[Tuple[int, torch.Size]]]:
    """Pack ``p.grad`` of every parameter into one contiguous fp32 bucket (zeros for missing grads)."""
    total = sum(p.numel() for p in params)
    dev = params[0].device
    bucket = torch.empty(total, dtype=torch.float32, device=dev)
    layout = []
    off = 0
    for p in params:
        n = p.numel()
        if p.grad is None:
            bucket[off : off + n].zero_()
        else:
            g = p.grad
            if g.is_sparse:
                g = g.to_dense()
            bucket[off : off + n].copy_(g.reshape(-1))
        layout.append((off, p.shape))
        off += n
    return bucket, layout


class SparseGradPlan:
    """What the sparse gradient reduction needs to know, gathered in the FORWARD pass (``plan_sparse_grad_exchange``):
    every rank's visibility mask (which splats can have a non-zero gradient there), the union mask, the index lists both
    phases of the reduction walk -- all with static sizes, built while the forward's latency-bound binning kernels run --
    and, on the host, read back together with the renderer's own intersection count (so without a synchronisation of its
    own), how many rows every rank holds for every owner block and how many rows every block's union has."""

    def __init__(self, N, world, rank, block, masks, union, send_idx, urank, uidx, pinned, event):
        self.N, self.world, self.rank, self.block = N, world, rank, block
        self.masks, self.union = masks, union  # uint8 [world, world * block], bool [world * block]
        # int32, all GLOBAL and of length n_pad = world * block, the same on every rank but for send_idx:
        #   send_idx  my visible splats in ascending order; entries behind my row count (sum(rows[rank])) are undefined
        #             (the torch route pads with -1, gs_dp_plan leaves them unwritten)
        #   uidx      the splats of the union of ALL ranks' masks in ascending order, so owner o's union rows are the slice
        #             [uoff, uoff + urows[o]) with uoff = sum(urows[:o]); entries behind sum(urows) are undefined (-1 / unwritten)
        #   urank     urank[n] = position of splat n in uidx; an owner's accumulator row is urank[n] - uoff.  Defined on union
        #             splats ONLY: off the union the torch route holds cumsum(union) - 1 (the rank of the last union splat in
        #             front, -1 in front of the first), gs_dp_plan writes nothing -- nothing may read it there (wire rows carry
        #             indices of visible splats only)
        # masks is uint8 [world, n_pad]; union is bool [n_pad] on the torch route and None on the native one.
        self.send_idx, self.urank, self.uidx = send_idx, urank, uidx
        self._pinned, self._event = pinned, event
        self._counts = None

    def counts(self):
        """(rows[r][o] held by rank r for owner o, union rows per owner) as host integers."""
        if self._counts is None:
            if self._event is not None:
                self._event.synchronize()
            c = self._pinned.view(self.world + 1, self.world).tolist()
            self._counts = (c[: self.world], c[self.world])
        return self._counts


def plan_sparse_grad_exchange(radii: Tensor, world_size: Optional[int] = None) -> Optional[SparseGradPlan]:
    """Call in the forward pass, right after projection (``meta["radii"]`` [C_local, N]): all-gathers the per-splat
    visibility masks of all ranks (1 byte per splat and rank: 1 MB at 1 M splats against the 236 MB of gradients), builds
    the index lists of the reduction and starts the asynchronous read-back of the row counts.  Splat n belongs to owner
    block n // ceil(N / world).  On the GPU the lists come from three kernels (gs_dp_visibility, gs_dp_plan: two launches);
    the torch formulation below (CPU / gloo tests, world > 16) is ~35 small launches."""
    if world_size is None:
        world_size = dist.get_world_size() if dist.is_initialized() else 1
    if _single(world_size):
        return None
    rank = dist.get_rank()
    N = radii.shape[-1]
    block = -(-N // world_size)
    n_pad = world_size * block
    dev = radii.device
    native = radii.is_cuda and world_size <= 16 and radii.dtype == torch.int32
    if native:
        from . import _backend as B

        # gs_dp_plan's two-launch scan covers 65536 tiles (134 M padded splats); beyond that the torch formulation below
        native = int(B.query("gs_dp_plan_tiles", n_pad)) <= 65536
    if native:
        r2 = radii.reshape(-1, N).contiguous()
        vis = torch.empty(n_pad, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            B.call("gs_dp_visibility", r2.shape[0], N, n_pad, B.ptr(r2), B.ptr(vis), st)
    else:
        vis = torch.zeros(n_pad, dtype=torch.uint8, device=dev)
        vis[:N] = (radii.reshape(-1, N) > 0).any(0)
    masks = torch.empty((world_size, n_pad), dtype=torch.uint8, device=dev)
    _all_gather_into(masks.view(-1), vis)
    if native:
        counts = torch.zeros(world_size * world_size + world_size, dtype=torch.int32, device=dev)
        send_idx = torch.empty(n_pad, dtype=torch.int32, device=dev)
        urank, uidx = torch.empty_like(send_idx), torch.empty_like(send_idx)
        tiles = torch.empty(int(B.query("gs_dp_plan_tiles", n_pad)) * 2, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            B.call("gs_dp_plan", world_size, rank, n_pad, block, B.ptr(masks), B.ptr(tiles), B.ptr(counts), B.ptr(send_idx), B.ptr(urank),
                   B.ptr(uidx), st)
        union = None
        pinned = torch.empty(counts.numel(), dtype=torch.int32).pin_memory()
        pinned.copy_(counts, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        return SparseGradPlan(N, world_size, rank, block, masks, union, send_idx, urank, uidx, pinned, ev)
    union = masks.any(0)
    rows = masks.view(world_size, world_size, block).sum(-1, dtype=torch.int32)      # [rank, owner]
    urows = union.view(world_size, block).sum(-1, dtype=torch.int32)                 # [owner]
    both = torch.cat([rows.reshape(-1), urows]).to(torch.int64)
    # index lists (static sizes, -1 padded; ascending order keeps every owner's rows contiguous)
    send_idx = torch.nonzero_static(vis, size=n_pad, fill_value=-1).view(-1).to(torch.int32)
    urank = torch.cumsum(union, 0, dtype=torch.int32) - 1                            # position in the list of ALL union splats
    uidx = torch.nonzero_static(union, size=n_pad, fill_value=-1).view(-1).to(torch.int32)
    if both.is_cuda:
        pinned = torch.empty(both.numel(), dtype=torch.int64).pin_memory()
        pinned.copy_(both, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
    else:
        pinned, ev = both.clone(), None
    return SparseGradPlan(N, world_size, rank, block, masks, union, send_idx, urank, uidx, pinned, ev)


def _reduce_received_rows(recv: Tensor, out_splits: List[int], urank: Tensor, uoff: int, uidx_mine: Tensor, umax: int,
                          scale: float) -> Tensor:
    """The owner's accumulator [umax, 1 + D]: row u = (index of the u-th union splat of my block, or -1 for padding |
    scale * sum over senders of the received row of that splat).  ``recv`` holds one chunk per sender; column 0 of a row is
    its splat index (int32 bit pattern)."""
    D1 = recv.shape[1]
    n_u = int(uidx_mine.numel())
    if recv.is_cuda:
        import ctypes

        from . import _backend as B

        W = len(out_splits)
        acc = torch.empty((umax, D1), dtype=torch.float32, device=recv.device)
        inv = torch.empty(W * umax, dtype=torch.int32, device=recv.device)
        starts = (ctypes.c_int64 * (W + 1))(*([0] + [sum(out_splits[: k + 1]) for k in range(W)]))
        with torch.cuda.device(recv.device):
            B.call("gs_dp_reduce_rows", recv.shape[0], D1 - 1, W, B.ptr(recv), ctypes.addressof(starts), B.ptr(urank), int(uoff), umax,
                   n_u, B.ptr(uidx_mine) if n_u else None, float(scale), B.ptr(inv), B.ptr(acc),
                   torch.cuda.current_stream(recv.device).cuda_stream)
        return acc
    acc = torch.zeros((umax, D1), dtype=torch.float32, device=recv.device)
    col0 = torch.full((umax,), -1, dtype=torch.int32)
    col0[:n_u] = uidx_mine
    acc[:, 0] = col0.view(torch.float32)
    if recv.shape[0]:
        idx = recv[:, 0].contiguous().view(torch.int32).long()
        ok = idx >= 0
        acc[:, 1:].index_add_(0, urank[idx[ok]].long() - uoff, recv[ok, 1:] * scale)
    return acc


def _sparse_all_reduce(plist: List[Tensor], plan: SparseGradPlan, average: bool) -> None:
    """Sum of the splat gradients over ranks moving only the rows some camera saw.  Wire rows carry their splat index in
    column 0 (an int32 bit pattern: 4 bytes on top of the 236 of a degree-3 gradient row), so neither side has to
    reconstruct the other's order.

    Phase 1 (reduce-scatter): rank r sends owner o its visible rows of block o as one variable-split all-to-all; the
    owner adds them into the compact accumulator of its block's UNION (one row per splat some camera saw).  Phase 2
    (all-gather): every owner hands out that accumulator, padded to the largest union, and every rank writes the rows back
    at the indices they carry.  Rows outside the union are zero on every rank and stay untouched (the render loss gives
    culled splats exactly zero gradient; a loss term that touches EVERY splat, such as an opacity regulariser, must be
    reduced densely -- see all_reduce_splat_grads).  Local work: one pack, one gather-reduce, one unpack kernel over the
    visible rows; every index list comes from the plan built in the forward; no host synchronisation beyond
    the plan's counts."""
    W, rank, N, block = plan.world, plan.rank, plan.N, plan.block
    rows, urows = plan.counts()
    dev = plist[0].device
    widths = [p.numel() // N for p in plist]
    D = sum(widths)
    for p in plist:
        assert p.shape[0] == N, "sparse gradient exchange: every parameter must have one row per splat"
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        elif p.grad.is_sparse:
            p.grad = p.grad.to_dense()
        elif not p.grad.is_contiguous():
            p.grad = p.grad.contiguous()
    G = [p.grad.view(N, -1) for p in plist]
    if os.environ.get("GS_DP_DEBUG", "0") == "1":
        # the sparse form only moves rows of the union: a loss term that reaches splats NO camera saw (an opacity or scale
        # regulariser over all splats) would be left unreduced -- catch it instead of diverging silently
        outside = ~plan.masks.any(0)[:N]
        for p, g in zip(plist, G):
            if bool((g[outside] != 0).any()):
                raise RuntimeError("sparse gradient exchange: non-zero gradient rows outside the union of the visibility masks "
                                   "(a loss term over all splats?) -- reduce those parameters densely (plan=None)")
    # ---- phase 1: [index | values] rows of my visible splats, grouped by owner (ascending indices)
    n_mine = sum(rows[rank])
    idx = plan.send_idx[:n_mine]
    parts = [(idx, 1, False)] + [(g, wdt, True) for g, wdt in zip(G, widths)]
    send = _pack_rows(parts, n_mine, G[0], idx) if n_mine else torch.empty((0, D + 1), dtype=torch.float32, device=dev)
    in_splits = [int(c) for c in rows[rank]]
    out_splits = [int(rows[r][rank]) for r in range(W)]
    recv = send.new_empty((sum(out_splits), D + 1))
    _all_to_all_single(recv, send, out_splits, in_splits)
    umax = max(int(u) for u in urows)
    uoff, n_u = sum(int(u) for u in urows[:rank]), int(urows[rank])
    # the owner's accumulator: one row per union splat of my block (column 0 = its index), padded to the largest union; every
    # row is the sum of the <= world rows received for it (gather-reduce: no atomics, no zero-fill)
    acc = _reduce_received_rows(recv, out_splits, plan.urank, uoff, plan.uidx[uoff:uoff + n_u], umax, (1.0 / W) if average else 1.0)
    # ---- phase 2: every owner's union rows to everybody; padding rows carry index -1 and are skipped
    allrows = acc.new_empty((W * umax, D + 1))
    _all_gather_into(allrows.view(-1), acc.view(-1))
    if umax:  # (the row index is column 0 of the wire rows themselves: a strided int32 view, no copy)
        _unpack_rows(allrows, [(None, 1, False)] + [(g, wdt, True) for g, wdt in zip(G, widths)], allrows.view(torch.int32)[:, 0])


def _scatter_add_rows(acc: Tensor, idx: Tensor, rows: Tensor) -> None:
    """acc[idx[r]] += rows[r] (one pass of float atomics on the GPU; index_add_ elsewhere)."""
    if acc.is_cuda:
        from . import _backend as B

        with torch.cuda.device(acc.device):
            B.call("gs_scatter_add_rows_f32", rows.shape[0], rows.shape[1], B.ptr(rows.contiguous()), B.ptr(idx.contiguous()),
                   B.ptr(acc), torch.cuda.current_stream(acc.device).cuda_stream)
    else:
        acc.index_add_(0, idx, rows)


def all_reduce_splat_grads(
    params: Union[Dict[str, Tensor], Sequence[Tensor]],
    world_size: Optional[int] = None,
    average: bool = True,
    algorithm: str = "auto",
    plan: Optional[SparseGradPlan] = None,
) -> None:
    """Sum (or average) the splat gradients of all ranks in place.

    The exchange is 236 B/splat at SH degree 3 (means 3 + quats 4 + scales 3 + opacities 1 + SH 48 floats),
    81 % of it the SH gradient.  ``algorithm``:
      * "direct" (default on RCCL): NO packing -- every gradient tensor is reduced where it lies.  Large
        tensors whose size divides by the world size go through reduce_scatter_tensor (into a 1/world temp)
        + all_gather_into_tensor (back into the gradient): every rank talks to its 7 xGMI peers at once and
        nothing is copied; the rest use an in-place all_reduce.  Packing the bucket and copying it back would
        cost 4 x 236 MB of HBM traffic per step at 1 M splats, as much time as the collective itself.
      * "rs_ag": one packed bucket, reduce_scatter_tensor + all_gather_into_tensor.
      * "all_reduce": one packed bucket, single all_reduce (what "auto" uses on gloo, which has no reduce_scatter).
    ``average=True`` matches a single-process batch whose loss is a mean over all C images.
    ``plan`` (from ``plan_sparse_grad_exchange``, built in the forward): only the rows of splats that some camera saw
    travel (``_sparse_all_reduce``); every parameter must then have one row per splat, and its gradient must be zero for
    splats no camera saw -- true for the render loss, NOT for a regulariser over all splats (reduce such parameters with
    ``plan=None``; ``GS_DP_DEBUG=1`` checks the assumption on every call).
    """
    if world_size is None:
        world_size = dist.get_world_size() if dist.is_initialized() else 1
    plist = list(params.values()) if isinstance(params, dict) else list(params)
    keys = list(params.keys()) if isinstance(params, dict) else [None] * len(plist)
    keys = [k for k, p in zip(keys, plist) if p.requires_grad]
    plist = [p for p in plist if p.requires_grad]
    if _single(world_size) or not plist:
        return
    if plan is not None:
        _sparse_all_reduce(plist, plan, average)
        return
    if algorithm == "auto":
        algorithm = os.environ.get("GS_DP_ALGO", "direct" if "nccl" in _backend_name() else "all_reduce")
    if algorithm == "direct":
        scale = 1.0 / world_size
        # WHICH collectives are issued depends on rank-invariant facts only (the parameters' sizes, the world size, the
        # backend): a rank whose gradients do not lie in one buffer (its forward did not carve them: no camera of its own,
        # a repeated backward, a user-made .grad) stages them through a scratch span of the same canonical length and joins
        # the same reduce-scatter + all-gather as its peers.
        numels = [p.numel() for p in plist]
        used = sum(numels)
        if used * 4 >= _DIRECT_RS_AG_MIN_BYTES and all(p.dtype == torch.float32 for p in plist):
            length = _span_length(numels, world_size)
            # ONE layout of the span on every rank, whichever way a rank gets there: the pieces in _canonical_order (a
            # function of the dict keys / the list order only).  A rank reduces in place only when its gradients lie in
            # exactly that order; any other arrangement is staged into it (round-4 advisor finding: in-place ranks used
            # the carving order, staging ranks the dict order -- quats [N,4] and scales [N,3] swapped places between them)
            canon = [plist[i] for i in _canonical_order(keys)]
            span = _one_span(canon, length)
            staged = span is None
            if staged:
                if not _STAGING_LOGGED[0] and os.environ.get("GS_DP_QUIET") != "1" and any(p.is_cuda for p in plist):
                    _STAGING_LOGGED[0] = True
                    import warnings

                    warnings.warn("all_reduce_splat_grads: the gradients of this rank do not lie in rasterization()'s one buffer in the "
                                  f"canonical order (parameter names {keys}; known names: {sorted(_CARVE_RANK)}): staging them through a "
                                  "scratch span every step (correct, one extra copy each way).  Pass the parameters as a dict with the "
                                  "trainer's names to reduce in place.")
                span = _stage_span(canon, length)
            if "nccl" not in _backend_name():  # (gloo: no reduce_scatter_tensor; the tests' route)
                _all_reduce_sum(span)
                if average:
                    span.mul_(scale)
            else:
                # every gradient is a piece of ONE buffer (what rasterization() hands out, _wrapper.GradPrefill): one
                # reduce-scatter + one all-gather over the whole span instead of a pair (or an all-reduce) per tensor --
                # fewer, larger collectives; the alignment padding between and behind the pieces is summed along and never read
                shard = span.new_empty(length // world_size)
                _wire(2.0 * length * span.element_size() * (world_size - 1) / world_size)
                dist.reduce_scatter_tensor(shard, span, op=dist.ReduceOp.SUM)
                if average:
                    shard.mul_(scale)
                dist.all_gather_into_tensor(span, shard)
            if staged:
                _unstage_span(canon, span)
            return
        for p in plist:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            elif p.grad.is_sparse:
                p.grad = p.grad.to_dense()
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            flat = g.view(-1)
            _all_reduce_sum(flat)
            if average:
                flat.mul_(scale)
            if g is not p.grad:
                p.grad = g
        return
    bucket, layout = flatten_grads(plist)
    if algorithm == "rs_ag":
        n = bucket.numel()
        pad = (-n) % world_size
        if pad:
            bucket = torch.cat([bucket, bucket.new_zeros(pad)])
        shard = bucket.new_empty(bucket.numel() // world_size)
        dist.reduce_scatter_tensor(shard, bucket, op=dist.ReduceOp.SUM)
        if average:
            shard.mul_(1.0 / world_size)
        dist.all_gather_into_tensor(bucket, shard)
        bucket = bucket[:n]
    elif algorithm == "all_reduce":
        _all_reduce_sum(bucket)
        if average:
            bucket.mul_(1.0 / world_size)
    else:
        raise ValueError(f"unknown algorithm {algorithm!r}")
    for p, (off, shape) in zip(plist, layout):
        g = bucket[off : off + p.numel()].view(shape)
        if p.grad is None or p.grad.is_sparse:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def _span_length(numels: List[int], world_size: int) -> int:
    """Length (floats) of the canonical gradient span: every piece padded to 256 bytes (the carving rule of
    _wrapper.GradPrefill), the total rounded up to a multiple of the world size.  Rank-invariant."""
    n = sum((k + 63) // 64 * 64 for k in numels)
    return n + (-n) % world_size


# the order in which rasterization() carves the per-gaussian gradients out of its one buffer (_wrapper.PREFILL_ORDER, the one list both
# autograd nodes build their request from), by the names trainers give those parameters (the reference's trainers: means, scales,
# quats, opacities, sh0, shN | colors; the dynamic trainer adds motion, omega, trbf_center, trbf_scale)
def _carve_rank() -> dict:
    from ._wrapper import PREFILL_ORDER

    rank = {k: i for i, k in enumerate(PREFILL_ORDER)}
    rank["sh"] = rank["colors"]  # (colours and SH coefficients never ride in the same call: one slot)
    for alias, k in (("sh0", "sh"), ("sh_coeffs", "sh"), ("features_dc", "sh"), ("shN", "sh_rest"), ("features_rest", "sh_rest")):
        rank[alias] = rank[k]
    return rank


_CARVE_RANK = _carve_rank()
_STAGING_LOGGED = [False]


def _canonical_order(keys: List[Optional[str]]) -> List[int]:
    """Rank-invariant order of the span's pieces: parameters with a known name in the carving order of rasterization()
    (so a trainer's dict -- means, scales, quats, ... in the reference's -- maps onto the buffer its gradients already lie in),
    everything else behind them in the order given.  Depends on the keys / positions only, never on where a rank's gradients
    happen to live."""
    return sorted(range(len(keys)), key=lambda i: (_CARVE_RANK.get(keys[i], len(_CARVE_RANK) + 1), i))


def _one_span(plist: List[Tensor], length: int) -> Optional[Tensor]:
    """The flat fp32 tensor of ``length`` floats covering every ``p.grad`` IN PLACE, when they are all dense contiguous
    pieces of ONE storage lying **in the order of ``plist``**, every piece starting where the 256-byte padding of the
    previous one ends (GradPrefill's carving: no foreign data -- e.g. the gradient of a parameter that is not in ``plist``
    -- can sit inside the span, so reducing the span touches only what was asked for, and the layout equals what
    ``_stage_span`` builds from the same list on a rank that has to stage); None otherwise."""
    grads = [p.grad for p in plist]
    if any(g is None or g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() for g in grads):
        return None
    st = grads[0].untyped_storage()
    if any(g.untyped_storage().data_ptr() != st.data_ptr() for g in grads[1:]):
        return None
    lo = pos = grads[0].storage_offset()
    for g in grads:
        if g.storage_offset() != pos:
            return None
        pos += (g.numel() + 63) // 64 * 64
    # (the world-size rounding reaches into the slack rasterization() leaves behind the last piece -- never downwards: the
    # compositing gradient rows, which meta["means2d"].grad / .absgrad may still view, lie in front of the first piece)
    if lo + length > st.nbytes() // 4:
        return None
    return torch.empty(0, dtype=torch.float32, device=grads[0].device).set_(st, lo, (length,), (1,))


def _stage_span(plist: List[Tensor], length: int) -> Tensor:
    """Scratch span of the canonical layout holding a copy of every ``p.grad`` (zeros where a parameter has none)."""
    dev = next((p.grad.device for p in plist if p.grad is not None), plist[0].device)
    span = torch.zeros(length, dtype=torch.float32, device=dev)
    off = 0
    for p in plist:
        if p.grad is not None:
            g = p.grad.to_dense() if p.grad.is_sparse else p.grad
            span[off:off + p.numel()].view(p.shape).copy_(g)
        off += (p.numel() + 63) // 64 * 64
    return span


def _unstage_span(plist: List[Tensor], span: Tensor) -> None:
    off = 0
    for p in plist:
        piece = span[off:off + p.numel()].view(p.shape)
        if p.grad is None or p.grad.is_sparse or p.grad.dtype != torch.float32:
            p.grad = piece
        else:
            p.grad.copy_(piece)
        off += (p.numel() + 63) // 64 * 64


# below this an in-place all_reduce (latency-bound anyway); GS_DP_RS_AG_MIN_BYTES overrides (tests)
_DIRECT_RS_AG_MIN_BYTES = int(os.environ.get("GS_DP_RS_AG_MIN_BYTES", 8 << 20))


# ---------------------------------------------------------------------------
# launcher (reference distributed.py:260-360)
# ---------------------------------------------------------------------------
def _find_free_port() -> int:
    s = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def init_process_group(rank: int, world_size: int, init_method: Optional[str] = None,
                       backend: Optional[str] = None) -> None:
    """One process per GPU; RCCL ("nccl") when a GPU is present, gloo otherwise."""
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    if init_method is None:
        addr = os.environ.get("MASTER_ADDR", "127.0.0.1")
        port = os.environ.get("MASTER_PORT", "29500")
        init_method = f"tcp://{addr}:{port}"
    if backend == "nccl":
        torch.cuda.set_device(rank % torch.cuda.device_count())
    dist.init_process_group(backend=backend, init_method=init_method, world_size=world_size, rank=rank)


def _distributed_worker(local_rank: int, world_size: int, fn: Callable, args: Any, dist_url: str,
                        backend: Optional[str]) -> None:
    init_process_group(local_rank, world_size, init_method=dist_url, backend=backend)
    try:
        fn(local_rank, local_rank, world_size, args)
    finally:
        dist.barrier()
        dist.destroy_process_group()


def cli(fn: Callable, args: Any, verbose: bool = False, world_size: Optional[int] = None,
        backend: Optional[str] = None) -> bool:
    """Run ``fn(local_rank, world_rank, world_size, args)`` on every GPU of this node.

    Returns True when multi-process mode was used (same contract as the reference's ``cli``).
    """
    if world_size is None:
        world_size = torch.cuda.device_count() if torch.cuda.is_available() else 1
    if world_size <= 1:
        fn(0, 0, 1, args)
        return False
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist_url = f"tcp://127.0.0.1:{_find_free_port()}"
    if verbose:
        print(f"[gscodec_studio_amd.distributed] spawning {world_size} ranks at {dist_url}")
    import torch.multiprocessing as mp

    mp.spawn(_distributed_worker, nprocs=world_size, args=(world_size, fn, args, dist_url, backend), daemon=False)
    return True
