"""The grid sort at BASELINE config 2's size after the square crop (1003^2 = 1,006,009 splats, the 14 channels that are not shN,
the bench scene's seeded attributes):
  whole:   wall time of grid_sort_order (host normalisation, every round queued, one synchronise at the end)
  round:   the kernels of one round at a few radii of the schedule (HIP events): blur, keys, radix sort, assignment
  torch:   the same round restated in plain torch (reflect index + cumsum blur, torch.sort, gather + argmin over the 24 sums),
           run interleaved with the HIP round in this process; median and min..max of both
  size:    directory bytes of PngCompression with use_sort = False, "morton", "grid"
usage: python tools/bench_grid_sort.py [--rounds 7] [--out profiles/r15_grid_sort.txt] [--side 1003]"""
import argparse
import gc
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gscodec_studio_amd._helper import load_test_data  # noqa: E402
from gscodec_studio_amd.compression import PngCompression, grid_sort as G, grid_sort_reference as R  # noqa: E402

_LINES = []


def say(s=""):
    print(s, flush=True)
    _LINES.append(s)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return f"{statistics.median(ts):9.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f})"


def torch_round(q, order, side, r, perms):
    """One round in plain torch: q int32 [N, C], order int64 [N] -> new order.  Random draws from torch's generator (the hash is
    the HIP path's own); otherwise the arithmetic of grid_sort_reference."""
    n, c = q.shape
    w, b = 2 * r + 1, R.block_side(r)
    idx = torch.arange(-r, side + r, device=q.device).abs()
    idx = torch.where(idx >= side, 2 * (side - 1) - idx, idx)
    g = q[order].view(side, side, c)
    for axis in (1, 0):
        cs = torch.cumsum(g.index_select(axis, idx), dim=axis, dtype=torch.int32)
        s = cs.narrow(axis, w - 1, side).clone()
        s.narrow(axis, 1, side - 1).sub_(cs.narrow(axis, 0, side - 1))
        g = torch.div(2 * s + w, 2 * w, rounding_mode="floor")
    t = g.view(n, c)
    p = torch.arange(n, device=q.device)
    ox, oy = (int(v) for v in torch.randint(0, b, (2,)))
    block = ((p // side + oy) // b) * (side // b + 2) + (p % side + ox) // b
    key = (block << 32) | torch.randint(0, 1 << 32, (n,), device=q.device)
    pos = torch.sort(key, stable=True).indices
    grp = pos[: n // 4 * 4].view(-1, 4)
    blk = block[grp]
    grp = grp[(blk == blk[:, :1]).all(dim=1)]
    items = order[grp]
    d = (q[items][:, :, None, :] - t[grp][:, None, :, :]).pow(2).sum(dim=-1)  # [G, 4, 4]
    cost = d[:, torch.arange(4, device=q.device)[None, :], perms].sum(dim=-1)  # [G, 24]
    best = perms[cost.argmin(dim=1)]
    new = order.clone()
    new[grp.gather(1, best).reshape(-1)] = items.reshape(-1)
    return new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--side", type=int, default=0, help="crop the scene to side^2 splats (default: the largest square)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_grid_sort measures on the GPU"
    gc.collect()
    gc.freeze()
    dev = torch.device("cuda")
    means, quats, scales, opacities, colors, *_ = load_test_data(device="cpu", scene_grid=3)
    side = a.side or int(len(means) ** 0.5)
    n = side * side
    splats = {"means": means[:n], "scales": torch.log(scales[:n] + 1e-6), "quats": quats[:n], "opacities": torch.logit(opacities[:n].clamp(1e-4, 1 - 1e-4)),
              "sh0": ((colors[:n] - 0.5) / 0.2820947917738781).reshape(n, 1, 3)}
    splats = {k: v.to(dev).contiguous() for k, v in splats.items()}
    feats = torch.cat([v.reshape(n, -1) for v in splats.values()], dim=1)
    feats[:, :3] = torch.sign(feats[:, :3]) * torch.log1p(feats[:, :3].abs())
    radii = R.schedule(side)
    say(f"N = {n} splats (side {side}), C = {feats.shape[1]} channels, {len(radii)} rounds, radii {radii[0]} .. {radii[-1]}")

    # ---- whole call
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        order = G.grid_sort_order(feats)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    say(f"grid_sort_order, whole call (first call included): {', '.join(f'{t:.1f}' for t in ts)} ms")
    q_host = R.quantize_features(feats.cpu().numpy())
    for name, o in (("given order", np.arange(n)), ("grid order", order.cpu().numpy())):
        say(f"  neighbour metric, {name}: {R.neighbour_metric(q_host, o):.4g}")

    # ---- one round, per kernel, and the torch restatement interleaved
    q16 = torch.from_numpy(q_host.view(np.int16)).to(dev)
    q32 = q16.to(torch.int32)
    perms = torch.from_numpy(R.PERMUTATIONS).to(dev)
    rounds = G._Rounds(q16, side, 0)
    rounds.start()
    order64 = rounds.order.long()
    for r in sorted({radii[0], max(1, radii[0] // 5), min(10, radii[0]), 1}, reverse=True):
        b, bits = R.block_side(r), R.key_bits(side, r)
        parts = {"gs_gridsort_blur (2 launches)": lambda: rounds.blur(r), "gs_gridsort_keys": lambda: rounds.make_keys(b, 1),
                 f"gs_sort_pairs_u64_i32 ({bits} bits)": lambda: rounds.sort(bits), "gs_gridsort_assign": rounds.assign}
        rounds.round(r, 1)
        torch_round(q32, order64, side, r, perms)
        hip, tor, split = [], [], {k: [] for k in parts}
        for _ in range(a.rounds):
            hip.append(event_ms(lambda: rounds.round(r, 1)))
            tor.append(event_ms(lambda: torch_round(q32, order64, side, r, perms)))
            for k, fn in parts.items():
                split[k].append(event_ms(fn))
        say(f"radius {r} (block side {b}):")
        say(f"  HIP round                                   {stats(hip)}")
        for k, v in split.items():
            say(f"    {k:41s} {stats(v)}")
        say(f"  torch round                                 {stats(tor)}")
        say(f"  ratio of medians torch / HIP: {statistics.median(tor) / statistics.median(hip):.2f}; torch spread max / min: {max(tor) / min(tor):.2f}, "
            f"HIP spread max / min: {max(hip) / min(hip):.2f}")

    # ---- sizes
    for use_sort in (False, "morton", "grid"):
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            PngCompression(use_sort=use_sort, verbose=False).compress(d, splats)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            total = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        say(f"PngCompression(use_sort={use_sort!r}): {total} bytes in the directory ({dt:.1f} s to compress)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(_LINES) + "\n")


if __name__ == "__main__":
    main()
