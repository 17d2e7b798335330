"""The nearest-neighbour search at BASELINE config 2's 1,006,065 means (the garden crop tiled 3 x 3), K = 4 and 16, with the splats
  scene:     in scene order (tile after tile of the crop)
  shuffled:  in a seeded random order
  outliers:  in scene order with 1 % of them moved out to 50 x the extent (the single-level grid's weakest case: the moved
             points share the border cells and each of them searches most of the grid)
Per case, in one process:
  kernel:    gs_knn_search alone on the built grid (HIP events), rows and the init_scales epilogue
  calls:     knn(x, K) with x on the host as the trainers call it (copy in, box read-back, grid build, search, copy out),
             knn(x, K) with x on the device, init_scales(x) on the device -- alternating, round by round, with the call they
             replace: the body of the reference's examples/utils.py:knn (x.cpu().numpy(), sklearn NearestNeighbors fit +
             kneighbors, torch.from_numpy(...).to(x)) on the same host tensor, or "not installed" where sklearn does not import
  agreement: the largest relative difference between the two results
Every case runs in a child process of its own under a time limit (--case-seconds); the parent does not open the GPU and stops
at the first case that fails.  min..max over --rounds rounds; a speed-up is stated only where the difference exceeds the sum
of both spreads.
usage: python tools/bench_knn.py [--rounds 3] [--cases scene shuffled outliers] [--ks 4 16] [--grid 3] [--out profiles/r22_knn.txt]"""
import argparse
import gc
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("scene", "shuffled", "outliers")


def say(s=""):
    print(s, flush=True)


def span(ts, unit="ms", scale=1.0):
    return f"{min(ts) * scale:.3f} .. {max(ts) * scale:.3f} {unit}"


def points_of(case, grid):
    import torch

    from gscodec_studio_amd._helper import load_test_data

    x = load_test_data(device="cpu", scene_grid=grid)[0].contiguous()
    g = torch.Generator().manual_seed(7)
    if case == "shuffled":
        x = x[torch.randperm(len(x), generator=g)].contiguous()
    elif case == "outliers":
        lo, hi = x.min(dim=0).values, x.max(dim=0).values
        far = torch.randperm(len(x), generator=g)[: len(x) // 100]
        direction = torch.nn.functional.normalize(torch.randn((len(far), 3), generator=g), dim=-1)
        x = x.clone()
        x[far] = (lo + hi) / 2 + direction * 50.0 * (hi - lo).max() * (0.5 + 0.5 * torch.rand((len(far), 1), generator=g))
    return x


def sklearn_knn():
    """The body of the reference's knn, or None where sklearn is not installed."""
    try:
        from sklearn.neighbors import NearestNeighbors
    except ImportError:
        return None
    import torch

    def knn(x, K=4):
        x_np = x.cpu().numpy()
        model = NearestNeighbors(n_neighbors=K, metric="euclidean").fit(x_np)
        distances, _ = model.kneighbors(x_np)
        return torch.from_numpy(distances).to(x)

    return knn


def run_case(case, a):
    import torch

    from gscodec_studio_amd import knn as M

    assert torch.cuda.is_available(), "bench_knn measures on the GPU"
    gc.collect()
    gc.freeze()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    x = points_of(case, a.grid)
    xd = x.cuda()
    ref_knn = sklearn_knn()
    grid = M._Grid("bench", xd)
    torch.cuda.synchronize()
    occupancy = torch.diff(grid.cell_starts).float()
    say(f"case {case}: N = {len(x)}, grid {grid.R[0]} x {grid.R[1]} x {grid.R[2]} = {grid.ncells} cells of side {grid.h:.5f}, "
        f"{int((occupancy > 0).sum())} occupied, longest cell {int(occupancy.max())} points")
    for K in a.ks:
        grid.search(K)  # warm-up: code object load
        grid.search(K, rows=False, init_scale=1.0)
        t_rows = [event_ms(lambda: grid.search(K)) for _ in range(a.rounds)]
        t_scales = [event_ms(lambda: grid.search(K, rows=False, init_scale=1.0)) for _ in range(a.rounds)]
        say(f"  K = {K:2d}  gs_knn_search, rows            {span(t_rows)}")
        say(f"          gs_knn_search, log scales only  {span(t_scales)}")
        M.knn(x, K)  # warm-up of the whole path: sort, allocator
        t_host, t_dev, t_init, t_ref = [], [], [], []
        out = want = None
        for _ in range(a.rounds):
            t, out = wall(lambda: M.knn(x, K))
            t_host.append(t)
            t_dev.append(wall(lambda: M.knn(xd, K))[0])
            t_init.append(wall(lambda: M.init_scales(xd, 1.0, K))[0])
            if ref_knn is not None:
                t, want = wall(lambda: ref_knn(x, K))
                t_ref.append(t)
        say(f"          knn(x, {K}), x on the host         {span(t_host, 'ms', 1e3)}")
        say(f"          knn(x, {K}), x on the device       {span(t_dev, 'ms', 1e3)}")
        say(f"          init_scales(x, K={K}), device      {span(t_init, 'ms', 1e3)}")
        if ref_knn is None:
            say("          the reference's knn (sklearn):  not installed")
            continue
        say(f"          the reference's knn (sklearn)   {span(t_ref, 's')}")
        gap = min(t_ref) - max(t_host)
        spreads = (max(t_ref) - min(t_ref)) + (max(t_host) - min(t_host))
        say(f"          slowest host-tensor call against the fastest sklearn call: {gap:.3f} s apart, spreads sum to {spreads:.3f} s: "
            + (f"speed-up {min(t_ref) / max(t_host):.0f} x .. {max(t_ref) / min(t_host):.0f} x" if gap > spreads else "no claim"))
        rel = ((out.double() - want.double()).abs() / want.double().clamp_min(1e-300)).max()
        say(f"          largest relative difference between the two results: {float(rel):.3e} (the tests' bar: 2^-21 = 4.77e-07)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=CASES)
    ap.add_argument("--ks", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--grid", type=int, default=3, help="tiles per side of the garden crop (3: config 2's 1,006,065 means)")
    ap.add_argument("--case-seconds", type=float, default=300.0, help="time limit of each case's process")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        run_case(a.child, a)
        return 0
    lines = []
    for case in a.cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--rounds", str(a.rounds), "--grid", str(a.grid), "--ks",
               *map(str, a.ks)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.case_seconds)
        except subprocess.TimeoutExpired as e:
            say((e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""))
            say(f"case {case}: ended at its time limit of {a.case_seconds:.0f} s; nothing after it was started")
            return 124
        say(r.stdout.rstrip("\n"))
        lines.append(r.stdout.rstrip("\n"))
        if r.returncode != 0:
            say(r.stderr[-4000:])
            say(f"case {case}: exit status {r.returncode}; nothing after it was started")
            return r.returncode
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
