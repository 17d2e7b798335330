"""The K-means codebook of the shN codec at BASELINE config 2's size after the square crop (1003^2 = 1,006,009 rows of the 45
higher-band coefficients of the bench scene) at 16,384, 32,768 and 65,536 clusters:
  ubench:   the issue rate of v_sad_u32 (tools/ubench.hip, run as a child process before this one opens the GPU)
  kernels:  gs_kmeans_assign and gs_kmeans_update of one iteration (HIP events), and the assign's achieved lane-operations per
            second (n k w sums of absolute differences) against 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 3.9e13
  calls:    kmeans_encode(method="torch") and kmeans_encode(method="fixed") alternating in this process, median and min..max of
            both.  One torch iteration is timed first; when ten of them would take more than a minute, the calls compared are
            calls of ONE iteration each (iters=1: start, one assign, one update, the 8-bit tail), and the output says so
  distortion: the mean float L1 distance from each row to its decoded centroid, both methods from the same start after the same
            number of iterations; where that number is one, also a whole ten-iteration call of the fixed method and its distortion
  few rows: the assign over the first 65,536 rows (the masked codec with few non-zero rows) with one centroid slice and with the
            library's choice of slices
The torch path asks torch.cdist for chunks of 2^24 // k rows, and cdist launches one 256-thread workgroup per (row, centroid)
pair: at a power-of-two k that is 2^24 workgroups = 2^32 threads, one more than a launch may have, and the call ends in "HIP
error: invalid configuration argument" (seen at k = 16,384).  The torch path is therefore run with k - 1 clusters wherever
k is such a size, and the output says so; the fixed path runs the k asked for.
A torch measurement that would start after --max-seconds is skipped and reported as such.
usage: python tools/bench_kmeans.py [--reps 3] [--clusters 16384 32768 65536] [--rows 0] [--out profiles/r21_kmeans.txt]"""
import argparse
import gc
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gscodec_studio_amd._helper import sh_workload  # noqa: E402
from gscodec_studio_amd.compression import kmeans as K, kmeans_decode, kmeans_encode  # noqa: E402

PEAK_LANE_OPS = 256 * 4 * 16 * 2.4e9
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


def wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stats(ts, unit="ms"):
    return f"{statistics.median(ts):10.3f} {unit}  (min {min(ts):.3f}, max {max(ts):.3f}, n = {len(ts)})"


def distortion(shn, result):
    cq, labels, meta = result
    back = kmeans_decode(cq, labels, meta)
    return float((back.reshape(shn.shape[0], -1) - shn.reshape(shn.shape[0], -1)).abs().sum(dim=1).mean())


def torch_clusters(k, n):
    """k, or k - 1 where the torch path's cdist launch would be refused (module docstring)."""
    rows = min(max(1, (1 << 24) // k), n)
    return k - 1 if rows * k * 256 >= 1 << 32 else k


def run_ubench(path):
    if not os.path.exists(path):
        say(f"ubench: not measured ({path} is not built: hipcc --offload-arch=gfx950 -O3 -o ubench tools/ubench.hip)")
        return
    out = subprocess.run([path], capture_output=True, text=True, timeout=300).stdout
    say("ubench (ns and cycles per wave-instruction per SIMD; 4 cycles = one 64-lane instruction per 16 lanes and clock):")
    for line in out.splitlines():
        if "v_sad_u32" in line or "v_fma_f32 x8" in line or "v_add_f32 x8" in line:
            say("  " + line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--clusters", type=int, nargs="+", default=[16384, 32768, 65536])
    ap.add_argument("--rows", type=int, default=0, help="use the first ROWS rows (default: the largest square, 1,006,009)")
    ap.add_argument("--max-seconds", type=float, default=600.0, help="start no torch measurement after this many seconds")
    ap.add_argument("--ubench", default=os.path.join(ROOT, "ubench"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run_ubench(a.ubench)
    assert torch.cuda.is_available(), "bench_kmeans measures on the GPU"
    gc.collect()
    gc.freeze()
    t_start = time.perf_counter()
    dev = torch.device("cuda")
    sh = sh_workload(scene_grid=3, device="cpu")["sh"]
    n = a.rows or int(len(sh) ** 0.5) ** 2
    shn = sh[:n, 1:].contiguous().to(dev)
    x = shn.reshape(n, -1)
    w = x.shape[1]
    say(f"n = {n} rows, w = {w} channels")
    lo, hi = K._range_of("bench", x)
    q_t = K._quantize(x, lo, hi)

    # ---- few rows: what the centroid slices buy
    m, km = min(n, 65536), min(a.clusters)
    sub = q_t[:, :m].contiguous()
    for slices in (1, K._slices(None, m, w, km)):
        steps = K._Steps(sub, sub[:, :km].t(), slices)
        steps.assign()
        say(f"few rows: gs_kmeans_assign, {m} rows, {km} clusters, {slices:3d} slice(s) {stats([event_ms(steps.assign) for _ in range(a.reps)])}")
        del steps

    for k in a.clusters:
        say(f"k = {k} clusters")
        # ---- the kernels of one iteration
        g = torch.Generator(device=dev).manual_seed(0)
        start = torch.randperm(n, device=dev, generator=g)[:k]
        steps = K._Steps(q_t, q_t[:, start].t(), K._slices(None, n, w, k))
        steps.assign()
        steps.update()
        t_assign = [event_ms(steps.assign) for _ in range(a.reps)]
        t_update = [event_ms(steps.update) for _ in range(a.reps)]
        rate = n * k * w / (statistics.median(t_assign) * 1e-3)
        say(f"  gs_kmeans_assign ({steps.k_slices} slice(s)) {stats(t_assign)}")
        say(f"    {n * k * w:.3e} lane-operations: {rate:.3e} per second = {100 * rate / PEAK_LANE_OPS:.1f} % of {PEAK_LANE_OPS:.2e}")
        say(f"  gs_kmeans_update                {stats(t_update)}")
        del steps

        # ---- whole calls of both methods, alternating
        wall_s(lambda: kmeans_encode(shn, n_clusters=k, iters=1, method="fixed"))  # warm-up
        if time.perf_counter() - t_start > a.max_seconds:
            say("  torch path: skipped (the time budget of this run was spent)")
            continue
        kt = torch_clusters(k, n)
        if kt != k:
            say(f"  torch path: run with {kt} clusters (at {k} its cdist launch of 2^32 threads is refused)")
        probe, res_torch = wall_s(lambda: kmeans_encode(shn, n_clusters=kt, iters=1, method="torch"))
        iters = 10 if probe * 10 <= 60.0 else 1
        say(f"  one torch iteration (a call with iters=1): {probe:.2f} s; the calls compared below run iters={iters}"
            + ("" if iters == 10 else " (ten would take more than a minute)"))
        t_torch, t_fixed = ([probe], []) if iters == 1 else ([], [])
        res_fixed = None
        for rep in range(a.reps):
            if iters == 10 or rep > 0:
                if time.perf_counter() - t_start > a.max_seconds:
                    say(f"  torch path: {a.reps - rep} repetition(s) skipped (the time budget of this run was spent)")
                    break
                t, res_torch = wall_s(lambda: kmeans_encode(shn, n_clusters=kt, iters=iters, method="torch"))
                t_torch.append(t)
            t, res_fixed = wall_s(lambda: kmeans_encode(shn, n_clusters=k, iters=iters, method="fixed"))
            t_fixed.append(t)
        if res_fixed is None:
            t, res_fixed = wall_s(lambda: kmeans_encode(shn, n_clusters=k, iters=iters, method="fixed"))
            t_fixed.append(t)
        say(f"  kmeans_encode(method=\"torch\", iters={iters}, n_clusters={kt}) {stats(t_torch, 's')}")
        say(f"  kmeans_encode(method=\"fixed\", iters={iters}) {stats(t_fixed, 's')}")
        gap = statistics.median(t_torch) - statistics.median(t_fixed)
        spreads = (max(t_torch) - min(t_torch)) + (max(t_fixed) - min(t_fixed))
        say(f"    difference of medians {gap:.3f} s, sum of the two spreads {spreads:.3f} s: "
            + (f"ratio of medians torch / fixed {statistics.median(t_torch) / statistics.median(t_fixed):.1f}" if abs(gap) > spreads
               and len(t_torch) > 1 else "no claim (the difference does not exceed the spreads, or one sample)"))
        say(f"  mean L1 distance row -> decoded centroid after {iters} iteration(s): torch {distortion(shn, res_torch):.6f}, "
            f"fixed {distortion(shn, res_fixed):.6f}")
        if iters == 1:
            t_ten = []
            for _ in range(a.reps):
                t, res_fixed = wall_s(lambda: kmeans_encode(shn, n_clusters=k, iters=10, method="fixed"))
                t_ten.append(t)
            say(f"  kmeans_encode(method=\"fixed\", iters=10) {stats(t_ten, 's')}; mean L1 distance row -> decoded centroid "
                f"{distortion(shn, res_fixed):.6f}")
        del res_torch, res_fixed
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(_LINES) + "\n")


if __name__ == "__main__":
    main()
