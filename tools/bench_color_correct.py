"""color_correct at [1, 1080, 1920, 3] (the evaluation image of the trainers), five iterations.  Alternates, in one process:
  (a) the plain-torch composition of the same statements on the GPU: per iteration the [P, 10] feature matrix, and per channel a
      torch.where copy of it and one torch.linalg.lstsq; if lstsq refuses these systems on this build the refusal is printed and
      the same composition is timed on the CPU instead (a few repetitions: it takes seconds)
  (c) gscodec_studio_amd.color_correct, at the default workgroup count and at others
then the kernels alone (accumulate, apply + accumulate, apply, solve), the launch count of a call, and max|(a) - (c)|.
usage: python tools/bench_color_correct.py [--steps 20] [--rounds 5]"""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gscodec_studio_amd import _backend as B  # noqa: E402
from gscodec_studio_amd.color_correct import DEFAULT_WORKGROUPS, color_correct, num_columns  # noqa: E402


def torch_color_correct(img, ref, num_iters=5, eps=0.5 / 255, check=True):
    """The statements of lib_bilagrid.color_correct in plain torch (lstsq on the row-masked matrix; ``check``: its host wait)."""
    n = img.shape[-1]
    x, b = img.reshape(-1, n), ref.reshape(-1, n)
    inside = lambda z: (z >= eps) & (z <= 1 - eps)  # noqa: E731
    keep0 = inside(x)
    for _ in range(num_iters):
        a = torch.cat([x[:, c:c + 1] * x[:, c:] for c in range(n)] + [x, torch.ones_like(x[:, :1])], dim=-1)
        cols = []
        for c in range(n):
            keep = keep0[:, c] & inside(x[:, c]) & inside(b[:, c])
            w = torch.linalg.lstsq(torch.where(keep[:, None], a, torch.zeros_like(a)), torch.where(keep, b[:, c], torch.zeros_like(b[:, c])),
                                   rcond=-1)[0]
            if check:
                assert torch.all(torch.isfinite(w))
            cols.append(w)
        x = torch.clip(a @ torch.stack(cols, dim=-1), 0, 1)
    return x.reshape(img.shape)


def timed(fn, steps, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return (time.perf_counter() - t0) / steps * 1e3


def report(title, fns, steps, rounds):
    sync = torch.cuda.synchronize
    for fn in fns.values():
        timed(fn, 3, sync)
    times = {t: [] for t in fns}
    for _ in range(rounds):
        for tag, fn in fns.items():
            times[tag].append(timed(fn, steps, sync))
    print(f"{title}, median of {rounds} rounds x {steps} (host clock around device-synchronised windows):", flush=True)
    for tag, ts in times.items():
        print(f"  {tag:58s} {statistics.median(ts):9.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f})", flush=True)
    return {t: statistics.median(ts) for t, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    gc.collect()
    gc.freeze()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    H, W, n, iters = 1080, 1920, 3, 5
    # a render and its ground truth: colours over all of [0, 1] (some rows clipped), a colour cast and noise
    img = torch.rand((1, H, W, n), device=dev, generator=g)
    mix = torch.eye(n, device=dev) * 0.9 + 0.05 * (2 * torch.rand((n, n), device=dev, generator=g) - 1)
    ref = (img @ mix + 0.08 * img * img + 0.02 * torch.randn(img.shape, device=dev, generator=g)).clip(0, 1)
    print(f"color_correct [1, {H}, {W}, {n}], num_iters {iters}, default workgroups {DEFAULT_WORKGROUPS}", flush=True)

    fns, torch_out = {}, None
    try:
        torch_out = torch_color_correct(img, ref, iters)
        torch.cuda.synchronize()
        fns["(a) torch composition on the GPU (lstsq, with its assert)"] = lambda: torch_color_correct(img, ref, iters)
        fns["(a') the same without the assert (no host wait)"] = lambda: torch_color_correct(img, ref, iters, check=False)
    except Exception as e:  # noqa: BLE001
        print(f"(a) torch.linalg.lstsq REFUSES these systems on the GPU of this build: {type(e).__name__}: {str(e).splitlines()[0]}", flush=True)
        ci, cr = img.cpu(), ref.cpu()
        torch_out = torch_color_correct(ci, cr, iters)
        ms = timed(lambda: torch_color_correct(ci, cr, iters), 2, lambda: None)
        print(f"  (a) torch composition on the CPU ({torch.get_num_threads()} threads), 2 repetitions: {ms:9.1f} ms", flush=True)
        torch_out = torch_out.to(dev)
    fns["(c) color_correct, default workgroups"] = lambda: color_correct(img, ref, iters)
    for wg in (64, 128, 512, 1024):
        fns[f"(c) color_correct, workgroups={wg}"] = lambda wg=wg: color_correct(img, ref, iters, workgroups=wg)
    report("whole call", fns, a.steps, a.rounds)
    ours = color_correct(img, ref, iters)
    try:  # the composition in float64 (where a value lies within float32 rounding of a threshold its mask can differ)
        f64 = torch_color_correct(img.double(), ref.double(), iters)
    except Exception:  # noqa: BLE001
        f64 = torch_color_correct(img.cpu().double(), ref.cpu().double(), iters).to(dev)
    print(f"  max|(a) - float64| = {float((torch_out - f64).abs().max()):.3e}   max|(c) - float64| = {float((ours - f64).abs().max()):.3e}   "
          f"max|(a) - (c)| = {float((ours - torch_out).abs().max()):.3e}", flush=True)
    print(f"  launches of one call: {2 * iters + 1} ({iters + 1} passes, {iters} solves)", flush=True)

    # the kernels alone
    P, blocks, K = H * W, DEFAULT_WORKGROUPS, num_columns(n)
    rec = int(B.query("gs_color_correct_record_doubles", n))
    partials = torch.empty((1, n, blocks, rec), dtype=torch.float64, device=dev)
    warp = torch.zeros((1, K, n), dtype=torch.float64, device=dev)
    for c in range(n):
        warp[0, n * (n + 1) // 2 + c, c] = 1.0  # the identity warp
    out, solved = torch.empty_like(img), torch.empty_like(warp)
    lo, hi, st = 0.5 / 255, 1 - 0.5 / 255, torch.cuda.current_stream(dev).cuda_stream
    call = lambda w, o, p: B.call("gs_color_correct_pass", img.data_ptr(), n, img.data_ptr(), n, ref.data_ptr(), 1, P, n, lo, hi, w, o, p, blocks, st)  # noqa: E731
    call(None, None, partials.data_ptr())
    med = report("kernels", {
        "pass: accumulate": lambda: call(None, None, partials.data_ptr()),
        "pass: apply + accumulate": lambda: call(warp.data_ptr(), out.data_ptr(), partials.data_ptr()),
        "pass: apply": lambda: call(warp.data_ptr(), out.data_ptr(), None),
        "solve (3 systems of 10 x 10, 256 records each)": lambda: B.call("gs_color_correct_solve", partials.data_ptr(), 1, n, blocks, solved.data_ptr(), st),
    }, a.steps * 5, a.rounds)
    rd, wr = P * n * 4 * 3, P * n * 4
    t = med["pass: apply + accumulate"]
    print(f"  apply + accumulate moves {(rd * n + wr) / 1e6:.0f} MB through the load / store units ({n} workgroup rows read x, x0 and ref; "
          f"{(rd + wr) / 1e6:.0f} MB unique): {(rd + wr) / t / 1e6:.0f} GB/s unique at {t:.4f} ms", flush=True)


if __name__ == "__main__":
    main()
