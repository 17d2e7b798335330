"""The optimizer step after the render backward, at BASELINE config 2 (1,006,065 gaussians, SH 3: 59.4 M floats in the trainer's six
tensors means / quats / scales / opacities / sh0 / shN, gradients from one rasterization() backward).  Alternates, in one process:
  (a) six torch.optim.Adam (default: foreach)     (b) six torch.optim.Adam(fused=True)     (c) six optimizers.Adam, one by one
  (d) optimizers.step_all over six optimizers.Adam (one launch)
  (e) optimizers.step_all over six SelectiveAdam with the scene's visibility mask
then a whole training iteration (render forward + backward + optimizer) with (a) against (d).
usage: python tools/bench_optimizer.py [--steps 50] [--rounds 5] [--iters 30]"""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gscodec_studio_amd import rasterization  # noqa: E402
from gscodec_studio_amd._helper import sh_workload  # noqa: E402
from gscodec_studio_amd.optimizers import Adam, SelectiveAdam, step_all, visibility_mask  # noqa: E402

NAMES = ("means", "quats", "scales", "opacities", "sh0", "shN")
LRS = {"means": 1.6e-4, "quats": 1e-3, "scales": 5e-3, "opacities": 5e-2, "sh0": 2.5e-3, "shN": 2.5e-3 / 20}


def make_params(w):
    sh = w["sh"]
    init = {"means": w["means"], "quats": w["quats"], "scales": torch.log(w["scales"]),
            "opacities": torch.logit(w["opacities"].clamp(1e-4, 1 - 1e-4)), "sh0": sh[:, :1], "shN": sh[:, 1:]}
    return {k: torch.nn.Parameter(init[k].contiguous().clone()) for k in NAMES}


def render(ps, w):
    return rasterization(ps["means"], ps["quats"], torch.exp(ps["scales"]), torch.sigmoid(ps["opacities"]), (ps["sh0"], ps["shN"]),
                         w["viewmats"], w["Ks"], w["width"], w["height"], sh_degree=3)


def make_opts(ps, cls, **kw):
    return {k: cls([{"params": [p], "lr": LRS[k], "name": k}], eps=1e-15, betas=(0.9, 0.999), **kw) for k, p in ps.items()}


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    gc.collect()
    gc.freeze()
    w = sh_workload(scene_grid=3, device="cuda")
    base = make_params(w)
    rc, ra, meta = render(base, w)
    rc.sum().backward()
    grads = {k: p.grad.detach().clone() for k, p in base.items()}
    vis = visibility_mask(meta, w["N"])
    torch.cuda.synchronize()
    N = w["N"]
    floats = sum(p.numel() for p in base.values())
    row_floats = floats // N
    n_vis = int(vis.sum())
    zero_rows = int((torch.stack([grads[k].reshape(N, -1).abs().amax(1) for k in NAMES]).amax(0) == 0).sum())
    print(f"config 2: N = {N:,} gaussians, {floats:,} floats in {len(NAMES)} tensors ({row_floats} per gaussian); "
          f"visible (radii > 0): {n_vis:,} = {n_vis / N * 100:.1f} %; rows with an all-zero gradient: {zero_rows / N * 100:.1f} %", flush=True)

    variants = {}

    def variant(tag, cls, use_step_all=False, selective=False, **kw):
        ps = {k: torch.nn.Parameter(v.detach().clone()) for k, v in base.items()}
        for k, p in ps.items():
            p.grad = grads[k].clone()
        opts = make_opts(ps, cls, **kw)
        if selective:
            fn = lambda: step_all(opts, visibility=vis, zero_grad=False)  # noqa: E731
        elif use_step_all:
            fn = lambda: step_all(opts, zero_grad=False)  # noqa: E731
        else:
            def fn():
                for o in opts.values():
                    o.step()
        fn()  # state allocation, code objects
        torch.cuda.synchronize()
        variants[tag] = (fn, ps, opts)

    variant("(a) 6x torch.optim.Adam (foreach)", torch.optim.Adam)
    try:
        variant("(b) 6x torch.optim.Adam(fused=True)", torch.optim.Adam, fused=True)
    except Exception as e:  # noqa: BLE001
        print(f"(b) torch.optim.Adam(fused=True) is not available in this torch build: {type(e).__name__}: {e}; skipped", flush=True)
    variant("(c) 6x optimizers.Adam, one by one", Adam)
    variant("(d) step_all, dense", Adam, use_step_all=True)
    variant("(e) step_all, 6x SelectiveAdam", SelectiveAdam, selective=True)

    for fn, _, _ in variants.values():
        timed(fn, 5)
    times = {t: [] for t in variants}
    for _ in range(a.rounds):
        for tag, (fn, _, _) in variants.items():
            times[tag].append(timed(fn, a.steps))
    dense_bytes = 28 * floats
    sel_bytes = N + 28 * n_vis * row_floats
    print(f"optimizer phase, median of {a.rounds} rounds x {a.steps} steps (host clock around device-synchronised windows):", flush=True)
    for tag, ts in times.items():
        med = statistics.median(ts)
        extra = ""
        if tag.startswith("(d)"):
            extra = f"  {dense_bytes / 1e9:.3f} GB algorithmic (28 B x floats) -> {dense_bytes / med / 1e9:.2f} TB/s"
        elif tag.startswith("(e)"):
            extra = f"  {sel_bytes / 1e9:.3f} GB algorithmic (N + 28 B x visible-row floats) -> {sel_bytes / med / 1e9:.2f} TB/s"
        print(f"  {tag:40s} {med:8.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f}){extra}", flush=True)

    # a whole training iteration: render forward + backward + optimizer, (a) against (d)
    def iteration(ps, opts, use_step_all):
        def fn():
            rc, _, _ = render(ps, w)
            rc.sum().backward()
            if use_step_all:
                step_all(opts)
            else:
                for o in opts.values():
                    o.step()
                    o.zero_grad(set_to_none=True)
        return fn

    it = {"(a) render fwd + bwd + 6x torch.optim.Adam": iteration(*variants["(a) 6x torch.optim.Adam (foreach)"][1:], False),
          "(d) render fwd + bwd + step_all": iteration(*variants["(d) step_all, dense"][1:], True)}
    for fn in it.values():
        timed(fn, 3)
    its = {t: [] for t in it}
    for _ in range(a.rounds):
        for tag, fn in it.items():
            its[tag].append(timed(fn, a.iters))
    print(f"training iteration, median of {a.rounds} rounds x {a.iters} iterations:", flush=True)
    for tag, ts in its.items():
        print(f"  {tag:44s} {statistics.median(ts):8.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f})", flush=True)


if __name__ == "__main__":
    main()
