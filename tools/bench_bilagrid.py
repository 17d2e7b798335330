"""The bilateral-grid colour correction, forward + backward, at [1, 1080, 1920, 3] with the default (16, 16, 8) grid and N = 200 grids.
Alternates, in one process:
  slice:  (a) the plain-torch composition of lib_bilagrid.slice (meshgrid, cat, F.grid_sample over 12 channels, permute, matmul, add)
          (b) bilagrid.slice with the explicit [1, H, W, 2] meshgrid     (c) bilagrid.slice_image
  TV:     (a) the plain-torch total_variation_loss (index_select copies)  (c) bilagrid.total_variation_loss
then the slice forward and backward alone against their byte floors, and a whole training iteration at BASELINE config 2
(render + slice + photometric_loss + TV + step_all) with (a) against (c) and without any grid.
usage: python tools/bench_bilagrid.py [--steps 30] [--rounds 5] [--iters 20]"""
import argparse
import gc
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gscodec_studio_amd import rasterization  # noqa: E402
from gscodec_studio_amd._helper import sh_workload  # noqa: E402
from gscodec_studio_amd.bilagrid import BilateralGrid, slice as bslice, slice_image, total_variation_loss  # noqa: E402
from gscodec_studio_amd.losses import photometric_loss  # noqa: E402
from gscodec_studio_amd.optimizers import step_all  # noqa: E402

NAMES = ("means", "quats", "scales", "opacities", "sh0", "shN")
LRS = {"means": 1.6e-4, "quats": 1e-3, "scales": 5e-3, "opacities": 5e-2, "sh0": 2.5e-3, "shN": 2.5e-3 / 20}
NUM = 200


def torch_slice(grids, colors, image_ids):
    """simple_trainer.py:927-934 + lib_bilagrid.slice / BilateralGrid.forward, as a ROCm user runs them today (the len(unique)
    host synchronisation of the reference left out: a batch of one image has one index)."""
    C, H, W, _ = colors.shape
    gy, gx = torch.meshgrid((torch.arange(H, device=colors.device) + 0.5) / H, (torch.arange(W, device=colors.device) + 0.5) / W,
                            indexing="ij")
    xy = torch.stack([gx, gy], dim=-1).unsqueeze(0).expand(C, H, W, 2)
    g = grids[image_ids]
    z = (colors @ torch.tensor([[0.299, 0.587, 0.114]], device=colors.device).T) * 2.0 - 1.0
    xyz = torch.cat([(xy - 0.5) * 2, z], dim=-1).unsqueeze(1)
    m = F.grid_sample(g, xyz, mode="bilinear", align_corners=True, padding_mode="border").permute(0, 2, 3, 4, 1)
    m = m.reshape(C, H, W, 3, 4)
    return torch.matmul(m[..., :3], colors.unsqueeze(-1)).squeeze(-1) + m[..., 3]


def torch_tv(x):
    tv = 0
    for i in range(2, x.dim()):
        n = x.shape[i]
        x1 = x.index_select(i, torch.arange(1, n, device=x.device))
        x2 = x.index_select(i, torch.arange(0, n - 1, device=x.device))
        tv = tv + torch.pow(x1 - x2, 2).sum() / max(x1[0].numel(), 1)
    return tv / x.shape[0]


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def report(title, fns, steps, rounds):
    for fn in fns.values():
        timed(fn, 3)
    times = {t: [] for t in fns}
    for _ in range(rounds):
        for tag, fn in fns.items():
            times[tag].append(timed(fn, steps))
    print(f"{title}, median of {rounds} rounds x {steps} (host clock around device-synchronised windows):", flush=True)
    med = {t: statistics.median(ts) for t, ts in times.items()}
    for tag, ts in times.items():
        print(f"  {tag:58s} {med[tag]:8.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f}, spread {max(ts) - min(ts):.4f})", flush=True)
    return med, {t: max(ts) - min(ts) for t, ts in times.items()}


def verdict(name, med, spread, ka, kc):
    gap, both = med[ka] - med[kc], spread[ka] + spread[kc]
    word = "beyond both spreads" if abs(gap) > both else "INSIDE the spreads: no claim"
    print(f"  {name}: (a) - (c) = {gap:+.4f} ms, (a) / (c) = {med[ka] / med[kc]:.2f}x, sum of the two spreads {both:.4f} ms -> {word}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-iteration", action="store_true")
    a = ap.parse_args()
    gc.collect()
    gc.freeze()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    H, W = 1080, 1920
    bil = BilateralGrid(NUM).to(dev)
    with torch.no_grad():
        bil.grids.add_(0.05 * torch.randn(bil.grids.shape, device=dev, generator=g))
    colors = torch.rand((1, H, W, 3), device=dev, generator=g).requires_grad_(True)
    cot = torch.randn((1, H, W, 3), device=dev, generator=g)
    ids = torch.tensor([7], device=dev)
    gy, gx = torch.meshgrid((torch.arange(H, device=dev) + 0.5) / H, (torch.arange(W, device=dev) + 0.5) / W, indexing="ij")
    grid_xy = torch.stack([gx, gy], dim=-1).unsqueeze(0)

    def step(fn):
        def run():
            (fn() * cot).sum().backward()
            colors.grad = None
            bil.grids.grad = None
        return run

    ka, kb, kc = "(a) torch composition (meshgrid + F.grid_sample + matmul)", "(b) bilagrid.slice, explicit [1, H, W, 2] xy", "(c) bilagrid.slice_image"
    med, spread = report(f"slice forward + backward at [1, {H}, {W}, 3], grid (16, 16, 8), N = {NUM} (includes the (out * cot).sum() of all three)",
                         {ka: step(lambda: torch_slice(bil.grids, colors, ids)), kb: step(lambda: bslice(bil, grid_xy, colors, ids, affine_mats=False)["rgb"]),
                          kc: step(lambda: slice_image(bil, colors, ids))}, a.steps, a.rounds)
    verdict("slice", med, spread, ka, kc)

    # forward and backward alone (no autograd graph walk): the floors
    from gscodec_studio_amd import _wrapper as Wr
    gr, c4 = bil.grids.detach(), colors.detach()
    n_px = H * W
    fwd = lambda: Wr.bilagrid_slice_fwd(gr, (1, H, W), None, None, c4, c4.stride(), ids, 1, True, False)  # noqa: E731
    bwd = lambda: Wr.bilagrid_slice_bwd(gr, (1, H, W), None, None, c4, c4.stride(), ids, 1, cot, None)  # noqa: E731
    bwd_rgb = lambda: Wr.bilagrid_slice_bwd(gr, (1, H, W), None, None, c4, c4.stride(), ids, 1, cot, None, want_grids=False)  # noqa: E731
    med2, _ = report("slice kernels alone", {"forward (12 B read + 12 B written per pixel)": fwd,
                                             "backward (24 B read + 12 B written per pixel; clears and fills v_grids)": bwd,
                                             "backward without the grid gradient": bwd_rgb}, a.steps * 4, a.rounds)
    tf, tb, tr = list(med2.values())
    print(f"  forward: {24 * n_px / 1e6:.1f} MB -> {24 * n_px / tf / 1e9:.2f} TB/s achieved", flush=True)
    tiles = ((W + 63) // 64) * ((H + 31) // 32)
    print(f"  backward: {36 * n_px / 1e6:.1f} MB of image traffic + {gr.numel() * 4 / 1e6:.1f} MB cleared for N = {NUM} grids; {tiles} workgroups, each "
          f"adding at most its box of 2 x 2 .. 3 x 3 xy corners x 8 x 12 floats once: <= {tiles * 864 * 4 / 1e6:.1f} MB of float atomics "
          f"(the per-pixel form: {96 * 4 * n_px / 1e6:.0f} MB); the grid gradient costs {tb - tr:+.4f} ms of the backward's {tb:.4f}", flush=True)

    x = bil.grids

    def tv_step(fn):
        def run():
            (10 * fn(x)).backward()
            x.grad = None
        return run

    ta, tc = "(a) torch total_variation_loss (index_select)", "(c) bilagrid.total_variation_loss"
    med3, spread3 = report(f"TV forward + backward at {tuple(x.shape)}", {ta: tv_step(torch_tv), tc: tv_step(total_variation_loss)}, a.steps, a.rounds)
    verdict("TV", med3, spread3, ta, tc)
    print(f"  (c): {x.numel() * 4 * 3 / 1e6:.1f} MB (read, read, write) -> {x.numel() * 12 / med3[tc] / 1e9:.2f} TB/s over the whole call", flush=True)
    if a.skip_iteration:
        return

    w = sh_workload(scene_grid=3, device=dev)
    sh = w["sh"]
    init = {"means": w["means"], "quats": w["quats"], "scales": torch.log(w["scales"]),
            "opacities": torch.logit(w["opacities"].clamp(1e-4, 1 - 1e-4)), "sh0": sh[:, :1], "shN": sh[:, 1:]}
    pixels = torch.rand((1, w["height"], w["width"], 3), device=dev, generator=torch.Generator(device=dev).manual_seed(5))

    def iteration(mode):
        ps = {k: torch.nn.Parameter(init[k].contiguous().clone()) for k in NAMES}
        opts = {k: torch.optim.Adam([{"params": [p], "lr": LRS[k], "name": k}], eps=1e-15, betas=(0.9, 0.999)) for k, p in ps.items()}
        grid = BilateralGrid(NUM).to(dev)
        gopt = torch.optim.Adam(grid.parameters(), lr=2e-3, eps=1e-15)

        def fn():
            rc, _, _ = rasterization(ps["means"], ps["quats"], torch.exp(ps["scales"]), torch.sigmoid(ps["opacities"]),
                                     (ps["sh0"], ps["shN"]), w["viewmats"], w["Ks"], w["width"], w["height"], sh_degree=3)
            if mode == "torch":
                rc = torch_slice(grid.grids, rc, ids)
                loss = photometric_loss(rc, pixels)[0] + 10 * torch_tv(grid.grids)
            elif mode == "fused":
                rc = slice_image(grid, rc, ids)
                loss = photometric_loss(rc, pixels)[0] + 10 * total_variation_loss(grid.grids)
            else:
                loss = photometric_loss(rc, pixels)[0]
            loss.backward()
            step_all(opts)
            if mode != "none":
                gopt.step()
                gopt.zero_grad(set_to_none=True)
        return fn

    ia, ic, i0 = "(a) render + torch slice + photometric_loss + torch TV + step_all + grid Adam", "(c) render + slice_image + photometric_loss + fused TV + step_all + grid Adam", "(-) no bilateral grid"
    med4, spread4 = report(f"training iteration at config 2 with N = {NUM} grids", {ia: iteration("torch"), ic: iteration("fused"), i0: iteration("none")},
                           a.iters, a.rounds)
    verdict("iteration", med4, spread4, ia, ic)
    print(f"  the grid costs {med4[ic] - med4[i0]:+.4f} ms per iteration fused, {med4[ia] - med4[i0]:+.4f} ms in torch (torch.optim.Adam over "
          f"{NUM} grids included in both)", flush=True)


if __name__ == "__main__":
    main()
