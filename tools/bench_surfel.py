"""2D Gaussian splatting at BASELINE config 2's scene (1,006,065 splats, SH degree 3, one 1920x1080 camera):
``rasterization_2dgs(render_mode="RGB+ED", distloss=True)`` forward and forward + backward, interleaved in one process with
``rasterization(render_mode="RGB+ED")`` on the same splats (context, not a bar: a different primitive with 9 + 2 + 1 + D + 3
gradient values per splat instead of 2 + 3 + 1 + D), then the six kernels alone.
usage: python tools/bench_surfel.py [--steps 10] [--rounds 5] [--scene-grid 3]"""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gscodec_studio_amd import rasterization, rasterization_2dgs, surfel  # noqa: E402
from gscodec_studio_amd._helper import sh_workload  # noqa: E402


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def report(title, fns, steps, rounds):
    for fn in fns.values():
        timed(fn, 2)
    times = {t: [] for t in fns}
    for _ in range(rounds):
        for tag, fn in fns.items():
            times[tag].append(timed(fn, steps))
    print(f"{title}, median of {rounds} rounds x {steps} (host clock around device-synchronised windows):", flush=True)
    med = {t: statistics.median(ts) for t, ts in times.items()}
    for tag, ts in times.items():
        print(f"  {tag:64s} {med[tag]:9.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f}, spread {max(ts) - min(ts):.4f})", flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scene-grid", type=int, default=3)
    a = ap.parse_args()
    gc.collect()
    gc.freeze()
    dev = "cuda"
    w = sh_workload(scene_grid=a.scene_grid, device=dev)
    W, H = w["width"], w["height"]
    names = ("means", "quats", "scales", "opacities", "sh")
    P = {k: w[k].clone().requires_grad_(True) for k in names}
    gen = torch.Generator(device=dev).manual_seed(3)
    cot = {k: torch.randn(s, device=dev, generator=gen) for k, s in
           dict(rgbd=(1, H, W, 4), a=(1, H, W, 1), n=(1, H, W, 3), d=(1, H, W, 1)).items()}

    def surfel_call():
        return rasterization_2dgs(P["means"], P["quats"], P["scales"], P["opacities"], P["sh"], w["viewmats"], w["Ks"], W, H, sh_degree=3,
                                  render_mode="RGB+ED", distloss=True)

    def splat_call():
        return rasterization(P["means"], P["quats"], P["scales"], P["opacities"], P["sh"], w["viewmats"], w["Ks"], W, H, sh_degree=3,
                             render_mode="RGB+ED", packed=False)

    def clear():
        for p in P.values():
            p.grad = None

    def surfel_fwd():
        with torch.no_grad():
            surfel_call()

    def splat_fwd():
        with torch.no_grad():
            splat_call()

    def surfel_step():
        rc, ra, rn, nfd, rd, rm, _ = surfel_call()
        ((rc * cot["rgbd"]).sum() + (ra * cot["a"]).sum() + (rn * cot["n"]).sum() + (nfd * cot["n"]).sum() + (rd * cot["d"]).sum()).backward()
        clear()

    def splat_step():
        rc, ra, _ = splat_call()
        ((rc * cot["rgbd"]).sum() + (ra * cot["a"]).sum()).backward()
        clear()

    with torch.no_grad():
        meta = surfel_call()[6]
        meta3 = splat_call()[2]
    print(f"scene: {w['N']} splats, {W}x{H}; 2DGS: {int((meta['radii'] > 0).sum())} visible, {meta['flatten_ids'].numel()} intersections; "
          f"3DGS: {int((meta3['radii'] > 0).sum())} visible, {meta3['flatten_ids'].numel()} intersections", flush=True)
    k2f, k3f = "rasterization_2dgs RGB+ED distloss, forward", "rasterization RGB+ED (3DGS, context), forward"
    k2s, k3s = "rasterization_2dgs RGB+ED distloss, forward + backward", "rasterization RGB+ED (3DGS, context), forward + backward"
    med = report("whole calls, interleaved", {k2f: surfel_fwd, k3f: splat_fwd, k2s: surfel_step, k3s: splat_step}, a.steps, a.rounds)
    print(f"  2DGS backward (step - forward): {med[k2s] - med[k2f]:.4f} ms; 3DGS: {med[k3s] - med[k3f]:.4f} ms", flush=True)

    # the kernels alone: each operator's node run by itself on fixed inputs
    t = {k: w[k].clone().requires_grad_(True) for k in ("means", "quats", "scales")}
    radii, means2d, depths, rts, normals = surfel.fully_fused_projection_2dgs(t["means"], t["quats"], t["scales"], w["viewmats"], w["Ks"], W, H)
    proj_out = (means2d, depths, rts, normals)
    proj_cot = tuple(torch.randn(o.shape, device=dev, generator=gen) for o in proj_out)
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in dict(means2d=means2d, rts=rts, normals=normals).items()}
    colors = torch.cat([torch.rand((1, w["N"], 3), device=dev, generator=gen), depths.detach()[..., None]], -1).requires_grad_(True)
    opac = w["opacities"][None].clone().requires_grad_(True)
    densify = torch.zeros_like(means2d, requires_grad=True)
    ras_in = (leaf["means2d"], leaf["rts"], colors, opac, leaf["normals"], densify)
    ras = lambda: surfel.rasterize_to_pixels_2dgs(*ras_in, W, H, 16, meta["isect_offsets"], meta["flatten_ids"], distloss=True)  # noqa: E731
    ras_out = ras()
    ras_cot = (cot["rgbd"], cot["a"], cot["n"], cot["d"], cot["d"])
    depth = ras_out[0].detach()[..., -1:].clone().requires_grad_(True)
    c2w = torch.linalg.inv(w["viewmats"])
    nrm = surfel.depth_to_normal(depth, c2w, w["Ks"])

    def nograd(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    report("kernels alone (each with its allocations and, in the backward, its zero-fill)", {
        "gs_projection_2dgs_fwd": nograd(lambda: surfel.fully_fused_projection_2dgs(t["means"], t["quats"], t["scales"], w["viewmats"], w["Ks"], W, H)),
        "gs_projection_2dgs_bwd": lambda: torch.autograd.grad(proj_out, tuple(t.values()), proj_cot, retain_graph=True),
        "gs_rasterize_2dgs_fwd": nograd(ras),
        "gs_rasterize_2dgs_bwd": lambda: torch.autograd.grad(ras_out, ras_in, ras_cot, retain_graph=True),
        "gs_depth_to_normal_fwd": nograd(lambda: surfel.depth_to_normal(depth, c2w, w["Ks"])),
        "gs_depth_to_normal_bwd": lambda: torch.autograd.grad(nrm, depth, cot["n"], retain_graph=True),
    }, a.steps, a.rounds)


if __name__ == "__main__":
    main()
