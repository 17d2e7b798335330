"""The trainers' photometric loss, forward + backward, at [1, 3, 1080, 1920] and [8, 3, 1080, 1920] (the trainers' [B, H, W, C]
tensors).  Alternates, in one process:
  (a) the float32 F.conv2d SSIM (five depthwise 11x11 convolutions) + F.l1_loss -- what a ROCm user writes without fused_ssim
  (b) losses.fused_ssim + F.l1_loss     (c) losses.photometric_loss
then a whole training iteration at BASELINE config 2 (render forward + backward + loss + optimizers.step_all) with (a) against (c).
usage: python tools/bench_loss.py [--steps 30] [--rounds 5] [--iters 20]"""
import argparse
import gc
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gscodec_studio_amd import rasterization  # noqa: E402
from gscodec_studio_amd._helper import sh_workload  # noqa: E402
from gscodec_studio_amd.losses import fused_ssim, photometric_loss  # noqa: E402
from gscodec_studio_amd.optimizers import step_all  # noqa: E402

LAM = 0.2
NAMES = ("means", "quats", "scales", "opacities", "sh0", "shN")
LRS = {"means": 1.6e-4, "quats": 1e-3, "scales": 5e-3, "opacities": 5e-2, "sh0": 2.5e-3, "shN": 2.5e-3 / 20}


def conv2d_ssim(img1, img2, padding="valid"):
    """The 3DGS loss_utils ssim() restated: float32 depthwise F.conv2d with the 11-tap Gaussian window (sigma 1.5)."""
    C = img1.shape[1]
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
    w1 = torch.tensor((g / g.sum()).astype(np.float32), device=img1.device)
    win = (w1[:, None] * w1[None, :]).expand(C, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, win, padding=5, groups=C)  # noqa: E731
    mu1, mu2 = conv(img1), conv(img2)
    s11, s22, s12 = conv(img1 * img1) - mu1 * mu1, conv(img2 * img2) - mu2 * mu2, conv(img1 * img2) - mu1 * mu2
    S = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s11 + s22 + 9e-4))
    return (S[:, :, 5:-5, 5:-5] if padding == "valid" else S).mean()


def loss_a(colors, pixels):
    ssim = conv2d_ssim(colors.permute(0, 3, 1, 2), pixels.permute(0, 3, 1, 2))
    return F.l1_loss(colors, pixels) * (1.0 - LAM) + (1.0 - ssim) * LAM


def loss_b(colors, pixels):
    ssim = fused_ssim(colors.permute(0, 3, 1, 2), pixels.permute(0, 3, 1, 2), padding="valid")
    return F.l1_loss(colors, pixels) * (1.0 - LAM) + (1.0 - ssim) * LAM


def loss_c(colors, pixels):
    return photometric_loss(colors, pixels, ssim_lambda=LAM)[0]


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
        print(f"  {tag:52s} {med[tag]:8.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f})", flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-iteration", action="store_true")
    a = ap.parse_args()
    gc.collect()
    gc.freeze()
    for B in (1, 8):
        g = torch.Generator(device="cuda").manual_seed(B)
        colors = torch.rand((B, 1080, 1920, 3), device="cuda", generator=g).requires_grad_(True)
        pixels = torch.rand((B, 1080, 1920, 3), device="cuda", generator=g)

        def step(fn):
            def run():
                fn(colors, pixels).backward()
                colors.grad = None
            return run

        med = report(f"loss forward + backward at [{B}, 3, 1080, 1920]",
                     {"(a) F.conv2d SSIM (float32) + F.l1_loss": step(loss_a), "(b) fused_ssim + F.l1_loss": step(loss_b),
                      "(c) photometric_loss": step(loss_c)}, a.steps, a.rounds)
        ka, kc = [k for k in med if k.startswith("(a)")][0], [k for k in med if k.startswith("(c)")][0]
        n = B * 3 * 1080 * 1920
        print(f"  (a) / (c) = {med[ka] / med[kc]:.1f}x; (c) at 44 B / element ({44 * n / 1e6:.0f} MB): "
              f"{44 * n / med[kc] / 1e9:.2f} TB/s over the whole call", flush=True)
        del colors, pixels
    if a.skip_iteration:
        return
    w = sh_workload(scene_grid=3, device="cuda")
    sh = w["sh"]
    init = {"means": w["means"], "quats": w["quats"], "scales": torch.log(w["scales"]),
            "opacities": torch.logit(w["opacities"].clamp(1e-4, 1 - 1e-4)), "sh0": sh[:, :1], "shN": sh[:, 1:]}
    pixels = torch.rand((1, w["height"], w["width"], 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))

    def iteration(loss_fn):
        ps = {k: torch.nn.Parameter(init[k].contiguous().clone()) for k in NAMES}
        opts = {k: torch.optim.Adam([{"params": [p], "lr": LRS[k], "name": k}], eps=1e-15, betas=(0.9, 0.999)) for k, p in ps.items()}

        def fn():
            rc, _, _ = rasterization(ps["means"], ps["quats"], torch.exp(ps["scales"]), torch.sigmoid(ps["opacities"]),
                                     (ps["sh0"], ps["shN"]), w["viewmats"], w["Ks"], w["width"], w["height"], sh_degree=3)
            loss_fn(rc, pixels).backward()
            step_all(opts)
        return fn

    med = report("training iteration at config 2 (render fwd + bwd + loss + step_all)",
                 {"(a) ... + F.conv2d SSIM + F.l1_loss": iteration(loss_a), "(c) ... + photometric_loss": iteration(loss_c)},
                 a.iters, a.rounds)
    va, vc = list(med.values())
    print(f"  (a) / (c) = {va / vc:.2f}x", flush=True)


if __name__ == "__main__":
    main()
