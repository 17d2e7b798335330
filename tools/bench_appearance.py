"""The appearance module (appearance.AppearanceOptModule, csrc/appearance.hip) at BASELINE config 2's size (1,006,065 splats), with
one camera and with four.  Alternates, in one process and with interleaved repeats:
  (a) a plain-torch restatement of the reference's statements: embedding expand, feature expand, F.normalize, the basis tensor built
      by indexed assignments, the cat, the Sequential head, + colors, sigmoid
  (c) module.colors(features, embed_ids, means, camtoworlds, sh_degree, base=colors)
forward alone (under no_grad) and forward + backward (gradients of features, means, base, embeddings and head), with the run-to-run
spread of both; then the two kernels alone; then a whole iteration (module + rasterization(sh_degree=None) + photometric_loss +
backward + step_all + Adam over the module) both ways.
usage: python tools/bench_appearance.py [--steps 10] [--rounds 5] [--iters 5] [--cameras 1 4] [--skip-iteration]"""
import argparse
import gc
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gscodec_studio_amd import _backend as B, rasterization  # noqa: E402
from gscodec_studio_amd._helper import sh_workload  # noqa: E402
from gscodec_studio_amd.appearance import AppearanceOptModule  # noqa: E402
from gscodec_studio_amd.losses import photometric_loss  # noqa: E402
from gscodec_studio_amd.optimizers import Adam, step_all  # noqa: E402

gc.collect()
gc.freeze()

LRS = {"means": 1.6e-4, "scales": 5e-3, "quats": 1e-3, "opacities": 5e-2, "features": 2.5e-3, "colors": 2.5e-3}


def bases_by_assignment(num, d):
    """The basis tensor as the reference builds it: an empty [..., num] tensor filled column by column."""
    out = torch.empty((*d.shape[:-1], num), dtype=d.dtype, device=d.device)
    x, y, z = d.unbind(-1)
    out[..., 0] = 0.2820947917738781
    if num > 1:
        out[..., 1], out[..., 2], out[..., 3] = -0.48860251190292 * y, 0.48860251190292 * z, -0.48860251190292 * x
    if num > 4:
        z2, c1, s1 = z * z, x * x - y * y, 2 * x * y
        tb = -1.092548430592079 * z
        out[..., 4], out[..., 5], out[..., 6] = 0.5462742152960395 * s1, tb * y, 0.9461746957575601 * z2 - 0.3153915652525201
        out[..., 7], out[..., 8] = tb * x, 0.5462742152960395 * c1
    if num > 9:
        c2, s2 = x * c1 - y * s1, x * s1 + y * c1
        tc, tb = -2.285228997322329 * z2 + 0.4570457994644658, 1.445305721320277 * z
        out[..., 9], out[..., 10], out[..., 11] = -0.5900435899266435 * s2, tb * s1, tc * y
        out[..., 12] = z * (1.865881662950577 * z2 - 1.119528997770346)
        out[..., 13], out[..., 14], out[..., 15] = tc * x, tb * c1, -0.5900435899266435 * c2
    return out


class TorchAppearance(nn.Module):
    """The module as a ROCm user writes it in torch today (sh_degree <= 3)."""

    def __init__(self, n, feature_dim, embed_dim=16, sh_degree=3):
        super().__init__()
        self.embed_dim, self.sh_degree = embed_dim, sh_degree
        self.embeds = nn.Embedding(n, embed_dim)
        self.color_head = nn.Sequential(nn.Linear(embed_dim + feature_dim + (sh_degree + 1) ** 2, 64), nn.ReLU(inplace=True),
                                        nn.Linear(64, 64), nn.ReLU(inplace=True), nn.Linear(64, 3))

    def forward(self, features, embed_ids, dirs, sh_degree):
        C, N = dirs.shape[:2]
        embeds = self.embeds(embed_ids)[:, None, :].expand(-1, N, -1)
        features = features[None].expand(C, -1, -1)
        dirs = F.normalize(dirs, dim=-1)
        nb, K = (sh_degree + 1) ** 2, (self.sh_degree + 1) ** 2
        bases = torch.zeros(C, N, K, device=features.device)
        bases[:, :, :nb] = bases_by_assignment(nb, dirs)
        return self.color_head(torch.cat([embeds, features, bases], dim=-1))


def trainer_colors(kind, module, features, ids, means, camtoworlds, deg, base):
    if kind == "fused":
        return module.colors(features, ids, means, camtoworlds, deg, base=base)
    dirs = means[None, :, :] - camtoworlds[:, None, :3, 3]
    return torch.sigmoid(module(features, ids, dirs, deg) + base)


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
        print(f"  {tag:64s} {med[tag]:8.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f}, spread {max(ts) - min(ts):.4f})", flush=True)
    return med, {t: max(ts) - min(ts) for t, ts in times.items()}


def verdict(name, med, spread, ka, kc):
    gap, both = med[ka] - med[kc], spread[ka] + spread[kc]
    word = "beyond both spreads" if abs(gap) > both else "INSIDE the spreads: no claim"
    print(f"  {name}: (a) - (c) = {gap:+.4f} ms, (a) / (c) = {med[ka] / med[kc]:.2f}x, sum of the two spreads {both:.4f} ms -> {word}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cameras", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--skip-iteration", action="store_true")
    a = ap.parse_args()
    dev = "cuda"
    W, H, deg = 1920, 1080, 3
    for C in a.cameras:
        w = sh_workload(3, W, H, n_cameras=C, device=dev)
        N = w["N"]
        g = torch.Generator(device=dev).manual_seed(1)
        torch.manual_seed(0)
        fused = AppearanceOptModule(C, 32).to(dev)
        plain = TorchAppearance(C, 32).to(dev)
        plain.load_state_dict(fused.state_dict(), strict=True)
        mods = {"torch": plain, "fused": fused}
        features = (0.5 * torch.randn((N, 32), device=dev, generator=g)).requires_grad_(True)
        base = torch.logit(w["rgb"].clamp(0.02, 0.98)).requires_grad_(True)
        means = w["means"].clone().requires_grad_(True)
        camtoworlds = torch.linalg.inv(w["viewmats"])
        ids = torch.arange(C, device=dev)
        cot = torch.randn((C, N, 3), device=dev, generator=g)
        print(f"==== {N} splats, {C} camera(s), feature_dim 32, embed_dim 16, sh_degree 3", flush=True)

        def fwd(kind):
            def run():
                with torch.no_grad():
                    trainer_colors(kind, mods[kind], features, ids, means, camtoworlds, deg, base)
            return run

        def fwd_bwd(kind):
            def run():
                (trainer_colors(kind, mods[kind], features, ids, means, camtoworlds, deg, base) * cot).sum().backward()
                features.grad = base.grad = means.grad = None
                mods[kind].zero_grad(set_to_none=True)
            return run

        ka, kc = "(a) torch restatement of the reference's statements", "(c) fused: module.colors(...)"
        with torch.no_grad():
            diff = (trainer_colors("torch", plain, features, ids, means, camtoworlds, deg, base)
                    - trainer_colors("fused", fused, features, ids, means, camtoworlds, deg, base)).abs().max()
        print(f"  largest difference of the two colour tensors: {float(diff):.2e}", flush=True)
        med, spread = report("module forward", {ka: fwd("torch"), kc: fwd("fused")}, a.steps, a.rounds)
        verdict("forward", med, spread, ka, kc)
        med, spread = report("module forward + backward (includes the (out * cot).sum() of both)",
                             {ka: fwd_bwd("torch"), kc: fwd_bwd("fused")}, a.steps, a.rounds)
        verdict("forward + backward", med, spread, ka, kc)

        # ---- the kernels alone
        h = fused.color_head
        ws = [t.detach().contiguous() for t in (h[0].weight, h[0].bias, h[2].weight, h[2].bias, h[4].weight, h[4].bias)]
        emb = fused.embeds(ids).detach().contiguous()
        cams = camtoworlds[:, :3, 3].contiguous()
        out = torch.empty((C, N, 3), device=dev)
        v_f, v_m, v_b = torch.empty((N, 32), device=dev), torch.empty((N, 3), device=dev), torch.empty((N, 3), device=dev)
        rows, cols = int(B.query("gs_appearance_partial_rows", N, 32, 16, 16, 0)), int(B.query("gs_appearance_partial_cols", C, 32, 16))
        partials = torch.empty((rows, cols), device=dev)
        st = torch.cuda.current_stream().cuda_stream
        head = (N, C, 32, 16, 16, 16, features.data_ptr(), emb.data_ptr(), None, means.data_ptr(), cams.data_ptr(),
                *[t.data_ptr() for t in ws], base.data_ptr(), 1)
        k_fwd = lambda: B.call("gs_appearance_fwd", *head, 0, out.data_ptr(), st)  # noqa: E731
        k_bwd = lambda: B.call("gs_appearance_bwd", *head, cot.data_ptr(), 0, v_f.data_ptr(), None, v_m.data_ptr(), v_b.data_ptr(),  # noqa: E731
                               partials.data_ptr(), st)
        names = ("gs_appearance_fwd", "gs_appearance_bwd")
        med2, _ = report("kernels alone", dict(zip(names, (k_fwd, k_bwd))), a.steps * 2, a.rounds)
        flop_f = 2.0 * (64 * 64 + 64 * 64 + 3 * 64) * C * N
        print(f"  forward: {flop_f / 1e9:.1f} GFLOP -> {flop_f / med2[names[0]] / 1e9:.1f} TFLOP/s; backward (recompute + five more products): "
              f"{(flop_f * 3) / med2[names[1]] / 1e9:.1f} TFLOP/s; partials [{rows}, {cols}] = {rows * cols * 4 / 1e6:.1f} MB", flush=True)
        del out, v_f, v_m, v_b, partials
        if a.skip_iteration:
            continue

        # ---- a whole training iteration
        pixels = torch.rand((C, H, W, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
        start = {"means": w["means"], "quats": w["quats"], "scales": torch.log(w["scales"]), "opacities": torch.logit(w["opacities"].clamp(1e-4, 1 - 1e-4)),
                 "features": features.detach(), "colors": base.detach()}

        def iteration(kind):
            ps = {k: torch.nn.Parameter(v.contiguous().clone()) for k, v in start.items()}
            opts = {k: Adam([{"params": [p], "lr": LRS[k], "name": k}], eps=1e-15) for k, p in ps.items()}
            torch.manual_seed(0)
            mod = (AppearanceOptModule(C, 32) if kind == "fused" else TorchAppearance(C, 32)).to(dev)
            mopt = torch.optim.Adam([{"params": mod.embeds.parameters(), "lr": 1e-2, "weight_decay": 1e-6},
                                     {"params": mod.color_head.parameters(), "lr": 1e-3}])

            def fn():
                colors = trainer_colors(kind, mod, ps["features"], ids, ps["means"], camtoworlds, deg, ps["colors"])
                rc, _, _ = rasterization(ps["means"], ps["quats"], torch.exp(ps["scales"]), torch.sigmoid(ps["opacities"]), colors,
                                         w["viewmats"], w["Ks"], W, H, sh_degree=None, packed=False)
                photometric_loss(rc, pixels, ssim_lambda=0.2)[0].backward()
                step_all(opts)
                mopt.step()
                mopt.zero_grad(set_to_none=True)
            return fn

        ia, ic = "(a) torch module + rasterization + loss + backward + step_all + Adam", "(c) fused module + the same"
        med4, spread4 = report("training iteration", {ia: iteration("torch"), ic: iteration("fused")}, a.iters, a.rounds)
        verdict("iteration", med4, spread4, ia, ic)
        del w, features, base, means, cot, pixels, start
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
