"""The per-step work of the densification strategies at BASELINE config 2's scene (1 camera, 1080p, gradients from a real
rasterization() backward).  Alternates, in one process, A = a plain-torch restatement of what the reference's strategy does on a step
(written here, float32) and B = this package's fused call:
  * DefaultStrategy._update_state, unpacked and packed, absgrad off and on;
  * inject_noise_to_position (A uses this package's quat_scale_to_covar_preci);
  * a whole training iteration (render forward + backward + photometric_loss + step_all) + each strategy's step_post_backward on
    non-refining steps;
and reports compute_relocation at N = 50,000 and the wall time of one refining step of each strategy.  Every time is the median over
rounds of (device time between two events) / calls and of (host clock around a device-synchronised window) / calls, with min and max;
the spread of A is the bar B has to clear.
usage: python tools/bench_strategy.py [--calls 50] [--rounds 7] [--iters 20]"""
import argparse
import gc
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gscodec_studio_amd import quat_scale_to_covar_preci, rasterization  # noqa: E402
from gscodec_studio_amd._helper import sh_workload  # noqa: E402
from gscodec_studio_amd.losses import photometric_loss  # noqa: E402
from gscodec_studio_amd.optimizers import Adam, step_all  # noqa: E402
from gscodec_studio_amd.relocation import compute_relocation  # noqa: E402
from gscodec_studio_amd.strategy import DefaultStrategy, MCMCStrategy, ops  # noqa: E402

NAMES = ("means", "quats", "scales", "opacities", "sh0", "shN")
LRS = {"means": 1.6e-4, "quats": 1e-3, "scales": 5e-3, "opacities": 5e-2, "sh0": 2.5e-3, "shN": 2.5e-3 / 20}


def torch_update_state(state, info, absgrad, packed, with_radii):
    """What the reference's DefaultStrategy._update_state does, in plain torch (its torch.where is a host synchronisation)."""
    g = (info["means2d"].absgrad if absgrad else info["means2d"].grad).clone()
    g[..., 0] *= info["width"] / 2.0 * info["n_cameras"]
    g[..., 1] *= info["height"] / 2.0 * info["n_cameras"]
    if packed:
        ids, radii = info["gaussian_ids"], info["radii"]
    else:
        sel = info["radii"] > 0.0
        ids = torch.where(sel)[1]
        g, radii = g[sel], info["radii"][sel]
    state["grad2d"].index_add_(0, ids, g.norm(dim=-1))
    state["count"].index_add_(0, ids, torch.ones_like(ids, dtype=torch.float32))
    if with_radii:
        state["radii"][ids] = torch.maximum(state["radii"][ids], radii / float(max(info["width"], info["height"])))


def torch_inject_noise(params, scaler):
    """What the reference's inject_noise_to_position does, over this package's quat_scale_to_covar_preci."""
    with torch.no_grad():
        opacities = torch.sigmoid(params["opacities"].flatten())
        covars, _ = quat_scale_to_covar_preci(params["quats"], torch.exp(params["scales"]), compute_covar=True, compute_preci=False, triu=False)
        noise = torch.randn_like(params["means"]) * (1 / (1 + torch.exp(-100 * ((1 - opacities) - 0.995)))).unsqueeze(-1) * scaler
        params["means"].add_(torch.einsum("bij,bj->bi", covars, noise))


def timed(fn, calls):
    """(device ms per call by events, wall ms per call) of `calls` back-to-back calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls, (time.perf_counter() - t0) / calls * 1e3


def report(title, fns, calls, rounds, min_bytes=None):
    for fn in fns.values():
        timed(fn, 3)
    dev, wall = {t: [] for t in fns}, {t: [] for t in fns}
    for _ in range(rounds):
        for tag, fn in fns.items():  # interleaved
            d, w = timed(fn, calls)
            dev[tag].append(d)
            wall[tag].append(w)
    print(f"{title}: median of {rounds} rounds x {calls} calls, ms per call", flush=True)
    for tag in fns:
        print(f"  {tag:44s} device {statistics.median(dev[tag]):8.4f} (min {min(dev[tag]):.4f}, max {max(dev[tag]):.4f})   "
              f"wall {statistics.median(wall[tag]):8.4f} (min {min(wall[tag]):.4f}, max {max(wall[tag]):.4f})", flush=True)
    tags = list(fns)
    if len(tags) == 2:
        a, b = tags
        for name, t in (("device", dev), ("wall", wall)):
            ma, mb = statistics.median(t[a]), statistics.median(t[b])
            spread = max(t[a]) - min(t[a])
            verdict = "B faster than A by more than A's spread" if ma - mb > spread else "NO gain beyond A's run-to-run spread"
            print(f"  {name}: A / B = {ma / mb:.2f}x, A - B = {ma - mb:.4f} ms, spread of A = {spread:.4f} ms -> {verdict}", flush=True)
    if min_bytes is not None:
        mb = statistics.median(dev[tags[-1]])
        print(f"  B moves at least {min_bytes / 1e6:.1f} MB: {min_bytes / mb / 1e6:.0f} GB/s over the device time of a call", flush=True)
    return dev, wall


def trainer(init):
    ps = {k: torch.nn.Parameter(init[k].contiguous().clone()) for k in NAMES}
    opts = {k: Adam([{"params": [p], "lr": LRS[k], "name": k}], eps=1e-15) for k, p in ps.items()}
    return ps, opts


def render(ps, w, **kw):
    kw.setdefault("packed", False)
    return rasterization(ps["means"], ps["quats"], torch.exp(ps["scales"]), torch.sigmoid(ps["opacities"]), (ps["sh0"], ps["shN"]),
                         w["viewmats"], w["Ks"], w["width"], w["height"], sh_degree=3, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    gc.collect()
    gc.freeze()
    w = sh_workload(scene_grid=3, device="cuda")
    sh = w["sh"]
    init = {"means": w["means"], "quats": w["quats"], "scales": torch.log(w["scales"]),
            "opacities": torch.logit(w["opacities"].clamp(1e-4, 1 - 1e-4)), "sh0": sh[:, :1], "shN": sh[:, 1:]}
    N = init["means"].shape[0]
    pixels = torch.rand((1, w["height"], w["width"], 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    print(f"scene: {N} gaussians, 1 camera {w['width']}x{w['height']}", flush=True)

    # ---- DefaultStrategy._update_state
    for packed in (False, True):
        ps, _ = trainer(init)
        colors, _, info = render(ps, w, absgrad=True, packed=packed)
        info["means2d"].retain_grad()
        photometric_loss(colors, pixels, ssim_lambda=0.2)[0].backward()
        rows = info["radii"].numel()
        visible = int((info["radii"] > 0).sum())
        for absgrad in (False, True):
            g = info["means2d"].absgrad if absgrad else info["means2d"].grad
            strategy = DefaultStrategy(absgrad=absgrad, refine_scale2d_stop_iter=1000)
            sa = {k: torch.zeros(N, device="cuda") for k in ("grad2d", "count", "radii")}
            sb = strategy.initialize_state()
            # radii of every row, the gradient and a read-modify-write of the three statistics of every visible gaussian
            # (a 64-byte-strided gradient row costs its whole 64 bytes)
            grad_bytes = 8 if g.stride(-2) == 2 else 64
            min_bytes = rows * 4 + (8 if packed else 0) * rows + visible * (grad_bytes + 3 * 8)
            report(f"_update_state {'packed' if packed else 'unpacked'}, absgrad={absgrad} ({rows} rows, {visible} visible, gradient row "
                   f"stride {g.stride(-2)} floats)",
                   {"A torch restatement": lambda: torch_update_state(sa, info, absgrad, packed, True),
                    "B DefaultStrategy._update_state": lambda: strategy._update_state(ps, sb, info, packed=packed)},
                   a.calls, a.rounds, min_bytes=min_bytes)
            torch.cuda.synchronize()
            rel = float((sa["grad2d"] - sb["grad2d"]).norm() / sa["grad2d"].norm())
            print(f"  A vs B after the same number of calls: grad2d relL2 {rel:.2e}, count equal {torch.equal(sa['count'], sb['count'])}, "
                  f"radii equal {torch.equal(sa['radii'], sb['radii'])}", flush=True)
        del colors, info

    # ---- inject_noise_to_position
    pa, _ = trainer(init)
    pb, _ = trainer(init)
    scaler = LRS["means"] * 5e5
    report("inject_noise_to_position", {"A torch restatement": lambda: torch_inject_noise(pa, scaler),
                                        "B ops.inject_noise_to_position": lambda: ops.inject_noise_to_position(pb, {}, {}, scaler)},
           a.calls, a.rounds, min_bytes=N * (14 + 3) * 4 + N * 3 * 4)  # (+ the noise written by randn_like)

    # ---- compute_relocation at N = 50,000, ratios drawn as relocate draws them
    n_rel = 50_000
    opac = torch.sigmoid(init["opacities"])
    sampled = torch.multinomial(opac, n_rel, replacement=True)
    binoms = MCMCStrategy().initialize_state()["binoms"].cuda()
    o_s, s_s = opac[sampled].contiguous(), torch.exp(init["scales"])[sampled].contiguous()
    ratios = torch.bincount(sampled)[sampled] + 1
    print(f"compute_relocation: ratios 1..{int(ratios.max())}, mean {float(ratios.float().mean()):.2f}", flush=True)
    report(f"compute_relocation N = {n_rel}", {"compute_relocation": lambda: compute_relocation(o_s, s_s, ratios.clone(), binoms)},
           a.calls, a.rounds)
    worst = torch.full((n_rel,), 51, device="cuda")
    report(f"compute_relocation N = {n_rel}, every ratio 51", {"compute_relocation": lambda: compute_relocation(o_s, s_s, worst.clone(), binoms)},
           a.calls, a.rounds)

    # ---- a whole training iteration with each strategy's step_post_backward, non-refining steps
    def iteration(kind, fused):
        ps, opts = trainer(init)
        strategy = DefaultStrategy(refine_scale2d_stop_iter=1000) if kind == "default" else MCMCStrategy()
        state = strategy.initialize_state()
        plain = {k: torch.zeros(N, device="cuda") for k in ("grad2d", "count", "radii")}

        def fn():
            colors, _, info = render(ps, w)
            loss = photometric_loss(colors, pixels, ssim_lambda=0.2)[0]
            strategy.step_pre_backward(ps, opts, state, 7, info)
            loss.backward()
            if kind == "default":
                if fused:
                    strategy.step_post_backward(ps, opts, state, 7, info)
                else:
                    torch_update_state(plain, info, False, False, True)
                step_all(opts)
            else:
                step_all(opts)
                if fused:
                    strategy.step_post_backward(ps, opts, state, 7, info, lr=LRS["means"])
                else:
                    torch_inject_noise(ps, LRS["means"] * strategy.noise_lr)
        return fn

    for kind in ("default", "mcmc"):
        report(f"training iteration at config 2 + {kind} strategy's per-step work",
               {"A torch restatement": iteration(kind, False), "B strategy.step_post_backward": iteration(kind, True)}, a.iters, a.rounds)

    # ---- one refining step of each strategy, for the record (wall time, device-synchronised)
    for kind in ("default", "mcmc"):
        ps, opts = trainer(init)
        strategy = DefaultStrategy() if kind == "default" else MCMCStrategy(cap_max=2 * N)
        state = strategy.initialize_state()
        for step in (598, 599, 600):
            colors, _, info = render(ps, w)
            loss = photometric_loss(colors, pixels, ssim_lambda=0.2)[0]
            strategy.step_pre_backward(ps, opts, state, step, info)
            loss.backward()
            step_all(opts)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "default":
                strategy.step_post_backward(ps, opts, state, step, info)
            else:
                strategy.step_post_backward(ps, opts, state, step, info, lr=LRS["means"])
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            print(f"{kind} strategy, step_post_backward at step {step}{' (refining)' if step == 600 else ''}: {dt:.3f} ms wall, "
                  f"{len(ps['means'])} gaussians afterwards", flush=True)


if __name__ == "__main__":
    main()
