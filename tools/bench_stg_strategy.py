"""The per-step work of the spacetime strategies at BASELINE config 5's scene (2 M dynamic splats, the parameter dict of
`bench.py --dynamic`, one 1080p camera).  Alternates, in one process and with interleaved repeats, A = a plain-torch restatement of
the reference's statements (written here, float32) and B = this package's call:
  * the per-step freeze of STG_Strategy (`grad * mask`, `logical_not`, `grad * ~mask` against one gs_stg_freeze_grads launch);
  * the mask build `_zero_omegabymotion` (the elementwise / reduction chain against one gs_stg_omega_mask launch), without the
    parameter replacement, which is the same host work on both sides;
  * a whole dynamic training iteration -- render_dynamic forward + backward, photometric_loss, step_all -- without any strategy work,
    with the torch restatement of the reference's step (its _update_state, tools/bench_strategy.py, and the freeze), and with
    STG_Strategy.step_post_backward, on a statistics-only step (7) and on a statistics-and-freeze step (8507).
Every time is the median over rounds of (device time between two events) / calls and of (host clock around a device-synchronised
window) / calls, with min and max; the spread of A is the bar B has to clear.
usage: python tools/bench_stg_strategy.py [--splats 2000000] [--calls 50] [--rounds 7] [--iters 10]"""
import argparse
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_strategy import report, torch_update_state  # noqa: E402
from gscodec_studio_amd._helper import DYNAMIC_KEYS, dynamic_workload  # noqa: E402
from gscodec_studio_amd.compression_simulation import STGCompressionSimulation  # noqa: E402
from gscodec_studio_amd.dynamic import render_dynamic  # noqa: E402
from gscodec_studio_amd.losses import photometric_loss  # noqa: E402
from gscodec_studio_amd.optimizers import Adam, step_all  # noqa: E402
from gscodec_studio_amd.strategy import STG_Strategy, ops  # noqa: E402

LRS = {"means": 1.6e-4, "scales": 5e-3, "quats": 1e-3, "opacities": 5e-2, "trbf_center": 1e-4, "trbf_scale": 3e-2, "motion": 5.6e-4,
       "omega": 1e-4, "colors": 2.5e-3, "features_dir": 2.5e-3, "features_time": 2.5e-3}


def torch_omega_mask(params):
    """The statements of the reference's _zero_omegabymotion up to the parameter replacement."""
    with torch.no_grad():
        scales = torch.exp(params["scales"])
        pointopacity = torch.sigmoid(params["opacities"])
        omegamask = torch.sum(torch.abs(params["motion"][:, 0:3]), dim=1) > 0.3
        scalemask = torch.max(scales, dim=1).values.unsqueeze(1) > 0.2
        scalemaskb = torch.max(scales, dim=1).values.unsqueeze(1) < 0.6
        opacitymask = pointopacity > 0.7
        mask = torch.logical_and(torch.logical_and(omegamask.unsqueeze(1), scalemask), torch.logical_and(scalemaskb, opacitymask.unsqueeze(1)))
        omeganew = mask.float() * params["omega"]
        sel = torch.where(mask)[0]  # (unused there too: a host synchronisation)
    return mask, omeganew, sel


def torch_freeze(params, mask):
    """The reference's freeze statements: two new [N, 4] tensors and a new mask per step."""
    params["omega"].grad = params["omega"].grad * mask
    rotationmask = torch.logical_not(mask)
    params["quats"].grad = params["quats"].grad * rotationmask


def trainer(w):
    ps = {k: torch.nn.Parameter(w[k].contiguous().clone()) for k in DYNAMIC_KEYS}
    opts = {k: Adam([{"params": [p], "lr": LRS[k], "name": k}], eps=1e-15) for k, p in ps.items()}
    return ps, opts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, default=2_000_000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    gc.collect()
    gc.freeze()
    w = dynamic_workload(a.splats, 1920, 1080, device="cuda")
    N, W, H = w["N"], w["width"], w["height"]
    pixels = torch.rand((1, H, W, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    print(f"scene: {N} dynamic gaussians, 1 camera {W}x{H}", flush=True)

    # ---- the mask build
    ps, _ = trainer(w)
    with torch.no_grad():  # (ten times the workload's motion, for the mask alone: enough first-order motion to clear its 0.3)
        ps["motion"].mul_(10.0)
    mask_a, omega_a, _ = torch_omega_mask(ps)
    mask_b, omega_b = ops.stg_omega_mask(ps["motion"], ps["scales"], ps["opacities"], ps["omega"])
    torch.cuda.synchronize()
    print(f"omega mask: {int(mask_b.sum())} of {N} kept; differs from the torch restatement at {int((mask_a != mask_b).sum())} gaussians, "
          f"omega_new equal: {torch.equal(omega_a, omega_b)}", flush=True)
    # 3 of the 9 motion floats (their sectors in practice), 3 scales, 1 opacity, 4 omega read; 4 floats + 1 byte written
    report("_zero_omegabymotion, mask and masked omega (no parameter replacement)",
           {"A torch restatement": lambda: torch_omega_mask(ps),
            "B ops.stg_omega_mask": lambda: ops.stg_omega_mask(ps["motion"], ps["scales"], ps["opacities"], ps["omega"])},
           a.calls, a.rounds, min_bytes=N * (15 * 4 + 1))

    # ---- the per-step freeze
    mask = mask_b
    g = torch.Generator(device="cuda").manual_seed(7)
    grads = {k: torch.randn(N, 4, device="cuda", generator=g) for k in ("omega", "quats")}
    pa, _ = trainer(w)
    pb, _ = trainer(w)
    for p in (pa, pb):
        for k in ("omega", "quats"):
            p[k].grad = grads[k].clone()
    report("the per-step freeze of omega.grad and quats.grad",
           {"A torch restatement": lambda: torch_freeze(pa, mask),
            "B ops.stg_freeze_grads": lambda: ops.stg_freeze_grads(mask, pb["omega"].grad, pb["quats"].grad)},
           a.calls, a.rounds, min_bytes=N * (4 * 16 + 1))
    torch.cuda.synchronize()
    print(f"  A vs B after the same number of calls: omega.grad equal {torch.equal(pa['omega'].grad, pb['omega'].grad)}, "
          f"quats.grad equal {torch.equal(pa['quats'].grad, pb['quats'].grad)}", flush=True)
    del pa, pb, grads

    # ---- a whole dynamic training iteration
    def iteration(kind, step):
        ps, opts = trainer(w)
        sim = STGCompressionSimulation(quantization_sim_type="round", entropy_steps={}, device="cuda")
        strategy = STG_Strategy()
        strategy.omegamask = mask
        state = strategy.initialize_state()
        plain = {k: torch.zeros(N, device="cuda") for k in ("grad2d", "count")}

        def fn():
            colors, _, info = render_dynamic(ps, 0.5, w["viewmats"], w["Ks"], W, H, compression_sim=sim, step=1, packed=False)
            loss = photometric_loss(colors, pixels, ssim_lambda=0.2)[0]
            strategy.step_pre_backward(ps, opts, state, step, info)
            loss.backward()
            if kind == "strategy":
                strategy.step_post_backward(ps, opts, state, step, info, 0, 0, None, None)
            elif kind == "torch":
                torch_update_state(plain, info, False, False, False)
                if step > 8001:
                    torch_freeze(ps, mask)
            step_all(opts)
        return fn

    report("dynamic training iteration at config 5, statistics-only step (7), no strategy vs step_post_backward",
           {"A without strategy work": iteration("none", 7), "B STG_Strategy.step_post_backward": iteration("strategy", 7)}, a.iters, a.rounds)
    report("dynamic training iteration at config 5, statistics-only step (7), torch restatement vs step_post_backward",
           {"A torch restatement": iteration("torch", 7), "B STG_Strategy.step_post_backward": iteration("strategy", 7)}, a.iters, a.rounds)
    report("dynamic training iteration at config 5, statistics + freeze step (8507), torch restatement vs step_post_backward",
           {"A torch restatement": iteration("torch", 8507), "B STG_Strategy.step_post_backward": iteration("strategy", 8507)},
           a.iters, a.rounds)
    report("dynamic training iteration at config 5, statistics + freeze step (8507), no strategy vs step_post_backward",
           {"A without strategy work": iteration("none", 8507), "B STG_Strategy.step_post_backward": iteration("strategy", 8507)},
           a.iters, a.rounds)


if __name__ == "__main__":
    main()
