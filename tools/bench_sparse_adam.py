"""The optimizer step of the trainers' --sparse_grad mode, at BASELINE config 2's splat set (1,006,065 gaussians, SH 3: means 3,
scales 3, quats 4, opacities 1, sh0 3, shN 45 floats per gaussian).  Index lists: info["gaussian_ids"] of a packed render of the
bench scene with 1 camera (coalesced, as the trainer flags it) and with 4 cameras (duplicates).  Per index list, alternating in
one process, round after round:
  (a) optimizers.step_all over six optimizers.SparseAdam (one sort, one gs_sparse_adam_multi launch)
  (b) the six torch.optim.SparseAdam steps it replaces
  (c) optimizers.step_all over six dense optimizers.Adam on the same parameters (the densified gradients)
Every variant keeps its own parameters, state and gradients; the gradients are set once and stepped again and again
(zero_grad=False), so the timed region is the optimizer step alone.
usage: python tools/bench_sparse_adam.py [--steps 20] [--rounds 5]"""
import argparse
import gc
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gscodec_studio_amd import rasterization  # noqa: E402
from gscodec_studio_amd._helper import sh_workload  # noqa: E402
from gscodec_studio_amd.optimizers import Adam, SparseAdam, step_all  # noqa: E402

NAMES = ("means", "scales", "quats", "opacities", "sh0", "shN")
LRS = {"means": 1.6e-4, "quats": 1e-3, "scales": 5e-3, "opacities": 5e-2, "sh0": 2.5e-3, "shN": 2.5e-3 / 20}


def make_params(w):
    sh = w["sh"]
    init = {"means": w["means"], "quats": w["quats"], "scales": torch.log(w["scales"]),
            "opacities": torch.logit(w["opacities"].clamp(1e-4, 1 - 1e-4)), "sh0": sh[:, :1], "shN": sh[:, 1:]}
    return {k: torch.nn.Parameter(init[k].contiguous().clone()) for k in NAMES}


def make_opts(ps, cls):
    return {k: cls([{"params": [p], "lr": LRS[k], "name": k}], eps=1e-15, betas=(0.9, 0.999)) for k, p in ps.items()}


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    gc.collect()
    gc.freeze()
    for cams in (1, 4):
        w = sh_workload(scene_grid=3, n_cameras=cams, device="cuda")
        N = w["N"]
        base = make_params(w)
        with torch.no_grad():
            _, _, info = rasterization(base["means"], base["quats"], torch.exp(base["scales"]), torch.sigmoid(base["opacities"]),
                                       (base["sh0"], base["shN"]), w["viewmats"], w["Ks"], w["width"], w["height"], sh_degree=3, packed=True)
        gids = info["gaussian_ids"].clone()
        del info
        nnz, uniq = gids.numel(), int(gids.unique().numel())
        coalesced = cams == 1
        assert not coalesced or bool((gids[1:] > gids[:-1]).all()), "one camera: gaussian_ids must ascend strictly"
        gen = torch.Generator(device="cuda").manual_seed(cams)
        values = {k: torch.randn((nnz, *base[k].shape[1:]), device="cuda", generator=gen) * 0.01 for k in NAMES}
        print(f"{cams} camera(s): N = {N:,} gaussians, gaussian_ids nnz = {nnz:,}, distinct = {uniq:,} ({uniq / N * 100:.1f} % of the rows), "
              f"is_coalesced = {coalesced}", flush=True)

        variants = {}

        def variant(tag, cls, sparse, use_step_all):
            ps = {k: torch.nn.Parameter(v.detach().clone()) for k, v in base.items()}
            ids = gids.clone()
            for k, p in ps.items():
                g = torch.sparse_coo_tensor(ids[None], values[k].clone(), p.shape, is_coalesced=coalesced)
                p.grad = g if sparse else g.to_dense()
            opts = make_opts(ps, cls)
            if use_step_all:
                fn = lambda: step_all(opts, zero_grad=False)  # noqa: E731
            else:
                def fn():
                    for o in opts.values():
                        o.step()
            fn()  # state allocation, code objects
            torch.cuda.synchronize()
            variants[tag] = fn

        variant("(a) step_all, 6x optimizers.SparseAdam", SparseAdam, True, True)
        variant("(b) 6x torch.optim.SparseAdam", torch.optim.SparseAdam, True, False)
        variant("(c) step_all, 6x dense optimizers.Adam", Adam, False, True)
        for fn in variants.values():
            timed(fn, 3)
        times = {t: [] for t in variants}
        for _ in range(a.rounds):
            for tag, fn in variants.items():
                times[tag].append(timed(fn, a.steps))
        print(f"optimizer step, {a.rounds} alternating rounds x {a.steps} steps (host clock around device-synchronised windows), ms:", flush=True)
        for tag, ts in times.items():
            print(f"  {tag:42s} min {min(ts):8.4f}  max {max(ts):8.4f}   rounds: " + " ".join(f"{t:.4f}" for t in ts), flush=True)
        del variants, values, base, gids
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
