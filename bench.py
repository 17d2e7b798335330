#!/usr/bin/env python
"""bench.py -- headline benchmark of the rasterize hot path on MI355X.

Metric (BASELINE.json): Msplats/s fwd+bwd @1080p, 1M splats.  Workload = BASELINE config 2:
the reference's load_test_data(scene_grid=3) scene (N = 1,006,065 gaussians), SH degree 3,
one 1920x1080 camera per GPU, packed=False, near=0.01, far=1e10, radius_clip=0, eps2d=0.3,
tile 16; a "step" is rasterization() forward + backward of sum(render_colors) (the protocol
of the reference's profiling/main.py:104-133), inputs resident in HBM.

Multi-GPU (--gpus N, launched by torch.distributed.run): weak scaling over cameras, rank r
renders camera r of an N-camera batch over the whole scene; value counts splat-camera pairs:
N_splats * n_gpus / step time.  Two exchange patterns compute that batch (--dp-mode):
  camera    splats replicated, no communication in the forward, the step ends with the RCCL sum
            of the splat gradients (distributed.all_reduce_splat_grads; 236 B/splat);
  camera_sparse  the same with only the rows some camera saw on the wire (visibility masks gathered
            in the forward, distributed.plan_sparse_grad_exchange);
  gaussian  the reference's own multi-GPU layout (rasterization(distributed=True), reference
            rendering.py:279-478): every rank owns 1/N of the splats, projects + colours them
            for all N cameras, one all-to-all hands the projected splats to the camera's rank
            (44 B per splat-camera pair) and its dual returns their gradients (40 B); every
            rank ends with the gradient of its own splats, summed over all cameras.  Only the
            rows of visible splats travel (gaussian_dense: all rows, no count read-back).
  auto      (default) times a few untimed steps of both and runs the faster one; the choice and
            both calibration timings are reported in the JSON line.

A plain run (`bench.py --gpus 1 --steps K --warmup W`) does only what the headline needs: set-up, W warm-up steps, --ramp-s
seconds of untimed steps (the GPU reaches its sustained clocks), exactly K timed steps between device synchronisations, and the JSON
line (metric, value, unit, ms_per_step = the K steps' wall time / K, ...).  --dump-outputs DIR additionally writes what the
last timed step computed (see dump_outputs).  Everything below is measured only with --full, which also repeats the timed
region until --min-timed-s has been measured (ms_per_step is then the mean over all regions).

With --full, the JSON line carries two extra objects:
  roofline      the dominant kernel (largest average time per step among the C-ABI entry
                points, timed live with HIP events on the launch stream inside the timed
                region): algorithmic bytes / average
                duration vs the 8 TB/s HBM peak.
  cpu_baseline  the CPU oracle (oracle/gs_oracle.c, a port -- kind "port") timed on this host on the bench workload itself
                (1 warm-up + 3 fwd+bwd passes, ~3 s each on 128 threads; --cpu-scene-grid 1 selects 1/9 of it).
Also reported: ms_per_step_without_loss_forward (the reference times rasterization() and loss.backward() but evaluates
loss = render.sum() once, outside its timers (profiling/main.py:104-133); ``value`` keeps the sum's forward kernel inside
every step, this figure shows the step without it),
peak_mem_gb / step_mem_gb (the reference protocol's Mem column), ms_per_step_dense_image_grad (the same step
with a dense [C,H,W,3] image gradient instead of the protocol's broadcast one), psnr_vs_oracle (config 1).
"""
import argparse
import contextlib
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
# PMC traffic (FETCH_SIZE / WRITE_SIZE, separate rocprofv3 --pmc passes, gfx950 correction applied)
# measured for this workload and committed under profiles/; bench.py cannot run rocprof on itself.
TRAFFIC_JSON = os.path.join(ROOT, "profiles", "r06_pmc_traffic.json")
TRAFFIC_JSON_DYNAMIC = os.path.join(ROOT, "profiles", "r06_pmc_traffic_dynamic.json")  # (bench.py --dynamic, tools/pmc.sh with PMC_BENCH_ARGS)
HBM_COPY_GBS = 6290.0  # what a float4 copy was measured to reach on this part (MI355X_MICROARCH.md: 6.29 TB/s, 79 % of spec)
# entry point -> (kernel name fragment, the source file the kernel lives in)
_RASTER_SRC = ("rasterize.hip", "rasterize_dev.h", "rasterize_common.h", "dpp_reduce.h")
KERNEL_OF_ENTRY = {"gs_rasterize_bwd": ("raster_seg_bwd_kernel", _RASTER_SRC), "gs_rasterize_fwd": ("raster_tile_fwd_kernel", _RASTER_SRC),
                   "gs_sh_view_bwd": ("sh_bwd_kernel", ("sh.hip",)), "gs_projection_rows_bwd": ("projection_bwd_kernel<false, 3>", ("projection.hip",)),
                   "gs_sort_isect_pairs": ("sort_scatter_kernel<unsigned int, 16, true", ("radix_sort.hip",)),
                   "gs_projection_rows_fwd": ("projection_fwd_kernel<true", ("projection.hip", "projection_dev.h")),
                   "gs_projection_rows_dyn_fwd": ("projection_dyn_fwd_kernel", ("projection_dyn.hip", "projection_dev.h", "dynamic_dev.h", "quant_dev.h")),
                   "gs_projection_rows_dyn_bwd": ("projection_dyn_bwd_kernel", ("projection_dyn.hip", "projection_dev.h", "dynamic_dev.h", "quant_dev.h")),
                   "gs_temporal_slice_fwd": ("temporal_slice_fwd_kernel", ("dynamic.hip", "dynamic_dev.h")),
                   "gs_temporal_slice_bwd": ("temporal_slice_bwd_kernel", ("dynamic.hip", "dynamic_dev.h"))}


def _source_hash(name):
    import hashlib

    with open(os.path.join(ROOT, "gscodec_studio_amd", "csrc", name), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def measured_pmc(entry, workload_key, field="traffic_bytes_per_launch", path=None, wide=False):
    """A per-launch PMC figure of the kernel behind `entry` from the committed summary (HBM bytes by default), or None --
    also None when the kernel's source file has changed since the counters were collected (the JSON carries the hashes of
    the sources it was taken from: a stale figure is not reported)."""
    try:
        d = json.load(open(path or TRAFFIC_JSON))
        if d.get("workload_key") != workload_key:
            return None
        frag, srcs = KERNEL_OF_ENTRY.get(entry, (None, ()))
        if wide and entry == "gs_rasterize_bwd":  # 5..32 channels: the wide instance of the segmented backward
            frag, srcs = "raster_seg_bwd_wide_kernel", ("rasterize_wide.hip", "rasterize_dev.h", "rasterize_common.h", "dpp_reduce.h")
        if any(d.get("source_hashes", {}).get(src) != _source_hash(src) for src in srcs):
            return None
        for name, v in d["kernels"].items():
            if frag and frag in name:
                return v.get(field)
    except Exception:
        pass
    return None


BINNING_ENTRIES = {"gs_presort_split", "gs_isect_count_keys", "gs_presort_buckets", "gs_sort_pairs_u64_i32_drop", "gs_isect_count",
                   "gs_cumsum_i32", "gs_isect_finish_presorted", "gs_isect_emit_presorted", "gs_isect_emit", "gs_isect_emit_compact",
                   "gs_sort_isect_pairs", "gs_sort_pairs_u64_i32", "gs_isect_offset_encode"}


def measured_traffic(entry, workload_key):
    return measured_pmc(entry, workload_key)


# fp32 vector peak 157.3 TFLOP/s = 256 CU x 4 SIMD x 2.4 GHz x one wave64 instruction per 2 cycles (MI355X_MICROARCH.md)
VALU_PEAK_WAVE_INSTR_PER_S = 256 * 4 * 2.4e9 / 2


def measured_valu_issue_rate():
    """What the vector pipes were MEASURED to issue on this part (64 independent v_fma_f32 x 2048 iterations x 5 waves per SIMD on
    every SIMD, tools/mfma_reduce_ab.hip), as tools/pmc.sh recorded it next to the counters of the same session -- read from the
    committed file, None when it is not there (round 4 carried the figure as a constant in this file, which goes stale silently)."""
    try:
        return float(json.load(open(TRAFFIC_JSON))["valu_measured_issue_rate"]["wave_instr_per_s"])
    except Exception:
        return None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scene-grid", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--quantize", action="store_true", help="run the compression-simulation hooks before each render")
    ap.add_argument("--quantize-reference-calls", action="store_true",
                    help="with --quantize: the reference trainer's exact call pattern (torch.exp / torch.sigmoid / torch.cat after the "
                         "hooks, simple_trainer.py:779-786) instead of the opt-in fused form (activate=True, colors=(sh0, shN))")
    ap.add_argument("--ada-mask", action="store_true",
                    help="with --quantize: the learnable shN mask of the reference's compression benchmark (--shN_ada_mask_opt, "
                         "examples/benchmarks/compression/mcmc_tt_sim.sh:31-33) active in the hooks")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything besides the headline: the cold-protocol region, the per-entry-point pass and the "
                         "roofline, repeated timed regions (--min-timed-s), the dense-gradient variants, the config-1 PSNR, the "
                         "multi-GPU projection and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed to DIR/<name>.npy (float32, at most 64 MiB; see dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-scene-grid", type=int, default=0,
                    help="scene_grid of the cpu_baseline sample (0 = the bench scene itself: ~3 s per pass on 128 threads)")
    ap.add_argument("--min-timed-s", type=float, default=0.5,
                    help="with --full: the exactly-K-step timed region is repeated until this much time has been measured")
    ap.add_argument("--ramp-s", type=float, default=0.6,
                    help="untimed back-to-back steps for this long right before the timed regions (GPU clocks reach their sustained level)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the dense-image-gradient variant and the config-1 PSNR")
    ap.add_argument("--breakdown", action="store_true", help="print per-entry-point timings to stderr")
    ap.add_argument("--dp-mode", choices=["auto", "camera", "camera_sparse", "gaussian", "gaussian_dense"], default="auto",
                    help="multi-GPU exchange pattern (see the module docstring); ignored with one GPU")
    ap.add_argument("--calib-steps", type=int, default=5)
    ap.add_argument("--dynamic", action="store_true",
                    help="BASELINE config 5's step instead of config 2's: 2 M dynamic (spacetime) splats, round-quantize hooks over the "
                         "17 floats -> temporal slice -> render -> backward (see main_dynamic)")
    ap.add_argument("--dynamic-splats", type=int, default=2_000_000)
    ap.add_argument("--dynamic-channels", type=int, choices=[3, 9], default=3,
                    help="3: the dyngs trainer's RGB render (simple_trainer_dyngs.py:519-520); 9: the spacetime trainer's feature render "
                         "cat(colors, features_dir, tau * features_time) (simple_trainer_STG.py:531-551)")
    ap.add_argument("--dynamic-form", choices=["reference", "activate", "fused", "full"], default="full",
                    help="reference: the trainer's own call pattern (hooks -> torch.exp / sigmoid -> temporal_slice -> rasterization); "
                         "activate: simulate_compression(activate=True); fused: + rasterization(dynamic=...), the slice inside the "
                         "projection kernels; full: dynamic.render_dynamic -- hooks, activations and slice inside the projection kernels")
    ap.add_argument("--timestamp", type=float, default=0.5)
    ap.add_argument("--dynamic-order", choices=["shuffle", "morton"], default="shuffle",
                    help="memory order of the dynamic splats: a seeded shuffle (default, what a trained scene looks like) or a Z-order curve")
    ap.add_argument("--no-dp-projection", action="store_true",
                    help="(one GPU, with --full) skip the multi-GPU projection: the exchange modes re-timed on this GPU with their collectives "
                         "forced through RCCL (world 1), next to the bytes a world-8 run would put on the xGMI links")
    return ap.parse_args()


class CallTimer:
    """Times C-ABI entry points with HIP events recorded on the stream the kernels are launched on."""

    def __init__(self, backend, only=None):
        self.B = backend
        self.only = only
        self.events = {}
        self._orig = backend.call

    def __enter__(self):
        def timed_call(name, *args):
            if self.only is not None and name not in self.only:
                return self._orig(name, *args)
            st = torch.cuda.current_stream()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            r = self._orig(name, *args)
            e1.record(st)
            self.events.setdefault(name, []).append((e0, e1))
            return r

        self.B.call = timed_call
        # the operator modules hold a reference to the module, not the function, so patching
        # the attribute is enough
        return self

    def __exit__(self, *a):
        self.B.call = self._orig

    def totals_ms(self):
        torch.cuda.synchronize()
        return {k: [a.elapsed_time(b) for a, b in v] for k, v in self.events.items()}


DUMP_IMAGE_BYTES = 24 * 2**20  # a larger image is written as a seeded sample of its pixels, [n, channels]
DUMP_SPLAT_ROWS = 1 << 15      # per-splat arrays: a seeded sample of this many splats (the same rows in every array)
DUMP_LIMIT_BYTES = 64 * 2**20


def _seeded_rows(n, k, seed):
    if n <= k:
        return None
    return torch.from_numpy(np.sort(np.random.RandomState(seed).choice(n, k, replace=False)))


def dump_outputs(out_dir, images, per_splat):
    """--dump-outputs: what the last timed step handed its caller, as out_dir/<name>.npy in float32 (float64 stays float64).
    images: name -> [..., channels] tensor, written whole up to DUMP_IMAGE_BYTES, else as a seeded sample of its pixels.
    per_splat: name -> (tensor, splat axis), written as the DUMP_SPLAT_ROWS seeded splat rows along that axis.  The inputs of
    the bench are seeded too, so two builds run with the same arguments can be compared file by file."""
    arrays = {}
    for name, t in images.items():
        t = t.detach()
        if t.numel() * 4 > DUMP_IMAGE_BYTES:
            t = t.reshape(-1, t.shape[-1])
            t = t[_seeded_rows(t.shape[0], DUMP_IMAGE_BYTES // (4 * t.shape[-1]), 1).to(t.device)]
        arrays[name] = t
    for name, (t, axis) in per_splat.items():
        rows = _seeded_rows(t.shape[axis], DUMP_SPLAT_ROWS, 2)
        arrays[name] = t.detach() if rows is None else t.detach().index_select(axis, rows.to(t.device))
    arrays = {k: (v if v.dtype == torch.float64 else v.float()).cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, f"--dump-outputs: {total} bytes > {DUMP_LIMIT_BYTES}"
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)


def splat_outputs(params, meta):
    """The per-splat arrays a step hands its caller, for dump_outputs: the parameter gradients and the projection's radii,
    means2d, depths and conics.  The projection leaves the last three unwritten for culled splats (radius 0): zeroed here, so
    that only values the step computed are compared."""
    out = {f"{k}_grad": (p.grad, 0) for k, p in params.items() if p.grad is not None}
    radii = meta["radii"]
    out["radii"] = (radii, 1)
    for k in ("means2d", "depths", "conics"):
        t = meta[k].detach()
        if t.shape[:radii.dim()] == radii.shape:
            vis = (radii > 0).reshape(radii.shape + (1,) * (t.dim() - radii.dim()))
            out[k] = (torch.where(vis, t, torch.zeros((), dtype=t.dtype, device=t.device)), 1)
    return out


def algorithmic_bytes(stats):
    """Compulsory HBM bytes per launch of each entry point."""
    N, V, I, P, T, K = (stats[k] for k in ("N", "V", "I", "P", "T", "K"))
    return {
        "gs_projection_fwd": 40 * N + 4 * N + 24 * V,
        "gs_projection_rows_fwd": 40 * N + 4 * N + 24 * V + ((12 + 12 * K) * V + 12 * V if K > 0 else 0),  # (+ the SH colours)
        "gs_projection_rows_bwd": 92 * V + 40 * N + 4 * N + ((24 + 12 * K) * V + 12 * K * N if K > 0 else 0),  # (+ the SH backward)
        "gs_sh_fwd": (12 + 12 * K) * V + 12 * V,
        "gs_sh_view_fwd": (12 + 12 * K) * V + 12 * V + 4 * N,
        "gs_sh_view_bwd": (24 + 12 * K) * V + 12 * K * N + 12 * V + 12 * N,
        "gs_isect_depth_keys": 8 * N + 12 * N,
        "gs_gather_i32": 12 * N,
        "gs_isect_count": 12 * N + 4 * N,
        "gs_isect_count_keys": 16 * N + 4 * N + 12 * N,
        "gs_cumsum_gather_i32": 8 * N + 8 * N,
        "gs_cumsum_i32": 4 * N + 8 * N,
        "gs_isect_emit": 24 * V + 12 * I,
        "gs_isect_emit_compact": 24 * V + 12 * I,
        "gs_sort_pairs_u64_i32_drop": 24 * V,   # the splat-level depth pre-sort: one read + one write of the live keys
        "gs_presort_split": 0,                  # (16 K sampled elements)
        "gs_presort_buckets": 24 * V,           # the same pre-sort, bucketed: partition pass + local sorts
        "gs_sort_isect_pairs": 24 * I,
        "gs_sort_pairs_u64_i32": 24 * I,
        "gs_isect_offset_encode": 8 * I + 4 * T,
        "gs_isect_finish_presorted": (24 * V + 12 * I) + 24 * I + (8 * I + 4 * T),  # emit + pair sort + offsets in one call
        "gs_rasterize_fwd": 40 * I + 20 * P,
        "gs_rasterize_bwd": 40 * I + 24 * P + 36 * V,
        "gs_sh_bwd": (24 + 12 * K) * V + 12 * K * N + 12 * V,
        "gs_projection_bwd": 92 * V + 40 * N + 4 * N,
        # the compression-simulation hooks of config 3 (quats 4 + scales 3 + opacities 1 + sh0 3 floats per splat): SURVEY 8(d)'s
        # 8 A bytes per splat forward (x read, y written), 12 A backward (v_y + x read, v_x written)
        "gs_quantize_noise_multi_fwd": 8 * 11 * N,
        "gs_quantize_noise_multi_bwd": 12 * 11 * N,
    }


def cpu_baseline(args, sh_degree):
    """Oracle fwd+bwd on a bounded sample; returns the cpu_baseline object."""
    from gscodec_studio_amd._helper import sh_workload
    from oracle import gs_oracle as O

    grid = args.cpu_scene_grid or args.scene_grid
    w = sh_workload(scene_grid=grid, width=args.width, height=args.height, n_cameras=1,
                    sh_degree=sh_degree, device="cpu")
    a = {k: w[k].numpy() for k in ("means", "quats", "scales", "opacities", "sh", "viewmats", "Ks")}
    W, H = w["width"], w["height"]

    def one_pass():
        t0 = time.perf_counter()
        rc, ra, m = O.rasterization(a["means"], a["quats"], a["scales"], a["opacities"], a["sh"], a["viewmats"], a["Ks"],
                                    W, H, sh_degree=sh_degree)
        v_rc = np.ones_like(rc)
        v_m2, v_cn, v_col, v_op, _ = O.rasterize_bwd(m["means2d"], m["conics"], m["colors"], m["opacities"], W, H, 16,
                                                     m["isect_offsets"], m["flatten_ids"], ra, m["last_ids"], v_rc,
                                                     np.zeros_like(ra))
        c2w = np.linalg.inv(a["viewmats"].astype(np.float64)).astype(np.float32)
        dirs = a["means"][None] - c2w[:, None, :3, 3]
        O.sh_bwd(sh_degree, dirs, a["sh"][None], v_col, m["radii"] > 0)
        O.projection_bwd(a["means"], None, a["quats"], a["scales"], a["viewmats"], a["Ks"], W, H, 0.3, "pinhole",
                         m["radii"], m["conics"], None, v_m2, np.zeros_like(m["depths"]), v_cn, None, need_viewmats=False)
        return time.perf_counter() - t0

    n = a["means"].shape[0]
    one_pass()  # warm-up (page faults, OpenMP thread start)
    runs = sorted(one_pass() for _ in range(3))
    dt = runs[1]  # median of 3
    how = ("the bench workload itself (same scene, camera, resolution)" if grid == args.scene_grid else
           f"scene_grid={grid}: 1/{args.scene_grid ** 2 // grid ** 2} of the bench scene, same camera and resolution")
    how += "; 1 warm-up + 3 runs, median"
    return {
        "value": n / dt / 1e6, "unit": "Msplats/s", "cores": int(O.lib().orc_num_threads()), "kind": "port",
        "sample": f"oracle/gs_oracle.c fwd+bwd (C restatement of the reference's path, OpenMP), {n} gaussians, {W}x{H}, "
                  f"SH deg {sh_degree}; {how}: {dt:.1f} s wall",
        "host_cpus": os.cpu_count(),
    }


def dp_projection(args, t1_ms, stats):
    """What can be said about N = 8 from ONE GPU (the build rounds have no multi-GPU box): every exchange mode is re-run in a
    subprocess on this GPU with world 1 and its collectives FORCED through RCCL (GS_DIST_FORCE_COLLECTIVES=1: compaction, row
    gathers / scatters, plan and reduce kernels and RCCL's self-copies all run; nothing crosses a link), which gives the mode's
    LOCAL overhead per step -- conservatively: RCCL copying the whole payload to itself is counted as local work, although at
    world 8 seven eighths of it would be on the wire instead.  Next to it the payload a rank would put on the wire at world 8
    with one camera per rank (closed form from N / V, union of the visible sets taken as V: the bench cameras are yawed copies
    of camera 0) and the time the 7 xGMI links of an MI355X need for it at peak.
    implied_efficiency = t1 / (t1 + local overhead + wire floor): links at peak, nothing overlapped."""
    import subprocess

    N, V = stats["N"], stats["V"]
    D = 59  # floats of one degree-3 gradient row: means 3 + quats 4 + scales 3 + opacity 1 + SH 48
    wire8 = {
        "camera": 2 * (7 / 8) * 4 * D * N,                 # reduce-scatter + all-gather of every gradient tensor
        "camera_sparse": (7 / 8) * 4 * (D + 1) * (V + V),   # visible rows to their owners + the union rows back (index column)
        "gaussian": (7 / 8) * V * (52 + 44),               # projected visible rows out, their gradients back
    }
    out = {}
    for mode in ("camera", "camera_sparse", "gaussian"):
        env = dict(os.environ, GS_BENCH_PG="1", GS_DIST_FORCE_COLLECTIVES="1", MASTER_PORT=str(29600 + (os.getpid() % 300)))
        cmd = [sys.executable, os.path.abspath(__file__), "--full", "--gpus", "1", "--dp-mode", mode, "--steps", "20", "--warmup", "5",
               "--min-timed-s", "0.3", "--no-cpu-baseline", "--no-extras", "--no-dp-projection", "--scene-grid", str(args.scene_grid),
               "--width", str(args.width), "--height", str(args.height), "--sh-degree", str(args.sh_degree)]
        rec = {"wire_bytes_out_per_rank_world8": wire8[mode], "xgmi_floor_ms": wire8[mode] / (7 * 153e9) * 1e3}
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=180)
            ms = json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]
            rec["ms_per_step_world1_forced_collectives"] = ms
            rec["local_overhead_ms"] = max(ms - t1_ms, 0.0)
            rec["implied_efficiency_world8"] = t1_ms / (t1_ms + rec["local_overhead_ms"] + rec["xgmi_floor_ms"])
            rec["implied_speedup_world8"] = 8 * rec["implied_efficiency_world8"]
            if mode == "gaussian":
                # this mode is bound by HOST work and follows whatever else runs on the box (0.70 ... 0.79 from run to run): two
                # more runs, and the spread next to the first run's figure -- interference only ever slows a run down, so the
                # fastest of the three is the least disturbed one
                runs = [ms]
                for _ in range(2):
                    r2 = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=180)
                    runs.append(json.loads(r2.stdout.strip().splitlines()[-1])["ms_per_step"])
                best = min(runs)
                rec["ms_per_step_runs"] = runs
                rec["implied_efficiency_world8_least_disturbed_run"] = t1_ms / (t1_ms + max(best - t1_ms, 0.0) + rec["xgmi_floor_ms"])
        except Exception as e:  # (a projection must never take the measurement down with it)
            rec["error"] = f"{type(e).__name__}: {e}"[:200]
        out[mode] = rec
    return out


def psnr_vs_oracle(dev):
    """BASELINE config 1 (the reference's own CPU-runnable case): garden crop, 111,785 gaussians, camera 0, 648x420, RGB --
    PSNR of the GPU render against the CPU oracle's render of the same splats (peak 1.0)."""
    from gscodec_studio_amd import rasterization
    from gscodec_studio_amd._helper import load_test_data
    from oracle import gs_oracle as O

    means, quats, scales, opac, rgb, viewmats, Ks, W, H = load_test_data(device=dev, scene_grid=1)
    with torch.no_grad():
        rc, _, _ = rasterization(means, quats, scales, opac, rgb, viewmats[:1], Ks[:1], W, H, packed=False)
    c = lambda t: t.detach().cpu().numpy()  # noqa: E731
    o_rc, _, _ = O.rasterization(c(means), c(quats), c(scales), c(opac), c(rgb), c(viewmats[:1]), c(Ks[:1]), W, H)
    mse = float(np.mean((c(rc).astype(np.float64) - o_rc.astype(np.float64)) ** 2))
    return {"db": (10 * np.log10(1.0 / mse)) if mse > 0 else float("inf"), "mse": mse,
            "config": f"config 1: garden crop {means.shape[0]} gaussians, camera 0, {W}x{H}, RGB, GPU render vs CPU oracle render"}


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it (no WORLD_SIZE in the environment): start the N ranks
    here, one process per GPU, with the environment torch.distributed.run would give them (RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_ADDR=127.0.0.1 / MASTER_PORT) -- the reference's harness launches itself the same way (profiling/main.py:370 ->
    gsplat/distributed.py:304-360).  Rank 0 inherits this process's stdout, so its JSON line is the last line of stdout; the
    other ranks' stdout goes to stderr.  Any rank dying takes the others down and the exit code is non-zero.  Fewer visible
    GPUs than ranks is refused unless GS_BENCH_SHARE_GPU=1 (all ranks on cuda:0 over gloo: control flow only, not a speed)."""
    import signal
    import subprocess

    from gscodec_studio_amd.distributed import _find_free_port

    n = args.gpus
    share = os.environ.get("GS_BENCH_SHARE_GPU") == "1"
    n_dev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if n_dev < n and not share:
        print(f"bench.py: --gpus {n} needs {n} visible GPUs, found {n_dev} (set GS_BENCH_SHARE_GPU=1 to run all ranks on one "
              f"GPU over gloo: control flow only)", file=sys.stderr)
        return 2
    # The exchange patterns of --dp-mode auto were only ever exercised on one GPU (no multi-GPU box in the build rounds): should
    # the calibrated run fail on real links, ONE retry with the plainest pattern (camera-sharded, dense reduce-scatter +
    # all-gather of the gradients) still yields a measured line; it says so ("launch_fallback" in the JSON's config).
    rc = _launch_once(args, n, sys.argv[1:], {})
    if rc != 0 and args.dp_mode == "auto" and os.environ.get("GS_BENCH_NO_FALLBACK") != "1":
        print(f"bench.py: the --dp-mode auto run failed (rc {rc}); retrying once with --dp-mode camera", file=sys.stderr)
        rc = _launch_once(args, n, sys.argv[1:] + ["--dp-mode", "camera"], {"GS_BENCH_LAUNCH_FALLBACK": f"auto failed with rc {rc}"})
    return rc


def _launch_once(args, n, argv, extra_env):
    import signal
    import subprocess

    from gscodec_studio_amd.distributed import _find_free_port

    port = os.environ.get("MASTER_PORT") or str(_find_free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port, GS_BENCH_SELF_LAUNCHED="1", **extra_env)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=None if r == 0 else sys.stderr, start_new_session=True))
    rc = 0
    try:
        live = set(range(n))
        while live:
            for r in sorted(live):
                c = procs[r].poll()
                if c is None:
                    continue
                live.discard(r)
                if c != 0 and rc == 0:
                    rc = c if c > 0 else 128 - c
                    print(f"bench.py: rank {r} exited with {c}; stopping the other ranks", file=sys.stderr)
                    for q in live:  # (exactly the process groups started above)
                        try:
                            os.killpg(procs[q].pid, signal.SIGTERM)
                        except ProcessLookupError:
                            pass
            time.sleep(0.05)
    except KeyboardInterrupt:
        for q in procs:
            if q.poll() is None:
                os.killpg(q.pid, signal.SIGTERM)
        rc = 130
    return rc


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE config 5: one frame of the dynamic-splat trainer's step
DYN_QUANT_FLOATS = 17  # scales 3 + quats 4 + opacities 1 + colors 3 + features_dir 3 + features_time 3


def dynamic_algorithmic_bytes(N, V, I, P, T, D, A_hooks=DYN_QUANT_FLOATS):
    """Compulsory HBM bytes per launch of the entry points of config 5's step.  D = render channels."""
    proj_f = 40 * N + 4 * N + 24 * V + 4 * D * V            # SURVEY 8(d) projection + the colour columns of the visible rows
    proj_b = 92 * V + 40 * N + 4 * N + 4 * D * V
    slice_f, slice_b = 128 * N, 216 * N                     # csrc/dynamic.hip: 92 B in + 36 B out | 92 + 32 B in + 92 B out
    return {
        "gs_quantize_round_fwd": 8 * DYN_QUANT_FLOATS * N,  # 8 A bytes per splat (all six hooked tensors together)
        "gs_quantize_round_multi_fwd": 8 * A_hooks * N,     # (the hooks that run OUTSIDE the projection kernel, one launch)
        "gs_temporal_slice_fwd": slice_f, "gs_temporal_slice_bwd": slice_b,
        "gs_projection_rows_fwd": proj_f, "gs_projection_rows_bwd": proj_b,
        # fused: the projection reads the RAW rows itself -- means 12 + motion 36 + quats 16 + omega 16 + scales 12 + opacity 4 + trbf
        # centre / scale 8 (+ colours 4 D when they ride in the rows) per splat -- and writes radii + tile counts (8 N) and the visible
        # rows (64 + 4 V); its backward reads radii (4 N) and, for the V visible gaussians, the same inputs, the splat and gradient rows
        # (128) and writes the 23 (+ D) gradient floats
        "gs_projection_rows_dyn_fwd": (104 + (4 * D if D == 3 else 0)) * N + 8 * N + 68 * V,
        "gs_projection_rows_dyn_bwd": 4 * N + (104 + 128 + 92 + (8 * D if D == 3 else 0)) * V,
        "gs_rasterize_fwd": (28 + 4 * D) * I + (4 * D + 8) * P,   # 40 I + 20 P at D = 3
        "gs_rasterize_bwd": (28 + 4 * D) * I + (4 * D + 12) * P + (24 + 4 * D) * V,
        "gs_isect_finish_presorted": (24 * V + 12 * I) + 24 * I + (8 * I + 4 * T),
        "gs_presort_buckets": 24 * V, "gs_isect_count_keys": 16 * N + 4 * N + 12 * N, "gs_presort_split": 0,
    }


def main_dynamic(args):
    """`bench.py --dynamic`: BASELINE config 5's step on one frame -- N = 2 M dynamic splats, one 1080p camera:
    STGCompressionSimulation("round") hooks over the 17 hooked floats (reference simulation.py:508-780) -> activations ->
    temporal slice at a timestamp (simple_trainer_dyngs.py:506-521) -> rasterization -> backward of sum(render).
    --gpus N: frames round-robin, rank r renders its own timestamp of the same splats; the step ends with the RCCL sum of the
    parameter gradients (weak scaling over frames, value = N_splats x frames / step time)."""
    world, rank, use_pg, dev = init_ranks(args)
    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd import rasterization
    from gscodec_studio_amd._helper import DYNAMIC_KEYS, dynamic_workload
    from gscodec_studio_amd.compression_simulation import STGCompressionSimulation
    from gscodec_studio_amd.distributed import all_reduce_splat_grads
    from gscodec_studio_amd.dynamic import render_dynamic, temporal_slice

    B.lib()
    gc.collect()
    gc.freeze()  # (see main())
    w = dynamic_workload(args.dynamic_splats, args.width, args.height, device=dev, order=args.dynamic_order)
    N, W_, H_ = w["N"], w["width"], w["height"]
    viewmats, Ks = w["viewmats"], w["Ks"]
    params = {k: w[k].clone().requires_grad_(True) for k in DYNAMIC_KEYS}
    sim = STGCompressionSimulation(quantization_sim_type="round", entropy_steps={}, device=dev)
    t_frame = (args.timestamp + 0.37 * rank) % 1.0
    D = args.dynamic_channels
    form = args.dynamic_form
    last_meta = {}
    last_out = {}  # (--dump-outputs) the render of the last step

    def features(q, tau):
        if D == 3:
            return q["colors"]                                                              # simple_trainer_dyngs.py:519-520
        return torch.cat((q["colors"], q["features_dir"], tau * q["features_time"]), dim=1)  # simple_trainer_STG.py:531

    def step():
        for p in params.values():
            p.grad = None
        if form == "full":
            rc, ra, meta = render_dynamic(params, t_frame, viewmats, Ks, W_, H_, compression_sim=sim, step=1,
                                          features="colors" if D == 3 else "stg", packed=False)
            rc.sum().backward()
            if use_pg:
                all_reduce_splat_grads(params, world_size=world, average=False)
            last_meta.update(meta)
            if args.dump_outputs:
                last_out.update(render_colors=rc, render_alphas=ra)
            return
        if form == "reference":
            q, _ = sim.simulate_compression(params, step=1)
            scales, opac, tscale = torch.exp(q["scales"]), torch.sigmoid(q["opacities"]), torch.exp(q["trbf_scale"])
        else:
            q, _ = sim.simulate_compression(params, step=1, activate=True)
            scales, opac, tscale = q["scales"], q["opacities"], torch.exp(q["trbf_scale"])
        tau = (t_frame - q["trbf_center"]).detach() if D == 9 else None
        if form == "fused":
            rc, ra, meta = rasterization(q["means"], q["quats"], scales, opac, features(q, tau), viewmats, Ks, W_, H_, packed=False,
                                         dynamic=(q["motion"], q["omega"], q["trbf_center"], tscale, t_frame))
        else:
            means_t, quats_t, opac_t, _ = temporal_slice(q["means"], q["motion"], q["quats"], q["omega"], opac, q["trbf_center"], tscale,
                                                         t_frame)
            rc, ra, meta = rasterization(means_t, quats_t, scales, opac_t, features(q, tau), viewmats, Ks, W_, H_, packed=False)
        rc.sum().backward()
        if use_pg:
            all_reduce_splat_grads(params, world_size=world, average=False)
        last_meta.update(meta)
        if args.dump_outputs:
            last_out.update(render_colors=rc, render_alphas=ra)

    def max_over_ranks(x):
        if not use_pg:
            return float(x)
        t = torch.tensor([x], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def barrier():
        if use_pg:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    from gscodec_studio_amd import _step
    step_driver_on = _step.ENABLED
    if args.full:
        # pass A (untimed): every C-ABI entry point with events, on the operator path (see main())
        _step.ENABLED = False
        for _ in range(2):
            step()
        with CallTimer(B) as ct:
            for _ in range(2):
                step()
        _step.ENABLED = step_driver_on
        for _ in range(2):
            step()
        per_call = {k: float(np.mean(v)) for k, v in ct.totals_ms().items()}
        calls_per_step = {k: len(v) / 2 for k, v in ct.events.items()}
        per_step = {k: per_call[k] * calls_per_step[k] for k in per_call}
        dominant = max((k for k in per_step if not k.startswith("gs_step_")), key=per_step.get)

    def timed_region(n_steps, timer_only=None):
        barrier()
        with (CallTimer(B, only=timer_only) if timer_only is not None else contextlib.nullcontext()) as ct_:
            t0_ = time.perf_counter()
            for _ in range(n_steps):
                step()
            barrier()
            t1_ = time.perf_counter()
        return max_over_ranks(t1_ - t0_), ct_

    gc.collect()
    gc.disable()
    if args.ramp_s > 0:
        barrier()
        t0 = time.perf_counter()
        for _ in range(5):
            step()
        barrier()
        for _ in range(int(min(5000, args.ramp_s / max(max_over_ranks(time.perf_counter() - t0) / 5, 1e-5)))):
            step()
    torch.cuda.reset_peak_memory_stats(dev)
    elapsed, ct = timed_region(args.steps, {dominant} if args.full else None)
    peak_mem = torch.cuda.max_memory_allocated(dev)
    regions = [elapsed]
    if args.full:
        dom_all = list(ct.totals_ms().get(dominant, ())) or [per_call[dominant]]
        for _ in range(int(min(200, max(0, np.ceil(args.min_timed_s / max(elapsed, 1e-6)) - 1)))):
            regions.append(timed_region(args.steps, set())[0])
        dom_ms = float(np.mean(dom_all))
    gc.enable()
    ms_per_step = sum(regions) / (len(regions) * args.steps) * 1e3
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_out, splat_outputs(params, last_meta))

    if rank == 0:
        meta = last_meta
        V, I = int((meta["radii"] > 0).sum()), int(meta["flatten_ids"].numel())
        P, T = W_ * H_, meta["tile_width"] * meta["tile_height"]
        out = {
            "metric": "Msplats/s fwd+bwd @1080p (2M dynamic splats, config 5 step)",
            "value": N * world / (ms_per_step * 1e-3) / 1e6, "unit": "Msplats/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "timed": {"regions": len(regions), "steps_per_region": args.steps, "total_s": sum(regions), "untimed_ramp_s": args.ramp_s,
                      "ms_per_step_min_region": min(regions) / args.steps * 1e3, "ms_per_step_max_region": max(regions) / args.steps * 1e3},
            "peak_mem_gb": peak_mem / 2**30,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {
                "workload": f"BASELINE config 5, one frame per step: {N} dynamic gaussians (load_test_data grid {w['scene_grid']}, seeded shuffle, "
                            f"synthetic motion / omega / trbf), STGCompressionSimulation('round') hooks over {DYN_QUANT_FLOATS} floats -> "
                            f"temporal slice at t = {t_frame:.2f} -> rasterization([N, {D}]) {world}x1 camera {W_}x{H_}, packed=False, tile 16 "
                            f"-> backward of sum(render)",
                "form": {"reference": "the trainer's call pattern: hooks, torch.exp / sigmoid, temporal_slice(), rasterization()",
                         "activate": "simulate_compression(activate=True), temporal_slice(), rasterization()",
                         "fused": "simulate_compression(activate=True), rasterization(dynamic=...): the slice inside the projection kernels",
                         "full": "dynamic.render_dynamic(raw parameters, sim): round hooks, activations and slice inside the projection kernels "
                                 "(rasterization(dynamic=DynamicSlice(raw=..., quantize=...)))"}[form],
                "visible": V, "n_isects": I, "channels": D, "native_step_driver": bool(step_driver_on), "splat_order": w["order"],
                "parallelism": f"frames round-robin over {world} rank(s)" + (", RCCL sum of the parameter gradients" if world > 1 else ""),
            },
        }
        if args.full:
            # floats per splat the hooks quantize outside the projection kernel: all 17, or -- form "full" -- what the kernel does not take
            A_hooks = DYN_QUANT_FLOATS if form != "full" else (6 if D == 3 else 9)
            alg = dynamic_algorithmic_bytes(N, V, I, P, T, D, A_hooks)
            dyn_key = f"dynamic_{N}_{W_}x{H_}_ch{D}_{form}"
            # whole step: SURVEY 8(d)'s closed form with the [N, D] colours in place of the SH rows, plus the hooks (8 A each way is the
            # survey's figure; the round STE's backward is the identity: 0) and the slice both ways
            total_alg = (alg["gs_quantize_round_fwd"] + alg["gs_temporal_slice_fwd"] + alg["gs_projection_rows_fwd"]
                         + (32 * V + 4 * N + 12 * I) + 24 * I + (8 * I + 4 * T) + alg["gs_rasterize_fwd"]
                         + alg["gs_rasterize_bwd"] + alg["gs_projection_rows_bwd"] + alg["gs_temporal_slice_bwd"])
            achieved = alg.get(dominant, 0) / (dom_ms * 1e-3) / 1e9
            gpu_entry_ms = sum(per_step.values())
            out["roofline"] = {
                "bound": "hbm", "kernel": dominant, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                "traffic": measured_pmc(dominant, dyn_key, path=TRAFFIC_JSON_DYNAMIC, wide=D > 4), "kernel_ms": dom_ms,
                "algorithmic_bytes": alg.get(dominant, 0),
                "own_bound": "valu" if dominant in ("gs_rasterize_bwd", "gs_rasterize_fwd") else "hbm",
                "whole_step": {"algorithmic_bytes": total_alg, "achieved": total_alg / (ms_per_step * 1e-3) / 1e9,
                               "frac": total_alg / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                               "formula": "hooks 8*17 N + slice (128 + 216) N + SURVEY 8(d) with [N, D] colours"},
                "per_entry_point_ms": {k: round(v, 4) for k, v in sorted(per_step.items(), key=lambda kv: -kv[1])},
                "entry_points_ms": gpu_entry_ms,
                # what the step spends OUTSIDE the C-ABI entry points (torch's own kernels: `p + 0.` copies of the un-hooked parameters,
                # exp / sigmoid, cat, sum, gradient accumulation) when the GPU is the bound: step time - entry-point time
                "outside_entry_points_ms": ms_per_step - gpu_entry_ms,
                "streaming": {k: {"ms": round(per_step[k], 4), "calls_per_step": calls_per_step[k], "algorithmic_bytes": alg[k],
                                  "achieved": alg[k] / (per_step[k] * 1e-3) / 1e9, "unit": "GB/s",
                                  "frac": alg[k] / (per_step[k] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                  "frac_of_measured_copy_rate": alg[k] / (per_step[k] * 1e-3) / 1e9 / HBM_COPY_GBS,
                                  # HBM bytes per launch from the committed counter passes (None: not collected / sources changed)
                                  "traffic": measured_pmc(k, dyn_key, path=TRAFFIC_JSON_DYNAMIC)}
                              for k in ("gs_quantize_round_fwd", "gs_quantize_round_multi_fwd", "gs_temporal_slice_fwd", "gs_temporal_slice_bwd", "gs_projection_rows_fwd",
                                        "gs_projection_rows_bwd", "gs_projection_rows_dyn_fwd", "gs_projection_rows_dyn_bwd")
                              if k in per_step and per_step[k] > 0},
            }
    if use_pg:
        dist.barrier()
        dist.destroy_process_group()
    import ctypes
    ctypes.CDLL(None).fflush(None)
    if rank == 0:
        sys.stdout.flush()
        print(json.dumps(out), flush=True)


def init_ranks(args, force_pg=False):
    """One process per GPU: rank / world from the launcher's environment, the process group (RCCL; gloo with GS_BENCH_SHARE_GPU=1)
    -> (world, rank, use_pg, dev)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if (os.environ.get("GS_BENCH_TEST_KILL_RANK") == str(rank) and world > 1 and
            (os.environ.get("GS_BENCH_TEST_KILL_ALWAYS") == "1" or not os.environ.get("GS_BENCH_LAUNCH_FALLBACK"))):
        sys.exit(17)  # (tests/test_gpu_bench_launch.py: a rank that dies -- in the first attempt only, or in every attempt)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # GS_BENCH_PG=1 / a forced mode: one GPU still goes through the process group and RCCL (debugging aid)
    use_pg = world > 1 or force_pg or os.environ.get("GS_BENCH_PG") == "1"
    if use_pg:
        import datetime

        # a collective that never completes (mismatched call sequences on real links) ends the rank after this long instead
        # of the default 10 minutes; the launcher then stops the others and falls back (self_launch)
        pg_timeout = datetime.timedelta(seconds=int(os.environ.get("GS_BENCH_PG_TIMEOUT_S", "300")))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")  # one node by contract; the host name may not resolve
        if os.environ.get("GS_BENCH_SHARE_GPU") == "1":
            # debugging aid for 1-GPU boxes: all ranks on cuda:0, exchanges through host memory on gloo (RCCL refuses two
            # ranks on one device) -- exercises the N > 1 control flow, says nothing about its speed
            local_rank = 0
            torch.cuda.set_device(0)
            dist.init_process_group(backend="gloo", world_size=world, rank=rank, timeout=pg_timeout)
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="nccl", world_size=world, rank=rank, timeout=pg_timeout,
                                    device_id=torch.device("cuda", local_rank))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world} (launch with torch.distributed.run)"
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    return world, rank, use_pg, dev


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    if args.dynamic:
        return main_dynamic(args)
    world, rank, use_pg, dev = init_ranks(args, force_pg=args.dp_mode.startswith("gaussian"))

    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd import rasterization
    from gscodec_studio_amd._helper import sh_workload
    from gscodec_studio_amd import distributed as D
    from gscodec_studio_amd.distributed import all_reduce_splat_grads, plan_sparse_grad_exchange

    B.lib()  # fail loudly if the HIP library is missing
    # everything imported so far goes to the permanent generation: a full collection over it is 30-50 ms, and the untimed calibration
    # and the cold-protocol region below run with the collector on (the headline regions park it altogether)
    gc.collect()
    gc.freeze()
    w = sh_workload(scene_grid=args.scene_grid, width=args.width, height=args.height, n_cameras=world,
                    sh_degree=args.sh_degree, device=dev, camera_mode="jitter0")  # equal work per rank (weak scaling)
    N = w["N"]
    names = ("means", "quats", "scales", "opacities", "sh")
    viewmats, Ks = w["viewmats"][rank: rank + 1].contiguous(), w["Ks"][rank: rank + 1].contiguous()
    sim = None
    if args.quantize:
        from gscodec_studio_amd.compression_simulation import CompressionSimulation

        sim = CompressionSimulation(entropy_model_enable=False, entropy_steps={}, device=dev, ada_mask_opt=args.ada_mask, ada_mask_step=0,
                                    cap_max=N)

    last_meta = {}
    last_out = {}  # (--dump-outputs) the render of the last step
    dense_grad = [None]  # set to a dense tensor of ones for the dense-image-gradient variant

    def make_step(mode):
        """One fwd+bwd pass (+ the mode's exchange).  `camera`: all splats on every rank; `gaussian`: a contiguous
        1/world slice of the same scene on every rank."""
        gaussian = mode.startswith("gaussian")
        if gaussian:
            # "gaussian": only the rows of visible splats travel; "gaussian_dense": every (camera, gaussian) row
            os.environ["GS_DIST_SPARSE"] = "0" if mode == "gaussian_dense" else "1"
            lo, hi = rank * N // world, (rank + 1) * N // world
            params = {k: w[k][lo:hi].clone().requires_grad_(True) for k in names}
        else:
            params = {k: w[k].clone().requires_grad_(True) for k in names}

        if sim is not None:
            # the hooks work on the trainer's RAW parameters (reference simple_trainer.py:779-800): log-scales, opacity
            # logits, sh0 / shN; the activations follow the hooks
            with torch.no_grad():
                params["scales"] = params["scales"].log().requires_grad_(True)
                params["opacities"] = torch.logit(params["opacities"].clamp(1e-6, 1 - 1e-6)).requires_grad_(True)
                params["sh0"] = params["sh"][:, :1, :].clone().requires_grad_(True)
                params["shN"] = params["sh"][:, 1:, :].clone().requires_grad_(True)
                del params["sh"]

        def step():
            for p in params.values():
                p.grad = None
            if sim is not None and args.quantize_reference_calls:
                q, _ = sim.simulate_compression({k: params[k] for k in ("scales", "quats", "opacities", "sh0", "shN")}, step=1)
                quats, scales, opac = q["quats"], torch.exp(q["scales"]), torch.sigmoid(q["opacities"])
                sh = torch.cat([q["sh0"], q["shN"]], dim=1)
            elif sim is not None:
                # the opt-in fused form: activations inside the quantizer kernels, sh0 / shN handed over as they are
                q, _ = sim.simulate_compression({k: params[k] for k in ("scales", "quats", "opacities", "sh0", "shN")}, step=1,
                                                activate=True)
                quats, scales, opac, sh = q["quats"], q["scales"], q["opacities"], (q["sh0"], q["shN"])
            else:
                quats, scales, opac, sh = params["quats"], params["scales"], params["opacities"], params["sh"]
            rc, ra, meta = rasterization(params["means"], quats, scales, opac, sh, viewmats, Ks,
                                         w["width"], w["height"], sh_degree=args.sh_degree, packed=False,
                                         distributed=gaussian)
            plan = plan_sparse_grad_exchange(meta["radii"], world) if (mode == "camera_sparse" and use_pg) else None
            if dense_grad[0] is None:
                rc.sum().backward()  # the reference's timing protocol (profiling/main.py:125-133): a broadcast gradient of ones
            elif isinstance(dense_grad[0], str):  # "expanded-one"
                # what the reference's timed backward() actually contains: loss = render.sum() is evaluated ONCE, outside
                # its timers; loss.backward() then creates a one-element gradient and expands it
                rc.backward(gradient=torch.ones((), dtype=rc.dtype, device=rc.device).expand_as(rc))
            else:
                rc.backward(gradient=dense_grad[0])  # a training loss hands the compositing backward a DENSE [C,H,W,3] gradient
            if mode in ("camera", "camera_sparse") and use_pg:
                all_reduce_splat_grads(params, world_size=world, average=False, plan=plan)
            last_meta.update(meta)
            if args.dump_outputs:
                last_out.update(render_colors=rc, render_alphas=ra)

        step.params = params
        return step

    def max_over_ranks(x):
        if not use_pg:
            return float(x)
        t = torch.tensor([x], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def barrier():
        if use_pg:
            dist.barrier()
        torch.cuda.synchronize()

    # multi-GPU: pick the exchange pattern (untimed calibration; every rank sees the same max-over-ranks numbers)
    mode, calib = ("camera" if args.dp_mode == "auto" else args.dp_mode), {}
    if use_pg and args.dp_mode == "auto":
        for m in ("camera", "camera_sparse", "gaussian", "gaussian_dense"):
            st = make_step(m)
            for _ in range(2):
                st()
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.calib_steps):
                st()
            barrier()
            calib[m] = max_over_ranks((time.perf_counter() - t0) / args.calib_steps * 1e3)
            del st
            torch.cuda.empty_cache()
        mode = min(calib, key=calib.get)
    step = make_step(mode)

    for _ in range(args.warmup):
        step()
    barrier()
    if args.full:
        # the protocol as the reference runs it (profiling/main.py:28-37): W warm-up steps, then K steps between synchronisations -- no
        # ramp, no repetitions.  Reported as ms_per_step_cold_protocol next to the headline (which is taken at sustained clocks, below)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        cold_ms = max_over_ranks(time.perf_counter() - t0) / args.steps * 1e3

    from gscodec_studio_amd import _step
    step_driver_on = _step.ENABLED
    if args.full or args.breakdown:
        # pass A (untimed): find the dominant entry point.  rasterization()'s fast path issues its forward through the native
        # step driver (gs_step_fwd_*: bundles of operator calls made inside the library, invisible to this timer), so this pass
        # runs the OPERATOR path -- the same launches through the same entry points, one ctypes call each -- to time them one
        # by one; the timed regions below run the default path and carry events around the dominant operator only.
        _step.ENABLED = False
        for _ in range(2):
            step()
        with CallTimer(B) as ct:
            for _ in range(2):
                step()
        _step.ENABLED = step_driver_on
        for _ in range(2):
            step()
        per_call = {k: float(np.mean(v)) for k, v in ct.totals_ms().items()}
        calls_per_step = {k: len(v) / 2 for k, v in ct.events.items()}
        per_step = {k: per_call[k] * calls_per_step[k] for k in per_call}
        dominant = max((k for k in per_step if not k.startswith("gs_step_")), key=per_step.get)
        if args.breakdown and rank == 0:
            for k, v in sorted(per_step.items(), key=lambda kv: -kv[1]):
                print(f"  {k:32s} {v:8.3f} ms/step", file=sys.stderr)

    # timed region: exactly K steps between barrier + synchronize on both sides.  With --full, only the dominant entry point carries
    # events, and as K = 20 steps last ~20 ms, the region is REPEATED (every repetition bracketed the same way, the number of
    # repetitions agreed by all ranks) until --min-timed-s has been measured; ms_per_step is total time / total steps.
    def timed_region(n_steps, timer_only=None):
        barrier()
        with (CallTimer(B, only=timer_only) if timer_only is not None else contextlib.nullcontext()) as ct_:
            t0_ = time.perf_counter()
            for _ in range(n_steps):
                step()
            barrier()
            t1_ = time.perf_counter()
        return max_over_ranks(t1_ - t0_), ct_

    # the cyclic garbage collector is paused while measuring (a generation-2 sweep over the few thousand event objects of
    # the timers showed up as a 40 ms stall in some regions).  Collected ONCE here, followed by untimed steps: a 40 ms
    # collection leaves the GPU idle long enough for its clocks to drop, and a region started right after it read ~4%
    # slow at K = 20 (3% at K = 50) until they had ramped up again -- the regions run back to back instead.
    gc.collect()
    gc.disable()
    for _ in range(max(2, min(args.warmup, 5))):
        step()
    # Bring the GPU to its SUSTAINED clocks before anything is timed: after the pauses above (collection, calibration, the
    # per-entry-point pass) the first ~0.5 s of back-to-back steps still speed up region by region (0.751 -> 0.719 ms/step over 15
    # regions of 50 steps on one box, kernels unchanged: power management ramping), and the driver's 20-step command spends its
    # whole measurement inside that ramp.  Untimed, the same number of steps on every rank (the steps contain collectives).
    if args.ramp_s > 0:
        barrier()
        t0 = time.perf_counter()
        for _ in range(5):
            step()
        barrier()
        n_ramp = int(min(5000, args.ramp_s / max(max_over_ranks(time.perf_counter() - t0) / 5, 1e-5)))
        for _ in range(n_ramp):
            step()
    torch.cuda.reset_peak_memory_stats(dev)
    mem_before = torch.cuda.memory_allocated(dev)
    D.WIRE["bytes"] = 0
    elapsed, ct = timed_region(args.steps, {dominant} if args.full else None)
    wire_bytes_per_step = D.WIRE["bytes"] / args.steps
    peak_mem = torch.cuda.max_memory_allocated(dev)
    regions = [elapsed]
    if args.full:
        # (with the native step driver on, the compositing FORWARD is launched inside gs_step_fwd_finish and never passes through
        # this timer: at sizes where it, not the backward, dominates -- small scenes -- its duration comes from pass A instead)
        dom_all = list(ct.totals_ms().get(dominant, ())) or [per_call[dominant]]
        dom_source = "timed region" if dominant in ct.events else "pass A (operator path, untimed steps)"
        dom_ms = float(np.mean(dom_all))
        n_rep = int(min(200, max(0, np.ceil(args.min_timed_s / max(elapsed, 1e-6)) - 1)))
        for _ in range(n_rep):  # (the repetitions run without event timers: nothing but the steps inside the region)
            e_, _ = timed_region(args.steps, set())
            regions.append(e_)
    ms_per_step = sum(regions) / (len(regions) * args.steps) * 1e3
    if args.breakdown and rank == 0:
        print("  regions (ms/step): " + " ".join(f"{r / args.steps * 1e3:.3f}" for r in regions), file=sys.stderr)

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_out, splat_outputs(step.params, last_meta))

    # variant: a DENSE image gradient (what a real training loss produces) next to the broadcast one of the protocol
    dense_ms = nosum_ms = None
    if args.full and not args.no_extras:
        dense_grad[0] = torch.ones((1, w["height"], w["width"], 3), dtype=torch.float32, device=dev)
        for _ in range(3):
            step()
        e_, _ = timed_region(args.steps, set())
        dense_ms = e_ / args.steps * 1e3
        dense_grad[0] = "expanded-one"
        for _ in range(3):
            step()
        e_, _ = timed_region(args.steps, set())
        nosum_ms = e_ / args.steps * 1e3
        dense_grad[0] = None
    gc.enable()

    if rank == 0:
        meta = last_meta
        # gaussian mode: meta["radii"] is the pre-exchange tensor (this rank's splats x all cameras, as in the reference);
        # the splats visible in THIS rank's camera are the ones with tiles
        vis = (meta["tiles_per_gauss"] > 0) if mode.startswith("gaussian") else (meta["radii"] > 0)
        stats = dict(N=N, V=int(vis.sum()), I=int(meta["flatten_ids"].numel()),
                     P=w["width"] * w["height"], T=meta["tile_width"] * meta["tile_height"], K=(args.sh_degree + 1) ** 2)
        out = {
            "metric": "Msplats/s fwd+bwd @1080p (1M splats)",
            "value": N * world / (ms_per_step * 1e-3) / 1e6,
            "unit": "Msplats/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "timed": {"regions": len(regions), "steps_per_region": args.steps, "total_s": sum(regions), "untimed_ramp_s": args.ramp_s,
                      "ms_per_step_min_region": min(regions) / args.steps * 1e3, "ms_per_step_max_region": max(regions) / args.steps * 1e3},
            # reference protocol reports memory too (profiling/main.py:141-151): peak allocation during the timed steps,
            # and what the steps add on top of the resident scene + parameters
            "peak_mem_gb": peak_mem / 2**30, "step_mem_gb": (peak_mem - mem_before) / 2**30,
            # multi-GPU: payload bytes leaving THIS rank per step (counted from the collectives' shapes) and the time the
            # 7 xGMI links of one MI355X (7 x 153 GB/s, MI355X_MICROARCH.md) need for them at peak -- a lower bound that
            # the measured step time can be read against
            "wire": {"bytes_out_per_rank_per_step": wire_bytes_per_step, "xgmi_floor_ms": wire_bytes_per_step / (7 * 153e9) * 1e3,
                     "xgmi_peak_gbs_per_gpu": 7 * 153} if use_pg else None,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {
                "workload": f"BASELINE config 2: load_test_data(scene_grid={args.scene_grid}) -> {N} gaussians, "
                            f"SH degree {args.sh_degree}, {world}x1 camera {w['width']}x{w['height']}, packed=False, "
                            f"tile 16, fwd + bwd of sum(render)" + ((", quantize hooks on" + (" + learnable shN mask" if args.ada_mask else "") + (" (reference call pattern)" if args.quantize_reference_calls else " (fused activations, split SH" + (", mask applied by the renderer" if args.ada_mask else "") + ")")) if args.quantize else ""),
                "visible": stats["V"], "n_isects": stats["I"], "native_step_driver": bool(step_driver_on), "parallelism": (f"camera-sharded dp{world}" + ((", RCCL sum of splat gradients" + (" (visible rows only)" if mode == "camera_sparse" else "")) if world > 1 else "")) if mode.startswith("camera")
                else f"gaussian-sharded x{world}, 1 camera per rank, all-to-all of projected splats + dual for gradients"
                     + (" (visible rows only)" if mode == "gaussian" else " (all rows)"),
                **({"dp_mode": mode, "dp_calibration_ms_per_step": calib} if use_pg else {}),
                **({"launch_fallback": os.environ["GS_BENCH_LAUNCH_FALLBACK"]} if os.environ.get("GS_BENCH_LAUNCH_FALLBACK") else {}),
            },
        }
        if args.full:
            alg = algorithmic_bytes(stats)
            achieved = alg.get(dominant, 0) / (dom_ms * 1e-3) / 1e9
            # whole step: SURVEY.md 8(d)'s closed form (every stage once: projection, SH, binning with the sort at its
            # compulsory one read + one write, compositing, and the three backward stages) -- NOT the sum over every entry
            # point the library exports (round 2 summed alternatives the step never calls and overstated this by 40 %)
            Ns, Vs, Is, Ps, Ts, Ks_ = (stats[k] for k in ("N", "V", "I", "P", "T", "K"))
            total_alg = (48 * Ns + (80 + 12 * Ks_) * Vs + 84 * Is + 4 * Ts + 20 * Ps) + \
                        ((44 + 12 * Ks_) * Ns + (164 + 12 * Ks_) * Vs + 40 * Is + 24 * Ps)
            called_alg = sum(alg[k] for k in per_step if k in alg)
            # gs_projection_rows_bwd with prefilled outputs: radii of every pair, then only the visible gaussians' inputs (40 B), splat and
            # gradient rows (92 B used), SH rows in and out (24 K B) and the 44 B of per-gaussian gradients
            kernel_only = {"gs_projection_rows_bwd": 4 * Ns + (92 + 40 + 44 + 24 + 24 * Ks_) * Vs}
            out["ms_per_step_cold_protocol"] = cold_ms
            out["ms_per_step_dense_image_grad"] = dense_ms
            out["ms_per_step_without_loss_forward"] = nosum_ms
            out["roofline"] = {
                "bound": "hbm", "kernel": dominant, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": measured_traffic(dominant, f"grid{args.scene_grid}_{w['width']}x{w['height']}_sh{args.sh_degree}"),
                "kernel_ms": dom_ms, "kernel_ms_source": dom_source,
                # `bound` / `frac` are the contract's HBM figures; the kernel's OWN bound is the vector issue rate:
                # frac_of_own_bound = VALU instructions per launch (committed PMC pass) / live kernel time / the MEASURED issue rate
                "own_bound": "valu" if dominant in ("gs_rasterize_bwd", "gs_rasterize_fwd") else "hbm",
                "frac_of_own_bound": (lambda vi, r: (vi / (dom_ms * 1e-3) / r) if (vi and r and dominant in ("gs_rasterize_bwd", "gs_rasterize_fwd"))
                                      else achieved / HBM_COPY_GBS)(
                    measured_pmc(dominant, f"grid{args.scene_grid}_{w['width']}x{w['height']}_sh{args.sh_degree}", "valu_wave_instr_per_launch"),
                    measured_valu_issue_rate()),
                # the compositing kernels are VALU-issue bound, not HBM bound: SQ_INSTS_VALU per launch
                # (committed PMC pass) over the live kernel time, against one wave64 VALU instruction per 2 cycles per SIMD
                "valu": (lambda vi: None if vi is None else {
                    "wave_instr_per_launch": vi, "achieved": vi / (dom_ms * 1e-3), "peak": VALU_PEAK_WAVE_INSTR_PER_S,
                    "unit": "wave64 VALU instr/s", "frac": vi / (dom_ms * 1e-3) / VALU_PEAK_WAVE_INSTR_PER_S,
                    "measured_issue_rate": measured_valu_issue_rate(),
                    "frac_of_measured_issue_rate": (lambda r: None if not r else vi / (dom_ms * 1e-3) / r)(measured_valu_issue_rate())})(
                    measured_pmc(dominant, f"grid{args.scene_grid}_{w['width']}x{w['height']}_sh{args.sh_degree}",
                                 "valu_wave_instr_per_launch")),
                "algorithmic_bytes": alg.get(dominant, 0),
                "whole_step": {"algorithmic_bytes": total_alg, "achieved": total_alg / (ms_per_step * 1e-3) / 1e9,
                               "frac": total_alg / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                               "formula": "SURVEY 8(d): Fwd 48N+(80+12K)V+84I+4T+20P + Bwd (44+12K)N+(164+12K)V+40I+24P",
                               "algorithmic_bytes_of_called_entry_points": called_alg},
                "per_entry_point_ms": {k: round(v, 4) for k, v in sorted(per_step.items(), key=lambda kv: -kv[1])},
                # the stages whose OWN bound is HBM streaming (projection + SH each way; the quantizer hooks with --quantize):
                # algorithmic bytes over the entry point's event time (pass A), against the 8 TB/s spec AND against what a
                # float4 copy reaches on this part (6.29 TB/s)
                "streaming": {k: {"ms": round(per_step[k], 4), "algorithmic_bytes": alg[k], "achieved": alg[k] / (per_step[k] * 1e-3) / 1e9,
                                  "unit": "GB/s", "frac": alg[k] / (per_step[k] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                  "frac_of_measured_copy_rate": alg[k] / (per_step[k] * 1e-3) / 1e9 / HBM_COPY_GBS,
                                  # the API's dense outputs are mostly zeros that the compositing forward's side job wrote: what THIS
                                  # kernel itself moves (rows of visible gaussians only) over the same time
                                  **({"kernel_only_bytes": kernel_only[k], "kernel_only_frac": kernel_only[k] / (per_step[k] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                      "kernel_only_frac_of_measured_copy_rate": kernel_only[k] / (per_step[k] * 1e-3) / 1e9 / HBM_COPY_GBS}
                                     if k in kernel_only else {})}
                              for k in ("gs_projection_rows_fwd", "gs_projection_rows_bwd", "gs_quantize_noise_multi_fwd",
                                        "gs_quantize_noise_multi_bwd") if k in per_step and k in alg and per_step[k] > 0},
                # the binning chain (count -> depth pre-sort -> emit -> pair sort -> offsets), the stage whose OWN bound is HBM:
                # SURVEY 8(d)'s bytes of isect (32V + 4N + 12I) + sort (24I) + offsets (8I + 4T) over the sum of its entry
                # points' event times (pass A above)
                "binning": (lambda ms_, by_: {"ms": ms_, "algorithmic_bytes": by_, "achieved": by_ / (ms_ * 1e-3) / 1e9 if ms_ > 0 else None,
                                               "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": by_ / (ms_ * 1e-3) / 1e9 / HBM_PEAK_GBS if ms_ > 0 else None,
                                               "entry_points": sorted(k for k in per_step if k in BINNING_ENTRIES)})(
                    sum(v for k, v in per_step.items() if k in BINNING_ENTRIES),
                    (32 * Vs + 4 * Ns + 12 * Is) + 24 * Is + (8 * Is + 4 * Ts)),
            }
            if not args.no_extras and world == 1:
                out["psnr_vs_oracle"] = psnr_vs_oracle(dev)
            if world == 1 and not use_pg and not args.no_dp_projection and not args.quantize:
                out["multi_gpu_projection"] = dp_projection(args, ms_per_step, stats)
            if not args.no_cpu_baseline and world == 1:
                out["cpu_baseline"] = cpu_baseline(args, args.sh_degree)
    if use_pg:
        dist.barrier()
        dist.destroy_process_group()
    # RCCL writes its version banner through C stdio, which a pipe buffers until exit: push it out now, so that the JSON
    # line really is the last line of stdout
    import ctypes
    ctypes.CDLL(None).fflush(None)
    if rank == 0:
        sys.stdout.flush()
        print(json.dumps(out), flush=True)  # the last line of stdout, after any library banners


if __name__ == "__main__":
    main()
