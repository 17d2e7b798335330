"""SeqHevcCompression at BASELINE config 2's size, T = 16 frames of a drifting sequence.  The class PADS the count to the next
square where the per-plane codecs crop it: the workload's 1,006,065 splats become 1004 x 1004 planes (1,008,016; cropping would give
the 1003 x 1003 = 1,006,009 of tools/bench_plane_codec.py).
  kernels:  gs_plane_seq_fwd / gs_plane_seq_inv alone (HIP events, min..max of 5) on the three-channel scales and the four-channel
            quats sequence, beside the per-frame loop that is the only way to run such a closed loop without them: per frame
            gs_plane_transform_fwd, gs_plane_transform_inv and a torch subtraction (3 T launches, every intermediate through
            memory).  The per-frame kernels take 8-bit planes only, so the loop is a COST MODEL of the closed loop -- the same
            launches on the same amounts of data -- and does not produce the sequence codec's levels
  sweep:    gop 1 against gop T at qp 4, 22 and 34 (every lossy attribute at that qp): directory bytes, the PSNR of every coded plane
            sequence against the 8-bit planes it was made from (frames 0 and T - 1), and the PSNR of a render of the decompressed
            frames 0 and T - 1 against a render of the uncompressed ones (camera 0, 1080p)
  files:    whole compress / decompress calls at qp 22, gop T and gop 1, min..max of three rounds
The splats are the synthetic workload's: means and colours of the garden crop, scales, quats and opacities drawn at random; frame
t + 1 is frame t plus N(0, 0.5 % of the attribute's spread) on every attribute.  No higher SH bands.
Each step runs in a child process of its own under a time limit, and the first failure ends the run.
usage: python tools/bench_seq_codec.py [--out FILE] [--steps kernels,sweep,files]"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_plane_codec import dir_bytes, event_ms, host_ms, psnr, render, setup  # noqa: E402

STEPS = {"kernels": 300, "sweep": 600, "files": 420}  # seconds
FRAMES = 16
ROUNDS = 3
QPS = (4, 22, 34)
PLANES = ("scales", "quats", "opacities", "sh0")
DRIFT = 0.005


def sequence():
    import torch

    splats, camera = setup()
    gen = torch.Generator(device="cuda").manual_seed(3)
    frames = [splats]
    for _ in range(FRAMES - 1):
        frames.append({k: v + DRIFT * v.std() * torch.randn(v.shape, device="cuda", generator=gen) if v.numel() else v for k, v in frames[-1].items()})
    return frames, camera


def qp_dict(qp):
    return {"means": -1, "opacities": qp, "quats": qp, "scales": qp, "sh0": qp, "shN": {"sh1": qp, "sh2": qp, "sh3": qp}}


def step_kernels(say):
    import torch

    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd.compression import SeqHevcCompression, quantize_grid_sequence
    from gscodec_studio_amd.compression import plane_seq_codec as SC

    frames, _ = sequence()
    videos = SeqHevcCompression(use_sort="morton", verbose=False).reorganize(frames)
    side = videos["means"].shape[1]
    stream = torch.cuda.current_stream().cuda_stream
    say(f"on {torch.cuda.get_device_name(0)}")
    say(f"kernels, T = {FRAMES} frames of {side} x {side} planes in Morton order of frame 0, min..max of 5:")
    for name in ("scales", "quats"):
        planes = quantize_grid_sequence(videos[name], bits=8)[0][0]
        t, h, w, ch = planes.shape
        for qp, gop in ((4, FRAMES), (22, FRAMES), (22, 1)):
            levels, recon = SC.seq_transform_levels(planes, qp, gop, recon=True)
            out = torch.empty_like(planes)
            assert torch.equal(SC.seq_inverse_transform(levels, qp, gop, h, w), recon)
            one_levels = torch.empty_like(levels[0])
            diff = torch.empty(planes[0].shape, dtype=torch.int16, device="cuda")

            def per_frame_loop():
                for f in range(t):
                    B.call("gs_plane_transform_fwd", h, w, ch, qp, B.ptr(planes[f]), B.ptr(one_levels), stream)
                    B.call("gs_plane_transform_inv", h, w, ch, qp, B.ptr(one_levels), B.ptr(out[f]), stream)
                    torch.sub(planes[f], out[f - 1], out=diff)

            runs = (("gs_plane_seq_fwd (with recon)", lambda: B.call("gs_plane_seq_fwd", t, gop, h, w, ch, qp, B.ptr(planes), B.ptr(levels), B.ptr(recon), stream)),
                    ("gs_plane_seq_fwd (levels only)", lambda: B.call("gs_plane_seq_fwd", t, gop, h, w, ch, qp, B.ptr(planes), B.ptr(levels), None, stream)),
                    ("gs_plane_seq_inv", lambda: B.call("gs_plane_seq_inv", t, gop, h, w, ch, qp, B.ptr(levels), B.ptr(out), stream)),
                    ("per-frame loop, 3 T launches", per_frame_loop))
            for tag, fn in runs:
                lo, hi = event_ms(fn)
                say(f"  {name} ({ch} channels, {levels.numel()} coefficients) qp {qp:2d} gop {gop:2d}  {tag:32s} {lo:9.3f}..{hi:9.3f} ms")


def step_sweep(say):
    import numpy as np
    import torch

    from gscodec_studio_amd.compression import SeqHevcCompression, plane_seq_decode, quantize_grid_sequence

    frames, camera = sequence()
    ends = (0, FRAMES - 1)
    truth = {t: render(frames[t], camera) for t in ends}
    say(f"sweep, T = {FRAMES}, use_sort = 'morton' (frame 0's order for gop {FRAMES}, every frame's own for gop 1):")
    say("    qp  gop   directory bytes   plane PSNR (dB), frame 0 | frame T - 1: scales / quats / opacities / sh0          render PSNR (dB) frame 0, T - 1")
    with tempfile.TemporaryDirectory() as tmp:
        for qp in QPS:
            for gop in (1, FRAMES):
                codec = SeqHevcCompression(use_sort="morton", verbose=False, qp=qp_dict(qp), gop=gop, use_all_intra=(gop == 1))
                videos = codec.reorganize(frames)
                d = os.path.join(tmp, f"qp{qp}_gop{gop}")
                codec.compress(d)
                p = {t: [] for t in ends}
                for k in PLANES:
                    planes = quantize_grid_sequence(videos[k], bits=8)[0][0]
                    dec = plane_seq_decode(np.fromfile(os.path.join(d, f"{k}.bin"), np.uint8))
                    for t in ends:
                        p[t].append(psnr(dec[t], planes[t], 255.0))
                back = codec.deorganize(codec.decompress(d))
                r = [psnr(render(back[t], camera), truth[t], 1.0) for t in ends]
                cols = " | ".join(" / ".join(f"{v:6.2f}" for v in p[t]) for t in ends)
                say(f"    {qp:2d}  {gop:3d}   {dir_bytes(d):15d}   {cols:78s}   {r[0]:6.2f}, {r[1]:6.2f}")
                del videos, back
                torch.cuda.empty_cache()


def step_files(say):
    from gscodec_studio_amd.compression import SeqHevcCompression

    frames, _ = sequence()
    with tempfile.TemporaryDirectory() as tmp:
        say(f"files, whole calls (use_sort = 'morton', qp 22 everywhere, no shN), min..max of {ROUNDS} rounds:")
        for gop in (FRAMES, 1):
            codec = SeqHevcCompression(use_sort="morton", verbose=False, qp=qp_dict(22), gop=gop, use_all_intra=(gop == 1))
            d = os.path.join(tmp, f"gop{gop}")
            times = {"reorganize": [], "compress": [], "decompress": []}
            for r in range(ROUNDS + 1):  # round 0 warms up
                got = (host_ms(lambda: codec.reorganize(frames)), host_ms(lambda: codec.compress(d)), host_ms(lambda: codec.decompress(d)))
                if r:
                    for k, v in zip(times, got):
                        times[k].append(v)
            for k, v in times.items():
                say(f"  gop {gop:2d}  {k:10s} {min(v):10.1f}..{max(v):10.1f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="(internal) run one step in this process")
    ap.add_argument("--steps", default=",".join(STEPS), help="the steps to run, in this order (default: all); with --append the "
                    "report is continued, so that a long run can be split over several calls")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.step is None:  # the driver: holds no GPU itself
        if not a.append:
            if a.out and os.path.exists(a.out):
                os.remove(a.out)
            say("tools/bench_seq_codec.py: SeqHevcCompression (transform-coded plane sequences with temporal prediction)")
        for step in a.steps.split(","):
            limit = STEPS[step]
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + (["--out", a.out] if a.out else [])
            try:
                r = subprocess.run(cmd, timeout=limit)
            except subprocess.TimeoutExpired:
                say(f"step {step}: no result within {limit} s; stopping")
                return 1
            if r.returncode != 0:
                say(f"step {step}: exit status {r.returncode}; stopping")
                return 1
        return 0
    import torch

    assert torch.cuda.is_available(), "bench_seq_codec needs a GPU"
    {"kernels": step_kernels, "sweep": step_sweep, "files": step_files}[a.step](say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
