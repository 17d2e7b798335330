"""HevcCompression at BASELINE config 2's size after the square crop (1003^2 = 1,006,009 splats), beside PngCompression:
  sweep:    for use_sort in (False, "morton", "grid") and qp in (4, 10, 16, 22, 28, 34): the bytes of the directory next to
            PngCompression's for the same splats, the PSNR of every transform-coded plane against the 8-bit plane it was made from,
            and the PSNR of a render of the decompressed splats against a render of the uncompressed ones (camera 0, 1080p)
  kernels:  gs_plane_transform_fwd / _inv and gs_plane_ans_encode / _decode alone (HIP events) on the scales and the quats plane
  files:    whole HevcCompression.compress / decompress calls alternating with PngCompression's, min..max of three rounds
The splats are the synthetic workload's: means and colours of the garden crop, scales, quats and opacities drawn at random -- so
three of the four coded planes are NOISE, the hardest input a transform codec has; the sizes say what the codec does on those
planes, not what it does on a trained scene.  No higher SH bands in the directory (their K-means is not what is measured here).
Each step runs in a child process of its own under a time limit, and the first failure ends the run.
usage: python tools/bench_plane_codec.py [--out FILE]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = {"sweep-none": 420, "sweep-morton": 420, "sweep-grid": 600, "kernels": 240, "files": 420}  # seconds
ROUNDS = 3
QPS = (4, 10, 16, 22, 28, 34)
PLANES = ("scales", "quats", "opacities", "sh0")


def setup():
    import torch

    from gscodec_studio_amd._helper import load_test_data, rescale_intrinsics

    means, quats, scales, opacities, colors, viewmats, Ks, w0, h0 = load_test_data(device="cpu", scene_grid=3)
    n = len(means)
    splats = {"means": means, "scales": torch.log(scales + 1e-6), "quats": quats, "opacities": torch.logit(opacities.clamp(0.02, 0.98)),
              "sh0": (colors.reshape(n, 1, 3) - 0.5) / 0.2820947917738781, "shN": torch.zeros(n, 0, 3)}
    camera = (viewmats[:1].cuda(), rescale_intrinsics(Ks, w0, h0, 1920, 1080)[:1].cuda())
    return {k: v.float().cuda() for k, v in splats.items()}, camera


def render(splats, camera):
    import torch

    from gscodec_studio_amd import rasterization

    img, _, _ = rasterization(splats["means"], splats["quats"], torch.exp(splats["scales"]), torch.sigmoid(splats["opacities"]),
                              splats["sh0"], camera[0], camera[1], 1920, 1080, sh_degree=0, packed=False)
    return img.clamp(0, 1)


def psnr(a, b, peak):
    import torch

    mse = float(torch.mean((a.double() - b.double()) ** 2))
    return float("inf") if mse == 0 else 10 * __import__("math").log10(peak * peak / mse)


def dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def event_ms(fn, rounds=5):
    import torch

    fn()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts), max(ts)


def host_ms(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def step_sweep(say, use_sort):
    import numpy as np

    from gscodec_studio_amd.compression import HevcCompression, PngCompression, plane_decode, quantize_grid
    from gscodec_studio_amd.compression._container import prepare_splats

    splats, camera = setup()
    truth = render(splats, camera)
    kept, side = prepare_splats(splats, 0.005, use_sort, False)
    planes = {k: quantize_grid(kept[k], side, bits=8, kbit=True)[0][0].reshape(side, side, -1) for k in PLANES}
    with tempfile.TemporaryDirectory() as tmp:
        d_png = os.path.join(tmp, "png")
        png = PngCompression(use_sort=use_sort, verbose=False)
        png.compress(d_png, splats)
        png_planes = sum(os.path.getsize(os.path.join(d_png, f"{k}.png")) for k in PLANES)
        say(f"use_sort = {use_sort!r}, {side * side} splats: PngCompression {dir_bytes(d_png)} bytes, {png_planes} of them the four planes; "
            f"render PSNR {psnr(render(png.decompress(d_png), camera), truth, 1.0):.2f} dB")
        say("    qp   directory bytes   plane bytes    plane PSNR (dB) scales / quats / opacities / sh0     render PSNR (dB)")
        for qp in QPS:
            d = os.path.join(tmp, f"hevc{qp}")
            codec = HevcCompression(use_sort=use_sort, verbose=False, qp=qp)
            codec.compress(d, splats)
            sizes = sum(os.path.getsize(os.path.join(d, f"{k}.bin")) for k in PLANES)
            p = [psnr(plane_decode(np.fromfile(os.path.join(d, f"{k}.bin"), np.uint8)), planes[k], 255.0) for k in PLANES]
            r = psnr(render(codec.decompress(d), camera), truth, 1.0)
            say(f"    {qp:2d}   {dir_bytes(d):15d}   {sizes:11d}    {' / '.join(f'{v:6.2f}' for v in p):50s}   {r:6.2f}")


def step_kernels(say):
    import numpy as np
    import torch

    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd.compression import plane_codec as PC, plane_codec_reference as R, quantize_grid
    from gscodec_studio_amd.compression._container import prepare_splats

    splats, _ = setup()
    kept, side = prepare_splats(splats, 0.005, "morton", False)
    stream = torch.cuda.current_stream().cuda_stream
    say(f"kernels, {side} x {side} planes in Morton order, S = {R.DEFAULT_STREAM_LEN}, P = {R.DEFAULT_BITS}, min..max of 5:")
    for name in ("scales", "quats"):
        plane = quantize_grid(kept[name], side, bits=8, kbit=True)[0][0].contiguous()
        ch = plane.shape[2]
        for qp in (4, 28):
            levels = PC.transform_levels(plane, qp)
            out = torch.empty_like(plane)
            blob = PC.plane_encode(plane, qp)
            assert torch.equal(PC.plane_decode(blob), PC.inverse_transform(levels, qp, side, side))
            head, freq, off, pay, _ = R.parse_container(blob)
            n = levels.numel()
            symbols = torch.from_numpy(R.levels_to_symbols(levels.cpu().numpy())[0]).cuda()
            cum = torch.from_numpy(R.cumulative16(freq).view(np.int16)).cuda()
            S, P = head.stream_len, head.bits
            nt = -(-n // S)
            slot = int(B.query("gs_plane_ans_slot_bytes", S, P))
            scratch = torch.empty(nt * slot, dtype=torch.uint8, device="cuda")
            lengths, states = (torch.empty(nt, dtype=torch.int32, device="cuda") for _ in range(2))
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            d_pay, d_off, dec = torch.from_numpy(np.array(pay)).cuda(), torch.from_numpy(off).cuda(), torch.empty(n, dtype=torch.uint8, device="cuda")
            runs = (("gs_plane_transform_fwd", lambda: B.call("gs_plane_transform_fwd", side, side, ch, qp, B.ptr(plane), B.ptr(levels), stream)),
                    ("gs_plane_transform_inv", lambda: B.call("gs_plane_transform_inv", side, side, ch, qp, B.ptr(levels), B.ptr(out), stream)),
                    ("gs_plane_ans_encode", lambda: B.call("gs_plane_ans_encode", n, S, P, B.ptr(symbols), B.ptr(cum), B.ptr(scratch), scratch.numel(),
                                                           B.ptr(lengths), B.ptr(states), B.ptr(status), stream)),
                    ("gs_plane_ans_decode", lambda: B.call("gs_plane_ans_decode", n, S, P, B.ptr(d_pay), d_pay.numel(), B.ptr(d_off), B.ptr(cum),
                                                           B.ptr(dec), stream)))
            for tag, fn in runs:
                t = event_ms(fn)
                say(f"  {name} ({ch} channels, {n} coefficients, {nt} streams) qp {qp:2d}  {tag:24s} {t[0]:9.3f}..{t[1]:9.3f} ms")
            assert int(status) == 0 and torch.equal(dec, symbols) and int(lengths.sum()) + 4 * nt == d_pay.numel()


def step_files(say):
    from gscodec_studio_amd.compression import HevcCompression, PngCompression

    splats, _ = setup()
    codecs = {"hevc qp 4": HevcCompression(use_sort="morton", verbose=False, qp=4), "hevc qp 28": HevcCompression(use_sort="morton", verbose=False, qp=28),
              "png": PngCompression(use_sort="morton", verbose=False)}
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {k: os.path.join(tmp, k.replace(" ", "_")) for k in codecs}
        times = {(k, op): [] for k in codecs for op in ("compress", "decompress")}
        for r in range(ROUNDS + 1):  # round 0 warms up
            for k, codec in codecs.items():
                tc = host_ms(lambda: codec.compress(dirs[k], splats))
                td = host_ms(lambda: codec.decompress(dirs[k]))
                if r:
                    times[(k, "compress")].append(tc)
                    times[(k, "decompress")].append(td)
        say(f"files, whole calls on the full directory (use_sort = 'morton', no shN), the codecs alternating, min..max of {ROUNDS} rounds:")
        for (k, op), t in times.items():
            say(f"  {k:10s} {op:10s} {min(t):10.1f}..{max(t):10.1f} ms")


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
            say("tools/bench_plane_codec.py: HevcCompression (transform-coded planes) beside PngCompression")
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

    assert torch.cuda.is_available(), "bench_plane_codec needs a GPU"
    if a.step.startswith("sweep"):
        if a.step == "sweep-none":
            say(f"on {torch.cuda.get_device_name(0)}")
        step_sweep(say, {"sweep-none": False, "sweep-morton": "morton", "sweep-grid": "grid"}[a.step])
    else:
        {"kernels": step_kernels, "files": step_files}[a.step](say)
    return 0


if __name__ == "__main__":
    sys.exit(main())
