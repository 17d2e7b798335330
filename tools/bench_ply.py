"""The .ply reader and writer at BASELINE config 2's size: 1,006,065 splats (the garden crop tiled 3 x 3), SH degree 3, the
62-float layout -- a 249.5 MB file.  The file is written once into --dir and read back once before anything is timed, so every
timed read comes out of the page cache: the numbers are those of the host copy, the upload and the kernels, not of a disk.
In one process, alternating round by round:
  calls:      load_ply, load_ply_to_rasterizer_inputs and save_ply, whole calls (wall clock around a synchronised device)
  reference:  a numpy restatement of the statements of the reference's load_ply / save_ply (examples/simple_trainer.py:414-510)
              over structured arrays: np.fromfile + the 62 float64 column copies + the upload, and the download + one Python
              tuple per splat + tofile.  plyfile's own header parsing and element handling is NOT in it (the package is
              absent), which flatters the reference.
  kernels:    gs_ply_unpack and gs_ply_pack alone on rows that are already on the device (HIP events), the word route against
              the byte route, with the bytes each moves per second next to the float4 copy of this part (6.29 TB/s)
min..max over --rounds rounds; a difference is claimed only where it exceeds the sum of both spreads.
usage: python tools/bench_ply.py [--rounds 3] [--grid 3] [--dir /tmp] [--no-reference] [--out profiles/r23_ply.txt]"""
import argparse
import ctypes
import gc
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_GBS = 6290.0  # bench.py: what a float4 copy reaches on an MI355X

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def span(ts, unit="ms", scale=1e3):
    return f"{min(ts) * scale:.2f} .. {max(ts) * scale:.2f} {unit}"


def claim(name_a, a, name_b, b):
    """a against b (lists of seconds, a the faster by intent): a ratio only where the gap exceeds the summed spreads."""
    gap, spreads = min(b) - max(a), (max(a) - min(a)) + (max(b) - min(b))
    if gap > spreads:
        return f"{name_a} against {name_b}: {min(b) / max(a):.1f} x .. {max(b) / min(a):.1f} x faster"
    return f"{name_a} against {name_b}: no claim (gap {gap * 1e3:.1f} ms, spreads sum to {spreads * 1e3:.1f} ms)"


def reference_load(path, header, device):
    """The reference's load_ply statements on a structured array (float64 column copies, the reshapes, float32, upload)."""
    import numpy as np
    import torch

    v = np.fromfile(path, header.numpy_dtype(), count=header.count, offset=header.payload_offset)
    n = header.count
    names = v.dtype.names
    means = np.stack((v["x"], v["y"], v["z"]), axis=1)

    def group(prefix):
        size = len([p for p in names if p.startswith(prefix)])
        data = np.zeros((n, size))
        for i in range(size):
            data[:, i] = v[f"{prefix}{i}"]
        return data

    sh0, shN, scales, quats = group("f_dc_"), group("f_rest_"), group("scale_"), group("rot_")
    sh0 = sh0.reshape(n, 3, -1).transpose(0, 2, 1)
    shN = shN.reshape(n, 3, -1).transpose(0, 2, 1)
    opacities = v["opacity"].reshape(-1, 1)
    out = {"means": means, "sh0": sh0, "shN": shN, "opacities": opacities.astype(np.float32).squeeze(1), "scales": scales, "quats": quats}
    return {k: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).to(device) for k, a in out.items()}


def reference_save(splats, path, header_text):
    """The reference's save_ply statements: download, concatenate, one Python tuple per splat into a structured array, write."""
    import numpy as np

    means = splats["means"].detach().cpu().numpy()
    normals = np.zeros_like(means)
    sh0 = splats["sh0"].detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    shN = splats["shN"].detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    opacities = splats["opacities"].detach().unsqueeze(1).cpu().numpy()
    scales = splats["scales"].detach().cpu().numpy()
    quats = splats["quats"].detach().cpu().numpy()
    attributes = np.concatenate((means, normals, sh0, shN, opacities, scales, quats), axis=1)
    elements = np.empty(means.shape[0], dtype=[(f"c{i}", "f4") for i in range(attributes.shape[1])])
    elements[:] = list(map(tuple, attributes))
    with open(path, "wb") as f:
        f.write(header_text)
        elements.tofile(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grid", type=int, default=3, help="tiles per side of the garden crop (3: config 2's 1,006,065 splats)")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--no-reference", action="store_true", help="skip the numpy restatement of the reference (tens of seconds a round)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd import ply as P
    from gscodec_studio_amd._helper import load_test_data

    assert torch.cuda.is_available(), "bench_ply measures on the GPU"
    dev = torch.device("cuda:0")
    gc.collect()
    gc.freeze()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def event_s(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    means = load_test_data(device=dev, scene_grid=a.grid)[0].contiguous()
    n = int(means.shape[0])
    g = torch.Generator(device=dev).manual_seed(23)
    splats = {"means": means, "sh0": torch.randn((n, 1, 3), device=dev, generator=g), "shN": 0.1 * torch.randn((n, 15, 3), device=dev, generator=g),
              "opacities": torch.randn(n, device=dev, generator=g), "scales": torch.randn((n, 3), device=dev, generator=g) - 4.0,
              "quats": torch.randn((n, 4), device=dev, generator=g)}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        path, path2, path3 = (os.path.join(tmp, f) for f in ("bench.ply", "bench_out.ply", "bench_ref.ply"))
        P.save_ply(splats, path)  # also the warm-up of the pinned buffers and of the code objects
        header = P.read_ply_header(path)
        size = os.path.getsize(path)
        back = P.load_ply(path)
        assert all(torch.equal(back[k], splats[k]) for k in splats)
        P.load_ply_to_rasterizer_inputs(path)
        say(f"N = {n} splats, SH degree 3, {header.stride} bytes a row, file of {size / 1e6:.1f} MB in the page cache "
            f"({(size - header.payload_offset) / 1e6:.1f} MB of rows)")
        t_load, t_fused, t_save, t_rload, t_rsave = [], [], [], [], []
        for _ in range(a.rounds):
            t_load.append(wall(lambda: P.load_ply(path))[0])
            t_fused.append(wall(lambda: P.load_ply_to_rasterizer_inputs(path))[0])
            t_save.append(wall(lambda: P.save_ply(splats, path2))[0])
            if not a.no_reference:
                t, ref = wall(lambda: reference_load(path, header, dev))
                t_rload.append(t)
                assert all(torch.equal(ref[k], splats[k]) for k in splats)
                t_rsave.append(wall(lambda: reference_save(splats, path3, P.ply_header_text(n)))[0])
        say("whole calls (file in, tensors on the device out, and back):")
        say(f"  load_ply                        {span(t_load)}   ({size / max(t_load) / 1e9:.2f} .. {size / min(t_load) / 1e9:.2f} GB/s of file)")
        say(f"  load_ply_to_rasterizer_inputs   {span(t_fused)}")
        say(f"  save_ply                        {span(t_save)}   ({size / max(t_save) / 1e9:.2f} .. {size / min(t_save) / 1e9:.2f} GB/s of file)")
        if a.no_reference:
            say("  the reference's statements in numpy: not run (--no-reference)")
        else:
            with open(path2, "rb") as f2, open(path3, "rb") as f3:
                assert f2.read() == f3.read(), "save_ply and the reference's statements wrote different files"
            say(f"  reference load_ply statements   {span(t_rload, 's', 1.0)}   (numpy over a structured array; plyfile's parsing left out)")
            say(f"  reference save_ply statements   {span(t_rsave, 's', 1.0)}   (the same; both files are equal byte for byte)")
            say("  " + claim("load_ply", t_load, "the reference's statements", t_rload))
            say("  " + claim("save_ply", t_save, "the reference's statements", t_rsave))
        say("  " + claim("load_ply_to_rasterizer_inputs", t_fused, "load_ply", t_load) + "  (and the other way: "
            + claim("load_ply", t_load, "the fused load", t_fused) + ")")

        # the kernels alone, rows on the device
        rows = torch.from_numpy(np.fromfile(path, np.uint8, offset=header.payload_offset)).to(dev)
        stride = header.stride
        stream = torch.cuda.current_stream().cuda_stream
        for fused, label in ((False, "six tensors"), (True, "fused: one colour tensor, exp / sigmoid / normalise")):
            cols = P.column_table(header, fused)
            table, widths = (ctypes.c_uint32 * len(cols.entries))(*cols.entries), (ctypes.c_uint32 * 6)(*cols.widths)
            outs = [torch.empty((n, w), device=dev) if w else None for w in cols.widths]
            ptrs = (ctypes.c_void_p * 6)(*[None if t is None else t.data_ptr() for t in outs])
            moved = n * stride + 4 * n * sum(cols.widths)
            for force, route in ((0, "word route"), (1, "byte route")):
                def run():
                    B.call("gs_ply_unpack", n, stride, B.ptr(rows), ctypes.addressof(table), ctypes.addressof(widths), ctypes.addressof(ptrs),
                           int(fused), int(fused), force, stream)
                run()
                ts = [event_s(run) for _ in range(a.rounds)]
                say(f"gs_ply_unpack, {label}, {route}: {span(ts)}   {moved / max(ts) / 1e9:.0f} .. {moved / min(ts) / 1e9:.0f} GB/s of "
                    f"{moved / 1e6:.0f} MB ({moved / min(ts) / 1e9 / HBM_COPY_GBS * 100:.0f} % of a float4 copy's {HBM_COPY_GBS / 1e3:.2f} TB/s)")
        cols = P.column_table(header)
        flat = [splats[k].reshape(n, -1) for k in ("means", "sh0", "shN", "opacities", "scales", "quats")]
        table, widths = (ctypes.c_uint32 * len(cols.entries))(*cols.entries), (ctypes.c_uint32 * 6)(*cols.widths)
        ptrs = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in flat])
        packed = torch.empty_like(rows)

        def run_pack():
            B.call("gs_ply_pack", n, stride, ctypes.addressof(table), ctypes.addressof(widths), ctypes.addressof(ptrs), B.ptr(packed), stream)
        run_pack()
        torch.cuda.synchronize()
        assert torch.equal(packed, rows)
        ts = [event_s(run_pack) for _ in range(a.rounds)]
        moved = n * stride + 4 * n * sum(cols.widths)
        say(f"gs_ply_pack: {span(ts)}   {moved / max(ts) / 1e9:.0f} .. {moved / min(ts) / 1e9:.0f} GB/s of {moved / 1e6:.0f} MB "
            f"({moved / min(ts) / 1e9 / HBM_COPY_GBS * 100:.0f} % of a float4 copy's {HBM_COPY_GBS / 1e3:.2f} TB/s)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
