"""The entropy coder of EntropyCodingCompression at BASELINE config 2's size after the square crop (1003^2 = 1,006,009 splats):
scales [N, 3] + quats [N, 4] = 7 channels of 8-bit min-max symbols.
  encode:  symbol histogram (+ channel-major copy), lane-per-stream rANS encode, scan, pack -- the kernels alone (HIP events) and
           the whole ans_encode call (frequency tables on the host, read-back of the payload, container)
  decode:  container validation, upload, decode kernel, gs_grid_dequantize -- kernels alone and the whole call
  size:    file bytes of <name>.bin (+ <name>_prob.npy) against the empirical zeroth-order entropy of the symbols
and beside them the 8-bit PNG route PngCompression takes for the same two attributes (quantize, per-row filter choice, zlib level 6;
read: inflate, unfilter, dequantize), in the given splat order and in Morton order (the order changes the PNG size only; the static
per-channel model of the ANS coder does not see it).
usage: python tools/bench_ans.py [--rounds 5] [--stream-len 1024]"""
import argparse
import gc
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gscodec_studio_amd import _backend as B  # noqa: E402
from gscodec_studio_amd._helper import load_test_data  # noqa: E402
from gscodec_studio_amd.compression import ans, ans_reference as R, dequantize_grid, log_transform, morton_order, png_read, png_write, quantize_grid  # noqa: E402


def host_ms(fn, rounds):
    fn()
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def event_ms(fn, rounds):
    fn()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def line(tag, t, n_sym=None):
    rate = f"  {n_sym / t[0] / 1e3:9.1f} Msymbols/s" if n_sym else ""
    print(f"  {tag:74s} {t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f}){rate}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stream-len", type=int, default=R.DEFAULT_STREAM_LEN)
    a = ap.parse_args()
    gc.collect()
    gc.freeze()
    dev = torch.device("cuda")
    means, quats, scales, opacities, *_ = load_test_data(device="cpu", scene_grid=3)
    side = int(len(means) ** 0.5)
    n = side * side
    attrs = {"scales": torch.log(scales[:n] + 1e-6).to(dev), "quats": torch.nn.functional.normalize(quats[:n], dim=-1).to(dev)}
    order = morton_order(log_transform(means[:n].to(dev)))
    S, P = a.stream_len, R.DEFAULT_BITS
    n_sym = 7 * n
    print(f"N = {n} splats (side {side}), scales + quats = 7 channels = {n_sym} symbols, S = {S}, P = {P}", flush=True)

    sym, meta, prob, blob = {}, {}, {}, {}
    for k, v in attrs.items():
        (plane,), meta[k] = quantize_grid(v, side, bits=8)
        sym[k] = plane.reshape(n, -1).contiguous()
        prob[k] = ans.probabilities(ans.symbol_histogram(sym[k]))
        blob[k] = ans.ans_encode(sym[k], prob[k], stream_len=S)
        assert torch.equal(ans.ans_decode(blob[k], prob[k]), sym[k])

    # ---- encode
    stream = torch.cuda.current_stream().cuda_stream
    bufs = {}
    for k in attrs:
        c = sym[k].shape[1]
        nt = c * (-(-n // S))
        freq = R.normalize_frequencies(prob[k], P)
        bufs[k] = dict(c=c, nt=nt, counts=torch.zeros((c, 256), dtype=torch.int32, device=dev), cm=torch.empty((c, n), dtype=torch.uint8, device=dev),
                       freq=torch.from_numpy(freq.view(np.int32)).to(dev), cum=torch.from_numpy(R.cumulative(freq).view(np.int32)).to(dev),
                       scratch=torch.empty(int(B.query("gs_ans_encode_bytes", n, c, S, P)), dtype=torch.uint8, device=dev),
                       lengths=torch.empty(nt, dtype=torch.int32, device=dev), states=torch.empty(nt, dtype=torch.int32, device=dev),
                       status=torch.zeros(1, dtype=torch.int32, device=dev), offsets=torch.zeros(nt + 1, dtype=torch.int64, device=dev))
        b = bufs[k]
        _, _, _, _, off, pay = R.parse_container(blob[k])
        b["payload"] = torch.empty(pay.size, dtype=torch.uint8, device=dev)
        b["d_payload"], b["d_off"] = torch.from_numpy(np.array(pay)).to(dev), torch.from_numpy(off).to(dev)
        b["out"], b["deq"] = torch.empty((n, c), dtype=torch.uint8, device=dev), torch.empty(n * c, dtype=torch.float32, device=dev)
        b["mins"], b["maxs"] = (torch.tensor(meta[k][m], dtype=torch.float32, device=dev) for m in ("mins", "maxs"))

    def hist():
        for k, b in bufs.items():
            b["counts"].zero_()
            B.call("gs_ans_histogram", n, b["c"], B.ptr(sym[k]), B.ptr(b["counts"]), B.ptr(b["cm"]), stream)

    def enc():
        for b in bufs.values():
            B.call("gs_ans_encode", n, b["c"], S, P, B.ptr(b["cm"]), B.ptr(b["freq"]), B.ptr(b["cum"]), B.ptr(b["scratch"]), b["scratch"].numel(),
                   B.ptr(b["lengths"]), B.ptr(b["states"]), B.ptr(b["status"]), stream)

    def scan_pack():
        for b in bufs.values():
            torch.cumsum(b["lengths"].long() + 4, dim=0, out=b["offsets"][1:])
            B.call("gs_ans_pack", b["nt"], S, P, B.ptr(b["scratch"]), B.ptr(b["lengths"]), B.ptr(b["states"]), B.ptr(b["offsets"]), B.ptr(b["payload"]),
                   b["payload"].numel(), stream)

    def dec():
        for b in bufs.values():
            B.call("gs_ans_decode", n, b["c"], S, P, B.ptr(b["d_payload"]), b["d_payload"].numel(), B.ptr(b["d_off"]), B.ptr(b["freq"]), B.ptr(b["cum"]),
                   B.ptr(b["out"]), stream)

    def deq():
        for b in bufs.values():
            B.call("gs_grid_dequantize", n * b["c"], b["c"], B.ptr(b["out"]), None, B.ptr(b["mins"]), B.ptr(b["maxs"]), 8, B.ptr(b["deq"]), stream)

    print("encode, both attributes, median of %d:" % a.rounds, flush=True)
    parts = {"gs_ans_histogram (+ channel-major copy)": hist, "gs_ans_encode": enc, "exclusive scan (torch.cumsum) + gs_ans_pack": scan_pack}
    total = 0.0
    for tag, fn in parts.items():
        t = event_ms(fn, a.rounds)
        total += t[0]
        line("kernels: " + tag, t, n_sym)
    print(f"  {'kernels: histogram + encode + pack, sum of the medians':74s} {total:9.3f} ms  {n_sym / total / 1e3:9.1f} Msymbols/s", flush=True)
    line("whole call: ans_encode x 2 (tables, launches, read-back, container)", host_ms(lambda: [ans.ans_encode(sym[k], prob[k], stream_len=S) for k in attrs], a.rounds), n_sym)
    for k, b in bufs.items():  # the hand-driven sequence wrote the same payload
        assert np.array_equal(b["payload"].cpu().numpy(), R.parse_container(blob[k])[5]) and int(b["status"]) == 0

    print("decode, both attributes:", flush=True)
    td, tq = event_ms(dec, a.rounds), event_ms(deq, a.rounds)
    line("kernels: gs_ans_decode", td, n_sym)
    line("kernels: gs_grid_dequantize", tq, n_sym)
    print(f"  {'kernels: decode + dequantise, sum of the medians':74s} {td[0] + tq[0]:9.3f} ms  {n_sym / (td[0] + tq[0]) / 1e3:9.1f} Msymbols/s", flush=True)
    line("whole call: (ans_decode + dequantize_grid) x 2 (validation, upload, launches)",
         host_ms(lambda: [dequantize_grid([ans.ans_decode(blob[k], prob[k])], meta[k]) for k in attrs], a.rounds), n_sym)
    for k, b in bufs.items():
        assert torch.equal(b["out"], sym[k])

    print("size:", flush=True)
    tot_bin = tot_ent = tot_prob = 0
    for k in attrs:
        s = sym[k].cpu().numpy()
        ent = sum(-float((c[c > 0] * np.log2(c[c > 0] / n)).sum()) for c in (np.bincount(s[:, j], minlength=256).astype(np.float64) for j in range(s.shape[1]))) / 8
        npy = 128 + prob[k].nbytes
        tot_bin, tot_ent, tot_prob = tot_bin + blob[k].size, tot_ent + ent, tot_prob + npy
        print(f"  {k}.bin {blob[k].size} bytes; empirical entropy {ent:.0f} bytes; ratio {blob[k].size / ent:.4f}; {k}_prob.npy {npy} bytes", flush=True)
    print(f"  both: {tot_bin} bytes of .bin = {tot_bin / tot_ent:.4f} x entropy ({8 * tot_bin / n_sym:.3f} bits per symbol), + {tot_prob} bytes of tables", flush=True)

    print("the 8-bit PNG route of PngCompression for the same two attributes:", flush=True)
    with tempfile.TemporaryDirectory() as d:
        for tag, perm in (("given order", None), ("Morton order", order)):
            vals = {k: (v if perm is None else v[perm]) for k, v in attrs.items()}

            def write():
                for k, v in vals.items():
                    (plane,), _ = quantize_grid(v, side, bits=8, kbit=True)
                    png_write(os.path.join(d, f"{k}.png"), plane.cpu().numpy())

            def read():
                for k in vals:
                    dequantize_grid([torch.from_numpy(png_read(os.path.join(d, f"{k}.png")))], {**meta[k], "quantization": 8}, device=dev)

            tw = host_ms(write, max(2, a.rounds // 2))
            tr = host_ms(read, max(2, a.rounds // 2))
            size = sum(os.path.getsize(os.path.join(d, f"{k}.png")) for k in vals)
            line(f"{tag}: quantize + png_write x 2", tw, n_sym)
            line(f"{tag}: png_read + dequantize x 2", tr, n_sym)
            print(f"  {tag}: {size} bytes of .png = {size / tot_ent:.4f} x the symbols' zeroth-order entropy ({8 * size / n_sym:.3f} bits per symbol)", flush=True)


if __name__ == "__main__":
    main()
