"""The hash-grid Gaussian route of EntropyCodingCompression at BASELINE config 2's size after the square crop (1003^2 = 1,006,009
splats), for scales [N, 3] and quats [N, 4], beside the factorized route:
  params:  gs_gauss_ans_params alone (the MLP + normalisation + quantisation on the encoder's features), and the whole
           gaussian_params call (NaN check of the tables, hash-grid encoder launch, params kernel)
  coder:   gs_gauss_ans_encode and gs_gauss_ans_decode alone (HIP events), both attributes
  files:   whole EntropyCodingCompression.compress / decompress calls, the Gaussian route alternating with the factorized route,
           min..max of three rounds; the bytes of <name>.bin (and of what travels beside it) for both routes
The entropy models are trained for --train-steps steps of the simulation's rate term on these splats first (default 3000; the
splats themselves stay fixed): the sizes say what THAT model is worth, not what a full training run reaches.  Each step -- the
training included, which hands its models on through a temporary file -- runs in a child process of its own under a time limit,
and the first failure ends the run.
usage: python tools/bench_gauss_ans.py [--out FILE] [--train-steps 3000]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = {"train": 900, "params": 300, "coder": 300, "files": 600}  # seconds
ROUNDS = 3
ATTRS = ("scales", "quats")


def setup(train_steps, models_path, say=print):
    """The splats and the simulation; ``train_steps`` > 0: train its models and save them, else load them."""
    import torch

    from gscodec_studio_amd._helper import load_test_data
    from gscodec_studio_amd.compression_simulation import HashGridCompressionSimulation

    means, quats, scales, opacities, colors, *_ = load_test_data(device="cpu", scene_grid=3)
    n = len(means)
    g = torch.Generator().manual_seed(0)
    splats = {"means": means, "scales": torch.log(scales + 1e-6), "quats": quats, "opacities": torch.logit(opacities.clamp(0.02, 0.98)),
              "sh0": colors.reshape(n, 1, 3), "shN": 0.05 * torch.randn(n, 3, 3, generator=g)}
    splats = {k: v.float().cuda() for k, v in splats.items()}
    steps = {"means": -1, "scales": 1, "quats": 1, "opacities": -1, "sh0": -1, "shN": -1}
    sim = HashGridCompressionSimulation(entropy_model_enable=True, entropy_steps=steps, device="cuda")
    params = {k: torch.nn.Parameter(v.clone()) for k, v in splats.items()}
    with torch.no_grad():
        sim._estiblish_bbox(params["means"][:1_000_000])
    torch.manual_seed(0)
    for it in range(train_steps):
        _, bits = sim.simulate_compression(params, step=10)
        rate = {a: b.sum() / b.numel() for a, b in bits.items() if b is not None}
        sum(rate.values()).backward()
        for a in ATTRS:
            sim.entropy_model_optimizers[a].step()
            sim.entropy_model_optimizers[a].zero_grad(set_to_none=True)
            sim.entropy_model_schedulers[a].step()
        if it in (0, train_steps - 1):
            say(f"  training step {it + 1}: estimated bits per value on the 5 % sample: "
                + ", ".join(f"{a} {float(r.detach()):.3f}" for a, r in rate.items()))
    if train_steps > 0:
        torch.save({a: sim.entropy_models[a].state_dict() for a in ATTRS}, models_path)
    else:
        for a, state in torch.load(models_path, map_location="cuda", weights_only=True).items():
            sim.entropy_models[a].load_state_dict(state, strict=True)
    splats["shN"] = splats["shN"][:, :0]  # no higher bands in the directory: their K-means is not what is measured here
    return splats, sim


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


def prepared(splats, sim):
    """The cropped, ordered splats, their 8-bit symbols and each attribute's model at the decoded means."""
    import torch

    from gscodec_studio_amd.compression import dequantize_grid, gauss_ans as GA, inverse_log_transform, quantize_grid
    from gscodec_studio_amd.compression._container import prepare_splats

    kept, side = prepare_splats(splats, 0.005, "morton", False)
    planes, m = quantize_grid(kept["means"], side, bits=16)
    pos = inverse_log_transform(dequantize_grid(planes, m))
    out = {}
    for a in ATTRS:
        (plane,), meta = quantize_grid(kept[a], side, bits=8)
        sym = plane.reshape(side * side, -1).contiguous()
        mu_q, k = GA.gaussian_params(sim.entropy_models[a], pos, meta["mins"], meta["maxs"])
        out[a] = dict(sym=sym, meta=meta, mu_q=mu_q, k=k)
    torch.cuda.synchronize()
    return side * side, pos, out


def step_params(say, splats, sim):
    import torch

    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd.compression import gauss_ans as GA

    n, pos, data = prepared(splats, sim)
    stream = torch.cuda.current_stream().cuda_stream
    say(f"params, N = {n} splats, min..max of 5:")
    for a in ATTRS:
        model, meta = sim.entropy_models[a], data[a]["meta"]
        pr = model.param_regressor
        c = pr.channel
        feat = pr.hash_grid((pos - pr.bound_min) / (pr.bound_max - pr.bound_min)).contiguous()
        w = [t.detach().float().contiguous() for t in (pr.mlp_regressor[0].weight, pr.mlp_regressor[0].bias, pr.mlp_regressor[2].weight,
                                                       pr.mlp_regressor[2].bias)]
        mins, maxs = (torch.tensor(meta[key], dtype=torch.float32, device="cuda") for key in ("mins", "maxs"))
        mu_q = torch.empty((c, n), dtype=torch.int16, device="cuda")
        k = torch.empty((c, n), dtype=torch.uint8, device="cuda")
        tau = GA._tables(torch.device("cuda"))[1]
        t = event_ms(lambda: B.call("gs_gauss_ans_params", n, c, B.ptr(feat), *[B.ptr(x) for x in w], B.ptr(mins), B.ptr(maxs), B.ptr(tau),
                                    B.ptr(mu_q), B.ptr(k), None, None, stream))
        assert torch.equal(mu_q.t(), data[a]["mu_q"]) and torch.equal(k.t(), data[a]["k"])
        say(f"  {a}: gs_gauss_ans_params alone ({c} channels)                          {t[0]:9.3f}..{t[1]:9.3f} ms")
        t = event_ms(lambda: GA.gaussian_params(model, pos, meta["mins"], meta["maxs"]))
        say(f"  {a}: gaussian_params (NaN check, encoder launch, params kernel)        {t[0]:9.3f}..{t[1]:9.3f} ms")


def step_coder(say, splats, sim):
    import numpy as np
    import torch

    from gscodec_studio_amd import _backend as B
    from gscodec_studio_amd.compression import gauss_ans as GA, gauss_ans_reference as R

    n, _, data = prepared(splats, sim)
    S = R.DEFAULT_STREAM_LEN
    stream = torch.cuda.current_stream().cuda_stream
    table = GA._tables(torch.device("cuda"))[0]
    bufs = {}
    for a, d in data.items():
        c = d["sym"].shape[1]
        nt = c * (-(-n // S))
        blob = GA.gauss_ans_encode(d["sym"], d["mu_q"], d["k"], stream_len=S)
        assert torch.equal(GA.gauss_ans_decode(blob, d["mu_q"], d["k"]), d["sym"])
        _, _, _, off, pay = R.parse_container(blob)
        bufs[a] = dict(c=c, cm=d["sym"].t().contiguous(), mu=d["mu_q"].t().contiguous(), k=d["k"].t().contiguous(),
                       scratch=torch.empty(int(B.query("gs_gauss_ans_encode_bytes", n, c, S)), dtype=torch.uint8, device="cuda"),
                       lengths=torch.empty(nt, dtype=torch.int32, device="cuda"), states=torch.empty(nt, dtype=torch.int32, device="cuda"),
                       status=torch.zeros(1, dtype=torch.int32, device="cuda"), payload=torch.from_numpy(np.array(pay)).cuda(),
                       off=torch.from_numpy(off).cuda(), out=torch.empty((n, c), dtype=torch.uint8, device="cuda"), blob=blob)

    def enc():
        for b in bufs.values():
            B.call("gs_gauss_ans_encode", n, b["c"], S, B.ptr(b["cm"]), B.ptr(b["mu"]), B.ptr(b["k"]), B.ptr(table), B.ptr(b["scratch"]),
                   b["scratch"].numel(), B.ptr(b["lengths"]), B.ptr(b["states"]), B.ptr(b["status"]), stream)

    def dec():
        for b in bufs.values():
            B.call("gs_gauss_ans_decode", n, b["c"], S, B.ptr(b["payload"]), b["payload"].numel(), B.ptr(b["off"]), B.ptr(b["mu"]),
                   B.ptr(b["k"]), B.ptr(table), B.ptr(b["out"]), stream)

    n_sym = 7 * n
    say(f"coder, both attributes = {n_sym} symbols, S = {S}, min..max of 5:")
    for tag, fn in (("gs_gauss_ans_encode", enc), ("gs_gauss_ans_decode", dec)):
        t = event_ms(fn)
        say(f"  {tag:70s} {t[0]:9.3f}..{t[1]:9.3f} ms   {n_sym / t[1] / 1e3:8.1f} Msymbols/s or more")
    for a, b in bufs.items():
        assert int(b["status"]) == 0 and torch.equal(b["out"], data[a]["sym"])
        assert int(b["lengths"].sum()) + 4 * b["lengths"].numel() == b["payload"].numel()


def step_files(say, splats, sim):
    import torch

    from gscodec_studio_amd.compression import EntropyCodingCompression

    reg = {a: {"encode": "_compress_gaussian_ans", "decode": "_decompress_gaussian_ans"} for a in ATTRS}
    codecs = {"gaussian": EntropyCodingCompression(use_sort="morton", verbose=False, n_clusters=256, attribute_codec_registry=reg),
              "factorized": EntropyCodingCompression(use_sort="morton", verbose=False, n_clusters=256)}
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {k: os.path.join(tmp, k) for k in codecs}
        times = {(k, op): [] for k in codecs for op in ("compress", "decompress")}
        out = {}
        for r in range(ROUNDS + 1):  # round 0 warms up
            for k, codec in codecs.items():
                tc = host_ms(lambda: codec.compress(dirs[k], splats, entropy_models=sim.entropy_models))
                td = host_ms(lambda: out.__setitem__(k, codec.decompress(dirs[k])))
                if r:
                    times[(k, "compress")].append(tc)
                    times[(k, "decompress")].append(td)
        assert all(torch.equal(out["gaussian"][a], out["factorized"][a]) for a in out["factorized"])
        say(f"files, whole calls on the full directory (means, opacities, sh0 as PNG, no shN), the two routes "
            f"alternating, min..max of {ROUNDS} rounds:")
        for (k, op), t in times.items():
            say(f"  {k:10s} {op:10s} {min(t):10.1f}..{max(t):10.1f} ms")
        say("size:")
        n_sym = 0
        for a in ATTRS:
            g_bin = os.path.getsize(os.path.join(dirs["gaussian"], f"{a}.bin"))
            g_side = sum(os.path.getsize(os.path.join(dirs["gaussian"], f)) for f in os.listdir(dirs["gaussian"]) if f.startswith(f"{a}_entropy_model_"))
            f_bin = os.path.getsize(os.path.join(dirs["factorized"], f"{a}.bin"))
            f_side = os.path.getsize(os.path.join(dirs["factorized"], f"{a}_prob.npy"))
            n_a = out["gaussian"][a].numel()
            n_sym += n_a
            say(f"  {a}: Gaussian route {g_bin} bytes of .bin ({8 * g_bin / n_a:.3f} bit/symbol) + {g_side} bytes of model files;  "
                f"factorized route {f_bin} bytes of .bin ({8 * f_bin / n_a:.3f} bit/symbol) + {f_side} bytes of table")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--train-steps", type=int, default=3000)
    ap.add_argument("--models", default=None, help="(internal) where the train step leaves the models")
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="(internal) run one step in this process")
    a = ap.parse_args()

    def say(line):
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if a.step is None:  # the driver: holds no GPU itself
        if a.out and os.path.exists(a.out):
            os.remove(a.out)
        say(f"tools/bench_gauss_ans.py: entropy models trained for {a.train_steps} steps of the rate term")
        with tempfile.TemporaryDirectory() as tmp:
            for step, limit in STEPS.items():
                cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--train-steps", str(a.train_steps), "--models",
                       os.path.join(tmp, "models.pt")] + (["--out", a.out] if a.out else [])
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

    assert torch.cuda.is_available(), "bench_gauss_ans needs a GPU"
    if a.step == "train":
        say(f"on {torch.cuda.get_device_name(0)}")
        setup(a.train_steps, a.models, say)
        return 0
    splats, sim = setup(0, a.models)
    {"params": step_params, "coder": step_coder, "files": step_files}[a.step](say, splats, sim)
    return 0


if __name__ == "__main__":
    sys.exit(main())
