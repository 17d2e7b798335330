"""Timing of the hash-grid Gaussian entropy model (csrc/hashgrid.hip) at config 2's size -- 1,006,065 splats, of which the
trainer samples 5 % (50,303) per step -- against a plain-torch restatement of the same arithmetic on the same GPU
(gathers whose autograd is index_put / index_add_, torch.distributions.Normal), alternating the two in one process.

Measured, at both sizes: the encoder forward and backward alone, the bits kernels forward and backward alone, a whole
Entropy_gaussian(3) forward + backward, and the share of that time spent in the regressor's torch launches (two GEMMs, ReLU
and their backward).  At the full size: the compression-simulation part of a training iteration (hooks, bits of the sample,
backward of the rate term, entropy-model optimizer steps; no rendering) with HashGridCompressionSimulation against the
factorized prior's CompressionSimulation, whose estimator runs on all splats.

Every figure is min..max of the per-round means of ROUNDS rounds; a difference is only called one where it exceeds the
summed spreads.  The torch restatement's input gradient is autograd's (the derivative of the renormalised forward), not the
reference's dy_dx formula: same work, other numbers near the border -- it is a yardstick for time only.

    python tools/bench_hashgrid.py [--out FILE]
"""
import argparse
import gc
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gscodec_studio_amd.compression_simulation import (CompressionSimulation, Entropy_gaussian,  # noqa: E402
                                                       HashGridCompressionSimulation, STE_binary)
from gscodec_studio_amd.compression_simulation.entropy_model import _GaussianBits  # noqa: E402

gc.collect()
gc.freeze()

N_ALL, N_SAMPLE = 1_006_065, 50_303
ROUNDS = 3
AXES = {"xyz": [0, 1, 2], "xy": [0, 1], "xz": [0, 2], "yz": [1, 2]}
PRIMES = (1, 2654435761, 805459861)


def torch_encode(u, encoders):
    """[N, 3] in [0, 1] -> [N, levels * F]: the kernel's arithmetic as torch ops (float32, device tensors)."""
    outs = []
    for name, enc in encoders:
        E = STE_binary.apply(enc.params)
        x = u[:, AXES[name]]
        oob = ~((x >= 0) & (x <= 1)).all(1)
        x = torch.where(oob[:, None], torch.full_like(x, 0.5), x)
        res, off = enc.host_lists()
        D = enc.num_dim
        for l, R in enumerate(res):
            T = off[l + 1] - off[l]
            p = x * float(R - 2) + 0.5
            g = torch.floor(p.detach())
            f, gi = p - g, g.long()
            acc, wn = 0.0, 0.0
            for i in range(1 << D):
                w, border, c = 1.0, torch.zeros_like(oob), []
                for d in range(D):
                    bit = (i >> d) & 1
                    cd = torch.clamp(gi[:, d] + 1, max=R - 1) if bit else gi[:, d]
                    w = w * (f[:, d] if bit else 1 - f[:, d])
                    border = border | (cd == 0) | (cd == R - 1)
                    c.append(cd)
                stride, index = 1, torch.zeros_like(c[0])
                for cd in c:
                    if stride <= T:
                        index = (index + cd * stride) & 0xFFFFFFFF
                        stride = (stride * R) & 0xFFFFFFFF
                if stride > T:
                    index = torch.zeros_like(c[0])
                    for cd, prime in zip(c, PRIMES):
                        index = index ^ ((cd * prime) & 0xFFFFFFFF)
                w = w * (~border)
                wn = wn + w
                acc = acc + w[:, None] * E[off[l] + index % T]
            wn = torch.where(wn == 0, torch.full_like(wn, 1e-9), wn)
            outs.append(torch.where(oob[:, None], torch.zeros_like(acc), acc / wn[:, None]))
    return torch.cat(outs, 1)


def torch_bits(x, net, q, lower_bound):
    C = x.shape[1]
    m1 = torch.distributions.normal.Normal(net[:, :C], torch.clamp(net[:, C:], min=1e-9))
    like = torch.abs(m1.cdf(x + 0.5 * q) - m1.cdf(x - 0.5 * q))
    return -torch.log2(lower_bound(like))


def mean_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


class Table:
    def __init__(self, out):
        self.out = out
        self.lines = []

    def say(self, line=""):
        print(line, flush=True)
        self.lines.append(line)
        if self.out:
            with open(self.out, "w") as f:
                f.write("\n".join(self.lines) + "\n")

    def versus(self, label, hip, ref, iters=(20, 5), ref_name="torch"):
        """Alternate the two for ROUNDS rounds -> (hip min, hip max, ref min, ref max) in ms."""
        for fn in (hip, ref):  # warm-up of every shape
            fn()
            fn()
        a, b = [], []
        for _ in range(ROUNDS):
            a.append(mean_ms(hip, iters[0]))
            b.append(mean_ms(ref, iters[1]))
        lo = min(b) / max(a)
        verdict = f"{lo:.1f}x or more" if min(b) - max(a) > (max(a) - min(a)) + (max(b) - min(b)) and lo > 1 else (
            "slower" if min(a) - max(b) > (max(a) - min(a)) + (max(b) - min(b)) else "no difference beyond the spreads")
        self.say(f"{label:58s} HIP {min(a):8.3f}..{max(a):8.3f} ms   {ref_name} {min(b):8.3f}..{max(b):8.3f} ms   {verdict}")
        return min(a), max(a), min(b), max(b)


def model_and_inputs(n, channel=3):
    torch.manual_seed(0)
    m = Entropy_gaussian(channel).cuda()
    with torch.no_grad():
        for _, e in m.param_regressor.hash_grid._encoders():
            e.params.copy_(0.7 * torch.randn_like(e.params))
        m.param_regressor.mlp_regressor[2].bias[channel:] += 1.0
    pos = ((torch.rand(n, 3, device="cuda") * 2 - 1) * 95).requires_grad_(True)
    x = (0.5 * torch.randn(n, channel, device="cuda")).requires_grad_(True)
    return m, pos, x


def clear(*tensors):
    for t in tensors:
        t.grad = None


def bench_size(tab, n):
    tab.say(f"--- N = {n:,} points, Entropy_gaussian(3), reference configuration (24 levels x 2 features, 441,568 table rows) ---")
    m, pos, x = model_and_inputs(n)
    pr = m.param_regressor
    hg, encoders = pr.hash_grid, pr.hash_grid._encoders()
    tables = [e.params for _, e in encoders]
    q, bound = 12 / 255, 1e-6
    u = ((pos.detach() - pr.bound_min) / (pr.bound_max - pr.bound_min)).requires_grad_(True)
    with torch.no_grad():
        d = float((hg(u) - torch_encode(u, encoders)).abs().max())
    tab.say(f"encoder: max |HIP - torch restatement| = {d:.2e}")

    with torch.no_grad():
        tab.versus("encoder forward", lambda: hg(u), lambda: torch_encode(u, encoders))
    v = torch.randn(n, hg.output_dim, device="cuda")
    out_h, out_t = hg(u), torch_encode(u, encoders)

    def bwd(out):
        clear(u, *tables)
        out.backward(v, retain_graph=True)

    tab.versus("encoder backward (tables + positions)", lambda: bwd(out_h), lambda: bwd(out_t))
    del out_h, out_t

    net = pr.regress(pos.detach()).detach().requires_grad_(True)
    hq = torch.full((3,), 0.5 * q, device="cuda")
    with torch.no_grad():
        tab.versus("bits forward", lambda: _GaussianBits.apply(x, net, hq, bound), lambda: torch_bits(x, net, q, m.likelihood_lower_bound), (50, 20))
    vb = torch.rand(n, 3, device="cuda") + 0.5
    b_h, b_t = _GaussianBits.apply(x, net, hq, bound), torch_bits(x, net, q, m.likelihood_lower_bound)

    def bwd_bits(b):
        clear(x, net)
        b.backward(vb, retain_graph=True)

    tab.versus("bits backward", lambda: bwd_bits(b_h), lambda: bwd_bits(b_t), (50, 20))
    del b_h, b_t

    def whole_hip():
        clear(x, pos, *m.parameters())
        m(x, q, pos=pos).backward(vb)

    def whole_torch():
        clear(x, pos, *m.parameters())
        uu = (pos - pr.bound_min) / (pr.bound_max - pr.bound_min)
        torch_bits(x, pr.mlp_regressor(torch_encode(uu, encoders)), q, m.likelihood_lower_bound).backward(vb)

    w = tab.versus("whole model forward + backward", whole_hip, whole_torch)
    feats = hg(u).detach().requires_grad_(True)
    vn = torch.randn(n, 6, device="cuda")

    def mlp_only():
        clear(feats, *pr.mlp_regressor.parameters())
        pr.mlp_regressor(feats).backward(vn)

    mlp_only()
    t = [mean_ms(mlp_only, 20) for _ in range(ROUNDS)]
    tab.say(f"{'regressor MLP forward + backward alone (torch launches)':58s}     {min(t):8.3f}..{max(t):8.3f} ms   = "
            f"{100 * min(t) / w[1]:.0f}..{100 * max(t) / w[0]:.0f} % of the whole-model HIP time")


def bench_iteration(tab):
    n = N_ALL
    tab.say(f"--- compression-simulation part of a training iteration, {n:,} splats (no rendering) ---")
    steps = {"means": -1, "scales": 1, "quats": 1, "opacities": -1, "sh0": 1, "shN": -1}
    torch.manual_seed(1)
    P = lambda t: torch.nn.Parameter(t.cuda())  # noqa: E731
    splats = {"means": P(torch.randn(n, 3) * 3), "scales": P(torch.randn(n, 3) - 4), "quats": P(torch.randn(n, 4)),
              "opacities": P(torch.randn(n)), "sh0": P(torch.rand(n, 1, 3)), "shN": P(0.05 * torch.randn(n, 15, 3))}
    sims = {"hashgrid": HashGridCompressionSimulation(entropy_model_enable=True, entropy_steps=steps, device="cuda"),
            "factorized": CompressionSimulation(entropy_model_enable=True, entropy_steps=steps, device="cuda")}
    with torch.no_grad():
        sims["hashgrid"]._estiblish_bbox(splats["means"][:1_000_000])  # (torch.quantile's input limit is 16M elements)

    def iteration(sim):
        def run():
            clear(*splats.values())
            _, bits = sim.simulate_compression(splats, step=10)
            sum(b.sum() / b.numel() for b in bits.values() if b is not None).backward()
            for k, opt in sim.entropy_model_optimizers.items():
                if opt is not None:
                    opt.step()
                    opt.zero_grad(set_to_none=True)
        return run

    tab.versus("hooks + rate term + entropy optimizers", iteration(sims["hashgrid"]), iteration(sims["factorized"]), (10, 10),
               ref_name="factorized prior")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_hashgrid needs a GPU"
    tab = Table(args.out)
    tab.say(f"tools/bench_hashgrid.py on {torch.cuda.get_device_name(0)}: min..max of {ROUNDS} alternating rounds")
    bench_size(tab, N_SAMPLE)
    bench_size(tab, N_ALL)
    bench_iteration(tab)


if __name__ == "__main__":
    main()
