"""GPU parity of the fused factorized-prior bits estimator (gs_entropy_factorized_fwd/bwd) against the
float64 oracle and the golden vectors recorded from the reference module.

Tolerance: the reference (fp32 torch) itself deviates from exact arithmetic by up to ~3e-3 bits where the
two sigmoids nearly cancel (tests/golden/make_golden_entropy.py prints it), so bits are compared with
|err| <= 1e-4 |bits| + 4e-3; gradients with 1e-4 relative to the tensor's scale plus the same floor idea.

Beyond the golden fixtures (N <= 1024: one workgroup per (chunk, channel), one busy wave) the seeded cases of
tests/test_entropy_cpu.py::recipe are run at every compiled (layers, width) instance, at channel counts up to 32 and at
the smallest shapes that reach each path of the backward (CASES_C).  Ground truth is the float64 oracle, which
test_entropy_cpu.py pins against torch autograd on the same recipe.  Parameter gradients are held to
    rel_l2(HIP, f64) <= FACTOR * rel_l2(fp32 oracle, f64) + 2e-6     and     rel_l2(HIP, f64) <= 2e-2,
the first as in tests/test_gpu_parity_f64.py (the oracle sums in numpy's pairwise order, the kernel in fp32 registers,
wave sums and float atomics; the kernel's exp2 / rcp / log are the hardware units, the oracle's are libm), the second an
absolute cap far below the smallest structural fault (one wave of a 626-row run, one workgroup of five: >= 10 %).

Measured on an MI355X with this file (rel_l2 against float64, per tensor; 390 tensor/case pairs, all printed by the tests):
  case group                          e_hip              e_orc (fp32 oracle)   worst e_hip/e_orc   worst e_hip/bar
  16 instances, N 3001 C 3            4e-07 .. 4.3e-06   2e-07 .. 5e-06        4.66 (L3 W2 _matrices[0]: 1.2e-06 / 2.6e-07)   0.40
  channels 1..32, N 3001              5e-07 .. 3.1e-06   2e-07 .. 4e-06        5.26 (C 1 _matrices[0]: 1.2e-06 / 2.2e-07)     0.40
  loop / blocks / both / full / pad   4e-07 .. 1.4e-06   3e-07 .. 2.7e-06      1.74 (blocks _matrices[0])                     0.18
  halving 8191 / 8192                 4e-07 .. 1.0e-06   3e-07 .. 1e-06        2.87 (8192 _matrices[0]: 8.7e-07 / 3.0e-07)    0.27
  tiny 1 / 31 / 32 / 33               7e-06 .. 7.1e-05   4e-06 .. 6e-05        1.59 (31 _factor[0])                           0.35
  boundary rows (5 cases)             1e-06 .. 5.8e-06   5e-07 .. 6e-06        2.29 (pad _matrices[0]: 1.2e-06 / 5.3e-07)     0.30
  C ABI, replicas 1 / 7 / 32          5e-07 .. 1.5e-05   4e-07 .. 1.3e-05      1.93 (replicas 1 _matrices[0])                 0.20
FACTOR stays 4: the two ratios above 4 are tensors whose errors (1.2e-06) are both under the 2e-6 floor, where the ratio
is one rounding pattern over another; wherever e_hip exceeds the floor the ratio is at most 1.6, and no tensor uses more
than 40 % of its bar.  The hardware exp2 / rcp / log and tanh_fast cost no visible digits in the gradients.
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from util import N, T, golden, rel_l2

pytestmark = pytest.mark.gpu

from oracle import entropy_oracle as EO  # noqa: E402
from test_entropy_cpu import BOUND, CASES, bound_masks, load_case, recipe  # noqa: E402

FACTOR = 4.0  # see the module docstring
CAP = 2e-2


def build_module(gd, name):
    from gscodec_studio_amd.compression_simulation import Entropy_factorized_optimized_refactor as M

    mats, biases, factors = load_case(gd, name)
    m = M(channel=mats[0].shape[0], filters=tuple(int(f) for f in gd[f"{name}.filters"]))
    with torch.no_grad():
        for dst, src in ((m._matrices, mats), (m._bias, biases), (m._factor, factors)):
            for p, a in zip(dst, src):
                p.copy_(torch.from_numpy(a))
    return m.cuda(), mats, biases, factors


@pytest.mark.parametrize("name", [c for c in CASES if c != "wide"])  # "wide" = non-uniform widths, rejected
def test_bits_and_gradients_vs_oracle_and_reference(name):
    gd = golden("entropy.npz")
    m, mats, biases, factors = build_module(gd, name)
    x = T(gd[f"{name}.x"]).requires_grad_(True)
    q = gd[f"{name}.q"]
    Q = float(q) if q.ndim == 0 else T(q)
    bits = m(x, Q)
    ob = EO.factorized_bits_fwd(gd[f"{name}.x"], q, mats, biases, factors)
    err = np.abs(N(bits) - ob)
    assert np.all(err <= 1e-4 * np.abs(ob) + 4e-3), float(err.max())
    ref = gd[f"{name}.bits"]
    assert np.all(np.abs(N(bits) - ref) <= 2e-4 * np.abs(ref) + 6e-3)
    vb = gd[f"{name}.v_bits"]
    (bits * T(vb)).sum().backward()
    gx, gm, gb, gf = EO.factorized_bits_bwd(gd[f"{name}.x"], q, mats, biases, factors, vb)
    bad = np.abs(N(x.grad) - gx) > 2e-3 * (np.abs(gx) + np.abs(gx).mean())
    assert bad.mean() < 0.005, float(bad.mean())

    def close(got, want, what):
        scale = np.abs(want).max() + 1e-12
        e = np.abs(N(got) - want).max() / scale
        assert e < 2e-3, (what, e)

    for i in range(len(mats)):
        close(m._matrices[i].grad, gm[i], f"v_mat{i}")
        close(m._bias[i].grad, gb[i], f"v_bias{i}")
    for i in range(len(factors)):
        close(m._factor[i].grad, gf[i], f"v_factor{i}")
    # and against the reference's own autograd numbers
    for i in range(len(mats)):
        close(m._matrices[i].grad, gd[f"{name}.v_mat{i}"], f"ref v_mat{i}")


def test_large_ragged_sizes_and_lower_bound():
    """Sizes that are not multiples of 32 / of the block run, N % 32 == 0 (the reference then pads a full 32),
    and inputs deep in the tails (likelihood clamped at 1e-6 -> exactly -log2(1e-6) bits, gated gradient)."""
    from gscodec_studio_amd.compression_simulation import Entropy_factorized_optimized_refactor as M

    torch.manual_seed(0)
    np.random.seed(0)
    for n, C, filters in [(100_003, 3, (3, 3)), (65_536, 4, (3, 3, 3)), (31, 1, (3, 3, 3)), (1, 3, (3, 3))]:
        m = M(channel=C, filters=filters).cuda()
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.3 * torch.randn_like(p))
        x = (torch.rand(n, C, device="cuda") * 8 - 4).requires_grad_(True)
        with torch.no_grad():
            x[0, 0] = 300.0
        bits = m(x, 0.05)
        mats = [N(p) for p in m._matrices]
        biases = [N(p) for p in m._bias]
        factors = [N(p) for p in m._factor]
        ob = EO.factorized_bits_fwd(N(x), np.float32(0.05), mats, biases, factors)
        assert np.all(np.abs(N(bits) - ob) <= 1e-4 * np.abs(ob) + 4e-3)
        assert abs(float(bits[0, 0].detach()) - (-np.log2(1e-6))) < 1e-4
        bits.sum().backward()  # positive upstream gradient on a clamped element: incoming d/dlik < 0 -> passes
        assert bool(torch.isfinite(x.grad).all())
        x.grad = None
        (-m(x, 0.05)).sum().backward()  # negative upstream gradient: blocked at the bound
        assert float(x.grad[0, 0]) == 0.0


def test_simulation_hooks_return_bits_after_entropy_step():
    from gscodec_studio_amd.compression_simulation import CompressionSimulation

    steps = {"means": -1, "scales": 10, "quats": 10, "opacities": -1, "sh0": 20, "shN": -1}
    sim = CompressionSimulation(entropy_model_enable=True, entropy_steps=steps, device="cuda")
    n = 5000
    splats = {
        "means": torch.randn(n, 3, device="cuda"),
        "scales": torch.nn.Parameter(torch.randn(n, 3, device="cuda") - 4),
        "quats": torch.nn.Parameter(torch.randn(n, 4, device="cuda")),
        "opacities": torch.nn.Parameter(torch.randn(n, device="cuda")),
        "sh0": torch.nn.Parameter(torch.rand(n, 1, 3, device="cuda")),
        "shN": torch.nn.Parameter(torch.randn(n, 15, 3, device="cuda") * 0.05),
    }
    out, bits = sim.simulate_compression(splats, step=5)
    assert all(v is None for v in bits.values())
    out, bits = sim.simulate_compression(splats, step=15)
    assert bits["scales"].shape == (n, 3) and bits["quats"].shape == (n, 4) and bits["sh0"] is None and bits["opacities"] is None
    out, bits = sim.simulate_compression(splats, step=25)
    assert bits["sh0"].shape == (n, 3) and out["sh0"].shape == (n, 1, 3) and out["opacities"].shape == (n,)
    total = sum(b.sum() / b.numel() for b in bits.values() if b is not None)  # the trainer's bpp term (simple_trainer.py:992-1002)
    total.backward()
    assert splats["scales"].grad is not None and bool(torch.isfinite(splats["scales"].grad).all())
    g = sim.entropy_models["scales"]._matrices[0].grad
    assert g is not None and float(g.abs().sum()) > 0
    sim.entropy_model_optimizers["scales"].step()


# ---------------------------------------------------------------------------------------------------------------------
# seeded cases against the float64 oracle


def rows_per_block(n, C):
    """Mirrors launch_entropy (csrc/entropy.hip) and must follow it: 4096 rows per workgroup, halved down to 256 while the
    grid has fewer than 1024 workgroups."""
    chunk, rows = EO.chunk_len(n), 4096
    while rows > 256 and 32 * C * math.ceil(chunk / rows) < 1024:
        rows //= 2
    return rows


def boundary_rows(n, C):
    """First and last row of every chunk, of every rows_per_block run inside a chunk and of every 256-row pass (one
    iteration of the 256 threads' loop) inside a run.  Mirrors entropy_kernel's row0 / row_end and must follow it."""
    chunk, rpb = EO.chunk_len(n), rows_per_block(n, C)
    rows = set()
    for j in range(32):
        for r0 in range(j * chunk, min((j + 1) * chunk, n), rpb):
            r1 = min(r0 + rpb, (j + 1) * chunk, n)
            for q0 in range(r0, r1, 256):
                rows.update((q0, min(q0 + 256, r1) - 1))
    return np.array(sorted(rows))


def test_case_table_matches_the_launch_rule():
    """The shapes of CASES_C reach what their comments claim, by the mirrored launch rule."""
    geo = lambda n, C: (EO.chunk_len(n), rows_per_block(n, C), math.ceil(EO.chunk_len(n) / rows_per_block(n, C)))  # noqa: E731
    assert geo(20_000, 32) == (626, 4096, 1) and 626 - 2 * 256 == 114
    assert geo(40_003, 3) == (1251, 256, 5) and 1251 - 4 * 256 == 227
    assert geo(70_001, 16) == (2188, 2048, 2)
    assert geo(131_105, 32) == (4098, 4096, 2)
    assert geo(65_536, 4) == (2049, 256, 9) and 31 * 2049 < 65_536 < 32 * 2049
    assert geo(8_191, 3) == (256, 256, 1) and geo(8_192, 3) == (257, 256, 2)
    assert [EO.chunk_len(n) for n in (1, 31, 32, 33)] == [1, 1, 2, 2]
    assert geo(3_001, 3) == (94, 256, 1)
    rows = boundary_rows(40_003, 3)
    assert rows[0] == 0 and rows[-1] == 40_002 and {1250, 1251, 255, 256, 1023, 1024}.issubset(rows.tolist())
    assert 65_535 in boundary_rows(65_536, 4).tolist()


@functools.lru_cache(maxsize=None)
def reference(n, C, filters, per_channel=False):
    """float64 oracle (bits, likelihood before the bound, gradients) and the fp32 oracle's parameter gradients of one
    recipe; computed once per case and shared.  Do not modify."""
    rc = recipe(n, C, filters, per_channel)
    args = (rc["x"], rc["q"], rc["mats"], rc["biases"], rc["factors"], rc["v_bits"])
    gx, gm, gb, gf, bits, lik = EO.factorized_bits_bwd(*args, return_fwd=True)
    g32 = EO.factorized_bits_bwd(*args, dtype=np.float32)[1:]
    return dict(rc=rc, bits=bits, lik=lik, v_x=gx, grads=(gm, gb, gf), grads32=g32)


def run_module(rc, x, v_bits):
    """Forward and backward through the module on the GPU -> bits, v_x, (v_matrices, v_bias, v_factor) as numpy."""
    m = copy.deepcopy(rc["module"]).cuda()
    xt = T(x).requires_grad_(True)
    bits = m(xt, float(rc["q"]) if rc["q"].ndim == 0 else T(rc["q"]))
    bits.backward(T(v_bits))
    return N(bits), N(xt.grad), tuple([N(p.grad) for p in ps] for ps in (m._matrices, m._bias, m._factor))


def check_params(label, got, f64, f32):
    for kind, g, w, o in zip(("_matrices", "_bias", "_factor"), got, f64, f32):
        for i in range(len(w)):
            assert g[i].shape == w[i].shape
            e_hip, e_orc = rel_l2(g[i], w[i]), rel_l2(o[i], w[i])
            print(f"[entropy f64] {label:34s} {kind}[{i}] rel_l2: HIP {e_hip:.2e}  fp32 oracle {e_orc:.2e}  ratio {e_hip / max(e_orc, 1e-30):.2f}")
            assert e_hip <= FACTOR * e_orc + 2e-6, (label, kind, i, e_hip, e_orc)
            assert e_hip <= CAP, (label, kind, i, e_hip)


def vx_mismatch(got, want):
    return np.abs(got - want) > 2e-3 * (np.abs(want) + np.abs(want).mean())


def check_outputs(ref, bits, v_x):
    rc, ob, gx = ref["rc"], ref["bits"], ref["v_x"]
    clamped, borderline = bound_masks(ref["lik"])
    assert borderline.mean() <= 1e-3, borderline.mean()
    keep = ~borderline
    err = np.abs(bits - ob)
    assert np.all(err <= 1e-4 * np.abs(ob) + 4e-3), float(err.max())
    assert np.all(np.abs(bits[clamped & keep] - (-np.log2(BOUND))) <= 1e-4)
    # v_x is an uninitialised buffer: a row the kernel skips shows up as an entry the oracle does not match
    assert np.isfinite(v_x).all()
    bad = vx_mismatch(v_x, gx) & keep
    assert bad.mean() <= 0.005, float(bad.mean())
    # g_lik_b = -v_bits / (ln 2 lik_b): a negative upstream gradient is blocked at the bound, a positive one passes
    blocked, passing = clamped & keep & (rc["v_bits"] < 0), clamped & keep & (rc["v_bits"] > 0)
    assert np.all(v_x[blocked] == 0.0)
    assert not bad[blocked].any() and not bad[passing].any()


def check_case(label, n, C, filters, per_channel=False):
    ref = reference(n, C, tuple(filters), per_channel)
    rc = ref["rc"]
    bits, v_x, grads = run_module(rc, rc["x"], rc["v_bits"])
    check_outputs(ref, bits, v_x)
    check_params(label, grads, ref["grads"], ref["grads32"])


@pytest.mark.parametrize("L,W", [(l, w) for l in range(1, 5) for w in range(1, 5)])
def test_every_compiled_instance(L, W):
    check_case(f"instance L{L} W{W}", 3001, 3, (W,) * L)


@pytest.mark.parametrize("C", [1, 2, 5, 7, 16, 31, 32])
def test_every_channel_mapping(C):
    """p = (32 c + j) % C at channel counts the fixtures do not have; a per-channel Q for C = 5 and 7."""
    check_case(f"channels {C}", 3001, C, (3, 3), per_channel=C in (5, 7))


# name -> (N, C, filters): the smallest shapes that reach each path of the backward (geometry asserted in
# test_case_table_matches_the_launch_rule)
CASES_C = {
    # rows_per_block 4096, chunk 626: one workgroup per pair, threads loop 3 times, last pass 114 rows (waves 2, 3 partly idle)
    "loop": (20_000, 32, (3, 3, 3)),
    # rows_per_block 256, chunk 1251: 5 workgroups per pair, the last with 227 rows; 480 workgroups over 32 replicas
    "blocks": (40_003, 3, (3, 3)),
    # rows_per_block 2048, chunk 2188: 2 workgroups per pair, 8 loop passes in the first
    "both": (70_001, 16, (1,)),
    # rows_per_block 4096, chunk 4098: the second workgroup of a pair has 2 rows
    "full": (131_105, 32, (2,)),
    # N % 32 == 0: chunk 2049, 9 workgroups per pair (the last with 1 row); 32 * 2049 > N, so the last chunk is short (2017
    # rows) and its row_end is clamped by n.  No chunk is EMPTY at this size (the issue's table says "short or empty"):
    # empty chunks come with the tiny sizes below (N = 33: chunks 17..31)
    "pad": (65_536, 4, (4, 4, 4, 4)),
    # chunk 256 and 257: one versus two workgroups per pair at rows_per_block 256
    "halving-8191": (8_191, 3, (3, 3)),
    "halving-8192": (8_192, 3, (3, 3)),
    # chunk 1 or 2, most workgroups empty
    "tiny-1": (1, 5, (2, 2)),
    "tiny-31": (31, 5, (2, 2)),
    "tiny-32": (32, 5, (2, 2)),
    "tiny-33": (33, 5, (2, 2)),
}


@pytest.mark.parametrize("case", list(CASES_C))
def test_backward_paths(case):
    check_case(case, *CASES_C[case])


@pytest.mark.parametrize("case", ["loop", "blocks", "both", "full", "pad"])
def test_boundary_rows_carry_the_gradient(case):
    """Upstream gradient only on the first and last row of every chunk, run and 256-row pass: a dropped or doubled
    boundary row changes its parameter set's gradient by a fraction of order one (in the full runs it is below any L2 bar)."""
    n, C, filters = CASES_C[case]
    rc = recipe(n, C, filters)
    rows = boundary_rows(n, C)
    vb = np.zeros_like(rc["v_bits"])
    vb[rows] = rc["v_bits"][rows]
    x = rc["x_body"]  # no tails: every term is finite, so zero upstream gradient gives exactly zero
    _, v_x, grads = run_module(rc, x, vb)
    args = (x[rows], rc["q"], rc["mats"], rc["biases"], rc["factors"], vb[rows])
    gx, *g64 = EO.factorized_bits_bwd(*args, rows=rows, n_total=n)
    g32 = EO.factorized_bits_bwd(*args, rows=rows, n_total=n, dtype=np.float32)[1:]
    check_params(f"{case} boundary rows", grads, g64, g32)
    assert not vx_mismatch(v_x[rows], gx).any()
    rest = np.ones(n, bool)
    rest[rows] = False
    assert np.all(v_x[rest] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI directly

GUARD = 4096          # floats on each side of an output buffer
SENTINEL = 0x7FC0BEEF  # a NaN bit pattern no kernel produces


def guarded(numel, fill=None):
    """-> (whole allocation, interior view of `numel` floats); everything not filled holds SENTINEL."""
    whole = torch.empty(numel + 2 * GUARD, dtype=torch.float32, device="cuda")
    whole.view(torch.int32).fill_(SENTINEL)
    inner = whole[GUARD:GUARD + numel]
    if fill is not None:
        inner.fill_(fill)
    return whole, inner


def guards_intact(whole, numel):
    torch.cuda.synchronize()
    w = whole.view(torch.int32)
    return bool((w[:GUARD] == SENTINEL).all()) and bool((w[GUARD + numel:] == SENTINEL).all())


def untouched(whole):
    torch.cuda.synchronize()
    return bool((whole.view(torch.int32) == SENTINEL).all())


def unpack(packed, filters):
    """[C, P] in the kernel's layout (per layer [matrix row-major | bias | factor]) -> the module's tensors."""
    C, widths, o = packed.shape[0], (1,) + tuple(filters) + (1,), 0
    mats, biases, factors = [], [], []
    for i in range(len(filters) + 1):
        wi, wo = widths[i], widths[i + 1]
        mats.append(packed[:, o:o + wo * wi].reshape(C, wo, wi))
        o += wo * wi
        biases.append(packed[:, o:o + wo].reshape(C, wo, 1))
        o += wo
        if i < len(filters):
            factors.append(packed[:, o:o + wo].reshape(C, wo, 1))
            o += wo
    assert o == packed.shape[1]
    return mats, biases, factors


class Abi:
    """Arguments of the two entry points for one recipe; fwd() / bwd() take overrides by name (pointers as tensors or None)."""

    def __init__(self, rc):
        self.rc, self.n, self.C, self.filters = rc, rc["n"], rc["C"], rc["filters"]
        self.params = rc["module"].packed_parameters().detach().cuda()
        self.P = self.params.shape[1]
        self.base = dict(n=self.n, channels=self.C, layers=len(self.filters), width=self.filters[0], x=T(rc["x"]),
                         half_q=T(np.broadcast_to(0.5 * rc["q"], (self.C,)).astype(np.float32)), params=self.params,
                         v_bits=T(rc["v_bits"]), replicas=32)

    def _run(self, name, keys, over):
        from gscodec_studio_amd import _backend as B

        a = dict(self.base, **over)
        vals = [B.ptr(a[k]) if isinstance(a[k], torch.Tensor) or a[k] is None else a[k] for k in keys]
        B.call(name, *vals, B.current_stream(torch.device("cuda:0")))

    def fwd(self, **over):
        self._run("gs_entropy_factorized_fwd", ("n", "channels", "layers", "width", "x", "half_q", "params", "bound", "bits"),
                  dict(over, bound=float(BOUND)))

    def bwd(self, **over):
        self._run("gs_entropy_factorized_bwd", ("n", "channels", "layers", "width", "x", "half_q", "params", "bound", "v_bits",
                                                "v_x", "v_params", "replicas"), dict(over, bound=float(BOUND)))


@pytest.mark.parametrize("n", [31, 40_003, 65_536])
def test_abi_writes_stay_inside_the_buffers(n):
    ref = reference(n, 3, (3, 3))
    abi = Abi(ref["rc"])
    E, R = n * 3, 32 * 3 * abi.P
    bits_w, bits = guarded(E)
    vx_w, v_x = guarded(E)
    vp_w, v_params = guarded(R, fill=0.0)
    abi.fwd(bits=bits)
    abi.bwd(v_x=v_x, v_params=v_params)
    assert guards_intact(bits_w, E) and guards_intact(vx_w, E) and guards_intact(vp_w, R)
    check_outputs(ref, N(bits).reshape(n, 3), N(v_x).reshape(n, 3))
    total = N(v_params.view(32, 3, abi.P).double().sum(0))
    check_params(f"abi N={n}", unpack(total, (3, 3)), ref["grads"], ref["grads32"])


def test_abi_replicas_add_into_the_buffer():
    """The kernel spreads its atomics over `replicas` copies and ADDS: the host wrapper sums the copies of a zeroed buffer."""
    n, C, filters = CASES_C["blocks"]
    ref = reference(n, C, filters)
    abi = Abi(ref["rc"])
    E, CP = n * C, C * abi.P
    totals, v_xs = {}, []
    for r in (1, 7, 32):
        whole, v_params = guarded(r * CP, fill=0.0)
        v_x = torch.empty(E, dtype=torch.float32, device="cuda")
        abi.bwd(v_x=v_x, v_params=v_params, replicas=r)
        assert guards_intact(whole, r * CP)
        copies = v_params.view(r, CP)
        if r == 32:
            assert int((copies != 0).any(1).sum()) > 1
        totals[r] = N(copies.double().sum(0)).reshape(C, abi.P)
        check_params(f"abi replicas={r}", unpack(totals[r], filters), ref["grads"], ref["grads32"])
        v_xs.append(v_x)
    assert torch.equal(v_xs[0], v_xs[1]) and torch.equal(v_xs[0], v_xs[2])
    for r in (7, 32):  # only the fp32 summation order differs
        assert rel_l2(totals[r], totals[1]) <= 1e-5, (r, rel_l2(totals[r], totals[1]))
    # a pre-filled buffer comes back as constant + gradient.  The constant is the power of two next to the gradient's rms, so
    # that overwriting instead of adding is an error of order one; carrying it makes each of the <= 160 adds into an entry
    # (480 workgroups, 3 parameter sets) round at up to 2^-24 (const + |partial sum|) instead of 2^-24 |partial sum|:
    # 160 * 2^-24 * const <= 9.5e-6 * sqrt(2) rms per entry on top of the 1e-5 of a different summation order
    g = totals[1]
    const = 2.0 ** round(math.log2(np.sqrt((g * g).mean())))
    whole, v_params = guarded(CP, fill=const)
    abi.bwd(v_x=torch.empty(E, dtype=torch.float32, device="cuda"), v_params=v_params, replicas=1)
    assert guards_intact(whole, CP)
    back = N(v_params.double()).reshape(C, abi.P) - const
    assert rel_l2(back, g) <= 2.5e-5, rel_l2(back, g)


def test_abi_rejections_and_empty_input_write_nothing():
    abi = Abi(recipe(*CASES_C["blocks"]))
    E, R = abi.n * abi.C, 32 * abi.C * abi.P
    outs = dict(bits=guarded(E), v_x=guarded(E), v_params=guarded(R))
    ptrs = {k: v[1] for k, v in outs.items()}
    both = [(abi.fwd, dict(bits=ptrs["bits"])), (abi.bwd, dict(v_x=ptrs["v_x"], v_params=ptrs["v_params"]))]
    bad = [(dict(channels=0), "channels must be in 1..32"), (dict(channels=33), "channels must be in 1..32"),
           (dict(layers=0), "unsupported filters"), (dict(layers=5), "unsupported filters"),
           (dict(width=0), "unsupported filters"), (dict(width=5), "unsupported filters"),
           (dict(x=None), "null pointer"), (dict(half_q=None), "null pointer"), (dict(params=None), "null pointer")]
    for fn, out in both:
        for over, text in bad:
            with pytest.raises(RuntimeError, match=rf"status [1-9].*{text}"):
                fn(**dict(out, **over))
    with pytest.raises(RuntimeError, match=r"status [1-9].*null pointer"):
        abi.fwd(bits=None)
    for k in ("v_bits", "v_x", "v_params"):
        with pytest.raises(RuntimeError, match=r"status [1-9].*null pointer"):
            abi.bwd(**dict(both[1][1], **{k: None}))
    with pytest.raises(RuntimeError, match=r"status [1-9].*replicas"):
        abi.bwd(replicas=0, **both[1][1])
    for fn, out in both:  # empty input: status 0 (no exception), nothing launched
        fn(n=0, **out)
    assert all(untouched(w) for w, _ in outs.values())


# ---------------------------------------------------------------------------------------------------------------------
# module-level behaviour the kernel depends on


def small_module():
    rc = recipe(3001, 3, (3, 3))
    return rc, copy.deepcopy(rc["module"]).cuda()


def test_non_contiguous_input_and_its_gradient():
    rc, m = small_module()
    wide = torch.zeros(3001, 6, device="cuda")
    wide[:, ::2] = T(rc["x"])
    wide.requires_grad_(True)
    xc = T(rc["x"]).requires_grad_(True)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    b_view, b_cont = m(view, 0.05), m(xc, 0.05)
    assert torch.equal(b_view, b_cont)
    vb = T(rc["v_bits"])
    b_view.backward(vb)
    b_cont.backward(vb)
    assert torch.equal(wide.grad[:, ::2], xc.grad) and bool((wide.grad[:, 1::2] == 0).all())


def test_expanded_cotangent_equals_explicit_ones():
    rc, m = small_module()
    grads = []
    for how in ("sum", "ones"):
        m.zero_grad(set_to_none=True)
        x = T(rc["x"]).requires_grad_(True)
        bits = m(x, 0.05)
        if how == "sum":
            bits.sum().backward()  # autograd sends a stride-0 expanded cotangent
        else:
            bits.backward(torch.ones_like(bits))
        grads.append((x.grad, [N(p.grad) for p in m.parameters()]))
    assert torch.equal(grads[0][0], grads[1][0])
    for a, b in zip(grads[0][1], grads[1][1]):
        assert rel_l2(a, b) <= 1e-5  # float atomics: the order of the sum differs from run to run


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_precision_input_is_widened(dtype):
    rc, m = small_module()
    x = T(rc["x"]).to(dtype)
    assert torch.equal(m(x, 0.05), m(x.float(), 0.05))


def test_likelihood_q_forms_and_stream():
    rc, m = small_module()
    x = T(rc["x"])
    with torch.no_grad():
        bits = m(x, 0.05)
        assert torch.equal(m.get_likelihood(x, 0.05), torch.exp2(-bits))
        assert torch.equal(m(x, torch.tensor([0.05])), bits) and torch.equal(m(x, torch.tensor(0.05, device="cuda")), bits)
        for wrong in (2, 4):
            with pytest.raises(ValueError):
                m(x, torch.full((wrong,), 0.05))
        # a second module, called on a non-default stream: the launch follows torch's current stream
        m2 = copy.deepcopy(m)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            bits2 = m2(x, 0.05)
        side.synchronize()
        assert torch.equal(bits2, bits)
