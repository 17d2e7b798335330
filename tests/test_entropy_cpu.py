"""CPU tests of the bits-estimator oracle against the golden vectors recorded from the reference's
Entropy_factorized_optimized_refactor (tests/golden/make_golden_entropy.py), and of the host-side
module (parameter names/shapes, packed layout, wiring) -- no GPU compute.

The oracle is also pinned against a float64 torch-autograd restatement of the operation (``autograd_bits``), on every
(layers, width) instance, channel count, size and Q form that tests/test_gpu_entropy.py feeds it: the GPU tests take
the oracle as ground truth at shapes the golden vectors do not reach.  ``recipe`` is the shared seeded input generator
of both files."""
import functools
import math

import numpy as np
import pytest
import torch

from util import golden

from oracle import entropy_oracle as EO

CASES = ["scales", "quats", "opacities", "sh0_qvec", "wide", "deep", "narrow"]


def load_case(gd, name):
    n_layers = len(gd[f"{name}.filters"]) + 1
    mats = [gd[f"{name}.mat{i}"] for i in range(n_layers)]
    biases = [gd[f"{name}.bias{i}"] for i in range(n_layers)]
    factors = [gd[f"{name}.factor{i}"] for i in range(n_layers - 1)]
    return mats, biases, factors


BOUND = 1e-6
Q_SCALAR = 0.05


def per_channel_q(C):
    return np.linspace(0.03, 0.12, C).astype(np.float32)  # distinct per channel, around the scalar 0.05


@functools.lru_cache(maxsize=None)
def recipe(n, C, filters, per_channel=False, seed=0):
    """Seeded inputs of the entropy tests (CPU pin of the oracle and GPU parity): the module with its own initialisation
    (init_scale=10) plus 0.3 randn on every tensor (distinct parameter sets, non-zero factors); x uniform in [-2, 2] with
    ~2 % of the elements overwritten by +-uniform(50, 300) (deep tails: likelihood clamped at the bound); v_bits
    uniform(0.5, 1.5) with the sign flipped on 10 % (both branches of the lower-bound gate).  ``x_body`` is x without the
    tails.  Cached: callers must not modify the arrays or the module's parameters."""
    from gscodec_studio_amd.compression_simulation import Entropy_factorized_optimized_refactor as M

    rs = np.random.RandomState(seed)
    state = np.random.get_state()
    np.random.seed(seed + 1)  # the module draws its biases from numpy's global generator
    m = M(channel=C, filters=filters)
    np.random.set_state(state)
    gen = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():
        for p in list(m._matrices) + list(m._bias) + list(m._factor):
            p.add_(0.3 * torch.randn(p.shape, generator=gen))
    x_body = rs.uniform(-2.0, 2.0, (n, C)).astype(np.float32)
    tail = rs.rand(n, C) < 0.02
    tail_val = (rs.uniform(50.0, 300.0, (n, C)) * np.where(rs.rand(n, C) < 0.5, -1.0, 1.0)).astype(np.float32)
    x = np.where(tail, tail_val, x_body)
    v_bits = (rs.uniform(0.5, 1.5, (n, C)) * np.where(rs.rand(n, C) < 0.1, -1.0, 1.0)).astype(np.float32)
    q = per_channel_q(C) if per_channel else np.float32(Q_SCALAR)
    return dict(n=n, C=C, filters=tuple(filters), module=m, x=x, x_body=x_body, v_bits=v_bits, q=q,
                mats=[p.detach().numpy().copy() for p in m._matrices], biases=[p.detach().numpy().copy() for p in m._bias],
                factors=[p.detach().numpy().copy() for p in m._factor])


def bound_masks(lik, bound=BOUND):
    """(clamped, borderline) from the float64 likelihood before the bound: clamped = below the bound, borderline = within a
    relative 1e-3 of it (an fp32 evaluation may decide those either way; entrywise checks leave them out)."""
    return lik < bound, np.abs(lik - bound) <= 1e-3 * bound


class _LowerBoundF64(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x)
        ctx.bound = bound
        return torch.clamp(x, min=bound)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ((x >= ctx.bound) | (g < 0)) * g, None


def autograd_bits(x, q, mats, biases, factors, bound=BOUND):
    """The operation as the header of csrc/entropy.hip states it, in float64 torch, differentiated by autograd (nothing
    shared with the oracle but EO.param_channel).  x [N, C] and the parameter lists are float64 leaf tensors."""
    n, C = x.shape
    n_idx, c_idx = np.meshgrid(np.arange(n), np.arange(C), indexing="ij")
    p = torch.from_numpy(EO.param_channel(n_idx.reshape(-1), c_idx.reshape(-1), n, C))
    half = 0.5 * q.reshape(-1).expand(C)[torch.from_numpy(c_idx.reshape(-1))]

    def f(h):
        h = h[:, None]
        for i in range(len(mats)):
            A = torch.nn.functional.softplus(mats[i])[p]  # softplus (matrix)
            h = torch.einsum("eoi,ei->eo", A, h) + biases[i][p][:, :, 0]  # identity (bias)
            if i < len(factors):
                h = h + torch.tanh(factors[i])[p][:, :, 0] * torch.tanh(h)  # tanh (factor)
        return h[:, 0]

    xe = x.reshape(-1)
    lower, upper = f(xe - half), f(xe + half)
    sign = -torch.sign(lower + upper).detach()
    lik = torch.abs(torch.sigmoid(sign * upper) - torch.sigmoid(sign * lower))
    return (-torch.log2(_LowerBoundF64.apply(lik, bound))).reshape(n, C)


def _pin_oracle(rc):
    """Oracle forward and backward against autograd: 1e-9 of each tensor's largest entry.  Returns the likelihood."""
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    x = t64(rc["x"])
    mats, biases, factors = ([t64(a) for a in rc[k]] for k in ("mats", "biases", "factors"))
    q = torch.tensor(np.asarray(rc["q"], np.float64))
    bits = autograd_bits(x, q, mats, biases, factors)
    (bits * torch.from_numpy(rc["v_bits"].astype(np.float64))).sum().backward()
    gx, gm, gb, gf, obits, lik = EO.factorized_bits_bwd(rc["x"], rc["q"], rc["mats"], rc["biases"], rc["factors"], rc["v_bits"],
                                                        return_fwd=True)
    assert np.array_equal(obits, EO.factorized_bits_fwd(rc["x"], rc["q"], rc["mats"], rc["biases"], rc["factors"]))

    def close(got, want, what):
        want = want.detach().numpy()
        assert got.shape == want.shape, what
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (what, np.abs(got - want).max(), np.abs(want).max())

    close(obits, bits, "bits")
    close(gx, x.grad, "v_x")
    for name, got, want in (("v_mat", gm, mats), ("v_bias", gb, biases), ("v_factor", gf, factors)):
        for i in range(len(want)):
            assert float(want[i].grad.abs().max()) > 0, (name, i)
            close(got[i], want[i].grad, f"{name}{i}")
    return lik


def _assert_shares(lik):
    clamped, borderline = bound_masks(lik)
    assert borderline.mean() <= 1e-3, borderline.mean()
    assert 0.005 <= clamped.mean() <= 0.03, clamped.mean()  # the gate is exercised but does not dominate


@pytest.mark.parametrize("L,W", [(l, w) for l in range(1, 5) for w in range(1, 5)])
def test_oracle_matches_autograd_on_every_instance(L, W):
    _assert_shares(_pin_oracle(recipe(700, 3, (W,) * L)))


@pytest.mark.parametrize("C", [1, 2, 3, 5, 7, 16, 31, 32])
def test_oracle_matches_autograd_on_every_channel_count(C):
    _assert_shares(_pin_oracle(recipe(1000, C, (3, 3))))


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 1000])
def test_oracle_matches_autograd_on_small_and_padded_sizes(n):
    _pin_oracle(recipe(n, 3, (3, 3)))


@pytest.mark.parametrize("C", [3, 5, 7])
def test_oracle_matches_autograd_with_per_channel_q(C):
    rc = recipe(1000, C, (3, 3), per_channel=True)
    assert len(set(rc["q"].tolist())) == C
    _pin_oracle(rc)


def test_recipe_exercises_the_bound_without_sitting_on_it():
    """~2 % tails: most of them clamped, (almost) none within 1e-3 of the bound, and no body element below it."""
    rc = recipe(20_000, 3, (3, 3))
    *_, lik = EO.factorized_bits_bwd(rc["x"], rc["q"], rc["mats"], rc["biases"], rc["factors"], rc["v_bits"], return_fwd=True)
    _assert_shares(lik)
    body = rc["x"] == rc["x_body"]
    assert 0.97 <= body.mean() <= 0.99
    assert lik[body].min() > 10 * BOUND
    blocked = (lik < BOUND) & (rc["v_bits"] < 0)
    assert blocked.sum() >= 10 and ((lik < BOUND) & (rc["v_bits"] > 0)).sum() >= 10  # both branches of the gate


def test_oracle_row_subset_equals_full_run():
    """rows= / n_total= (used by the GPU boundary-row checks) evaluate exactly the selected rows of the full input."""
    rc = recipe(1000, 5, (3, 3), per_channel=True)
    rows = np.array([0, 31, 32, 33, 500, 998, 999])
    args = (rc["q"], rc["mats"], rc["biases"], rc["factors"])
    vb = np.zeros_like(rc["v_bits"])
    vb[rows] = rc["v_bits"][rows]
    full = EO.factorized_bits_bwd(rc["x"], *args, vb, return_fwd=True)
    sub = EO.factorized_bits_bwd(rc["x"][rows], *args, vb[rows], rows=rows, n_total=1000, return_fwd=True)
    assert np.array_equal(full[0][rows], sub[0]) and np.array_equal(full[4][rows], sub[4]) and np.array_equal(full[5][rows], sub[5])
    for i in (1, 2, 3):
        for a, b in zip(full[i], sub[i]):
            assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max()  # same terms in another summation order: the bar of the pin


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_reference(name):
    gd = golden("entropy.npz")
    mats, biases, factors = load_case(gd, name)
    x, q, vb = gd[f"{name}.x"], gd[f"{name}.q"], gd[f"{name}.v_bits"]
    bits = EO.factorized_bits_fwd(x, q, mats, biases, factors)
    ref = gd[f"{name}.bits"]
    # the reference itself is fp32 and loses up to ~3e-3 bits to sigmoid cancellation (measured against float64)
    assert np.all(np.abs(bits - ref) <= 4e-3 + 2e-4 * np.abs(ref))
    gx, gm, gb, gf = EO.factorized_bits_bwd(x, q, mats, biases, factors, vb)
    rx = gd[f"{name}.v_x"]
    assert (np.abs(gx - rx) > 5e-3 * (np.abs(rx) + np.abs(rx).mean())).mean() < 0.01
    for i in range(len(mats)):
        for got, key in ((gm[i], f"v_mat{i}"), (gb[i], f"v_bias{i}")):
            r = gd[f"{name}.{key}"]
            assert np.abs(got - r).max() <= 5e-3 * np.abs(r).max()
    for i in range(len(factors)):
        r = gd[f"{name}.v_factor{i}"]
        assert np.abs(gf[i] - r).max() <= 5e-3 * np.abs(r).max()


def test_oracle_channel_mapping_is_the_reference_quirk():
    """p(n, c) = (32 c + n // chunk) % C: with the straightforward mapping p = c the oracle must NOT match."""
    gd = golden("entropy.npz")
    name = "quats"
    mats, biases, factors = load_case(gd, name)
    x, q = gd[f"{name}.x"], gd[f"{name}.q"]
    N_, C = x.shape
    assert EO.chunk_len(1024) == 33 and EO.chunk_len(1000) == 32 and EO.chunk_len(31) == 1
    n_idx, c_idx = np.meshgrid(np.arange(N_), np.arange(C), indexing="ij")
    p = EO.param_channel(n_idx, c_idx, N_, C)
    assert np.array_equal(p[:, 0], (np.arange(N_) // 33) % 4) and np.array_equal(p[:, 0], p[:, 3])  # C = 4: position only
    # permuting the parameter sets changes the result => the mapping matters and is pinned by the golden bits
    perm = [1, 2, 3, 0]
    bits = EO.factorized_bits_fwd(x, q, [m[perm] for m in mats], [b[perm] for b in biases], [f[perm] for f in factors])
    assert np.abs(bits - gd[f"{name}.bits"]).max() > 0.05


def test_oracle_gradient_matches_finite_differences():
    gd = golden("entropy.npz")
    name = "wide"
    mats, biases, factors = load_case(gd, name)
    x, q = gd[f"{name}.x"].astype(np.float64), gd[f"{name}.q"]
    vb = gd[f"{name}.v_bits"].astype(np.float64)
    gx, gm, gb, gf = EO.factorized_bits_bwd(x, q, mats, biases, factors, vb)
    f = lambda xx, mm: float((EO.factorized_bits_fwd(xx, q, mm, biases, factors) * vb).sum())  # noqa: E731
    eps = 1e-6
    for (n, c) in [(10, 0), (50, 1), (95, 0)]:
        xp, xm = x.copy(), x.copy()
        xp[n, c] += eps
        xm[n, c] -= eps
        fd = (f(xp, mats) - f(xm, mats)) / (2 * eps)
        assert abs(fd - gx[n, c]) <= 1e-4 * (abs(fd) + 1e-3)
    m1 = [m.astype(np.float64).copy() for m in mats]
    for idx in [(0, 1, 0), (1, 0, 1)]:
        mp = [m.copy() for m in m1]
        mm_ = [m.copy() for m in m1]
        mp[1][idx] += eps
        mm_[1][idx] -= eps
        fd = (f(x, mp) - f(x, mm_)) / (2 * eps)
        assert abs(fd - gm[1][idx]) <= 1e-4 * (abs(fd) + 1e-3)


def test_module_matches_reference_parameter_layout():
    from gscodec_studio_amd.compression_simulation import Entropy_factorized_optimized_refactor as M

    m = M(channel=4)  # default filters (3, 3, 3)
    names = [n for n, _ in m.named_parameters()]
    # captured by importing the reference module in the build container (channel=4, default filters): the last layer's
    # tensors are ALSO bound to the attributes matrix / bias / factor (reference entropy_model.py:112-126), so
    # named_parameters() lists them under those names and the state dict carries the three alias keys
    assert names == ["matrix", "bias", "factor", "_matrices.0", "_matrices.1", "_matrices.2", "_bias.0", "_bias.1", "_bias.2",
                     "_factor.0", "_factor.1"]
    assert list(m.state_dict().keys()) == ["matrix", "bias", "factor", "filters_len", "factor_len", "_matrices.0", "_matrices.1",
                                           "_matrices.2", "_matrices.3", "_bias.0", "_bias.1", "_bias.2", "_bias.3", "_factor.0",
                                           "_factor.1", "_factor.2", "likelihood_lower_bound.bound"]
    assert m.matrix is m._matrices[3] and m.bias is m._bias[3] and m.factor is m._factor[2]
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()}, strict=True)
    assert [tuple(p.shape) for p in m._matrices] == [(4, 3, 1), (4, 3, 3), (4, 3, 3), (4, 1, 3)]
    assert [tuple(p.shape) for p in m._bias] == [(4, 3, 1), (4, 3, 1), (4, 3, 1), (4, 1, 1)]
    assert [tuple(p.shape) for p in m._factor] == [(4, 3, 1)] * 3
    scale = 10.0 ** (1.0 / 4)
    assert np.allclose(m._matrices[1].detach().numpy(), np.log(np.expm1(1.0 / scale / 3)))
    assert float(m._factor[0].abs().max()) == 0.0 and float(m._bias[0].abs().max()) <= 0.5
    assert set(m.state_dict().keys()) >= {"filters_len", "factor_len", "likelihood_lower_bound.bound"}
    packed = m.packed_parameters()
    assert packed.shape == (4, 43)
    # layout: layer 0 = [matrix (3) | bias (3) | factor (3)], then 2 x [9 | 3 | 3], last [3 | 1]
    assert torch.equal(packed[:, 0:3], m._matrices[0].reshape(4, 3)) and torch.equal(packed[:, 3:6], m._bias[0].reshape(4, 3))
    assert torch.equal(packed[:, 9:18], m._matrices[1].reshape(4, 9)) and torch.equal(packed[:, 39:42], m._matrices[3].reshape(4, 3))
    packed.sum().backward()
    assert all(p.grad is not None for p in m.parameters())
    with pytest.raises(NotImplementedError):
        M(channel=3, filters=(3, 2))
    with pytest.raises(RuntimeError):
        m(torch.zeros(8, 4), 0.1)  # CPU tensors: no fallback


def test_simulation_wiring_without_compute():
    from gscodec_studio_amd.compression_simulation import CompressionSimulation, STGCompressionSimulation

    steps = {"means": -1, "scales": 10_000, "quats": 10_000, "opacities": -1, "sh0": 20_000, "shN": -1}
    sim = CompressionSimulation(entropy_model_enable=True, entropy_steps=steps, device="cpu")
    assert sim.entropy_model_option == {"means": False, "scales": True, "quats": True, "opacities": False, "sh0": True, "shN": False}
    assert sim.entropy_min_step == 10_000
    assert sim.entropy_models["scales"].filters == (3, 3) and sim.entropy_models["quats"].filters == (3, 3, 3)
    assert sim.entropy_models["opacities"] is None and sim.entropy_model_optimizers["opacities"] is None
    opt = sim.entropy_model_optimizers["sh0"]
    assert isinstance(opt, torch.optim.Adam) and len(opt.param_groups) == 8 and opt.param_groups[0]["lr"] == 1e-4
    with pytest.raises(NotImplementedError):
        CompressionSimulation(entropy_model_enable=True, entropy_model_type="gaussian_model", entropy_steps=steps)
    stg_steps = {"means": -1, "scales": 5, "quats": 5, "opacities": -1, "colors": 5, "features_dir": 5, "features_time": 5}
    stg = STGCompressionSimulation("round", entropy_model_enable=True, entropy_steps=stg_steps, device="cpu")
    assert stg.entropy_models["scales"].filters == (3, 3, 3) and stg.entropy_models["colors"].filters == (3, 3)
