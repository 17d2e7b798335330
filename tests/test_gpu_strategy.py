"""gscodec_studio_amd.strategy on the GPU: the three kernels (gs_densify_stats, gs_inject_noise, gs_relocation) against float64
restatements written here and against tests/golden/strategy.npz (the reference's own strategy code run on the CPU), the
set-changing operations with torch.optim.Adam and optimizers.Adam, and short training loops in which every branch of both
strategies fires."""
import copy
import math

import numpy as np
import pytest
import torch

from util import garden, golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KEYS = ("means", "scales", "quats", "opacities", "sh0")
LRS = {"means": 1.6e-4, "quats": 1e-3, "scales": 5e-3, "opacities": 5e-2, "sh0": 2.5e-3, "shN": 2.5e-3 / 20}


def T(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dtype is None else t.to(dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# gs_densify_stats
# ------------------------------------------------------------------------------------------------------------------------------
def _stats_f64(state, grad, radii, width, height):
    """One step of the running statistics in float64: grad [C, N, 2], radii [C, N] (numpy); state = (grad2d, count, radii)."""
    C = grad.shape[0]
    vis = radii > 0
    g = grad.astype(np.float64) * np.array([width / 2.0 * C, height / 2.0 * C])
    norm = np.sqrt((g * g).sum(-1))
    grad2d = state[0] + np.where(vis, norm, 0.0).sum(0)
    count = state[1] + vis.sum(0)
    rad = np.maximum(state[2], (radii.astype(np.float32) / np.float32(max(width, height))).max(0))  # (float32 division: exact compare)
    return grad2d, count, rad


def _info(grad, radii, packed, width, height, attr="grad"):
    """A rasterization() meta as the strategy reads it, from dense numpy arrays; the gradient sits in .grad or .absgrad."""
    C = grad.shape[0]
    if packed:
        cam, gid = np.nonzero(radii > 0)
        g, info = T(grad[cam, gid]), {"radii": T(radii[cam, gid]), "gaussian_ids": T(gid.astype(np.int64))}
    else:
        g, info = T(grad), {"radii": T(radii), "gaussian_ids": None}
    means2d = torch.zeros_like(g, requires_grad=True)
    setattr(means2d, attr, g)
    info.update({"means2d": means2d, "width": width, "height": height, "n_cameras": C})
    return info


@pytest.mark.parametrize("with_radii", [True, False])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_densify_stats_against_fixture_and_float64(C, packed, with_radii):
    from gscodec_studio_amd.strategy import DefaultStrategy

    fx = golden("strategy.npz")
    W, H = int(fx["width"]), int(fx["height"])
    N = fx["means"].shape[0]
    assert N % 2 == 1
    params = {"means": torch.nn.Parameter(T(fx["means"]))}
    rtol = 1e-5 if packed else 1e-6  # (the packed form sums with float atomics, in any order)
    strategy = DefaultStrategy(refine_scale2d_stop_iter=1000 if with_radii else 0)
    runs = []
    for run in range(2):
        state = strategy.initialize_state()
        assert ("radii" in state) == with_radii
        f64 = (np.zeros(N), np.zeros(N), np.zeros(N, np.float32))
        for i in range(2):  # two consecutive steps accumulate
            grad, radii = fx[f"c{C}_grad{i}"], fx[f"c{C}_radii{i}"]
            assert (radii.max(0) == 0).any() and (radii > 0).any()  # some gaussians invisible in every camera
            strategy._update_state(params, state, _info(grad, radii, packed, W, H), packed=packed)
            f64 = _stats_f64(f64, grad, radii, W, H)
            got = {k: v.cpu().numpy() for k, v in state.items() if torch.is_tensor(v)}
            assert np.array_equal(got["count"], fx[f"c{C}_count{i}"]) and np.array_equal(got["count"], f64[1])
            want32 = f64[0].astype(np.float32)
            seen = want32 != 0
            err = np.abs(got["grad2d"].astype(np.float64) - want32)[seen] / np.abs(want32.astype(np.float64))[seen]
            err_fx = np.abs(got["grad2d"].astype(np.float64) - fx[f"c{C}_grad2d{i}"])[seen] / np.abs(want32.astype(np.float64))[seen]
            print(f"\n[densify_stats C={C} packed={packed} step {i}] grad2d max rel err vs float64 {err.max():.2e}, "
                  f"vs the reference's float32 {err_fx.max():.2e}")
            np.testing.assert_allclose(got["grad2d"], want32, rtol=rtol, atol=0)
            np.testing.assert_allclose(got["grad2d"], fx[f"c{C}_grad2d{i}"], rtol=rtol, atol=0)
            assert np.array_equal(got["grad2d"] == 0, f64[1] == 0)
            if with_radii:  # C = 1: the reference's own result; C = 3: the scatter-max
                assert np.array_equal(got["radii"], fx[f"c{C}_radii_state{i}"]) and np.array_equal(got["radii"], f64[2])
        runs.append(got)
    if not packed:  # no atomics: bit-identical from run to run
        for k in runs[0]:
            assert np.array_equal(runs[0][k].view(np.int32), runs[1][k].view(np.int32)), k


def test_densify_stats_reads_strided_gradient_rows_and_absgrad():
    """The compositing backward hands out its gradients as column views of 16-float rows: they are read in place."""
    from gscodec_studio_amd.strategy import DefaultStrategy, ops

    fx = golden("strategy.npz")
    W, H, N = int(fx["width"]), int(fx["height"]), fx["means"].shape[0]
    grad, radii = fx["c3_grad0"], fx["c3_radii0"]
    rows = torch.full((3, N, 16), float("nan"), device=DEV)
    rows[..., 10:12] = T(grad)
    view = rows[..., 10:12]
    src, stride = ops._grad_rows(view)
    assert stride == 16 and src.data_ptr() == view.data_ptr()
    assert ops._grad_rows(T(grad))[1] == 2 and ops._grad_rows(T(grad)[:, :, [1, 0]].transpose(0, 1))[1] == 2
    params = {"means": torch.nn.Parameter(T(fx["means"]))}
    out = []
    for g in (view, T(grad)):
        strategy = DefaultStrategy(absgrad=True, refine_scale2d_stop_iter=10)
        state = strategy.initialize_state()
        info = _info(grad, radii, False, W, H, attr="absgrad")
        info["means2d"].absgrad = g
        strategy._update_state(params, state, info)
        out.append(state)
    for k in ("grad2d", "count", "radii"):
        assert torch.equal(out[0][k], out[1][k]), k
    assert np.array_equal(out[0]["count"].cpu().numpy(), fx["c3_count0"])
    # odd element offset: the scalar-load path gives the same bits
    shifted = torch.zeros(3 * N * 2 + 1, device=DEV)
    shifted[1:] = T(grad).reshape(-1)
    g2 = shifted[1:].view(3, N, 2)
    assert g2.data_ptr() % 8 == 4
    state = {k: torch.zeros(N, device=DEV) for k in ("grad2d", "count", "radii")}
    ops.densify_stats(g2, T(radii), None, W, H, 3, state["grad2d"], state["count"], state["radii"])
    for k in ("grad2d", "count", "radii"):
        assert torch.equal(state[k], out[0][k]), k


def _garden_params(n, seed=0):
    fx = garden(n)
    rs = np.random.RandomState(seed)
    sh = np.zeros((n, 16, 3), np.float32)
    sh[:, 0] = (fx["rgb"] - 0.5) / 0.2820947917738781
    sh[:, 1:] = rs.randn(n, 15, 3).astype(np.float32) * 0.05
    f = lambda a: T(np.asarray(a, np.float32))  # noqa: E731
    params = {"means": f(fx["means"]), "quats": f(fx["quats"]), "scales": f(np.log(fx["scales"] * 4 + 1e-4)),
              "opacities": f(rs.uniform(-2, 3, n)), "sh0": f(sh[:, :1]), "shN": f(sh[:, 1:])}
    cams = {"viewmats": f(fx["viewmats"][:1]), "Ks": f(fx["Ks"][:1]), "W": fx["width"], "H": fx["height"]}
    return params, cams


def _render(ps, cams, **kw):
    from gscodec_studio_amd import rasterization

    kw.setdefault("packed", False)
    return rasterization(ps["means"], ps["quats"], torch.exp(ps["scales"]), torch.sigmoid(ps["opacities"]),
                         torch.cat([ps["sh0"], ps["shN"]], 1), cams["viewmats"], cams["Ks"], cams["W"], cams["H"], sh_degree=3, **kw)


@pytest.mark.parametrize("absgrad", [True, False])
def test_step_post_backward_does_not_synchronise(absgrad):
    from gscodec_studio_amd.strategy import DefaultStrategy

    init, cams = _garden_params(3001)
    ps = {k: torch.nn.Parameter(v) for k, v in init.items()}
    strategy = DefaultStrategy(absgrad=absgrad, refine_scale2d_stop_iter=1000)

    def one_step(state, checked):
        colors, _, info = _render(ps, cams, absgrad=True)
        strategy.step_pre_backward(ps, {}, state, 7, info)
        colors.square().mean().backward()
        if checked:
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
        try:
            strategy.step_post_backward(ps, {}, state, 7, info)  # step 7: no refinement, no reset
        finally:
            torch.cuda.set_sync_debug_mode(0)
        return info

    one_step(strategy.initialize_state(), False)  # first call outside the checked window
    state = strategy.initialize_state()
    info = one_step(state, True)
    torch.cuda.synchronize()
    g = info["means2d"].absgrad if absgrad else info["means2d"].grad
    assert g.shape == (1, 3001, 2)
    radii = info["radii"].cpu().numpy()
    assert (radii > 0).sum() > 100 and (radii == 0).any()
    want = _stats_f64((np.zeros(3001), np.zeros(3001), np.zeros(3001, np.float32)), g.cpu().numpy(), radii, cams["W"], cams["H"])
    assert np.array_equal(state["count"].cpu().numpy(), want[1])
    np.testing.assert_allclose(state["grad2d"].cpu().numpy(), want[0].astype(np.float32), rtol=1e-6, atol=0)
    assert np.array_equal(state["radii"].cpu().numpy(), want[2])
    assert float(state["grad2d"].sum()) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# gs_relocation
# ------------------------------------------------------------------------------------------------------------------------------
def _relocation_f64(o, s, n, binoms):
    """The formula in float64 from the float32 inputs: o [N], s [N, 3], n [N] (clamped), binoms [n_max, n_max] float32 (numpy)."""
    o, s, B = o.astype(np.float64), s.astype(np.float64), binoms.astype(np.float64)
    x = 1.0 - np.power(1.0 - o, 1.0 / n)
    denom = np.zeros_like(o)
    for i in range(1, int(n.max()) + 1):
        on = n >= i
        for k in range(i):
            denom += np.where(on, B[i - 1, k] * ((-1.0) ** k / math.sqrt(k + 1.0)) * x ** (k + 1), 0.0)
    return x, s * (o / denom)[:, None]


def _relocation_f32_reference(o, s, n, binoms):
    """The reference kernel's loops (csrc/compute_relocation.cu:20-37) restated in float32 torch operations, same summation order."""
    f = torch.float32
    x = 1.0 - torch.pow(1.0 - o, (1.0 / n.to(f)))
    denom = torch.zeros_like(o)
    for i in range(1, int(n.max()) + 1):
        on = n >= i
        for k in range(i):
            term = (torch.tensor((-1.0) ** k, dtype=f) / torch.sqrt(torch.tensor(float(k + 1), dtype=f))).to(o.device) * torch.pow(x, k + 1)
            denom = torch.where(on, denom + binoms[i - 1, k] * term, denom)
    return x, (o / denom)[:, None] * s


def test_compute_relocation_accuracy():
    """Per ratio n, the kernel's largest relative error against float64 is at most max(1e-5, 2 x that of the float32 restatement
    of the reference kernel): a factor 2 for a different summation order and pow, where a wrong formula is off by orders of
    magnitude.  (The float32 loop is off by 3e-6 at n = 1 rising to some 1e-4 at n = 51; both tables are printed.)"""
    from gscodec_studio_amd._c_adapter import _C
    from gscodec_studio_amd.relocation import compute_relocation
    from gscodec_studio_amd.strategy import MCMCStrategy

    per, n_max = 64, 51
    rs = np.random.RandomState(5)
    ratios_np = np.concatenate([np.repeat(np.arange(1, n_max + 1), per), rs.randint(52, 200, 63), np.zeros(4, np.int64)])
    rs.shuffle(ratios_np)
    N = ratios_np.size
    assert N % 2 == 1
    o_np = rs.uniform(0.005, 0.99, N).astype(np.float32)
    s_np = np.exp(rs.uniform(np.log(1e-3), np.log(1.0), (N, 3))).astype(np.float32)
    binoms = MCMCStrategy().initialize_state()["binoms"].to(DEV)
    o, s, ratios = T(o_np), T(s_np), T(ratios_np)
    new_o, new_s = compute_relocation(o, s, ratios, binoms)
    assert int(ratios.min()) == 1 and int(ratios.max()) == n_max  # clamped in place, as the reference does
    n_np = np.clip(ratios_np, 1, n_max)
    assert np.array_equal(ratios.cpu().numpy(), n_np)
    assert new_o.shape == (N,) and new_s.shape == (N, 3) and new_o.dtype == new_s.dtype == torch.float32
    c_o, c_s = _C.compute_relocation(o, s, ratios.int(), binoms, n_max)
    assert torch.equal(c_o, new_o) and torch.equal(c_s, new_s)

    want_o, want_s = _relocation_f64(o_np, s_np, n_np, binoms.cpu().numpy())
    ref_o, ref_s = _relocation_f32_reference(o, s, T(n_np), binoms)

    def rel(got_o, got_s):
        e_o = np.abs(got_o.cpu().numpy().astype(np.float64) - want_o) / np.abs(want_o)
        e_s = (np.abs(got_s.cpu().numpy().astype(np.float64) - want_s) / np.abs(want_s)).max(-1)
        return np.maximum(e_o, e_s)

    e_kernel, e_ref = rel(new_o, new_s), rel(ref_o, ref_s)
    print("\n[compute_relocation] largest relative error against float64, per ratio n:  n  kernel  float32-restatement")
    bad = []
    for n in range(1, n_max + 1):
        sel = n_np == n
        k, r = e_kernel[sel].max(), e_ref[sel].max()
        print(f"  {n:3d}  {k:.2e}  {r:.2e}")
        if not k <= max(1e-5, 2 * r):
            bad.append((n, k, r))
    assert not bad, bad
    assert np.isfinite(new_s.cpu().numpy()).all()


def test_compute_relocation_empty():
    from gscodec_studio_amd.relocation import compute_relocation
    from gscodec_studio_amd.strategy import MCMCStrategy

    binoms = MCMCStrategy().initialize_state()["binoms"].to(DEV)
    new_o, new_s = compute_relocation(torch.empty(0, device=DEV), torch.empty((0, 3), device=DEV),
                                      torch.empty(0, dtype=torch.int64, device=DEV), binoms)
    assert new_o.shape == (0,) and new_s.shape == (0, 3) and new_o.is_cuda and new_s.is_cuda


# ------------------------------------------------------------------------------------------------------------------------------
# gs_inject_noise
# ------------------------------------------------------------------------------------------------------------------------------
def _rotmats_f64(quats):
    q = quats.double()
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)


@pytest.mark.parametrize("column_opacities", [False, True])
def test_inject_noise_to_position(column_opacities):
    from gscodec_studio_amd.strategy import ops

    N, seed, scaler = 10_001, 123, 1.6e-4 * 5e5
    g = torch.Generator(device=DEV).manual_seed(1)
    logits = torch.linspace(-12, 12, N, device=DEV)[torch.randperm(N, device=DEV, generator=g)]  # both sides of 1 - o = 0.995
    ps = {"means": torch.randn(N, 3, device=DEV, generator=g),
          "quats": torch.randn(N, 4, device=DEV, generator=g) * (0.2 + 3 * torch.rand(N, 1, device=DEV, generator=g)),  # unnormalised
          "scales": torch.log(0.002 + 0.3 * torch.rand(N, 3, device=DEV, generator=g)),
          "opacities": logits[:, None] if column_opacities else logits,
          "sh0": torch.rand(N, 1, 3, device=DEV, generator=g)}
    ps = {k: torch.nn.Parameter(v.contiguous()) for k, v in ps.items()}
    before = {k: v.detach().clone() for k, v in ps.items()}
    torch.manual_seed(seed)
    ops.inject_noise_to_position(ps, {}, {}, scaler)
    torch.manual_seed(seed)
    noise = torch.randn_like(before["means"])  # the one draw of the call, replayed

    o = torch.sigmoid(before["opacities"].double().flatten())
    gate = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - o) - 0.995)))
    R = _rotmats_f64(before["quats"])
    S2 = torch.exp(before["scales"].double()) ** 2
    covars = torch.einsum("nij,nj,nkj->nik", R, S2, R)
    want = torch.einsum("nij,nj->ni", covars, noise.double() * gate[:, None] * scaler)
    got = ps["means"].detach().double() - before["means"].double()
    rel = float((got - want).norm() / want.norm())
    print(f"\n[inject_noise column={column_opacities}] relL2 {rel:.2e}, largest change {float(want.abs().max()):.3e}, "
          f"{int((gate > 0.31).sum())} of {N} gaussians past the gate's midpoint")
    # the gate rises from 0 to g(1) = 0.62 around 1 - o = 0.995: all three regimes are present
    assert (gate > 0.6).any() and (gate < 1e-6).any() and ((gate > 0.1) & (gate < 0.5)).any()
    assert rel <= 1e-4
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4 * float(want.abs().max()))
    for k in ("quats", "scales", "opacities", "sh0"):
        assert torch.equal(ps[k].detach(), before[k]), k
    assert ps["opacities"].shape == before["opacities"].shape


# ------------------------------------------------------------------------------------------------------------------------------
# the set-changing operations
# ------------------------------------------------------------------------------------------------------------------------------
def _adam_classes():
    from gscodec_studio_amd.optimizers import Adam

    return {"torch": torch.optim.Adam, "hip": Adam}


def _fixture_trainer(fx, opt_name, prefix=""):
    cls = _adam_classes()[opt_name]
    params = {k: torch.nn.Parameter(T(fx[f"{prefix}{k}"])) for k in KEYS}
    opts = {}
    for k in KEYS:
        opts[k] = cls([{"params": [params[k]], "lr": LRS[k], "name": k}], eps=1e-15)
        opts[k].state[params[k]] = {"step": torch.tensor(7.0), "exp_avg": T(fx[f"{prefix}{k}_exp_avg"]),
                                    "exp_avg_sq": T(fx[f"{prefix}{k}_exp_avg_sq"])}
    return params, opts


def _check_against(fx, tag, params, opts, state, keys=KEYS, state_tag=None):
    for k in keys:
        p = params[k]
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_contiguous()
        assert opts[k].param_groups[0]["params"] == [p] and len(opts[k].state) == 1
        st = opts[k].state[p]
        assert float(st["step"]) == 7.0 and st["step"].device.type == "cpu"
        for got, name in ((p.detach(), f"{tag}_{k}"), (st["exp_avg"], f"{tag}_{k}_exp_avg"), (st["exp_avg_sq"], f"{tag}_{k}_exp_avg_sq")):
            assert np.array_equal(got.cpu().numpy(), fx[name]), name
    for k in ("grad2d", "count", "radii"):
        assert np.array_equal(state[k].cpu().numpy(), fx[f"{state_tag or tag}_state_{k}"]), k
    assert state["scene_scale"] == 1.0


def _step_and_compare(params, opts):
    """One step_all on the replaced parameters against torch.optim.Adam on a cloned copy (tolerances of test_gpu_optimizers.py)."""
    from gscodec_studio_amd.optimizers import step_all

    g = torch.Generator(device=DEV).manual_seed(11)
    twins, twin_opts = {}, {}
    for k, p in params.items():
        p.grad = torch.randn(p.shape, device=DEV, generator=g) * 0.1
        twins[k] = torch.nn.Parameter(p.detach().clone())
        twins[k].grad = p.grad.clone()
        twin_opts[k] = torch.optim.Adam([{"params": [twins[k]], "lr": LRS[k], "name": k}], eps=1e-15)
        twin_opts[k].state[twins[k]] = {n: v.clone() for n, v in opts[k].state[p].items()}
    before = {k: float(opts[k].state[p]["step"]) for k, p in params.items()}
    step_all(opts)
    for k in params:
        twin_opts[k].step()
        so, sr = opts[k].state[params[k]], twin_opts[k].state[twins[k]]
        assert float(so["step"]) == float(sr["step"]) == before[k] + 1.0
        torch.testing.assert_close(params[k].detach(), twins[k].detach(), rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(so["exp_avg"], sr["exp_avg"], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(so["exp_avg_sq"], sr["exp_avg_sq"], rtol=1e-6, atol=1e-9)
        assert params[k].grad is None


@pytest.mark.parametrize("opt_name", ["torch", "hip"])
def test_duplicate_remove_reset_opa_against_fixture(opt_name):
    from gscodec_studio_amd.strategy import ops

    fx = golden("strategy.npz")
    params, opts = _fixture_trainer(fx, opt_name)
    state = {"grad2d": T(fx["c1_grad2d1"]), "count": T(fx["c1_count1"]), "radii": T(fx["c1_radii_state1"]), "scene_scale": 1.0}
    ops.duplicate(params, opts, state, T(fx["is_dupli"]))
    _check_against(fx, "dup", params, opts, state)
    ops.remove(params, opts, state, T(fx["remove_mask"]))
    _check_against(fx, "rem", params, opts, state)
    ops.reset_opa(params, opts, state, float(fx["reset_value"]))
    _check_against(fx, "rst", params, opts, state, keys=("opacities",), state_tag="rem")
    _check_against(fx, "rem", params, opts, state, keys=tuple(k for k in KEYS if k != "opacities"))
    assert (fx["rst_opacities_exp_avg"] == 0).all() and (fx["rst_opacities"] < fx["rem_opacities"]).any()
    _step_and_compare(params, opts)


def test_grow_and_prune_masks_against_fixture(monkeypatch):
    from gscodec_studio_amd.strategy import DefaultStrategy
    from gscodec_studio_amd.strategy import default as default_mod

    fx = golden("strategy.npz")
    N = fx["means"].shape[0]
    params, opts = _fixture_trainer(fx, "hip")
    state = {"grad2d": T(fx["c1_grad2d1"]), "count": T(fx["c1_count1"]), "radii": T(fx["c1_radii_state1"]), "scene_scale": 1.0}
    seen = {}
    monkeypatch.setattr(default_mod, "duplicate", lambda **k: seen.__setitem__("is_dupli", k["mask"].cpu().numpy()))
    monkeypatch.setattr(default_mod, "split", lambda **k: seen.__setitem__("is_split", k["mask"].cpu().numpy()))
    monkeypatch.setattr(default_mod, "remove", lambda **k: seen.__setitem__("is_prune", k["mask"].cpu().numpy()))
    strategy = DefaultStrategy(refine_scale2d_stop_iter=1000, reset_every=500)
    step = int(fx["mask_step"])
    n_dupli, n_split = strategy._grow_gs(params, opts, state, step)
    n_prune = strategy._prune_gs(params, opts, state, step)
    assert (n_dupli, n_split, n_prune) == (int(fx["is_dupli"].sum()), int(fx["is_split"].sum()), int(fx["is_prune"].sum()))
    assert np.array_equal(seen["is_dupli"], fx["is_dupli"]) and np.array_equal(seen["is_prune"], fx["is_prune"])
    assert np.array_equal(seen["is_split"][:N], fx["is_split"]) and not seen["is_split"][N:].any() and len(seen["is_split"]) == N + n_dupli


def _random_trainer(n, opt_name, seed, column_opacities=False, dead_frac=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    opac = torch.rand(n, device=DEV, generator=g) * 6 - 3
    if dead_frac:
        opac[torch.rand(n, device=DEV, generator=g) < dead_frac] = -8.0
    vals = {"means": torch.randn(n, 3, device=DEV, generator=g), "scales": torch.log(0.01 + 0.2 * torch.rand(n, 3, device=DEV, generator=g)),
            "quats": torch.randn(n, 4, device=DEV, generator=g), "opacities": opac[:, None] if column_opacities else opac,
            "sh0": torch.rand(n, 1, 3, device=DEV, generator=g)}
    params = {k: torch.nn.Parameter(v.contiguous()) for k, v in vals.items()}
    cls = _adam_classes()[opt_name]
    opts = {}
    for k, p in params.items():
        opts[k] = cls([{"params": [p], "lr": LRS[k], "name": k}], eps=1e-15)
        opts[k].state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.randn(p.shape, device=DEV, generator=g),
                            "exp_avg_sq": torch.rand(p.shape, device=DEV, generator=g)}
    return params, opts


def _snapshot(params, opts):
    return ({k: p.detach().clone() for k, p in params.items()},
            {k: {n: v.clone() for n, v in opts[k].state[params[k]].items()} for k in params})


# rtol 1e-5 for the computed tensors, plus an absolute floor of 1e-6: they are float32 sums and differences of O(1) numbers (mean +
# offset, logit of an opacity near 0.5), each rounded to 6e-8 absolute, so a result that cancels towards 0 has no relative accuracy
COMPUTED = dict(rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("revised_opacity", [False, True])
@pytest.mark.parametrize("opt_name", ["torch", "hip"])
def test_split_replays_its_draw(opt_name, revised_opacity):
    from gscodec_studio_amd.strategy import ops

    n, seed = 1001, 77
    params, opts = _random_trainer(n, opt_name, 3)
    p0, s0 = _snapshot(params, opts)
    mask = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)) < 0.3
    state = {"grad2d": torch.rand(n, device=DEV), "count": torch.ones(n, device=DEV), "scene_scale": 1.0}
    st0 = {k: v.clone() for k, v in state.items() if torch.is_tensor(v)}
    torch.manual_seed(seed)
    ops.split(params, opts, state, mask, revised_opacity=revised_opacity)
    sel, rest = torch.where(mask)[0], torch.where(~mask)[0]
    m = len(sel)
    torch.manual_seed(seed)
    z = torch.randn(2, m, 3, device=DEV).double()
    R, s = _rotmats_f64(p0["quats"][sel]), torch.exp(p0["scales"][sel].double())
    want_means = (p0["means"][sel].double()[None] + torch.einsum("nij,nj,bnj->bni", R, s, z)).reshape(-1, 3)
    for k, p in params.items():
        assert len(p) == n + m and p.requires_grad and opts[k].param_groups[0]["params"] == [p]
        assert torch.equal(p[: n - m].detach(), p0[k][rest]), k
        st = opts[k].state[p]
        assert float(st["step"]) == 3.0
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[name][: n - m], s0[k][name][rest]) and not st[name][n - m:].any(), (k, name)
    new = {k: p.detach()[n - m:] for k, p in params.items()}
    torch.testing.assert_close(new["means"].double(), want_means, **COMPUTED)
    torch.testing.assert_close(new["scales"].double(), torch.log(s / 1.6).repeat(2, 1), **COMPUTED)
    if revised_opacity:
        o = torch.sigmoid(p0["opacities"][sel].double())
        torch.testing.assert_close(new["opacities"].double(), torch.logit(1.0 - torch.sqrt(1.0 - o)).repeat(2), **COMPUTED)
    else:
        assert torch.equal(new["opacities"], p0["opacities"][sel].repeat(2))
    for k in ("quats", "sh0"):
        assert torch.equal(new[k], p0[k][sel].repeat([2] + [1] * (p0[k].dim() - 1))), k
    for k, v in st0.items():
        assert torch.equal(state[k], torch.cat([v[rest], v[sel].repeat(2)])), k
    _step_and_compare(params, opts)


def _expected_relocation(p0, sampled, binoms, min_opacity):
    o = torch.sigmoid(p0["opacities"]).flatten()[sampled]
    s = torch.exp(p0["scales"])[sampled]
    ratios = np.clip(torch.bincount(sampled)[sampled].cpu().numpy() + 1, 1, 51)
    x, ns = _relocation_f64(o.cpu().numpy(), s.cpu().numpy(), ratios, binoms.cpu().numpy())
    x = np.clip(x, min_opacity, 1.0 - float(torch.finfo(torch.float32).eps))
    return T(np.log(x / (1.0 - x))), T(np.log(ns))


@pytest.mark.parametrize("column_opacities", [False, True])
@pytest.mark.parametrize("opt_name", ["torch", "hip"])
def test_relocate_replays_its_draw(opt_name, column_opacities):
    from gscodec_studio_amd.strategy import MCMCStrategy, ops

    n, seed = 2001, 31
    params, opts = _random_trainer(n, opt_name, 5, column_opacities=column_opacities, dead_frac=0.2)
    p0, s0 = _snapshot(params, opts)
    binoms = MCMCStrategy().initialize_state()["binoms"].to(DEV)
    mask = torch.sigmoid(p0["opacities"].flatten()) <= 0.005
    dead, alive = mask.nonzero(as_tuple=True)[0], (~mask).nonzero(as_tuple=True)[0]
    assert 100 < len(dead) < n // 2
    extra = {"per_gaussian": torch.ones(n, device=DEV)}
    torch.manual_seed(seed)
    ops.relocate(params, opts, extra, mask, binoms, min_opacity=0.005)
    torch.manual_seed(seed)
    sampled = alive[torch.multinomial(torch.sigmoid(p0["opacities"])[alive].flatten(), len(dead), replacement=True)]
    want_opac, want_scales = _expected_relocation(p0, sampled, binoms, 0.005)
    touched = torch.zeros(n, dtype=torch.bool, device=DEV)
    touched[sampled] = True
    touched[dead] = True
    assert len(torch.unique(sampled)) < len(sampled)  # some gaussians were drawn more than once
    for k, p in params.items():
        assert p.shape == p0[k].shape and p.requires_grad and opts[k].param_groups[0]["params"] == [p]
        assert torch.equal(p.detach()[~touched], p0[k][~touched]), k
        assert torch.equal(p.detach()[dead], p.detach()[sampled]), k  # the dead rows are copies of their sources
        if k not in ("opacities", "scales"):
            assert torch.equal(p.detach()[sampled], p0[k][sampled]), k
        st = opts[k].state[p]
        assert float(st["step"]) == 3.0
        untouched = torch.ones(n, dtype=torch.bool, device=DEV)
        untouched[sampled] = False
        for name in ("exp_avg", "exp_avg_sq"):
            assert not st[name][sampled].any() and torch.equal(st[name][untouched], s0[k][name][untouched]), (k, name)
    torch.testing.assert_close(params["opacities"].detach().flatten()[sampled].double(), want_opac, **COMPUTED)
    torch.testing.assert_close(params["scales"].detach()[sampled].double(), want_scales, **COMPUTED)
    assert not extra["per_gaussian"][sampled].any() and bool(extra["per_gaussian"][untouched].all())
    assert float(torch.sigmoid(params["opacities"].detach()).min()) >= 0.005 * (1 - 1e-5)
    _step_and_compare(params, opts)


@pytest.mark.parametrize("opt_name", ["torch", "hip"])
def test_sample_add_replays_its_draw(opt_name):
    from gscodec_studio_amd.strategy import MCMCStrategy, ops

    n, n_new, seed = 1501, 300, 13
    params, opts = _random_trainer(n, opt_name, 6)
    p0, s0 = _snapshot(params, opts)
    binoms = MCMCStrategy().initialize_state()["binoms"].to(DEV)
    extra = {"per_gaussian": torch.ones(n, device=DEV)}
    torch.manual_seed(seed)
    ops.sample_add(params, opts, extra, n_new, binoms, min_opacity=0.005)
    torch.manual_seed(seed)
    sampled = torch.multinomial(torch.sigmoid(p0["opacities"]).flatten(), n_new, replacement=True)
    want_opac, want_scales = _expected_relocation(p0, sampled, binoms, 0.005)
    untouched = torch.ones(n, dtype=torch.bool, device=DEV)
    untouched[sampled] = False
    for k, p in params.items():
        assert len(p) == n + n_new and p.requires_grad and opts[k].param_groups[0]["params"] == [p]
        assert torch.equal(p.detach()[:n][untouched], p0[k][untouched]), k
        assert torch.equal(p.detach()[n:], p.detach()[sampled]), k  # the new rows are copies of their (updated) sources
        if k not in ("opacities", "scales"):
            assert torch.equal(p.detach()[:n], p0[k]), k
        st = opts[k].state[p]
        assert float(st["step"]) == 3.0
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[name][:n], s0[k][name]) and not st[name][n:].any(), (k, name)
    torch.testing.assert_close(params["opacities"].detach()[sampled].double(), want_opac, **COMPUTED)
    torch.testing.assert_close(params["scales"].detach()[sampled].double(), want_scales, **COMPUTED)
    assert extra["per_gaussian"].shape == (n + n_new,) and bool(extra["per_gaussian"][:n].all()) and not extra["per_gaussian"][n:].any()
    _step_and_compare(params, opts)


def test_decoder_and_frozen_parameters():
    """Names containing "decoder" are left alone; a parameter without an optimizer is carried along if it is frozen, refused if
    it is trainable."""
    from gscodec_studio_amd.strategy import ops

    n = 101
    params, opts = _random_trainer(n, "hip", 8)
    params["mlp_decoder_weight"] = torch.nn.Parameter(torch.randn(7, 5, device=DEV))
    params["features"] = torch.nn.Parameter(torch.randn(n, 2, device=DEV), requires_grad=False)
    decoder = params["mlp_decoder_weight"]
    mask = torch.arange(n, device=DEV) % 3 == 0
    ops.duplicate(params, opts, {}, mask)
    assert params["mlp_decoder_weight"] is decoder
    assert len(params["features"]) == n + int(mask.sum()) and not params["features"].requires_grad
    params["features"] = torch.nn.Parameter(params["features"].detach())  # now trainable, still without optimizer
    with pytest.raises(AssertionError, match="Optimizer for features is not found"):
        ops.remove(params, opts, {}, torch.zeros(len(params["means"]), dtype=torch.bool, device=DEV))


# ------------------------------------------------------------------------------------------------------------------------------
# training loops in which every branch fires
# ------------------------------------------------------------------------------------------------------------------------------
def _loop_scene(n):
    """(initial parameters, cameras, target image): the garden splats start translucent and grey and are trained towards
    their own render."""
    init, cams = _garden_params(n)
    with torch.no_grad():
        pixels = _render(init, cams)[0].clamp(0, 1)
    start = {k: v.clone() for k, v in init.items()}
    start["sh0"] = torch.zeros_like(init["sh0"])
    start["shN"] = torch.zeros_like(init["shN"])
    start["opacities"] = torch.full_like(init["opacities"], -1.0)
    return start, cams, pixels


def _trainer_of(start):
    from gscodec_studio_amd.optimizers import Adam

    params = {k: torch.nn.Parameter(v.clone()) for k, v in start.items()}
    opts = {k: Adam([{"params": [p], "lr": LRS[k], "name": k}], eps=1e-15) for k, p in params.items()}
    return params, opts


def _check_lengths(params, opts, state):
    n = len(params["means"])
    for k, p in params.items():
        assert len(p) == n and p.is_contiguous() and torch.isfinite(p).all(), k
        assert opts[k].param_groups[0]["params"] == [p] and len(opts[k].state) <= 1
        for name, v in opts[k].state.get(p, {}).items():
            if name != "step":
                assert v.shape == p.shape and torch.isfinite(v).all(), (k, name)
    for k, v in state.items():
        if torch.is_tensor(v) and k != "binoms":
            assert v.shape == (n,) and torch.isfinite(v).all(), k
    return n


def _counting(monkeypatch, module, names):
    calls = {name: 0 for name in names}
    for name in names:
        real = getattr(module, name)

        def wrapper(*a, _real=real, _name=name, **k):
            calls[_name] += 1
            return _real(*a, **k)

        monkeypatch.setattr(module, name, wrapper)
    return calls


def test_default_strategy_training_loop(monkeypatch):
    from gscodec_studio_amd.losses import photometric_loss
    from gscodec_studio_amd.optimizers import step_all
    from gscodec_studio_amd.strategy import DefaultStrategy
    from gscodec_studio_amd.strategy import default as default_mod

    n0, steps = 2000, 300
    start, cams, pixels = _loop_scene(n0)
    size = torch.exp(start["scales"]).max(-1).values
    # every visible gaussian grows (grow_grad2d tiny): the smaller half is duplicated, the larger half split; after the first
    # reset the largest are pruned
    strategy = DefaultStrategy(grow_grad2d=1e-12, grow_scale3d=float(size.median()), prune_scale3d=1.2 * float(size.median()),
                               refine_start_iter=20, refine_every=20, reset_every=100, pause_refine_after_reset=5, refine_stop_iter=150,
                               refine_scale2d_stop_iter=1000, absgrad=True, revised_opacity=True)
    calls = _counting(monkeypatch, default_mod, ("duplicate", "split", "remove", "reset_opa"))
    params, opts = _trainer_of(start)
    strategy.check_sanity(params, opts)
    state = strategy.initialize_state(scene_scale=1.0)
    torch.manual_seed(0)
    losses, sizes = [], [n0]
    for step in range(steps):
        colors, _, info = _render(params, cams, absgrad=True)
        loss = photometric_loss(colors, pixels, ssim_lambda=0.2)[0]
        strategy.step_pre_backward(params, opts, state, step, info)
        loss.backward()
        strategy.step_post_backward(params, opts, state, step, info)
        step_all(opts)
        losses.append(float(loss.detach()))
        n = _check_lengths(params, opts, state)
        if n != sizes[-1]:
            sizes.append(n)
    print(f"\n[DefaultStrategy loop] loss {losses[0]:.4f} -> {losses[-1]:.4f}, gaussians {sizes}, calls {calls}")
    assert all(c > 0 for c in calls.values()), calls
    assert calls["reset_opa"] == 2  # steps 0 and 100
    assert math.isfinite(losses[-1]) and losses[-1] < losses[0]
    assert max(sizes) > n0


def test_mcmc_strategy_training_loop(monkeypatch):
    from gscodec_studio_amd.losses import photometric_loss
    from gscodec_studio_amd.optimizers import step_all
    from gscodec_studio_amd.strategy import MCMCStrategy
    from gscodec_studio_amd.strategy import mcmc as mcmc_mod

    n0, steps = 2000, 200
    start, cams, pixels = _loop_scene(n0)
    start["opacities"][::10] = -9.0  # dead from the start: relocated at the first refinement
    cap = int(n0 * 1.12)
    strategy = MCMCStrategy(cap_max=cap, refine_start_iter=20, refine_every=20, refine_stop_iter=150)
    calls = _counting(monkeypatch, mcmc_mod, ("relocate", "sample_add", "inject_noise_to_position"))
    params, opts = _trainer_of(start)
    strategy.check_sanity(params, opts)
    state = strategy.initialize_state()
    torch.manual_seed(0)
    losses, sizes = [], [n0]
    for step in range(steps):
        colors, _, info = _render(params, cams)
        loss = photometric_loss(colors, pixels, ssim_lambda=0.2)[0]
        strategy.step_pre_backward(params, opts, state, step, info)
        loss.backward()
        step_all(opts)
        strategy.step_post_backward(params, opts, state, step, info, lr=LRS["means"])
        losses.append(float(loss.detach()))
        n = _check_lengths(params, opts, state)
        assert n <= cap
        if n != sizes[-1]:
            sizes.append(n)
    print(f"\n[MCMCStrategy loop] loss {losses[0]:.4f} -> {losses[-1]:.4f}, gaussians {sizes}, calls {calls}")
    assert calls["relocate"] >= 1 and calls["sample_add"] == 3 and calls["inject_noise_to_position"] == steps
    assert sizes == [n0, int(1.05 * n0), int(1.05 * int(1.05 * n0)), cap]
    assert state["binoms"].is_cuda and state["binoms"].shape == (51, 51)
    assert math.isfinite(losses[-1]) and losses[-1] < losses[0]


@pytest.mark.parametrize("which", ["default", "mcmc"])
def test_reorder_keeps_the_rendered_image(which):
    """reorder=True: the same refinement, from the same state and the same random draws, then compression.reorder_splats --
    the set is a permutation of the un-reordered one (in Morton order) and renders the same image to 1e-4."""
    from gscodec_studio_amd.compression import morton_order
    from gscodec_studio_amd.losses import photometric_loss
    from gscodec_studio_amd.optimizers import Adam, step_all
    from gscodec_studio_amd.strategy import DefaultStrategy, MCMCStrategy

    n0, refine_at = 2000, 24
    start, cams, pixels = _loop_scene(n0)
    start["opacities"][::10] = -9.0
    size = torch.exp(start["scales"]).max(-1).values
    kw = dict(refine_start_iter=10, refine_every=refine_at, refine_stop_iter=100)
    if which == "default":
        make = lambda reorder: DefaultStrategy(grow_grad2d=1e-12, grow_scale3d=float(size.median()), reset_every=1000,  # noqa: E731
                                               reorder=reorder, **kw)
    else:
        # (noise_lr = 0: the position noise is drawn after the reordering, row i of it for another gaussian than before)
        make = lambda reorder: MCMCStrategy(cap_max=3000, noise_lr=0.0, reorder=reorder, **kw)  # noqa: E731
    strategy = make(False)
    params, opts = _trainer_of(start)
    state = strategy.initialize_state()
    extra = {"lr": LRS["means"]} if which == "mcmc" else {}
    torch.manual_seed(0)
    for step in range(refine_at + 1):
        colors, _, info = _render(params, cams)
        loss = photometric_loss(colors, pixels, ssim_lambda=0.2)[0]
        strategy.step_pre_backward(params, opts, state, step, info)
        loss.backward()
        if step == refine_at:
            break
        strategy.step_post_backward(params, opts, state, step, info, **extra)
        step_all(opts)
    # two copies of the trainer at the refining step
    twin_params = {k: torch.nn.Parameter(p.detach().clone()) for k, p in params.items()}
    twin_opts = {}
    for k, p in params.items():
        twin_opts[k] = Adam([{"params": [twin_params[k]], "lr": LRS[k], "name": k}], eps=1e-15)
        twin_opts[k].state[twin_params[k]] = {name: v.clone() for name, v in opts[k].state[p].items()}
    twin_state = {k: (v.clone() if torch.is_tensor(v) else copy.copy(v)) for k, v in state.items()}
    rng = torch.cuda.get_rng_state(DEV)
    strategy.step_post_backward(params, opts, state, refine_at, info, **extra)
    torch.cuda.set_rng_state(rng, DEV)
    make(True).step_post_backward(twin_params, twin_opts, twin_state, refine_at, info, **extra)

    n = _check_lengths(params, opts, state)
    assert _check_lengths(twin_params, twin_opts, twin_state) == n and n > n0
    perm = morton_order(params["means"].detach())
    assert not torch.equal(perm, torch.arange(n, device=DEV))
    for k in params:
        assert torch.equal(twin_params[k].detach(), params[k].detach()[perm]), k
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(twin_opts[k].state[twin_params[k]][name], opts[k].state[params[k]][name][perm]), (k, name)
    for k, v in state.items():
        if torch.is_tensor(v) and k != "binoms":
            assert torch.equal(twin_state[k], v[perm]), k
    if which == "mcmc":
        assert twin_state["binoms"].shape == (51, 51) and torch.equal(twin_state["binoms"], state["binoms"])
    with torch.no_grad():
        a, b = _render(params, cams)[0], _render(twin_params, cams)[0]
    rel = float((a - b).norm() / a.norm())
    print(f"\n[reorder {which}] {n0} -> {n} gaussians, image relL2 {rel:.2e}")
    assert rel <= 1e-4
