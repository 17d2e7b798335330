"""CPU: the 2D Gaussian splatting surface without a GPU.

* the float64 restatement (tests/surfel_reference.py), which the GPU tests use as ground truth, reproduces what the reference's
  own torch code recorded in tests/golden/surfel.npz (tests/golden/make_golden_surfel.py);
* the public names exist with the reference's parameter names and defaults;
* what is not built raises ``NotImplementedError``, CPU tensors are refused, and the native argument checks answer before any launch.
"""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import surfel_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "surfel.npz"))


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = np.abs(got - want) > 1e-4 + 1e-4 * np.abs(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} entries differ, worst {np.abs(got - want).max():.3e}"


def test_restatement_projection_reproduces_the_reference_fixture(fx):
    t = {k: torch.tensor(fx[f"proj.{k}"], dtype=torch.float64, requires_grad=True) for k in ("means", "quats", "scales", "viewmats")}
    W, H = (int(v) for v in fx["proj.size"])
    pr = R.project(t["means"], t["quats"], t["scales"], t["viewmats"], torch.tensor(fx["proj.Ks"], dtype=torch.float64), W, H)
    ref_radii = fx["proj.radii"]
    both = (pr["radii"].numpy() > 0) & (ref_radii > 0)
    # (the twin culls with the same tests up to its eps on d and its strict near / far comparisons: the sets agree on this scene
    # except where its sqrt of a negative extent gave no radius)
    assert both.sum() >= 100 and (pr["radii"].numpy() > 0).sum() - both.sum() <= 4
    # radii within 1: the reference's own tolerance, and its twin lacks the max(1e-4, .)
    assert np.abs(pr["radii"].numpy()[both] - ref_radii[both]).max() <= 1
    # the twin hands back transpose(K [a | b | mean_c]), and keeps s_z in the third column of R S, so its "normal" is the kernel's
    # unit normal times scales[:, 2] (and it alone has a gradient for that component): compared as such
    s_z = t["scales"].detach()[None, :, 2:3]
    outs = {"means2d": pr["means2d"], "depths": pr["depths"], "ray_transforms_T": pr["ray_transforms"].transpose(-1, -2),
            "normals": pr["normals"] * s_z}
    sel = torch.from_numpy(both)
    loss = 0
    for k, o in outs.items():
        _close(o.detach().numpy()[both], fx[f"proj.{k}"][both], f"projection {k}")
        m = sel.reshape(sel.shape + (1,) * (o.dim() - 2))
        loss = loss + (torch.where(m, o, torch.zeros_like(o)) * torch.tensor(fx[f"proj.cot.{k}"], dtype=torch.float64)).sum()
    loss.backward()
    # the fixture's loss runs over the twin's visible set; restrict both to splats visible in EVERY camera on both sides, where the
    # per-splat gradients are sums over the same cameras
    twin_only = (ref_radii > 0) != (pr["radii"].numpy() > 0)
    keep = ~twin_only.any(0)
    for k, cols in (("means", 3), ("quats", 4), ("scales", 2)):  # (scales[:, 2]: the twin's scaled normal alone reaches it)
        _close(t[k].grad.numpy()[keep, :cols], fx[f"proj.v_{k}"][keep, :cols], f"projection gradient of {k}")
    assert not t["scales"].grad.numpy()[:, 2].any()
    if not twin_only.any():
        _close(t["viewmats"].grad.numpy(), fx["proj.v_viewmats"], "projection gradient of viewmats")


@pytest.mark.parametrize("z_depth", [True, False])
def test_depth_to_normal_in_float64_matches_the_fixture(fx, z_depth):
    tag = "z" if z_depth else "ray"
    d = torch.tensor(fx["depth.depths"], dtype=torch.float64, requires_grad=True)
    c2w, Ks = torch.tensor(fx["depth.camtoworlds"], dtype=torch.float64), torch.tensor(fx["depth.Ks"], dtype=torch.float64)
    _close(R.depth_to_points(d, c2w, Ks, z_depth).detach().numpy(), fx[f"depth.{tag}.points"], "points")
    n = R.depth_to_normal(d, c2w, Ks, z_depth)
    _close(n.detach().numpy(), fx[f"depth.{tag}.normals"], "normals")
    (n * torch.tensor(fx["depth.cot"], dtype=torch.float64)).sum().backward()
    _close(d.grad.numpy(), fx[f"depth.{tag}.v_depths"], "gradient of the depths")
    # the package's torch depth_to_points is the same function
    from gscodec_studio_amd.utils import depth_to_points

    _close(depth_to_points(d.detach(), c2w, Ks, z_depth).numpy(), fx[f"depth.{tag}.points"], "utils.depth_to_points")


def test_restatement_sh_matches_the_oracle():
    from oracle import gs_oracle as O

    rs = np.random.RandomState(0)
    dirs, coeffs = rs.standard_normal((50, 3)).astype(np.float32), rs.standard_normal((50, 16, 3)).astype(np.float32)
    for deg in range(4):
        want = np.maximum(O.sh_fwd(deg, dirs, coeffs) + 0.5, 0.0)
        got = R.sh_colors(deg, torch.tensor(dirs, dtype=torch.float64), torch.tensor(coeffs, dtype=torch.float64)).numpy()
        assert np.abs(got - want).max() < 2e-5, deg


def test_public_names_have_the_reference_signatures(fx):
    import gscodec_studio_amd as g

    sigs = json.loads(str(fx["signatures"]))
    fns = {"rasterization_2dgs": g.rasterization_2dgs, "fully_fused_projection_2dgs": g.fully_fused_projection_2dgs,
           "rasterize_to_pixels_2dgs": g.rasterize_to_pixels_2dgs, "depth_to_points": g.utils.depth_to_points,
           "depth_to_normal": g.utils.depth_to_normal}
    assert set(sigs) == set(fns)
    for name, fn in fns.items():
        assert name in g.__all__ or name.startswith("depth_"), name
        got = [[n, None if p.default is inspect.Parameter.empty else repr(p.default)] for n, p in inspect.signature(fn).parameters.items()]
        assert got == sigs[name], (name, got, sigs[name])
    assert "utils" in g.__all__
    from gscodec_studio_amd.rendering import rasterization_2dgs

    assert rasterization_2dgs is g.rasterization_2dgs


def _scene(N=8, D=3):
    g = torch.Generator().manual_seed(0)
    return dict(means=torch.randn(N, 3, generator=g), quats=torch.randn(N, 4, generator=g), scales=torch.rand(N, 3, generator=g),
                opacities=torch.rand(N, generator=g), colors=torch.rand(N, D, generator=g), viewmats=torch.eye(4)[None],
                Ks=torch.tensor([[[30.0, 0, 16], [0, 30.0, 16], [0, 0, 1]]]), width=32, height=32)


def test_what_is_not_built_raises_before_any_launch():
    import gscodec_studio_amd as g

    s = _scene()
    with pytest.raises(NotImplementedError, match="packed"):
        g.rasterization_2dgs(**s, packed=True)
    with pytest.raises(NotImplementedError, match="packed"):
        g.rasterization_2dgs(**s, packed=True, sparse_grad=True)
    with pytest.raises(AssertionError, match="sparse_grad"):
        g.rasterization_2dgs(**s, sparse_grad=True)
    with pytest.raises(NotImplementedError, match="5 colour channels"):
        g.rasterization_2dgs(**_scene(D=4), render_mode="RGB+ED")
    with pytest.raises(NotImplementedError, match="5 colour channels"):
        g.rasterization_2dgs(**_scene(D=5))
    with pytest.raises(NotImplementedError, match="tile_size=8"):
        g.rasterization_2dgs(**s, tile_size=8)
    with pytest.raises(NotImplementedError, match="packed"):
        g.fully_fused_projection_2dgs(s["means"], s["quats"], s["scales"], s["viewmats"], s["Ks"], 32, 32, packed=True)
    C, N = 1, 8
    args = (torch.zeros(C, N, 2), torch.zeros(C, N, 3, 3), torch.zeros(C, N, 5), torch.zeros(C, N), torch.zeros(C, N, 3),
            torch.zeros(C, N, 2), 32, 32)
    offs, ids = torch.zeros(C, 2, 2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="5 colour channels"):
        g.rasterize_to_pixels_2dgs(*args, 16, offs, ids)
    args4 = args[:2] + (torch.zeros(C, N, 4),) + args[3:]
    with pytest.raises(NotImplementedError, match="tile_size=8"):
        g.rasterize_to_pixels_2dgs(*args4, 8, torch.zeros(C, 4, 4, dtype=torch.int32), ids)
    with pytest.raises(NotImplementedError, match="packed"):
        g.rasterize_to_pixels_2dgs(*args4, 16, offs, ids, packed=True)


def test_distloss_needs_a_depth_mode_and_cpu_tensors_are_refused():
    import gscodec_studio_amd as g

    s = _scene()
    with pytest.raises(AssertionError, match="distloss requires depth rendering"):
        g.rasterization_2dgs(**s, distloss=True, render_mode="RGB")
    with pytest.raises(RuntimeError, match="no CPU"):
        g.rasterization_2dgs(**s)
    with pytest.raises(RuntimeError, match="no CPU"):
        g.rasterization_2dgs(**s, render_mode="RGB+ED", distloss=True)
    with pytest.raises(RuntimeError, match="no CPU"):
        g.fully_fused_projection_2dgs(s["means"], s["quats"], s["scales"], s["viewmats"], s["Ks"], 32, 32)
    C, N = 1, 8
    with pytest.raises(RuntimeError, match="no CPU"):
        g.rasterize_to_pixels_2dgs(torch.zeros(C, N, 2), torch.zeros(C, N, 3, 3), torch.zeros(C, N, 3), torch.zeros(C, N), torch.zeros(C, N, 3),
                                   torch.zeros(C, N, 2), 32, 32, 16, torch.zeros(C, 2, 2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU"):
        g.utils.depth_to_normal(torch.ones(1, 5, 5, 1), torch.eye(4)[None], s["Ks"])


def test_native_argument_checks_answer_before_any_launch():
    from gscodec_studio_amd import _backend as B

    def fwd(channels, tile_size, width=16, height=16, tw=1, th=1, outputs=None):
        B.call("gs_rasterize_2dgs_fwd", 1, 1, 0, channels, None, None, None, None, None, None, None, width, height, tile_size, tw, th, None,
               None, 0, outputs, outputs, outputs, outputs, outputs, outputs, outputs, None)

    with pytest.raises(RuntimeError, match="unsupported number of colour channels 5"):
        fwd(5, 16)
    with pytest.raises(RuntimeError, match="unsupported number of colour channels 0"):
        fwd(0, 16)
    with pytest.raises(RuntimeError, match="tile_size must be 16"):
        fwd(3, 8)
    with pytest.raises(RuntimeError, match="does not cover"):
        fwd(3, 16, width=40, tw=2)
    with pytest.raises(RuntimeError, match="go together"):
        fwd(3, 16)
    with pytest.raises(RuntimeError, match="unsupported number of colour channels 7"):
        B.call("gs_rasterize_2dgs_bwd", 1, 1, 0, 7, *([None] * 7), 16, 16, 16, 1, 1, None, None, 0, *([None] * 15), None)
    with pytest.raises(RuntimeError, match="go together"):
        B.call("gs_projection_2dgs_bwd", 1, 1, 1, 1, 1, 1, 1, 1, 1, None, None, None, None, 1, None, 1, None, None)
    with pytest.raises(RuntimeError, match="null output pointer"):
        B.call("gs_projection_2dgs_fwd", 1, 1, 1, 1, 1, 1, 1, 8, 8, 0.3, 0.01, 1e10, 0.0, None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        B.call("gs_depth_to_normal_fwd", 1, 4, 4, None, None, None, 1, None, None)
