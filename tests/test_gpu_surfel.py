"""GPU: the 2D Gaussian splatting operators and ``rasterization_2dgs`` against the float64 restatement
(tests/surfel_reference.py) on the scenes of tests/surfel_cases.py.

The bar.  Forward outputs: relative L2 <= 1e-4 against float64 (the project's parity bar).  Each gradient: relative L2 <=
max(1e-4, 4 * e32), where e32 is the relative L2 of the SAME restatement run in float32 on the CPU against its float64 run -- what
float32 arithmetic alone does to that gradient (``s = zeta_xy / zeta_z`` is ill-conditioned for grazing splats, so a fixed 1e-4
cannot be promised) -- and the factor 4 covers the atomics' summation order and the hardware ``exp``.

Discrete decisions can flip between float32 and float64 and must not hide a failure: the restatement flags a pixel when, for any
splat it evaluates there, alpha vs 1/255, o exp(-sigma) vs 0.999, T (1 - alpha) vs 1e-4, T vs 0.5 or the two kernel weights vs each
other lie within 1e-4 relative.  Flagged pixels get weight zero in the loss on both sides and are left out of the forward
comparison; at most 2 % of the pixels may be flagged (asserted).  Every test prints its measured ratios (``pytest -s``).
"""
import functools

import numpy as np
import pytest
import torch

import surfel_cases as S
import surfel_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H = S.WIDTH, S.HEIGHT
MAX_FLAGGED = 0.02


def _bar(e32):
    return max(1e-4, 4.0 * e32)


def _report(test, rows):
    for name, err, bar in rows:
        print(f"[surfel] {test:<44s} {name:<22s} err {err:.3e}  bar {bar:.3e}  ratio {err / bar:.3f}")


def _check(test, rows):
    _report(test, rows)
    bad = [(n, e, b) for n, e, b in rows if not e <= b]
    assert not bad, f"{test}: beyond the bar: {bad}"


@functools.lru_cache(maxsize=None)
def _scene(name):
    sc = {"main": S.main_scene, "small": S.small_scene, "degenerate": S.degenerate_scene}[name]()
    return {k: torch.tensor(v, dtype=torch.float32) for k, v in sc.items()}  # the float32 values every side starts from


@functools.lru_cache(maxsize=None)
def _projection64(name):
    sc = _scene(name)
    with torch.no_grad():
        return R.project(sc["means"].double(), sc["quats"].double(), sc["scales"].double(), sc["viewmats"].double(), sc["Ks"].double(), W, H)


@functools.lru_cache(maxsize=None)
def _lists(name):
    """Tile lists of the library's own binning on the restatement's projection cast to float32 (so only the compositing differs)."""
    import gscodec_studio_amd as g

    pr = _projection64(name)
    C = pr["radii"].shape[0]
    m2, rad, dep = pr["means2d"].float().to(DEV), pr["radii"].to(DEV), pr["depths"].float().to(DEV)
    tw, th = (W + 15) // 16, (H + 15) // 16
    _, isect_ids, flatten_ids = g.isect_tiles(m2, rad, dep, 16, tw, th, n_cameras=C)
    offsets = g.isect_offset_encode(isect_ids, C, tw, th)
    return offsets, flatten_ids


def _composite_inputs(name, channels, seed=7):
    """float32 inputs of the compositing operator: the restatement's projection, colours whose last channel is the depth."""
    sc, pr = _scene(name), _projection64(name)
    C, N = pr["radii"].shape
    rs = np.random.RandomState(seed)
    rgb = torch.tensor(rs.uniform(0.0, 1.0, (C, N, 3)), dtype=torch.float32)
    depth = pr["depths"].float()[..., None]
    colors = {1: depth, 3: rgb, 4: torch.cat([rgb, depth], -1)}[channels]
    opac = sc["opacities"][None].repeat(C, 1) * torch.tensor(rs.uniform(0.9, 1.0, (C, 1)), dtype=torch.float32)
    opac[sc["opacities"][None].expand(C, -1) == 1.0] = 1.0  # (the clamped splats stay at exactly 1)
    return dict(means2d=pr["means2d"].float(), ray_transforms=pr["ray_transforms"].float(), colors=colors.contiguous(), opacities=opac,
                normals=pr["normals"].float(), backgrounds=torch.tensor(rs.uniform(0.0, 1.0, (C, channels)), dtype=torch.float32))


_OUT = ("colors", "alphas", "normals", "distort", "median")
_GRADS = ("means2d", "ray_transforms", "colors", "opacities", "normals", "densify", "backgrounds", "absgrad")


def _cotangents(C, channels, seed=11):
    rs = np.random.RandomState(seed)
    return {k: torch.tensor(rs.standard_normal((C, H, W, n))) for k, n in zip(_OUT, (channels, 1, 3, 1, 1))}


def _restatement_composite(inp, lists, use_bg, distloss, dtype, cots, mask=None):
    """-> (outputs, gradients, compositing dict); the loss is sum(mask * cot * output) over the five outputs."""
    t = {k: v.to(dtype).clone().requires_grad_(True) for k, v in inp.items()}
    offsets, flatten_ids = (x.cpu() for x in lists)
    cp = R.composite(t["means2d"], t["ray_transforms"], t["colors"], t["opacities"], t["normals"], t["backgrounds"] if use_bg else None,
                     W, H, offsets, flatten_ids, distloss, keep_pixel_grads=True)
    if mask is None:
        mask = ~cp["near_decision"]
    m = mask[..., None].to(dtype)
    sum((cp[k] * cots[k].to(dtype) * m).sum() for k in _OUT).backward()
    ab, plain = R.absgrad_from_pixels(cp["pixel_means2d"], t["means2d"].numel() // 2, dtype)
    v_rt = t["ray_transforms"].grad
    grads = dict(means2d=plain.reshape(t["means2d"].shape), ray_transforms=v_rt, colors=t["colors"].grad, opacities=t["opacities"].grad,
                 normals=t["normals"].grad, densify=v_rt[..., 0:2, 2] * t["ray_transforms"].detach()[..., 2, 2].unsqueeze(-1),
                 backgrounds=t["backgrounds"].grad if use_bg else None, absgrad=ab.reshape(t["means2d"].shape))
    return {k: cp[k].detach() for k in _OUT}, grads, cp, mask


def _gpu_composite(inp, lists, use_bg, distloss, cots, mask):
    import gscodec_studio_amd as g

    t = {k: v.to(DEV).requires_grad_(True) for k, v in inp.items()}
    densify = torch.zeros_like(t["means2d"], requires_grad=True)
    outs = g.rasterize_to_pixels_2dgs(t["means2d"], t["ray_transforms"], t["colors"], t["opacities"], t["normals"], densify, W, H, 16,
                                      lists[0], lists[1], backgrounds=t["backgrounds"] if use_bg else None, absgrad=True, distloss=distloss)
    outs = dict(zip(_OUT, outs))
    m = mask[..., None].float().to(DEV)
    sum((outs[k] * cots[k].float().to(DEV) * m).sum() for k in _OUT).backward()
    grads = {k: t[k].grad for k in ("means2d", "ray_transforms", "colors", "opacities", "normals")}
    grads.update(densify=densify.grad, backgrounds=t["backgrounds"].grad if use_bg else None, absgrad=t["means2d"].absgrad)
    return {k: v.detach() for k, v in outs.items()}, grads


def _compare_composite(test, name, channels, use_bg, distloss):
    inp, lists = _composite_inputs(name, channels), _lists(name)
    C = inp["means2d"].shape[0]
    cots = _cotangents(C, channels)
    out64, g64, cp, mask = _restatement_composite(inp, lists, use_bg, distloss, torch.float64, cots)
    flagged = 1.0 - float(mask.float().mean())
    assert flagged <= MAX_FLAGGED, f"{flagged:.4f} of the pixels lie near a decision threshold"
    _, g32, _, _ = _restatement_composite(inp, lists, use_bg, distloss, torch.float32, cots, mask)
    out, grads = _gpu_composite(inp, lists, use_bg, distloss, cots, mask)
    m = mask[..., None].double()
    rows = [(f"fwd {k}", R.rel_l2(out[k].cpu().double() * m, out64[k] * m), 1e-4) for k in _OUT]
    if not distloss:
        assert not out["distort"].any(), "the distortion map must be zeros without distloss"
    for k in _GRADS:
        if g64[k] is None:
            assert grads[k] is None
            continue
        rows.append((f"grad {k}", R.rel_l2(grads[k], g64[k]), _bar(R.rel_l2(g32[k], g64[k]))))
    _check(test, rows)
    return cp


def test_main_scene_coverage_and_compositing():
    """The main scene takes every path (asserted on the restatement's counters, before the GPU is looked at), then all five
    outputs and all seven gradients (+ absgrad) of ``rasterize_to_pixels_2dgs`` with 4 channels, backgrounds and distloss."""
    inp, lists = _composite_inputs("main", 4), _lists("main")
    with torch.no_grad():
        cp = R.composite(*(inp[k].double() for k in ("means2d", "ray_transforms", "colors", "opacities", "normals", "backgrounds")), W, H,
                         lists[0].cpu(), lists[1].cpu(), True)
    assert int(cp["list_lengths"].max()) > 256, cp["list_lengths"].tolist()
    assert int(cp["early"].sum()) >= 20 and int((~cp["early"]).sum()) >= 20
    assert int(cp["n_filter"].sum()) >= 50
    assert int(cp["n_clamped"].sum()) >= 4
    assert int((cp["n_contrib"] == 0).sum()) >= 1 and not cp["median"][cp["n_contrib"] == 0].any()
    assert int((~cp["T_min_reached"] & (cp["n_contrib"] > 0)).sum()) >= 1
    print(f"[surfel] main scene: longest list {int(cp['list_lengths'].max())}, early {int(cp['early'].sum())}, filter-branch "
          f"{int(cp['n_filter'].sum())}, clamped {int(cp['n_clamped'].sum())}, empty pixels {int((cp['n_contrib'] == 0).sum())}, "
          f"flagged {100 * float(cp['near_decision'].float().mean()):.3f} %")
    _compare_composite("main scene ch4 bg distloss", "main", 4, True, True)


@pytest.mark.parametrize("distloss", [False, True])
@pytest.mark.parametrize("use_bg", [False, True])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_compositing_sweep_small_scene(channels, use_bg, distloss):
    cp = _compare_composite(f"small ch{channels} bg{int(use_bg)} dist{int(distloss)}", "small", channels, use_bg, distloss)
    assert int(cp["list_lengths"].max()) <= 42


def test_projection_main_scene():
    import gscodec_studio_amd as g

    sc, pr = _scene("main"), _projection64("main")
    assert not pr["near_cull"].any(), "a culling quantity lies within 1e-4 of its threshold: pick another seed"
    names = ("means", "quats", "scales", "viewmats")
    outs = ("means2d", "depths", "ray_transforms", "normals")
    rs = np.random.RandomState(13)
    cots = {k: torch.tensor(rs.standard_normal(tuple(pr[k].shape))) for k in outs}

    def restate(dtype):
        t = {k: sc[k].to(dtype).clone().requires_grad_(True) for k in names}
        p = R.project(t["means"], t["quats"], t["scales"], t["viewmats"], sc["Ks"].to(dtype), W, H)
        sum((p[k] * cots[k].to(dtype)).sum() for k in outs).backward()
        return p, {k: t[k].grad for k in names}

    p64, g64 = restate(torch.float64)
    _, g32 = restate(torch.float32)
    t = {k: sc[k].to(DEV).requires_grad_(True) for k in names}
    radii, means2d, depths, ray_transforms, normals = g.fully_fused_projection_2dgs(t["means"], t["quats"], t["scales"], t["viewmats"],
                                                                                    sc["Ks"].to(DEV), W, H)
    got = dict(means2d=means2d, depths=depths, ray_transforms=ray_transforms, normals=normals)
    sum((got[k] * cots[k].float().to(DEV)).sum() for k in outs).backward()
    vis = p64["visible"]
    assert torch.equal(radii.cpu() > 0, vis), "visible masks differ"
    rr = p64["radius_raw"]
    near_int = ((rr - torch.round(rr)).abs() <= 1e-4 * rr) & vis
    diff = (radii.cpu() - p64["radii"]).abs()
    assert not diff[~near_int].any(), "radii differ away from an integer boundary"
    assert int(diff.max()) <= 1 and int((diff > 0).sum()) <= 0.01 * int(vis.sum())
    for k in outs:  # culled splats: zeros on both sides
        assert not got[k].detach().cpu()[~vis].any()
    rows = [(f"fwd {k}", R.rel_l2(got[k].detach(), p64[k].detach()), 1e-4) for k in outs]
    rows += [(f"grad {k}", R.rel_l2(t[k].grad, g64[k]), _bar(R.rel_l2(g32[k], g64[k]))) for k in names]
    assert not t["scales"].grad[:, 2].any() and not g64["scales"][:, 2].any()
    _check("projection main scene", rows)


_E2E_OUT = ("colors", "alphas", "normals", "normals_from_depth", "distort", "median")


def _e2e(test, name, render_mode, sh_degree, distloss, depth_mode, use_bg):
    import gscodec_studio_amd as g

    sc = _scene(name)
    N, C = sc["means"].shape[0], sc["viewmats"].shape[0]
    rs = np.random.RandomState(17)
    if sh_degree is None:
        colors = torch.tensor(rs.uniform(0.0, 1.0, (N, 3)), dtype=torch.float32)
    else:
        colors = torch.tensor(rs.standard_normal((N, 16, 3)) * 0.3, dtype=torch.float32)
    bg = torch.tensor(rs.uniform(0.0, 1.0, (C, 1 if render_mode in ("D", "ED") else 3)), dtype=torch.float32) if use_bg else None
    leaves = dict(means=sc["means"], quats=sc["quats"], scales=sc["scales"], opacities=sc["opacities"], colors=colors)

    t = {k: v.to(DEV).requires_grad_(True) for k, v in leaves.items()}
    res = g.rasterization_2dgs(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], sc["viewmats"].to(DEV), sc["Ks"].to(DEV), W, H,
                               sh_degree=sh_degree, backgrounds=bg.to(DEV) if use_bg else None, render_mode=render_mode, absgrad=True,
                               distloss=distloss, depth_mode=depth_mode)
    got, meta = dict(zip(_E2E_OUT, res[:6])), res[6]
    for key in ("camera_ids", "gaussian_ids", "radii", "means2d", "depths", "ray_transforms", "opacities", "normals", "tile_width",
                "tile_height", "tiles_per_gauss", "isect_ids", "flatten_ids", "isect_offsets", "width", "height", "tile_size", "n_cameras",
                "render_distort", "gradient_2dgs"):
        assert key in meta, key
    assert (got["normals_from_depth"] is None) == (render_mode not in ("RGB+D", "RGB+ED"))
    lists = (meta["isect_offsets"].cpu(), meta["flatten_ids"].cpu())
    cots = {k: torch.tensor(rs.standard_normal(tuple(v.shape))) for k, v in got.items() if v is not None}

    def restate(dtype, mask=None):
        r = {k: v.to(dtype).clone().requires_grad_(True) for k, v in leaves.items()}
        out = R.render(r["means"], r["quats"], r["scales"], r["opacities"], r["colors"], sc["viewmats"].to(dtype), sc["Ks"].to(dtype), W, H,
                       lists[0], lists[1], sh_degree=sh_degree, backgrounds=bg.to(dtype) if use_bg else None, render_mode=render_mode,
                       distloss=distloss, depth_mode=depth_mode)
        o, info = dict(zip(_E2E_OUT, out[:6])), out[6]
        if mask is None:
            flag = info["near_decision"]
            # a normal from depth reads its four neighbours' depths: left out where any of them is flagged
            wide = flag.clone()
            wide[:, 1:] |= flag[:, :-1]
            wide[:, :-1] |= flag[:, 1:]
            wide[:, :, 1:] |= flag[:, :, :-1]
            wide[:, :, :-1] |= flag[:, :, 1:]
            mask = {k: ~(wide if k == "normals_from_depth" else flag) for k in _E2E_OUT}
        info["ray_transforms"].retain_grad()
        sum((o[k] * cots[k].to(dtype) * mask[k][..., None].to(dtype)).sum() for k in cots).backward()
        grads = {k: r[k].grad for k in leaves}
        v_rt = info["ray_transforms"].grad
        grads["gradient_2dgs"] = v_rt[..., 0:2, 2] * info["depths"].detach()[..., None]
        return {k: (v.detach() if v is not None else None) for k, v in o.items()}, grads, info, mask

    o64, g64, info, mask = restate(torch.float64)
    flagged = float(info["near_decision"].float().mean())
    assert flagged <= MAX_FLAGGED, f"{flagged:.4f} of the pixels lie near a decision threshold"
    assert torch.equal(meta["radii"].cpu() > 0, info["visible"]), "visible masks differ"
    _, g32, _, _ = restate(torch.float32, mask)
    meta["gradient_2dgs"].retain_grad()
    sum((got[k] * cots[k].float().to(DEV) * mask[k][..., None].float().to(DEV)).sum() for k in cots).backward()
    rows = []
    for k in cots:
        m = mask[k][..., None].double()
        rows.append((f"fwd {k}", R.rel_l2(got[k].detach().cpu().double() * m, o64[k] * m), 1e-4))
    for k in leaves:
        if k == "colors" and render_mode in ("D", "ED"):
            assert t[k].grad is None or not t[k].grad.any()  # (the colours are not rendered)
            continue
        rows.append((f"grad {k}", R.rel_l2(t[k].grad, g64[k]), _bar(R.rel_l2(g32[k], g64[k]))))
    rows.append(("grad gradient_2dgs", R.rel_l2(meta["gradient_2dgs"].grad, g64["gradient_2dgs"]),
                 _bar(R.rel_l2(g32["gradient_2dgs"], g64["gradient_2dgs"]))))
    assert meta["means2d"].absgrad is not None and meta["means2d"].absgrad.shape == meta["means2d"].shape
    assert not hasattr(meta["gradient_2dgs"], "absgrad")
    _check(test, rows)


@pytest.mark.parametrize("render_mode,sh_degree,distloss,depth_mode,use_bg", [
    ("RGB", None, False, "expected", True),
    ("RGB", 3, False, "expected", False),
    ("ED", None, True, "expected", False),
    ("RGB+ED", 3, True, "expected", True),
    ("RGB+ED", None, True, "median", False),
    ("RGB+ED", 3, True, "median", True),
])
def test_rasterization_2dgs_small_scene(render_mode, sh_degree, distloss, depth_mode, use_bg):
    _e2e(f"e2e small {render_mode} sh{sh_degree} {depth_mode}", "small", render_mode, sh_degree, distloss, depth_mode, use_bg)


def test_rasterization_2dgs_main_scene():
    _e2e("e2e main RGB+ED sh3 expected", "main", "RGB+ED", 3, True, "expected", True)


def test_default_strategy_reads_gradient_2dgs():
    """DefaultStrategy(key_for_gradient="gradient_2dgs"): pre-backward, backward, post-backward; its running statistics equal what the
    restatement's gradient gives through the strategy's own formula (norm of the gradient scaled by (W / 2, H / 2) * n_cameras,
    summed over the cameras that see the splat; the count of those cameras)."""
    import gscodec_studio_amd as g
    from gscodec_studio_amd.strategy import DefaultStrategy

    sc = _scene("small")
    N, C = sc["means"].shape[0], sc["viewmats"].shape[0]
    rs = np.random.RandomState(19)
    colors = torch.tensor(rs.uniform(0.0, 1.0, (N, 3)), dtype=torch.float32)
    target = torch.tensor(rs.uniform(0.0, 1.0, (C, H, W, 3)))
    leaves = dict(means=sc["means"], quats=sc["quats"], scales=sc["scales"], opacities=sc["opacities"], colors=colors)
    params = torch.nn.ParameterDict({k: torch.nn.Parameter(v.to(DEV)) for k, v in leaves.items()})
    strategy = DefaultStrategy(key_for_gradient="gradient_2dgs")
    state = strategy.initialize_state()
    res = g.rasterization_2dgs(params["means"], params["quats"], params["scales"], params["opacities"], params["colors"],
                               sc["viewmats"].to(DEV), sc["Ks"].to(DEV), W, H)
    meta = res[6]
    lists = (meta["isect_offsets"].cpu(), meta["flatten_ids"].cpu())

    def restate(dtype, mask=None):
        r = {k: v.to(dtype).clone().requires_grad_(True) for k, v in leaves.items()}
        out = R.render(r["means"], r["quats"], r["scales"], r["opacities"], r["colors"], sc["viewmats"].to(dtype), sc["Ks"].to(dtype), W, H,
                       lists[0], lists[1])
        info = out[6]
        mask = ~info["near_decision"] if mask is None else mask
        info["ray_transforms"].retain_grad()
        (((out[0] - target.to(dtype)) ** 2) * mask[..., None].to(dtype)).sum().backward()
        grad = info["ray_transforms"].grad[..., 0:2, 2] * info["depths"].detach()[..., None]
        grad = grad * torch.tensor([W / 2.0 * C, H / 2.0 * C], dtype=dtype)
        sel = info["radii"] > 0
        return (grad.norm(dim=-1) * sel).sum(0), sel.sum(0).to(dtype), mask

    want64, count64, mask = restate(torch.float64)
    want32, _, _ = restate(torch.float32, mask)
    strategy.step_pre_backward(params, {}, state, 1, meta)
    (((res[0] - target.float().to(DEV)) ** 2) * mask[..., None].float().to(DEV)).sum().backward()
    strategy.step_post_backward(params, {}, state, 1, meta)
    assert torch.equal(state["count"].cpu().double(), count64)
    _check("DefaultStrategy gradient_2dgs", [("grad2d", R.rel_l2(state["grad2d"], want64), _bar(R.rel_l2(want32, want64)))])


@pytest.mark.parametrize("z_depth", [True, False])
@pytest.mark.parametrize("shape", [(2, 27, 40, 1), (1, 3, 3, 1)])
def test_depth_to_normal(shape, z_depth):
    from gscodec_studio_amd.utils import depth_to_normal

    rs = np.random.RandomState(23)
    B = shape[0]
    depths = torch.tensor(rs.uniform(1.5, 4.0, shape), dtype=torch.float32)
    viewmats, Ks = S.cameras()
    c2w = torch.tensor(np.linalg.inv(viewmats)[:B], dtype=torch.float32)
    Ks = torch.tensor(Ks[:B], dtype=torch.float32)
    cot = torch.tensor(rs.standard_normal(shape[:-1] + (3,)))

    def restate(dtype):
        d = depths.to(dtype).clone().requires_grad_(True)
        n = R.depth_to_normal(d, c2w.to(dtype), Ks.to(dtype), z_depth)
        (n * cot.to(dtype)).sum().backward()
        return n.detach(), d.grad

    n64, g64 = restate(torch.float64)
    _, g32 = restate(torch.float32)
    d = depths.to(DEV).requires_grad_(True)
    n = depth_to_normal(d, c2w.to(DEV), Ks.to(DEV), z_depth=z_depth)
    (n * cot.float().to(DEV)).sum().backward()
    assert n.shape == shape[:-1] + (3,)
    border = torch.ones(shape[:-1], dtype=torch.bool)
    border[:, 1:-1, 1:-1] = False
    assert not n.detach().cpu()[border].any()
    _check(f"depth_to_normal {shape} z_depth={z_depth}",
           [("fwd normals", R.rel_l2(n.detach(), n64), 1e-4), ("grad depths", R.rel_l2(d.grad, g64), _bar(R.rel_l2(g32, g64)))])


def test_degenerate_scene_forward():
    """Splats behind the camera, beyond far_plane, below radius_clip, one exactly edge-on (d == 0), one whose ray transform makes
    zeta_z == 0 at every pixel; then a call where every splat is culled."""
    import gscodec_studio_amd as g

    sc = _scene("degenerate")
    N, C = sc["means"].shape[0], sc["viewmats"].shape[0]
    kw = dict(near_plane=0.01, far_plane=50.0, radius_clip=2.5)
    with torch.no_grad():
        p64 = R.project(*(sc[k].double() for k in ("means", "quats", "scales", "viewmats", "Ks")), W, H, **kw)
    assert not p64["near_cull"].any()
    vis = p64["visible"]
    assert not vis[:2, :9].any() and not vis[2, 9], "the splats meant to be culled are not"
    assert int(((p64["radius_raw"] <= 2.5) & ~vis).sum()) >= 1 and int(vis.sum()) >= 10
    dsc = {k: v.to(DEV) for k, v in sc.items()}
    radii, means2d, depths, ray_transforms, normals = g.fully_fused_projection_2dgs(dsc["means"], dsc["quats"], dsc["scales"], dsc["viewmats"],
                                                                                    dsc["Ks"], W, H, **kw)
    assert torch.equal(radii.cpu() > 0, vis)
    assert int(radii[2, 9]) == 0 and not ray_transforms[2, 9].any()
    rows = [(f"fwd {k}", R.rel_l2(v, p64[k]), 1e-4) for k, v in dict(means2d=means2d, depths=depths, ray_transforms=ray_transforms, normals=normals).items()]

    # compositing with one visible splat's transform replaced by one whose zeta_z is zero at every pixel: it must not contribute
    rt = ray_transforms.clone()
    c0, n0 = (int(v[0]) for v in torch.nonzero(radii > 0, as_tuple=True))
    rt[c0, n0] = torch.tensor([[1.0, 0.0, 5.0], [0.0, 0.0, 7.0], [0.0, 0.0, 1.0]], device=DEV)
    tw, th = (W + 15) // 16, (H + 15) // 16
    _, isect_ids, flatten_ids = g.isect_tiles(means2d, radii, depths, 16, tw, th, n_cameras=C)
    offsets = g.isect_offset_encode(isect_ids, C, tw, th)
    rs = np.random.RandomState(29)
    colors = torch.cat([torch.tensor(rs.uniform(0, 1, (C, N, 2)), dtype=torch.float32).to(DEV), depths[..., None]], -1)
    opac = dsc["opacities"][None].repeat(C, 1)
    bg = torch.tensor(rs.uniform(0, 1, (C, 3)), dtype=torch.float32)
    outs = g.rasterize_to_pixels_2dgs(means2d, rt, colors, opac, normals, torch.zeros_like(means2d), W, H, 16, offsets, flatten_ids,
                                      backgrounds=bg.to(DEV), distloss=True)
    with torch.no_grad():
        cp = R.composite(means2d.cpu().double(), rt.cpu().double(), colors.cpu().double(), opac.cpu().double(), normals.cpu().double(),
                         bg.double(), W, H, offsets.cpu(), flatten_ids.cpu(), True)
    assert float(cp["near_decision"].float().mean()) <= MAX_FLAGGED
    m = (~cp["near_decision"])[..., None].double()
    rows += [(f"fwd composite {k}", R.rel_l2(o.cpu().double() * m, cp[k] * m), 1e-4) for k, o in zip(_OUT, outs)]
    _check("degenerate scene", rows)

    # every splat culled (far_plane below near_plane): zero images, backgrounds honoured, no error -- forward and backward
    t = {k: dsc[k].clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacities")}
    colors3 = torch.tensor(rs.uniform(0, 1, (N, 3)), dtype=torch.float32).to(DEV).requires_grad_(True)
    res = g.rasterization_2dgs(t["means"], t["quats"], t["scales"], t["opacities"], colors3, dsc["viewmats"], dsc["Ks"], W, H, far_plane=0.005,
                               backgrounds=bg.to(DEV), render_mode="RGB+ED", distloss=True)
    rc, ra, rn, nfd, rd, rm, meta = res
    assert meta["flatten_ids"].numel() == 0 and not (meta["radii"] > 0).any()
    assert torch.equal(rc[..., :3].cpu(), bg[:, None, None, :].expand(C, H, W, 3)) and not rc[..., 3].any()
    for o in (ra, rn, nfd, rd, rm):
        assert not o.any()
    (rc.sum() + ra.sum() + rn.sum() + rd.sum() + rm.sum()).backward()
    for k, v in t.items():
        assert v.grad is None or not v.grad.any(), k
