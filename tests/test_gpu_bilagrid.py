"""gscodec_studio_amd.bilagrid on the GPU (csrc/bilagrid.hip): slice, slice_image, BilateralGrid.forward and total_variation_loss
-- outputs and both gradients -- against tests/golden/bilagrid.npz (the reference's own output) and against the float64 restatement
of tests/test_bilagrid_cpu.py on fresh inputs, at the project's bar of 1e-4 relative L2 per tensor; the float32 F.grid_sample
composition's own distance from float64 is printed beside ours.  Then: the identity grid, slice_image against slice with the
explicit meshgrid, a strided render view, no host synchronisation, and five iterations of the small trainer loop with the grid in
place against the same loop with the torch composition."""
import numpy as np
import pytest
import torch

from test_bilagrid_cpu import CASES, GRID_KEYS, golden, ref_mats, ref_slice, ref_tv, rel_l2
from test_gpu_losses import LRS, _trainer_scene

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAR = 1e-4


def _module(grids):
    from gscodec_studio_amd.bilagrid import BilateralGrid

    n, _, l, h, w = grids.shape
    m = BilateralGrid(n, grid_X=w, grid_Y=h, grid_W=l).to(DEV)
    with torch.no_grad():
        m.grids.copy_(torch.as_tensor(grids, device=DEV))
    return m


def _random_grids(n, shape, seed, scale=0.1):
    X, Y, L = shape
    eye = torch.eye(3, 4, device=DEV).reshape(1, 12, 1, 1, 1)
    return eye + scale * torch.randn((n, 12, L, Y, X), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _oracle(grids, xy, rgb, idx, cot, dtype, mats_cot=None):
    """Outputs and gradients of the restatement in dtype: (rgb_out, mats, v_grids, v_rgb)."""
    g = grids.detach().to(dtype).requires_grad_(True)
    c = rgb.detach().to(dtype).requires_grad_(True)
    out, mats = ref_slice(g, xy.to(dtype), c, idx)
    loss = (out * cot.to(dtype)).sum() if mats_cot is None else (mats * mats_cot.to(dtype)).sum()
    loss.backward()
    return out.detach(), mats.detach(), g.grad, c.grad


def _report(tag, ours, f64, f32):
    names = ("rgb", "mats", "v_grids", "v_rgb")
    e_ours = {k: rel_l2(a, b) for k, a, b in zip(names, ours, f64) if a is not None}
    e_f32 = {k: rel_l2(a, b) for k, a, b in zip(names, f32, f64)}
    print(f"\n[{tag}] ours vs float64: " + " ".join(f"{k} {v:.2e}" for k, v in e_ours.items()) + " | torch float32 vs float64: "
          + " ".join(f"{k} {v:.2e}" for k, v in e_f32.items()))
    return e_ours


@pytest.mark.parametrize("case", CASES)
def test_slice_against_the_reference_fixture(case):
    from gscodec_studio_amd.bilagrid import slice as bslice

    fx, grids = golden()
    m = _module(grids[str(fx[f"{case}.grids"])])
    T = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    xy, idx, cot = T(fx[f"{case}.xy"]), T(fx[f"{case}.idx"]), T(fx[f"{case}.cot"])
    rgb = T(fx[f"{case}.rgb"]).requires_grad_(True)
    out = bslice(m, xy, rgb, idx)
    assert out["rgb"].shape == rgb.shape and out["rgb_affine_mats"].shape == (*rgb.shape[:-1], 3, 4)
    assert not out["rgb_affine_mats"].requires_grad
    (out["rgb"] * cot).sum().backward()
    vg = m.grids.grad.cpu()
    errs = {"rgb": rel_l2(out["rgb"].detach(), fx[f"{case}.out_rgb"]), "mats": rel_l2(out["rgb_affine_mats"], fx[f"{case}.out_mats"]),
            "v_rgb": rel_l2(rgb.grad, fx[f"{case}.v_rgb"])}
    if f"{case}.v_grids" in fx:
        errs["v_grids"] = rel_l2(vg, fx[f"{case}.v_grids"])
    elif f"{case}.v_grids_1" in fx:
        assert not vg[0].any() and not vg[2].any()
        errs["v_grids"] = rel_l2(vg[1], fx[f"{case}.v_grids_1"])
    else:
        nz = torch.tensor(fx[f"{case}.v_grids_nz_index"].astype(np.int64))
        errs["v_grids"] = rel_l2(vg.reshape(-1)[nz], fx[f"{case}.v_grids_nz_value"])
        rest = vg.reshape(-1).clone()
        rest[nz] = 0
        assert float(rest.abs().max()) <= 1e-6 * float(vg.abs().max())
    first = idx.reshape(rgb.shape[0], -1)[:, 0]
    f64 = _oracle(m.grids, xy, rgb, first, cot, torch.float64)
    f32 = _oracle(m.grids, xy, rgb, first, cot, torch.float32)
    e64 = _report(f"slice fixture {case}", (out["rgb"].detach(), out["rgb_affine_mats"], m.grids.grad, rgb.grad), f64, f32)
    print(f"[slice fixture {case}] ours vs the reference's float32 output: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= BAR for v in errs.values()), errs
    assert all(v <= BAR for v in e64.values()), e64
    # the extensions: a 1-D grid_idx, and (where every entry shares its coordinates) nothing else changes
    again = bslice(m, xy, rgb.detach(), first.contiguous(), affine_mats=False)
    assert set(again) == {"rgb"} and torch.equal(again["rgb"], out["rgb"].detach())


FRESH = [
    # tag, grid (X, Y, W), number of grids, point shape, which entry point
    ("1080p", (16, 16, 8), 4, (1, 1080, 1920), "image"),
    ("batch8", (16, 16, 8), 9, (8, 270, 480), "image"),
    ("batch8-xy", (16, 16, 8), 9, (8, 270, 480), "slice"),
    ("odd-grid-image", (5, 4, 3), 3, (2, 37, 53), "image"),
    ("thin-image", (16, 16, 8), 3, (2, 7, 300), "image"),
    ("rays-3d-general-path", (40, 40, 8), 3, (3, 1, 5000), "slice"),   # a box of 40 x 40 x 8 x 12 floats does not fit the LDS area
    ("rays-2d-point-kernel", (7, 9, 5), 5, (3000, 1, 1), "slice"),
    ("size-one-axes", (1, 6, 1), 2, (2, 1, 700), "slice"),
]


@pytest.mark.parametrize("tag, gshape, n, pshape, entry", FRESH, ids=[f[0] for f in FRESH])
def test_slice_and_slice_image_against_float64(tag, gshape, n, pshape, entry):
    from gscodec_studio_amd.bilagrid import slice as bslice, slice_image

    gen = torch.Generator(device=DEV).manual_seed(len(tag))
    m = _module(_random_grids(n, gshape, seed=3))
    B, D1, D2 = pshape
    rgb = (torch.rand((B, D1, D2, 3), device=DEV, generator=gen) * 1.3 - 0.15)  # some guidance values clamp
    cot = torch.randn((B, D1, D2, 3), device=DEV, generator=gen)
    idx = torch.randint(0, n, (B,), device=DEV, generator=gen)
    if entry == "image":
        gy, gx = torch.meshgrid((torch.arange(D1, device=DEV) + 0.5) / D1, (torch.arange(D2, device=DEV) + 0.5) / D2, indexing="ij")
        xy = torch.stack([gx, gy], dim=-1).unsqueeze(0)
        a = rgb.clone().requires_grad_(True)
        out = slice_image(m, a, idx)
        mats = None
    else:
        xy = torch.rand((B, D1, D2, 2), device=DEV, generator=gen) * 1.1 - 0.05  # some coordinates clamp
        shape = {"rays-2d-point-kernel": (B,), "batch8-xy": (B, D1, D2)}.get(tag, (B, D2))
        xy, rgb, cot = xy.reshape(*shape, 2), rgb.reshape(*shape, 3), cot.reshape(*shape, 3)
        a = rgb.clone().requires_grad_(True)
        res = bslice(m, xy, a, idx.reshape(B, *([1] * (len(shape) - 1)), 1).expand(*shape, 1))
        out, mats = res["rgb"], res["rgb_affine_mats"]
    (out * cot).sum().backward()
    f64 = _oracle(m.grids, xy, rgb, idx, cot, torch.float64)
    f32 = _oracle(m.grids, xy, rgb, idx, cot, torch.float32)
    errs = _report(f"{entry} {tag}", (out.detach(), mats, m.grids.grad, a.grad), f64, f32)
    assert all(v <= BAR for v in errs.values()), errs


@pytest.mark.parametrize("ndim", [2, 3, 4, 5])
def test_forward_matrices_and_their_gradients_against_float64(ndim):
    n, gshape = 4, (6, 5, 4)
    m = _module(_random_grids(n, gshape, seed=8))
    gen = torch.Generator(device=DEV).manual_seed(ndim)
    shape = {2: (300,), 3: (5, 70), 4: (3, 20, 31), 5: (n, 2, 9, 11)}[ndim]
    xy = torch.rand((*shape, 2), device=DEV, generator=gen)
    rgb = torch.rand((*shape, 3), device=DEV, generator=gen) * 1.2 - 0.1
    cot = torch.randn((*shape, 3, 4), device=DEV, generator=gen)
    idx = None if ndim == 5 else torch.randint(0, n, (shape[0],), device=DEV, generator=gen)
    a = rgb.clone().requires_grad_(True)
    mats = m(xy, a, idx)
    assert mats.shape == (*shape, 3, 4)
    (mats * cot).sum().backward()
    res = {}
    for dtype in (torch.float64, torch.float32):
        g = m.grids.detach().to(dtype).requires_grad_(True)
        c = rgb.detach().to(dtype).clone().requires_grad_(True)
        mm = ref_mats(g, xy.to(dtype), c, idx)
        (mm * cot.to(dtype)).sum().backward()
        res[dtype] = (mm.detach(), g.grad, c.grad)
    names = ("mats", "v_grids", "v_rgb")
    ours = {k: rel_l2(x, y) for k, x, y in zip(names, (mats.detach(), m.grids.grad, a.grad), res[torch.float64])}
    f32 = {k: rel_l2(x, y) for k, x, y in zip(names, res[torch.float32], res[torch.float64])}
    print(f"\n[forward {ndim}-D] ours vs float64: {ours} | torch float32 vs float64: {f32}")
    assert all(v <= BAR for v in ours.values()), ours


def test_identity_grid_returns_rgb_unchanged():
    from gscodec_studio_amd.bilagrid import BilateralGrid, slice_image

    m = BilateralGrid(3).to(DEV)
    rgb = torch.rand((2, 67, 91, 3), device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    out = slice_image(m, rgb, torch.tensor([2, 0], device=DEV))
    err = float((out.detach() - rgb).abs().max())
    print(f"\n[identity grid] max |out - rgb| = {err:.2e}")
    assert err <= 8 * torch.finfo(torch.float32).eps  # eight weights, each a rounded product of three factors, summed: <= 8 roundings of values <= 1


def test_slice_image_equals_slice_with_the_meshgrid():
    from gscodec_studio_amd.bilagrid import slice as bslice, slice_image

    C, H, Wd = 3, 135, 240
    m = _module(_random_grids(5, (16, 16, 8), seed=4))
    gen = torch.Generator(device=DEV).manual_seed(1)
    rgb = torch.rand((C, H, Wd, 3), device=DEV, generator=gen)
    cot = torch.randn((C, H, Wd, 3), device=DEV, generator=gen)
    ids = torch.tensor([4, 1, 2], device=DEV)
    gy, gx = torch.meshgrid((torch.arange(H, device=DEV) + 0.5) / H, (torch.arange(Wd, device=DEV) + 0.5) / Wd, indexing="ij")
    grid_xy = torch.stack([gx, gy], dim=-1).unsqueeze(0)  # the trainer's [1, H, W, 2]: broadcast over the batch (extension)
    res = []
    for implicit in (True, False):
        a = rgb.clone().requires_grad_(True)
        m.grids.grad = None
        out = slice_image(m, a, ids) if implicit else bslice(m, grid_xy, a, ids)["rgb"]
        (out * cot).sum().backward()
        res.append((out.detach(), m.grids.grad.clone(), a.grad))
    errs = [rel_l2(x, y.double()) for x, y in zip(*res)]
    print(f"\n[slice_image vs slice + meshgrid] rgb {errs[0]:.2e} v_grids {errs[1]:.2e} v_rgb {errs[2]:.2e}")
    assert all(e <= BAR for e in errs), errs


def test_strided_render_view_is_bit_identical_to_its_copy():
    from gscodec_studio_amd.bilagrid import slice_image

    m = _module(_random_grids(2, (16, 16, 8), seed=5))
    gen = torch.Generator(device=DEV).manual_seed(2)
    renders = torch.rand((2, 120, 200, 4), device=DEV, generator=gen)  # RGB + D
    cot = torch.randn((2, 120, 200, 3), device=DEV, generator=gen)
    ids = torch.tensor([1, 0], device=DEV)
    res = []
    for view in (True, False):
        r = renders.clone().requires_grad_(True)
        colors = r[..., 0:3] if view else r[..., 0:3].contiguous()
        assert colors.is_contiguous() != view
        out = slice_image(m, colors, ids)
        (out * cot).sum().backward()
        res.append((out.detach(), r.grad))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))
    assert not res[0][1][..., 3].any()


@pytest.mark.parametrize("key", GRID_KEYS)
def test_total_variation_against_the_reference_fixture(key):
    from gscodec_studio_amd.bilagrid import total_variation_loss

    fx, grids = golden()
    x = torch.tensor(grids[key], device=DEV, requires_grad=True)
    tv = total_variation_loss(x)
    assert tv.dim() == 0 and tv.dtype == torch.float32 and tv.is_cuda
    (3.0 * tv).backward()
    grad = (x.grad[2, 0:1] if key == "big" else x.grad) / 3.0
    rv = abs(float(tv) - float(fx[f"tv.{key}"])) / abs(float(fx[f"tv.{key}"]))
    rg = rel_l2(grad, fx[f"tv.{key}.grad"])
    print(f"\n[tv fixture {key}] value rel {rv:.2e} grad relL2 {rg:.2e}")
    assert rv <= BAR and rg <= BAR


@pytest.mark.parametrize("shape", [(200, 12, 8, 16, 16), (3, 12, 3, 4, 5), (2, 5, 1, 7, 1), (1, 12, 8, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_total_variation_against_float64(shape):
    from gscodec_studio_amd.bilagrid import BilateralGrid, total_variation_loss

    x = torch.randn(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(shape[0]))
    res = {}
    for dtype in (torch.float64, torch.float32):
        t = x.detach().to(dtype).clone().requires_grad_(True)
        v = ref_tv(t)
        v.backward()
        res[dtype] = (float(v), t.grad)
    a = x.detach().clone().requires_grad_(True)
    tv = total_variation_loss(a)
    tv.backward()
    v64, g64 = res[torch.float64]
    ours = (abs(float(tv) - v64) / abs(v64), rel_l2(a.grad, g64))
    f32 = (abs(res[torch.float32][0] - v64) / abs(v64), rel_l2(res[torch.float32][1], g64))
    print(f"\n[tv {shape}] ours vs float64: value {ours[0]:.2e} grad {ours[1]:.2e} | torch float32: value {f32[0]:.2e} grad {f32[1]:.2e}")
    assert ours[0] <= BAR and ours[1] <= BAR
    if shape[0] == 200:  # the module's method, and run-to-run bit-identity
        m = BilateralGrid(200).to(DEV)
        with torch.no_grad():
            m.grids.copy_(x)
        assert torch.equal(m.tv_loss().detach().view(torch.int32), tv.detach().view(torch.int32))


def test_bilagrid_does_not_synchronise():
    from gscodec_studio_amd.bilagrid import slice as bslice, slice_image, total_variation_loss
    from gscodec_studio_amd.losses import photometric_loss

    gen = torch.Generator(device=DEV).manual_seed(9)
    m = _module(_random_grids(6, (16, 16, 8), seed=6))
    colors = torch.rand((2, 256, 384, 3), device=DEV, generator=gen).requires_grad_(True)
    pixels = torch.rand((2, 256, 384, 3), device=DEV, generator=gen)
    ids = torch.tensor([5, 2], device=DEV)
    xy = torch.rand((2, 500, 2), device=DEV, generator=gen)
    rays = torch.rand((2, 500, 3), device=DEV, generator=gen)

    def step():
        corrected = slice_image(m, colors, ids)
        photometric_loss(corrected, pixels)[0].backward()
        (10 * total_variation_loss(m.grids)).backward()
        bslice(m, xy, rays, ids)["rgb"].sum().backward()

    step()  # first call: allocations outside the checked window
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(colors.grad).all() and torch.isfinite(m.grids.grad).all()


def test_trainer_loop_with_the_grid_against_the_torch_composition():
    from gscodec_studio_amd import rasterization
    from gscodec_studio_amd.bilagrid import BilateralGrid, slice_image, total_variation_loss
    from gscodec_studio_amd.losses import photometric_loss
    from gscodec_studio_amd.optimizers import step_all

    init, cams = _trainer_scene()
    with torch.no_grad():
        ps0 = {k: v.clone() for k, v in init.items()}
        ps0["sh0"] += 0.3 * torch.randn(ps0["sh0"].shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
        pixels = rasterization(ps0["means"], ps0["quats"], torch.exp(ps0["scales"]), torch.sigmoid(ps0["opacities"]),
                               torch.cat([ps0["sh0"], ps0["shN"]], 1), cams["viewmats"], cams["Ks"], cams["W"], cams["H"],
                               sh_degree=3)[0].clamp(0, 1)
        pixels = (pixels * torch.tensor([0.9, 1.05, 0.8], device=DEV) + 0.03).clamp(0, 1)  # an exposure the grid can absorb
    H, Wd = cams["H"], cams["W"]
    image_ids = torch.tensor([1], device=DEV)
    gy, gx = torch.meshgrid((torch.arange(H, device=DEV) + 0.5) / H, (torch.arange(Wd, device=DEV) + 0.5) / Wd, indexing="ij")
    grid_xy = torch.stack([gx, gy], dim=-1).unsqueeze(0)
    finals = []
    for fused in (False, True):
        ps = {k: torch.nn.Parameter(v.clone()) for k, v in init.items()}
        opts = {k: torch.optim.Adam([{"params": [p], "lr": LRS[k], "name": k}], eps=1e-15, betas=(0.9, 0.999)) for k, p in ps.items()}
        bil = BilateralGrid(3).to(DEV)
        bil_opt = torch.optim.Adam(bil.parameters(), lr=2e-3, eps=1e-15)
        for _ in range(5):
            colors, _, _ = rasterization(ps["means"], ps["quats"], torch.exp(ps["scales"]), torch.sigmoid(ps["opacities"]),
                                         torch.cat([ps["sh0"], ps["shN"]], 1), cams["viewmats"], cams["Ks"], cams["W"], cams["H"],
                                         sh_degree=3, deterministic=True)
            if fused:
                colors = slice_image(bil, colors, image_ids)
                tv = total_variation_loss(bil.grids)
            else:
                colors = ref_slice(bil.grids, grid_xy, colors, image_ids)[0]
                tv = ref_tv(bil.grids)
            loss = photometric_loss(colors, pixels, ssim_lambda=0.2)[0] + 10 * tv
            loss.backward()
            step_all(opts)
            bil_opt.step()
            bil_opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        finals.append({**{k: p.detach().clone() for k, p in ps.items()}, "grids": bil.grids.detach().clone()})
    eye = BilateralGrid(3).grids.detach().to(DEV)
    for k in finals[0]:
        start = eye if k == "grids" else init[k]
        moved = float((finals[0][k] - start).norm())
        rel = float((finals[1][k] - finals[0][k]).norm() / finals[0][k].norm())
        print(f"\n[trainer loop + grid] {k}: relL2 {rel:.2e} (moved {moved:.3e})")
        assert moved > 0 and rel <= 1e-4, (k, rel)
