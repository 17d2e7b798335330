"""gscodec_studio_amd.bilagrid without a GPU: the module imports and exports its names, the four entry points are part of the C ABI
and refuse null pointers and bad shapes before any launch, every input outside the contract is refused with a ValueError that
names the problem, BilateralGrid initialises to the identity and round-trips its state_dict, and the float64 torch restatement
kept here (F.grid_sample + the affine product, and the TV formula) reproduces tests/golden/bilagrid.npz -- the reference's own
output -- on the CPU.  The GPU tests use that restatement as their oracle."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bilagrid.npz")
CASES = ("image", "image_odd", "views", "chunks", "rays", "rays_big", "rays_one")
GRID_KEYS = ("big", "odd", "flat")


# ------------------------------------------------------------------------------------------------ the restatement (any dtype)
def grids_of(seed, shape, num=3):
    """The fixture's non-identity grids (num, 12, L, H, W) for shape = (grid_X, grid_Y, grid_W): numpy's legacy MT19937 stream."""
    X, Y, L = (int(v) for v in shape)
    eye = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64).reshape(1, 12, 1, 1, 1)
    return (eye + 0.3 * np.random.RandomState(int(seed)).standard_normal((num, 12, L, Y, X))).astype(np.float32)


def ref_mats(grids, xy, rgb, idx):
    """(..., 3, 4) matrices sliced from grids[idx[b]] for (B, ..., 2) xy and (B, ..., 3) rgb in grids' dtype; idx (B,) or None."""
    nd = rgb.dim()
    xy = xy.expand(*rgb.shape[:-1], 2)
    for _ in range(5 - nd):
        xy, rgb = xy.unsqueeze(1), rgb.unsqueeze(1)
    g = grids if idx is None else grids[idx]
    wgt = torch.tensor([0.299, 0.587, 0.114], dtype=grids.dtype, device=grids.device)
    z = (rgb * wgt).sum(-1, keepdim=True) * 2.0 - 1.0
    xyz = torch.cat([(xy - 0.5) * 2.0, z], dim=-1)
    m = F.grid_sample(g, xyz, mode="bilinear", align_corners=True, padding_mode="border").permute(0, 2, 3, 4, 1)
    m = m.reshape(*m.shape[:-1], 3, 4)
    for _ in range(5 - nd):
        m = m.squeeze(1)
    return m


def ref_slice(grids, xy, rgb, idx):
    """(rgb_out, matrices) of the restatement."""
    m = ref_mats(grids, xy, rgb, idx)
    return (m[..., :3] @ rgb.unsqueeze(-1)).squeeze(-1) + m[..., 3], m


def ref_tv(x):
    tv = 0
    for ax in (2, 3, 4):
        n = x.shape[ax]
        if n < 2:
            continue
        d = x.narrow(ax, 1, n - 1) - x.narrow(ax, 0, n - 1)
        tv = tv + (d * d).sum() / max(d[0].numel(), 1)
    return tv / x.shape[0]


def rel_l2(got, want):
    want = torch.as_tensor(want, dtype=torch.float64)
    return float((torch.as_tensor(got).double().cpu() - want.cpu()).norm() / want.norm().clamp_min(1e-300))


def golden():
    fx = dict(np.load(GOLDEN))
    grids = {k: grids_of(fx["seeds"][i], fx["shapes"][i]) for i, k in enumerate(GRID_KEYS)}
    return fx, grids


# ------------------------------------------------------------------------------------------------------------------- tests
def test_module_imports_and_exports():
    from gscodec_studio_amd import bilagrid

    assert set(bilagrid.__all__) == {"BilateralGrid", "slice", "slice_image", "total_variation_loss", "color_affine_transform"}
    for name in bilagrid.__all__:
        assert callable(getattr(bilagrid, name)), name
    for word in ("color_correct", "BilateralGridCP4D", "slice4d", "Out of scope", "Extensions"):
        assert word in bilagrid.__doc__, word


def test_entry_points_are_declared_exported_and_refuse_before_launch():
    from gscodec_studio_amd import _backend as B

    protos = B.prototypes()
    hdr = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    for name in ("gs_bilagrid_slice_fwd", "gs_bilagrid_slice_bwd", "gs_bilagrid_tv_fwd", "gs_bilagrid_tv_bwd"):
        assert name in protos and name + "(" in hdr, name
        assert hasattr(B.lib(), name), name
    assert B.header_abi_version() == 6
    st = (ctypes.c_int64 * 4)(0, 0, 3, 1)
    sp = ctypes.addressof(st)
    with pytest.raises(RuntimeError, match="null pointer"):
        B.call("gs_bilagrid_slice_fwd", None, 1, 8, 16, 16, 1, 1, 4, None, None, None, sp, None, 0, None, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):  # no output
        B.call("gs_bilagrid_slice_fwd", 64, 1, 8, 16, 16, 1, 1, 4, None, None, 64, sp, None, 0, None, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):  # xy without its strides
        B.call("gs_bilagrid_slice_fwd", 64, 1, 8, 16, 16, 1, 1, 4, 64, None, 64, sp, None, 0, 64, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        B.call("gs_bilagrid_slice_bwd", None, 1, 8, 16, 16, 1, 1, 4, None, None, None, sp, None, 0, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):  # no upstream gradient
        B.call("gs_bilagrid_slice_bwd", 64, 1, 8, 16, 16, 1, 1, 4, None, None, 64, sp, None, 0, None, None, 64, 64, None)
    # bad shapes, with fake (never dereferenced) non-null pointers
    with pytest.raises(RuntimeError, match="empty grid"):
        B.call("gs_bilagrid_slice_fwd", 64, 1, 0, 16, 16, 1, 1, 4, None, None, 64, sp, None, 0, 64, None, None)
    with pytest.raises(RuntimeError, match="empty point"):
        B.call("gs_bilagrid_slice_bwd", 64, 1, 8, 16, 16, 1, 0, 4, None, None, 64, sp, None, 0, 64, None, 64, 64, None)
    with pytest.raises(RuntimeError, match="2\\^31"):
        B.call("gs_bilagrid_slice_fwd", 64, 1, 8, 16, 16, 4, 65536, 32768, None, None, 64, sp, None, 0, 64, None, None)
    with pytest.raises(RuntimeError, match="2\\^31"):
        B.call("gs_bilagrid_slice_fwd", 64, 1, 1024, 1024, 1024, 1, 1, 4, None, None, 64, sp, None, 0, 64, None, None)
    with pytest.raises(RuntimeError, match="aligned"):
        B.call("gs_bilagrid_slice_fwd", 64, 1, 8, 16, 16, 1, 1, 4, None, None, 64, sp, None, 0, None, 68, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        B.call("gs_bilagrid_tv_fwd", None, 1, 12, 8, 16, 16, None, 0, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        B.call("gs_bilagrid_tv_bwd", None, 1, 12, 8, 16, 16, None, None, None)
    with pytest.raises(RuntimeError, match="empty shape"):
        B.call("gs_bilagrid_tv_fwd", 64, 1, 12, 0, 16, 16, 64, 1 << 20, 64, None)
    with pytest.raises(RuntimeError, match="2\\^31"):
        B.call("gs_bilagrid_tv_bwd", 64, 4096, 12, 64, 64, 64, 64, 64, None)
    with pytest.raises(RuntimeError, match="work area"):
        B.call("gs_bilagrid_tv_fwd", 64, 1, 12, 8, 16, 16, 64, 8, 64, None)
    assert int(B.query("gs_bilagrid_tv_work_bytes")) >= 8


def _grid(n=2):
    from gscodec_studio_amd.bilagrid import BilateralGrid

    return BilateralGrid(n)


def test_slice_refuses():
    from gscodec_studio_amd.bilagrid import slice as bslice

    m = _grid()
    xy, rgb, idx = torch.zeros(4, 2), torch.zeros(4, 3), torch.zeros(4, 1, dtype=torch.int64)
    with pytest.raises(ValueError, match="no CPU path"):
        bslice(m, xy, rgb, idx)
    with pytest.raises(ValueError, match="float32"):
        bslice(m, xy, rgb.double(), idx)
    with pytest.raises(ValueError, match="float32"):
        bslice(m, xy.half(), rgb, idx)
    with pytest.raises(ValueError, match="1-D"):
        bslice(m, torch.zeros(2), torch.zeros(3), idx)
    with pytest.raises(ValueError, match="5-D"):
        bslice(m, torch.zeros(2, 1, 2, 2, 2), torch.zeros(2, 1, 2, 2, 3), idx)
    with pytest.raises(ValueError, match="last dimension of xy"):
        bslice(m, torch.zeros(4, 3), rgb, idx)
    with pytest.raises(ValueError, match="last dimension of rgb"):
        bslice(m, xy, torch.zeros(4, 4), idx)
    with pytest.raises(ValueError, match="does not match"):
        bslice(m, torch.zeros(5, 2), rgb, idx)
    with pytest.raises(ValueError, match="requires a gradient"):
        bslice(m, xy.clone().requires_grad_(True), rgb, idx)
    with pytest.raises(ValueError, match="integer"):
        bslice(m, xy, rgb, idx.float())
    with pytest.raises(ValueError, match="grid_idx must be"):
        bslice(m, xy, rgb, torch.zeros(3, 1, dtype=torch.int64))
    m.grids.data = m.grids.data.double()
    with pytest.raises(ValueError, match="grids must be float32"):
        bslice(m, xy, rgb, idx)


def test_slice_image_forward_and_tv_refuse():
    from gscodec_studio_amd.bilagrid import slice_image, total_variation_loss

    m = _grid()
    img, ids = torch.zeros(2, 8, 8, 3), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="no CPU path"):
        slice_image(m, img, ids)
    with pytest.raises(ValueError, match="float32"):
        slice_image(m, img.double(), ids)
    with pytest.raises(ValueError, match="4-D"):
        slice_image(m, img[0], ids)
    with pytest.raises(ValueError, match="4-D"):
        slice_image(m, torch.zeros(2, 8, 8, 4), ids)
    with pytest.raises(ValueError, match="one index per image"):
        slice_image(m, img, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="no CPU path"):
        m(torch.zeros(4, 2), torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="idx is required"):
        m(torch.zeros(4, 2), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="1-D"):
        m(torch.zeros(2), torch.zeros(3), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="one entry per grid"):
        m(torch.zeros(3, 1, 2, 2, 2), torch.zeros(3, 1, 2, 2, 3))
    with pytest.raises(ValueError, match="no CPU path"):
        total_variation_loss(m.grids)
    with pytest.raises(ValueError, match="no CPU path"):
        m.tv_loss()
    with pytest.raises(ValueError, match="float32"):
        total_variation_loss(m.grids.double())
    with pytest.raises(ValueError, match="5-D"):
        total_variation_loss(m.grids[0])
    with pytest.raises(ValueError, match="tensor"):
        total_variation_loss([1.0])


def test_bilateral_grid_identity_attributes_and_state_dict():
    from gscodec_studio_amd.bilagrid import BilateralGrid, color_affine_transform

    m = BilateralGrid(3, grid_X=5, grid_Y=4, grid_W=3)
    assert (m.grid_width, m.grid_height, m.grid_guidance) == (5, 4, 3)
    assert isinstance(m.grids, torch.nn.Parameter) and m.grids.shape == (3, 12, 3, 4, 5) and m.grids.dtype == torch.float32
    assert m.grids.is_contiguous()
    eye = torch.eye(3, 4).reshape(12)
    assert torch.equal(m.grids.detach().permute(0, 2, 3, 4, 1), eye.expand(3, 3, 4, 5, 12))
    assert torch.equal(m.rgb2gray_weight, torch.tensor([[0.299, 0.587, 0.114]]))
    sd = m.state_dict()
    assert set(sd) == {"grids", "rgb2gray_weight"}  # the reference's keys
    assert BilateralGrid(1).grids.shape == (1, 12, 8, 16, 16)
    other = BilateralGrid(3, 5, 4, 3)
    with torch.no_grad():
        m.grids.add_(torch.randn(m.grids.shape, generator=torch.Generator().manual_seed(0)))
    other.load_state_dict(m.state_dict())
    assert torch.equal(other.grids, m.grids)
    # the identity matrices leave colours alone; color_affine_transform is the reference's two lines
    rgb = torch.rand(7, 3, generator=torch.Generator().manual_seed(1))
    mats = eye.reshape(3, 4).expand(7, 3, 4)
    assert torch.equal(color_affine_transform(mats, rgb), rgb)
    mats = torch.rand(7, 3, 4, generator=torch.Generator().manual_seed(2))
    want = torch.stack([mats[i, :, :3] @ rgb[i] + mats[i, :, 3] for i in range(7)])
    torch.testing.assert_close(color_affine_transform(mats, rgb), want)


def test_fixture_is_small_and_its_grids_regenerate():
    fx, grids = golden()
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert np.array_equal(grids["odd"], fx["grids_odd"]) and np.array_equal(grids["flat"], fx["grids_flat"])
    assert float(grids["big"].astype(np.float64).sum()) == float(fx["grids_big_sum"])
    assert not np.allclose(grids["big"][0, :, 0, 0, 0], np.eye(3, 4).reshape(12))  # non-identity


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference(case):
    """The reference ran in float32 on the CPU; the float64 restatement must agree with it to float32 rounding (1e-5 relative L2,
    an order below the 1e-4 the GPU tests hold the kernels to)."""
    fx, grids = golden()
    g = torch.tensor(grids[str(fx[f"{case}.grids"])], dtype=torch.float64, requires_grad=True)
    xy = torch.tensor(fx[f"{case}.xy"], dtype=torch.float64)
    rgb = torch.tensor(fx[f"{case}.rgb"], dtype=torch.float64, requires_grad=True)
    idx = torch.tensor(fx[f"{case}.idx"]).reshape(rgb.shape[0], -1)[:, 0]
    out, mats = ref_slice(g, xy, rgb, idx)
    (out * torch.tensor(fx[f"{case}.cot"], dtype=torch.float64)).sum().backward()
    errs = {"rgb": rel_l2(out.detach(), fx[f"{case}.out_rgb"]), "mats": rel_l2(mats.detach(), fx[f"{case}.out_mats"]),
            "v_rgb": rel_l2(rgb.grad, fx[f"{case}.v_rgb"])}
    vg = g.grad
    if f"{case}.v_grids" in fx:
        errs["v_grids"] = rel_l2(vg, fx[f"{case}.v_grids"])
    elif f"{case}.v_grids_1" in fx:
        assert bool(fx[f"{case}.v_grids_others_zero"]) and not vg[0].any() and not vg[2].any()
        errs["v_grids"] = rel_l2(vg[1], fx[f"{case}.v_grids_1"])
    else:
        nz = torch.tensor(fx[f"{case}.v_grids_nz_index"].astype(np.int64))
        errs["v_grids"] = rel_l2(vg.reshape(-1)[nz], fx[f"{case}.v_grids_nz_value"])
        rest = vg.reshape(-1).clone()
        rest[nz] = 0
        assert float(rest.abs().max()) <= 1e-6 * float(vg.abs().max())
    print(f"\n[restatement vs reference, {case}] " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= 1e-5 for v in errs.values()), errs


@pytest.mark.parametrize("key", GRID_KEYS)
def test_float64_tv_restatement_reproduces_the_reference(key):
    fx, grids = golden()
    x = torch.tensor(grids[key], dtype=torch.float64, requires_grad=True)
    tv = ref_tv(x)
    tv.backward()
    grad = x.grad[2, 0:1] if key == "big" else x.grad
    rv, rg = abs(float(tv.detach()) - float(fx[f"tv.{key}"])) / abs(float(fx[f"tv.{key}"])), rel_l2(grad, fx[f"tv.{key}.grad"])
    print(f"\n[tv restatement vs reference, {key}] value {rv:.2e} grad {rg:.2e}")
    assert rv <= 1e-5 and rg <= 1e-5
    if key == "flat":
        assert x.shape[3] == 1  # the axis of size 1 contributes nothing
