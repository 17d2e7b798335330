"""tests/projection_chain.py's hand-written glue against central differences of its own float64 forward (CPU only).

``O.projection_bwd`` and ``O.sh_bwd`` are pinned by tests/test_oracle_golden.py and ``UO.temporal_slice`` by tests/golden/dynamic.npz; what
this file holds is what the chain adds around them: the opacity x compensation product rule, the per-camera sums, the SH clamp gate, the
view-direction gradient added to ``v_means``, exp / sigmoid in front of the slice and the detached ``t - trbf_center`` inside it.

The bar calibrates itself: with central differences at step h and h / 2 the truncation error of FD(h / 2) is a third of
|FD(h) - FD(h / 2)|, so every entry must satisfy |chain - FD(h / 2)| <= 4 |FD(h) - FD(h / 2)| + 1e-9 max|chain|."""
import numpy as np
import pytest

from projection_chain import chain

W, H = 96, 80


def _scene(sh, sliced, seed=0):
    rs = np.random.RandomState(seed)
    n = 8
    P = dict(means=(rs.randn(n, 3) * np.array([0.5, 0.4, 0.4])), quats=rs.randn(n, 4),
             scales=np.exp(rs.uniform(np.log(0.05), np.log(0.3), (n, 3))), opacities=rs.uniform(0.2, 0.9, n))
    if sh:
        P["sh"] = rs.randn(n, 9, 3) * 1.5
    else:
        P["colors"] = rs.rand(n, 3)
    dyn = None
    if sliced:
        # raw log-scales, opacity logits and log trbf_scale: the activations go in front of the slice
        P["scales"], P["opacities"] = np.log(P["scales"]), np.log(P["opacities"] / (1 - P["opacities"]))
        P.update(motion=0.05 * rs.randn(n, 9), omega=0.2 * rs.randn(n, 4), trbf_center=rs.uniform(0, 1, (n, 1)),
                 trbf_scale=rs.uniform(-1.0, 0.3, (n, 1)))
        dyn = dict(t=0.37, raw=("scales", "opacities", "trbf_scale"))
    vm = np.tile(np.eye(4), (2, 1, 1))
    for c, a in enumerate((0.25, -0.3)):
        vm[c, :3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        vm[c, :3, 3] = (0.1 * c, -0.05, 4.0 + 0.5 * c)
    Ks = np.tile(np.array([[90.0, 0, W / 2], [0, 85.0, H / 2], [0, 0, 1]]), (2, 1, 1))
    return P, vm, Ks, dyn


@pytest.mark.parametrize("sliced", [False, True], ids=["static", "sliced"])
@pytest.mark.parametrize("sh", [False, True], ids=["colors", "sh2"])
@pytest.mark.parametrize("antialiased", [False, True], ids=["classic", "antialiased"])
def test_chain_gradients_equal_central_differences(antialiased, sh, sliced):
    P, vm, Ks, dyn = _scene(sh, sliced)
    kw = dict(antialiased=antialiased, sh_degree=2 if sh else None, dynamic=dyn)
    out, _ = chain(64, P, vm, Ks, W, H, **kw)
    vis = out["radii"] > 0
    assert vis.all(), "every splat in view of both cameras: no radius decision near the evaluation point"
    if sh:  # some colours clamped, some not, none near the gate
        v = out["sh_raw"] + 0.5
        assert (v < 0).any() and (v > 0).any() and np.abs(v).min() > 1e-2
    rs = np.random.RandomState(7)
    names = ("means2d", "depths", "conics", "opacities", "colors")
    cot = {k: rs.randn(*out[k].shape) for k in names}
    _, grads = chain(64, P, vm, Ks, W, H, cot=cot, vis=vis, **kw)

    if antialiased:
        c0 = out["compensations"]
        o0, w = out["opacities"] / c0, c0 / (c0 + 1e-6)

    def loss(Q):
        o, _ = chain(64, Q, vm, Ks, W, H, **kw)
        assert np.array_equal(o["radii"] > 0, vis)
        if antialiased:
            # the reference's compensation VJP divides by (compensation + 1e-6) where the derivative divides by the compensation
            # (its utils.cuh add_blur_vjp; oracle/gs_oracle.c restates it and so do the kernels): it is w = c / (c + 1e-6) times the
            # derivative, 1e-6 away from it, which central differences resolve.  So the opacity x compensation product is differenced
            # in the form whose exact derivative at this point that VJP is: d(o c) = c0 do + w o0 dc
            o["opacities"] = o["opacities"] / o["compensations"] * c0 + w * o0 * o["compensations"]
        return sum(float((cot[k] * o[k]).sum()) for k in names)

    def fd(key, idx, h):
        lo, hi = {k: np.array(v, np.float64) for k, v in P.items()}, {k: np.array(v, np.float64) for k, v in P.items()}
        lo[key][idx] -= h
        hi[key][idx] += h
        if key == "trbf_center":  # the slice moves the splat by a DETACHED t - trbf_center
            lo["_motion_center"] = hi["_motion_center"] = P["trbf_center"]
        return (loss(hi) - loss(lo)) / (2 * h)

    h = 1e-3
    for key, g in grads.items():
        assert np.abs(g).max() > 0, key
        for idx in np.ndindex(*g.shape):
            d1, d2 = fd(key, idx, h), fd(key, idx, h / 2)
            assert abs(g[idx] - d2) <= 4 * abs(d1 - d2) + 1e-9 * np.abs(g).max(), (key, idx, g[idx], d1, d2)


def test_chain_float32_run_is_close_to_its_float64_run():
    """The fp32 evaluation of the chain (the yardstick of the GPU test) is the same function: a few 1e-6 from float64 here."""
    P, vm, Ks, dyn = _scene(True, False)
    P = {k: v.astype(np.float32) for k, v in P.items()}
    rs = np.random.RandomState(1)
    o64, _ = chain(64, P, vm, Ks, W, H, antialiased=True, sh_degree=2)
    cot = {k: rs.randn(*o64[k].shape).astype(np.float32) for k in ("means2d", "depths", "conics", "opacities", "colors")}
    vis = o64["radii"] > 0
    _, g64 = chain(64, P, vm, Ks, W, H, antialiased=True, sh_degree=2, cot=cot, vis=vis)
    o32, g32 = chain(32, P, vm, Ks, W, H, antialiased=True, sh_degree=2, cot=cot, vis=vis)
    assert np.array_equal(o32["radii"], o64["radii"])
    for k in g64:
        assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64
        assert np.linalg.norm(g32[k] - g64[k]) <= 1e-4 * np.linalg.norm(g64[k]), k


@pytest.mark.parametrize("sh", [False, True], ids=["colors", "sh2"])
def test_chain_pose_gradient_equals_central_differences(sh):
    """``v_viewmats``: the projection's own, and with SH colours the view direction's dependence on the camera centre on top of it."""
    P, vm, Ks, _ = _scene(sh, False)
    kw = dict(sh_degree=2 if sh else None, need_viewmats=True)
    out, _ = chain(64, P, vm, Ks, W, H, **kw)
    vis = out["radii"] > 0
    assert vis.all()
    rs = np.random.RandomState(11)
    names = ("means2d", "depths", "conics", "opacities", "colors")
    cot = {k: rs.randn(*out[k].shape) for k in names}
    _, grads = chain(64, P, vm, Ks, W, H, cot=cot, vis=vis, **kw)
    g = grads["viewmats"]
    assert g.shape == vm.shape and not g[:, 3].any(), "the bottom row of a world-to-camera matrix is constant"
    if sh:  # the centre term is there: the colours' cotangent alone reaches the pose
        _, only = chain(64, P, vm, Ks, W, H, cot={"colors": cot["colors"]}, vis=vis, **kw)
        assert np.abs(only["viewmats"]).max() > 1e-3 * np.abs(g).max()

    def fd(idx, h):
        lo, hi = vm.copy(), vm.copy()
        lo[idx] -= h
        hi[idx] += h
        val = []
        for m in (hi, lo):
            o, _ = chain(64, P, m, Ks, W, H, **kw)
            assert np.array_equal(o["radii"] > 0, vis)
            val.append(sum(float((cot[k] * o[k]).sum()) for k in names))
        return (val[0] - val[1]) / (2 * h)

    h = 1e-3
    for idx in np.ndindex(vm.shape[0], 3, 4):
        d1, d2 = fd(idx, h), fd(idx, h / 2)
        assert abs(g[idx] - d2) <= 4 * abs(d1 - d2) + 1e-9 * np.abs(g).max(), (idx, g[idx], d1, d2)
