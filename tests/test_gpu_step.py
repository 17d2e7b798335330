"""The native step driver (gs_step_fwd_begin / gs_step_fwd_finish behind rasterization()'s fast path, _step.py) against the
operator path it bundles: the same launches through the same entry points, so images, every meta tensor and every gradient
must be IDENTICAL (gradients up to the order of the float atomics of the compositing backward, which is not fixed between
two runs of either path), over the call shapes the fast path accepts."""
import numpy as np
import pytest
import torch

from util import N, T, garden, garden_sh

pytestmark = pytest.mark.gpu


def _run(fast, kind, C=1, absgrad=False, backgrounds=False, antialiased=False, tile_size=16, covars=False, n=3000, dense_grad=False,
         need=("means", "quats", "scales", "opacities", "colors")):
    from gscodec_studio_amd import _step, rasterization

    g = garden(n, scale_mult=4.0)
    sh = garden_sh(g["rgb"])
    P = {"means": T(g["means"]), "quats": T(g["quats"]), "scales": T(g["scales"]), "opacities": T(g["opacities"])}
    if kind == "sh":
        P["colors"] = T(sh)
    elif kind == "split":
        P["colors"], P["shN"] = T(sh[:, :1]), T(sh[:, 1:])
    else:
        P["colors"] = T(g["rgb"])
    for k in P:
        P[k].requires_grad_(k in need or (k == "shN" and "colors" in need))
    cov = None
    if covars:
        from gscodec_studio_amd import _wrapper as W

        c6, _ = W.quat_scale_to_covar_preci(P["quats"].detach(), P["scales"].detach(), compute_preci=False, triu=False)
        cov = c6.detach().requires_grad_(True)
    colors = (P["colors"], P["shN"]) if kind == "split" else P["colors"]
    bg = torch.tensor([[0.1, 0.5, 0.9]] * C, device="cuda:0", requires_grad=True) if backgrounds else None
    prev = _step.ENABLED
    _step.ENABLED = fast
    try:
        rc, ra, meta = rasterization(P["means"], P["quats"], P["scales"], P["opacities"], colors, T(g["viewmats"][:C]), T(g["Ks"][:C]),
                                     g["width"], g["height"], sh_degree=None if kind == "rgb" else 3, packed=False, absgrad=absgrad,
                                     backgrounds=bg, rasterize_mode="antialiased" if antialiased else "classic", tile_size=tile_size,
                                     covars=cov)
    finally:
        _step.ENABLED = prev
    meta["means2d"].retain_grad()
    if dense_grad:
        gen = torch.Generator(device="cuda:0").manual_seed(1)
        (rc * torch.rand(rc.shape, device="cuda:0", generator=gen)).sum().backward()
    else:
        (rc.sum() + 0.5 * ra.sum()).backward()
    grads = {k: p.grad for k, p in P.items() if p.requires_grad}
    if cov is not None:
        grads["covars"] = cov.grad
    if bg is not None:
        grads["backgrounds"] = bg.grad
    grads["means2d"] = meta["means2d"].grad
    if absgrad:
        grads["absgrad"] = meta["means2d"].absgrad
    return rc.detach(), ra.detach(), meta, grads


CASES = [dict(kind="sh"), dict(kind="split"), dict(kind="rgb"), dict(kind="sh", C=3, absgrad=True, backgrounds=True),
         dict(kind="rgb", C=2, antialiased=True, tile_size=8), dict(kind="sh", covars=True), dict(kind="sh", dense_grad=True),
         dict(kind="split", need=("means", "colors")), dict(kind="sh", need=("opacities",)), dict(kind="rgb", need=("quats", "scales"))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_step_driver_equals_operator_path(case):
    a = _run(True, **case)
    b = _run(False, **case)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    vis = b[2]["radii"] > 0
    for k in ("radii", "depths", "tiles_per_gauss", "isect_ids", "flatten_ids", "isect_offsets"):
        x, y = a[2][k], b[2][k]
        if k == "depths":
            x, y = x[vis], y[vis]
        assert torch.equal(x, y), k
    for k in ("means2d", "conics", "opacities"):
        assert torch.equal(a[2][k][vis], b[2][k][vis]), k
    assert {k: a[2][k] for k in ("tile_width", "tile_height", "width", "height", "tile_size", "n_cameras")} == \
        {k: b[2][k] for k in ("tile_width", "tile_height", "width", "height", "tile_size", "n_cameras")}
    assert set(a[3]) == set(b[3])
    for k in a[3]:
        x, y = a[3][k], b[3][k]
        assert (x is None) == (y is None), k
        if x is None:
            continue
        # (the float atomics of the compositing backward land in a different order every run, on either path: quaternion /
        #  scale gradients are differences of large conic terms and move in the 4th digit between two runs of the SAME path)
        den = float(y.norm()) + 1e-30
        assert float((x - y).norm()) <= 3e-4 * den, (k, float((x - y).norm()) / den)


def test_step_driver_second_backward_and_no_grad():
    from gscodec_studio_amd import rasterization

    g = garden(2000, scale_mult=4.0)
    ps = [T(g[k]).requires_grad_(True) for k in ("means", "quats", "scales", "opacities")] + [T(garden_sh(g["rgb"])).requires_grad_(True)]
    rc, ra, meta = rasterization(*ps, T(g["viewmats"][:1]), T(g["Ks"][:1]), g["width"], g["height"], sh_degree=3, packed=False)
    g1 = torch.autograd.grad(rc.sum(), ps, retain_graph=True)
    g2 = torch.autograd.grad(rc.sum(), ps)  # the prefilled buffer was consumed by the first backward: the generic route
    for x, y in zip(g1, g2):
        assert float((x - y).abs().max()) <= 2e-5 * float(x.abs().max())
    with torch.no_grad():
        rc2, ra2, _ = rasterization(*ps, T(g["viewmats"][:1]), T(g["Ks"][:1]), g["width"], g["height"], sh_degree=3, packed=False)
    assert torch.equal(rc2, rc.detach()) and torch.equal(ra2, ra.detach())


# ---------------------------------------------------------------------------------------------------------------------------
# The driver's intersection buffers across calls (_step._finish: allocated BEFORE the read-back for the capacity of the last call
# of the same shape, outputs as prefix views, exact allocations when the count outgrows the capacity) over counts on both sides
# of the pair sort's switch from 1024- to 4096-key blocks at 2^21 pairs.
REUSE_W, REUSE_H, REUSE_BIG, REUSE_FILL = 1920, 1088, 146_000, 4_000  # 120 x 68 tiles; N = 150 000
REUSE_COUNTS = (2_060_000, 2_060_000, 2_097_152, 2_097_153, 2_125_000, 2_600_000, 1_000, 0, 2_060_000)


def _reuse_scene():
    """One camera at the origin looking down +z.  REUSE_BIG isotropic splats of 24-44 pixels radius anywhere in the image (tens of
    tiles each), then REUSE_FILL splats of sub-pixel size at tile centres (radius 2 with the 0.3 blur: strictly inside one tile)."""
    rs = np.random.RandomState(7)
    f, cx, cy = 1000.0, REUSE_W / 2, REUSE_H / 2
    nb, nf = REUSE_BIG, REUSE_FILL
    u = np.concatenate([rs.uniform(40, REUSE_W - 40, nb), 16.0 * rs.randint(0, REUSE_W // 16, nf) + 8.0])
    v = np.concatenate([rs.uniform(40, REUSE_H - 40, nb), 16.0 * rs.randint(0, REUSE_H // 16, nf) + 8.0])
    z = np.concatenate([rs.uniform(2.0, 8.0, nb), rs.uniform(1.0, 1.5, nf)])
    r_px = np.concatenate([rs.uniform(24.0, 44.0, nb), np.full(nf, 0.9)])
    means = np.stack([(u - cx) * z / f, (v - cy) * z / f, z], -1).astype(np.float32)
    scales = np.repeat((r_px / 3.0 * z / f)[:, None], 3, 1).astype(np.float32)
    quats = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (nb + nf, 1))
    K = np.array([[[f, 0, cx], [0, f, cy], [0, 0, 1]]], np.float32)
    return dict(means=T(means), quats=T(quats), scales=T(scales), opacities=T(rs.uniform(0.2, 0.9, nb + nf).astype(np.float32)),
                colors=T(rs.rand(nb + nf, 3).astype(np.float32)), viewmats=T(np.eye(4, dtype=np.float32)[None]), Ks=T(K))


def _reuse_render(S, means, fast, packed_pairs=True):
    """-> (native entry points called, render_colors, render_alphas, meta), forward only"""
    from gscodec_studio_amd import _backend, _step, _wrapper, rasterization

    calls = []
    real_call = _backend.call

    def recording_call(name, *a, **kw):
        calls.append(name)
        return real_call(name, *a, **kw)

    saved = (_step.ENABLED, _wrapper._PACKED_PAIRS, _backend.call)
    try:
        _step.ENABLED, _wrapper._PACKED_PAIRS, _backend.call = fast, packed_pairs, recording_call
        with torch.no_grad():
            rc, ra, meta = rasterization(means, S["quats"], S["scales"], S["opacities"], S["colors"], S["viewmats"], S["Ks"], REUSE_W,
                                         REUSE_H, packed=False)
        torch.cuda.synchronize()
    finally:
        _step.ENABLED, _wrapper._PACKED_PAIRS, _backend.call = saved
    return calls, rc, ra, meta


def test_step_driver_buffer_reuse_across_the_sort_block_switch():
    """Renders of ONE call shape whose intersection counts are hit exactly (a splat's tile count does not depend on the others:
    a prefix of the big splats just below the target, single-tile fillers for the rest, everything else behind the camera), in
    the order: first allocation, the same count again (kept buffer sized for a capacity above 2^21, count below: the sort's temp
    layout is LARGER for the count than a decreasing size query made it for the capacity), both sides of the switch inside a kept
    buffer, growth beyond the capacity, a tiny prefix of a large buffer, an empty frame, the large count again.  Every render
    against the operator path (exact allocations) bit for bit, and at the switch against the CPU oracle's binning, which shares
    no sort with either."""
    from gscodec_studio_amd import _step
    from oracle import gs_oracle as O

    S = _reuse_scene()
    N_all = REUSE_BIG + REUSE_FILL
    th, tw = REUSE_H // 16, REUSE_W // 16
    # calibration through the operators: tiles per splat with every splat in view
    _, _, _, meta = _reuse_render(S, S["means"], fast=False)
    tpg = meta["tiles_per_gauss"].reshape(-1).to(torch.int64)
    big_cum = torch.cumsum(tpg[:REUSE_BIG], 0)
    fill_ok = torch.nonzero(tpg[REUSE_BIG:] == 1).reshape(-1) + REUSE_BIG
    assert int(big_cum[-1]) >= max(REUSE_COUNTS) and int(tpg[:REUSE_BIG].max()) <= fill_ok.numel(), "the scene cannot reach the targets"
    assert float(tpg[:REUSE_BIG].double().mean()) >= 10.0  # (big splats cover tens of tiles)
    hidden = S["means"] * torch.tensor([1.0, 1.0, -1.0], device=S["means"].device)  # behind the camera: radii 0, N unchanged

    def means_for(target):
        k = int(torch.searchsorted(big_cum, torch.tensor(target, device=big_cum.device), right=True))  # big splats [0, k): sum <= target
        rest = target - (int(big_cum[k - 1]) if k else 0)
        keep = torch.zeros(N_all, dtype=torch.bool, device=S["means"].device)
        keep[:k] = True
        keep[fill_ok[:rest]] = True
        return torch.where(keep[:, None], S["means"], hidden).contiguous()

    key = (S["means"].device.index, 1, N_all, th, tw)
    _step._ISECT_CAP.pop(key, None)
    try:
        cap = 0
        for step, target in enumerate(REUSE_COUNTS):
            means = means_for(target)
            _, rc0, ra0, m0 = _reuse_render(S, means, fast=False)
            assert m0["flatten_ids"].numel() == target, (step, target, m0["flatten_ids"].numel())
            for packed_pairs in ((True, False) if step == 1 else (True,)):  # (the failing window once through the (key, id) pairs too)
                assert _step._ISECT_CAP.get(key, 0) == cap
                calls, rc, ra, m = _reuse_render(S, means, fast=True, packed_pairs=packed_pairs)
                what = (step, target, cap, packed_pairs)
                assert calls.count("gs_step_fwd_begin") == 1 and calls.count("gs_step_fwd_finish") == 2, (what, calls)
                assert "gs_isect_finish_presorted" not in calls and "gs_rasterize_fwd" not in calls, (what, calls)
                assert m["flatten_ids"].numel() == target and m["isect_ids"].numel() == target, what
                # kept buffers hand out prefix views of the capacity; outgrown (or first) ones are exact
                held = cap if (cap and _step._cap_serves(cap, target)) else target
                assert m["isect_ids"].untyped_storage().nbytes() == 8 * held, what
                assert m["flatten_ids"].untyped_storage().nbytes() == 4 * held, what
                for k in ("isect_ids", "flatten_ids", "isect_offsets", "tiles_per_gauss", "radii"):
                    assert torch.equal(m[k], m0[k]), (what, k)
                assert torch.equal(rc, rc0) and torch.equal(ra, ra0), what
                cap = _step._next_cap(target)
            if target in (2_097_152, 2_097_153):
                o_tpg, o_ids, o_flat = O.isect_tiles(N(m["means2d"]), N(m["radii"]), N(m["depths"]), 16, tw, th)
                assert np.array_equal(N(m["tiles_per_gauss"]), o_tpg)
                assert np.array_equal(N(m["isect_ids"]), o_ids) and np.array_equal(N(m["flatten_ids"]), o_flat)
                assert np.array_equal(N(m["isect_offsets"]), O.isect_offset_encode(o_ids, 1, tw, th))
    finally:
        _step._ISECT_CAP.pop(key, None)
