"""Dense pure-torch restatement of the 2D Gaussian splatting operators (test helper, not product code).

It states the semantics of ``csrc/surfel.hip`` (include/gsplat_hip.h, "2D Gaussian splatting") in the plainest vectorised form:
the projection per (camera, splat), the compositing per tile list over all pixels of the tile at once, every gradient from
autograd.  It is dtype-generic: run in float64 it is the ground truth of tests/test_gpu_surfel.py, run in float32 on the CPU it
measures how far float32 arithmetic alone moves a gradient (the ``e32`` of that file's bar).

Discrete decisions are written so that autograd follows the branch the kernel takes: ``where`` instead of ``minimum`` (no split
gradient on ties), zero gradient where ``o exp(-sigma) > 0.999``.
"""
import math

import torch

ALPHA_MAX, ALPHA_MIN, T_MIN, NEAR = 0.999, 1.0 / 255.0, 1e-4, 1e-4
TILE = 16


def quat_to_rotmat(quats):
    q = quats / quats.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(*quats.shape[:-1], 3, 3)


def _rel_close(q, thr, scale=None):
    """|q - thr| within NEAR relative of the threshold (of ``scale`` where the threshold is zero)."""
    s = torch.as_tensor(thr, dtype=q.dtype).abs() if scale is None else scale
    return (q - thr).abs() <= NEAR * s


def project(means, quats, scales, viewmats, Ks, width, height, near_plane=0.01, far_plane=1e10, radius_clip=0.0):
    """-> dict: radii int32 [C,N], means2d [C,N,2], depths [C,N], ray_transforms [C,N,3,3], normals [C,N,3] (zeros where culled),
    ``radius_raw`` = 3 sqrt(max(1e-4, .)) before the ceil, and ``near_cull`` [C,N]: some culling quantity of the splat lies within
    1e-4 relative of its threshold."""
    C, N = viewmats.shape[0], means.shape[0]
    Rc, tc = viewmats[:, :3, :3], viewmats[:, :3, 3]
    p = torch.einsum("cij,nj->cni", Rc, means) + tc[:, None, :]  # [C,N,3]
    RR = torch.einsum("cij,njk->cnik", Rc, quat_to_rotmat(quats))  # [C,N,3,3]
    WH = torch.stack([RR[..., 0] * scales[None, :, 0:1], RR[..., 1] * scales[None, :, 1:2], p], dim=-1)  # columns a, b, p
    K = torch.zeros_like(Ks)
    K[:, 0, 0], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2], K[:, 2, 2] = Ks[:, 0, 0], Ks[:, 0, 2], Ks[:, 1, 1], Ks[:, 1, 2], 1.0
    M = torch.einsum("cij,cnjk->cnik", K, WH)
    sg = torch.tensor([1.0, 1.0, -1.0], dtype=means.dtype)
    z = p[..., 2]
    in_depth = ~((z < near_plane) | (z > far_plane))
    d = (sg * M[..., 2, :] * M[..., 2, :]).sum(-1)
    ok_d = d != 0
    f = sg / torch.where(ok_d, d, torch.ones_like(d))[..., None]
    m2 = torch.stack([(f * M[..., 0, :] * M[..., 2, :]).sum(-1), (f * M[..., 1, :] * M[..., 2, :]).sum(-1)], dim=-1)
    ext = m2 * m2 - torch.stack([(f * M[..., 0, :] ** 2).sum(-1), (f * M[..., 1, :] ** 2).sum(-1)], dim=-1)
    radius_raw = 3.0 * torch.sqrt(torch.clamp(ext.max(dim=-1).values.detach(), min=1e-4))
    r = torch.ceil(radius_raw)
    inside = ~((m2[..., 0] + r <= 0) | (m2[..., 0] - r >= width) | (m2[..., 1] + r <= 0) | (m2[..., 1] - r >= height))
    visible = in_depth & ok_d & (r > radius_clip) & inside
    facing = -(RR[..., 2] * p).sum(-1)
    normals = torch.where(facing > 0, 1.0, -1.0)[..., None] * RR[..., 2]
    mx, my = m2[..., 0].detach(), m2[..., 1].detach()
    near_cull = (_rel_close(z, near_plane) | _rel_close(z, far_plane) | (radius_clip > 0) & _rel_close(r, radius_clip)
                 | _rel_close(mx + r, 0.0, mx.abs() + r) | _rel_close(mx - r, float(width)) | _rel_close(my + r, 0.0, my.abs() + r)
                 | _rel_close(my - r, float(height)) | _rel_close(facing, 0.0, RR[..., 2].norm(dim=-1) * p.norm(dim=-1))) & in_depth & ok_d
    vz = visible[..., None]
    return dict(radii=torch.where(visible, r, torch.zeros_like(r)).to(torch.int32), means2d=torch.where(vz, m2, torch.zeros_like(m2)),
                depths=torch.where(visible, z, torch.zeros_like(z)),
                ray_transforms=torch.where(vz[..., None], M, torch.zeros_like(M)), normals=torch.where(vz, normals, torch.zeros_like(normals)),
                radius_raw=radius_raw, near_cull=near_cull.detach(), visible=visible)


def sh_colors(degree, dirs, coeffs):
    """Real spherical harmonics up to degree 3 of the normalised ``dirs`` [...,3] with ``coeffs`` [...,K,3], then the renderer's
    ``clamp_min(. + 0.5, 0)``."""
    x, y, z = (dirs / dirs.norm(dim=-1, keepdim=True)).unbind(-1)
    basis = [torch.full_like(x, 0.2820947917738781)]
    if degree >= 1:
        basis += [-0.48860251190292 * y, 0.48860251190292 * z, -0.48860251190292 * x]
    if degree >= 2:
        z2, c1, s1 = z * z, x * x - y * y, 2 * x * y
        tb = -1.092548430592079 * z
        basis += [0.5462742152960395 * s1, tb * y, 0.9461746957575601 * z2 - 0.3153915652525201, tb * x, 0.5462742152960395 * c1]
    if degree >= 3:
        tc, t1 = -2.285228997322329 * z2 + 0.4570457994644658, 1.445305721320277 * z
        c2, s2 = x * c1 - y * s1, x * s1 + y * c1
        basis += [-0.5900435899266435 * s2, t1 * s1, tc * y, z * (1.865881662950577 * z2 - 1.119528997770346), tc * x, t1 * c1,
                  -0.5900435899266435 * c2]
    Bm = torch.stack(basis, dim=-1)  # [..., (degree+1)^2]
    out = (Bm[..., None] * coeffs[..., :Bm.shape[-1], :]).sum(-2)
    return torch.clamp_min(out + 0.5, 0.0)


def composite(means2d, ray_transforms, colors, opacities, normals, backgrounds, width, height, isect_offsets, flatten_ids, distloss,
              keep_pixel_grads=False):
    """Composites every tile's list (``isect_offsets`` [C,th,tw], ``flatten_ids`` [n_isects] into the flat [C*N] splats).

    -> dict: colors [C,H,W,D], alphas [C,H,W,1], normals [C,H,W,3], distort [C,H,W,1], median [C,H,W,1] and, per pixel,
    ``near_decision`` (bool), ``n_contrib``, ``n_filter`` (contributions through the 2D-filter branch), ``n_clamped``
    (contributions with o exp(-sigma) > 0.999), ``early`` (the pixel stopped before the end of its list), ``T_min_reached`` (T fell
    to 0.5 or below); ``list_lengths`` [C,th,tw].  With ``keep_pixel_grads`` also ``pixel_means2d``: (ids, [P,L,2] leaf copies of the
    2D means as each pixel uses them) per tile, whose ``.grad`` after a backward holds the per-pixel position gradients."""
    C, th, tw = isect_offsets.shape
    dt, D = means2d.dtype, colors.shape[-1]
    m2, M, col = means2d.reshape(-1, 2), ray_transforms.reshape(-1, 3, 3), colors.reshape(-1, D)
    opa, nrm = opacities.reshape(-1), normals.reshape(-1, 3)
    offs = isect_offsets.reshape(-1).tolist() + [int(flatten_ids.shape[0])]
    out = {k: torch.zeros((C, height, width, n), dtype=dt) for k, n in (("colors", D), ("alphas", 1), ("normals", 3), ("distort", 1), ("median", 1))}
    stats = {k: torch.zeros((C, height, width), dtype=torch.int64) for k in ("n_contrib", "n_filter", "n_clamped")}
    flags = {k: torch.zeros((C, height, width), dtype=torch.bool) for k in ("near_decision", "early", "T_min_reached")}
    pieces = {k: [] for k in out}
    pixel_means = []
    for c in range(C):
        for ty in range(th):
            for tx in range(tw):
                t = (c * th + ty) * tw + tx
                ids = flatten_ids[offs[t]:offs[t + 1]].long()
                i0, j0 = ty * TILE, tx * TILE
                i1, j1 = min(i0 + TILE, height), min(j0 + TILE, width)
                ii, jj = torch.meshgrid(torch.arange(i0, i1), torch.arange(j0, j1), indexing="ij")
                px, py = (jj.reshape(-1).to(dt) + 0.5)[:, None], (ii.reshape(-1).to(dt) + 0.5)[:, None]  # [P,1]
                P, L = px.shape[0], ids.shape[0]
                bg = backgrounds[c] if backgrounds is not None else torch.zeros(D, dtype=dt)
                if L == 0:
                    res = dict(colors=bg.expand(P, D), alphas=torch.zeros(P, 1, dtype=dt), normals=torch.zeros(P, 3, dtype=dt),
                               distort=torch.zeros(P, 1, dtype=dt), median=torch.zeros(P, 1, dtype=dt))
                else:
                    Mi = M[ids]  # [L,3,3]
                    hu = px[..., None] * Mi[None, :, 2, :] - Mi[None, :, 0, :]  # [P,L,3]
                    hv = py[..., None] * Mi[None, :, 2, :] - Mi[None, :, 1, :]
                    zeta = torch.linalg.cross(hu, hv)
                    zz = zeta[..., 2]
                    hit = zz != 0
                    zs = torch.where(hit, zz, torch.ones_like(zz))
                    w3 = (zeta[..., 0] / zs) ** 2 + (zeta[..., 1] / zs) ** 2
                    mloc = m2[ids][None].expand(P, L, 2)
                    if keep_pixel_grads:
                        mloc = mloc.detach().clone().requires_grad_(True)
                        pixel_means.append((ids, mloc))
                    w2 = 2.0 * ((mloc[..., 0] - px) ** 2 + (mloc[..., 1] - py) ** 2)
                    use3d = w3 <= w2
                    G = torch.exp(-0.5 * torch.where(use3d, w3, w2))
                    raw = opa[ids][None] * G
                    clamped = raw > ALPHA_MAX
                    alpha = torch.where(clamped, torch.full_like(raw, ALPHA_MAX), raw)
                    valid = hit & ~(alpha < ALPHA_MIN)
                    a = torch.where(valid, alpha, torch.zeros_like(alpha))
                    next_T = torch.cumprod(1 - a.detach(), dim=1)
                    stop = valid & (next_T <= T_MIN)
                    first = torch.where(stop.any(1), stop.to(torch.int64).argmax(1), torch.full((P,), L))  # index of the terminating splat
                    k = torch.arange(L)[None]
                    contrib = valid & (k < first[:, None])
                    a = torch.where(contrib, alpha, torch.zeros_like(alpha))
                    T_incl = torch.cumprod(1 - a, dim=1)
                    T_before = torch.cat([torch.ones(P, 1, dtype=dt), T_incl[:, :-1]], dim=1)
                    w = a * T_before
                    T_final = T_incl[:, -1:]
                    ci = col[ids]
                    depth = ci[:, -1][None]
                    wd = w * depth
                    dist = torch.zeros(P, 1, dtype=dt)
                    if distloss:
                        dist = (2.0 * (wd * (1 - T_before) - w * (torch.cumsum(wd, 1) - wd))).sum(1, keepdim=True)
                    med_ok = contrib & (T_before.detach() > 0.5)
                    med_idx = torch.where(med_ok, k, torch.full_like(k, -1)).max(1).values
                    median = torch.where(med_idx >= 0, ci[:, -1][med_idx.clamp(min=0)], torch.zeros(P, dtype=dt))[:, None]
                    res = dict(colors=w @ ci + T_final * bg, alphas=1 - T_final, normals=w @ nrm[ids], distort=dist, median=median)
                    # decisions close to their thresholds, over the splats the pixel evaluates (up to and including the one it stops at)
                    with torch.no_grad():
                        seen = k <= first[:, None]
                        matters = seen & hit & (alpha >= ALPHA_MIN * (1 - NEAR))
                        T_b = torch.cat([torch.ones(P, 1, dtype=dt), next_T[:, :-1]], dim=1)
                        nd = (seen & hit & _rel_close(alpha, ALPHA_MIN)) | (matters & _rel_close(raw, ALPHA_MAX)) \
                            | (matters & _rel_close(T_b * (1 - alpha), T_MIN)) | (matters & _rel_close(T_b, 0.5)) \
                            | (matters & ((w3 - w2).abs() <= NEAR * torch.maximum(w3, w2)))
                        sl = (c, slice(i0, i1), slice(j0, j1))
                        shp = (i1 - i0, j1 - j0)
                        flags["near_decision"][sl] = nd.any(1).reshape(shp)
                        flags["early"][sl] = (first < L).reshape(shp)
                        flags["T_min_reached"][sl] = (T_final[:, 0] <= 0.5).reshape(shp)
                        stats["n_contrib"][sl] = contrib.sum(1).reshape(shp)
                        stats["n_filter"][sl] = (contrib & ~use3d).sum(1).reshape(shp)
                        stats["n_clamped"][sl] = (contrib & clamped).sum(1).reshape(shp)
                for key in out:
                    pieces[key].append((c, i0, i1, j0, j1, res[key]))
    # assemble the images out of the tiles without in-place writes into a leaf (autograd-friendly)
    for key, lst in pieces.items():
        n = out[key].shape[-1]
        cams = []
        for c in range(C):
            rows = []
            for ty in range(th):
                row = [r.reshape(i1 - i0, j1 - j0, n) for (cc, i0, i1, j0, j1, r) in lst if cc == c and i0 == ty * TILE]
                rows.append(torch.cat(row, dim=1))
            cams.append(torch.cat(rows, dim=0))
        out[key] = torch.stack(cams, dim=0)
    lengths = torch.tensor([offs[t + 1] - offs[t] for t in range(C * th * tw)]).reshape(C, th, tw)
    out.update(stats)
    out.update(flags)
    out["list_lengths"] = lengths
    if keep_pixel_grads:
        out["pixel_means2d"] = pixel_means
    return out


def absgrad_from_pixels(pixel_means, n_flat, dtype):
    """sum over pixels of |d L / d means2d| per splat, from the leaf copies ``composite(keep_pixel_grads=True)`` returned (after
    a backward) -- plus the plain sum, which is the means2d gradient of the 2D-filter branch."""
    ab, pl = torch.zeros(n_flat, 2, dtype=dtype), torch.zeros(n_flat, 2, dtype=dtype)
    for ids, m in pixel_means:
        if m.grad is not None:
            ab.index_add_(0, ids, m.grad.abs().sum(0))
            pl.index_add_(0, ids, m.grad.sum(0))
    return ab, pl


def affine_inverse(viewmats):
    return torch.linalg.inv(viewmats)


def depth_to_points(depths, camtoworlds, Ks, z_depth=True):
    H, W = depths.shape[-3:-1]
    dt = depths.dtype
    x, y = torch.arange(W, dtype=dt), torch.arange(H, dtype=dt)
    fx, fy, cx, cy = (Ks[..., 0, 0, None, None], Ks[..., 1, 1, None, None], Ks[..., 0, 2, None, None], Ks[..., 1, 2, None, None])
    dx = ((x[None, :] - cx + 0.5) / fx).expand(*depths.shape[:-1])
    dy = ((y[:, None] - cy + 0.5) / fy).expand(*depths.shape[:-1])
    dirs = torch.einsum("...ij,...hwj->...hwi", camtoworlds[..., :3, :3], torch.stack([dx, dy, torch.ones_like(dx)], dim=-1))
    if not z_depth:
        dirs = dirs / dirs.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    return camtoworlds[..., None, None, :3, 3] + depths * dirs


def depth_to_normal(depths, camtoworlds, Ks, z_depth=True):
    pts = depth_to_points(depths, camtoworlds, Ks, z_depth)
    dx = pts[..., 2:, 1:-1, :] - pts[..., :-2, 1:-1, :]
    dy = pts[..., 1:-1, 2:, :] - pts[..., 1:-1, :-2, :]
    n = torch.linalg.cross(dx, dy)
    n = n / n.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    return torch.nn.functional.pad(n, (0, 0, 1, 1, 1, 1), value=0.0)


def render(means, quats, scales, opacities, colors, viewmats, Ks, width, height, isect_offsets, flatten_ids, sh_degree=None,
           backgrounds=None, render_mode="RGB", distloss=False, depth_mode="expected", near_plane=0.01, far_plane=1e10, radius_clip=0.0,
           keep_pixel_grads=False):
    """The chain of ``rasterization_2dgs`` on given tile lists -> (colors, alphas, normals (world), normals_from_depth | None,
    distort, median, info) with ``info`` = the projection dict + the compositing dict."""
    C = viewmats.shape[0]
    pr = project(means, quats, scales, viewmats, Ks, width, height, near_plane, far_plane, radius_clip)
    c2w = affine_inverse(viewmats)
    if sh_degree is not None:
        dirs = means[None] - c2w[:, None, :3, 3]
        col = sh_colors(sh_degree, dirs, colors[None].expand(C, *colors.shape))
        col = torch.where(pr["visible"][..., None], col, torch.zeros_like(col))
    else:
        col = colors.expand(C, -1, -1) if colors.dim() == 2 else colors
    if render_mode in ("RGB+D", "RGB+ED"):
        col = torch.cat([col, pr["depths"][..., None]], dim=-1)
        if backgrounds is not None and backgrounds.shape[-1] != col.shape[-1]:
            backgrounds = torch.cat([backgrounds, torch.zeros(C, 1, dtype=backgrounds.dtype)], dim=-1)
    elif render_mode in ("D", "ED"):
        col = pr["depths"][..., None]
        if backgrounds is not None and backgrounds.shape[-1] != 1:
            backgrounds = torch.zeros(C, 1, dtype=backgrounds.dtype)
    densify = torch.zeros_like(pr["means2d"])
    cp = composite(pr["means2d"], pr["ray_transforms"], col, opacities[None].expand(C, -1), pr["normals"], backgrounds, width, height,
                   isect_offsets, flatten_ids, distloss, keep_pixel_grads)
    rc, ra = cp["colors"], cp["alphas"]
    if render_mode in ("ED", "RGB+ED"):
        rc = torch.cat([rc[..., :-1], rc[..., -1:] / ra.clamp(min=1e-10)], dim=-1)
    nfd = None
    if render_mode in ("RGB+D", "RGB+ED"):
        nfd = depth_to_normal(rc[..., -1:] if depth_mode == "expected" else cp["median"], c2w, Ks)
    rn = torch.einsum("cij,chwj->chwi", c2w[:, :3, :3], cp["normals"])
    info = dict(pr)
    info.update(cp)
    info["densify"] = densify
    return rc, ra, rn, nfd, cp["distort"], cp["median"], info


def rel_l2(a, b):
    """|a - b| / |b| over all entries, in float64 (0 when both are zero)."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    den = float(b.norm())
    num = float((a - b).norm())
    return num / den if den > 0 else (0.0 if num == 0 else math.inf)
