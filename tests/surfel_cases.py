"""Seeded scenes of tests/test_gpu_surfel.py (numpy only, test helper).

All scenes share the image (40 x 27: 3 x 2 tiles of 16 pixels, partial tiles on both edges), the focal length 30 and two cameras:
the identity, and a 20 degree yaw with a translation.
"""
import numpy as np

WIDTH, HEIGHT, FOCAL, C = 40, 27, 30.0, 2
CX, CY = WIDTH / 2, HEIGHT / 2


def cameras():
    a = np.deg2rad(20.0)
    yaw = np.array([[np.cos(a), 0, np.sin(a), -0.4], [0, 1, 0, 0.1], [-np.sin(a), 0, np.cos(a), 0.3], [0, 0, 0, 1]])
    K = np.array([[FOCAL, 0, CX], [0, FOCAL, CY], [0, 0, 1]])
    return np.stack([np.eye(4), yaw]), np.stack([K, K])


def _rotmat(q):
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def _facing(means, quats, viewmats):
    """min over cameras of |normal . view direction| per splat"""
    n = _rotmat(quats)[:, :, 2]
    out = np.full(len(means), np.inf)
    for V in viewmats:
        p = means @ V[:3, :3].T + V[:3, 3]
        nc = n @ V[:3, :3].T
        out = np.minimum(out, np.abs((nc * p).sum(-1)) / np.linalg.norm(p, axis=-1))
    return out


def _random_splats(rs, n, viewmats, min_facing=0.25):
    means = rs.uniform([-2.5, -1.8, 2.0], [2.5, 1.8, 6.0], (n, 3))
    quats = rs.standard_normal((n, 4))
    for _ in range(64):  # re-draw grazing splats: s = zeta_xy / zeta_z is ill-conditioned there (|normal . view| > 0.2 is kept)
        bad = _facing(means, quats, viewmats) <= min_facing
        if not bad.any():
            break
        quats[bad] = rs.standard_normal((int(bad.sum()), 4))
    assert min_facing == 0.0 or (_facing(means, quats, viewmats) > 0.2).all()
    scales = np.exp(rs.uniform(np.log(0.02), np.log(0.4), (n, 3)))
    tiny = rs.permutation(n)[: n // 4]
    scales[tiny] = np.exp(rs.uniform(np.log(0.002), np.log(0.02), (len(tiny), 3)))
    low = rs.uniform(size=n) < 0.5
    opac = np.where(low, rs.uniform(0.02, 0.35, n), rs.uniform(0.35, 0.95, n))
    return means, quats, scales, opac


def _pixel_ray(px, py, z):
    """camera-0 (identity) position at depth z on the ray through the CENTRE of pixel (px, py)"""
    return np.array([(px + 0.5 - CX) / FOCAL * z, (py + 0.5 - CY) / FOCAL * z, z])


def main_scene(seed=0, n=600):
    """600 random splats plus hand-placed ones, so that every path of the compositing kernels is taken (the test asserts the
    coverage from the restatement's counters):
    * a band of the image (rows >= 19 in camera 0) gets its opacities scaled down: pixels that never terminate, some whose T stays
      above 0.5;
    * the lower left corner (columns < 7, rows >= 21) gets opacity 1e-3: pixels without any contribution;
    * 14 tiny bright splats in front of everything: contributions through the 2D-filter branch;
    * 5 opacity-1.0 splats facing camera 0, centred exactly on pixel centres: o exp(-sigma) > 0.999 there;
    * a stack of 16 nearly opaque splats in the busiest tile: pixels that terminate early, and a tile list longer than one batch."""
    rs = np.random.RandomState(seed)
    viewmats, Ks = cameras()
    means, quats, scales, opac = _random_splats(rs, n, viewmats)
    row = means[:, 1] / means[:, 2] * FOCAL + CY
    col = means[:, 0] / means[:, 2] * FOCAL + CX
    opac = np.where(row >= 19, opac * 0.06, opac)
    opac = np.where((row >= 21) & (col < 7), 1e-3, opac)
    extra_m, extra_q, extra_s, extra_o = [], [], [], []
    for i in range(14):  # tiny, in front, in the upper two thirds
        extra_m.append(_pixel_ray(3 + 2.5 * i + 0.3, 2 + (i * 5) % 15 + 0.2, 1.0 + 0.04 * i))
        extra_q.append([1.0, 0.1 * (i % 3), -0.1 * (i % 2), 0.05])
        extra_s.append([0.004, 0.006, 0.01])
        extra_o.append(0.5 + 0.03 * i)
    for i, (px, py) in enumerate([(5, 4), (17, 9), (30, 3), (22, 14), (36, 12)]):  # facing camera 0, on pixel centres
        extra_m.append(_pixel_ray(px, py, 1.5 + 0.1 * i))
        extra_q.append([1.0, 0.0, 0.0, 0.0])
        extra_s.append([0.06, 0.05, 0.02])
        extra_o.append(1.0)
    for i in range(16):  # a stack of nearly opaque splats in the middle of the depth range: pixels that terminate early
        extra_m.append(_pixel_ray(23.3 + 0.1 * (i % 4), 7.6 + 0.1 * (i % 3), 2.6 + 0.03 * i))
        extra_q.append([1.0, 0.08 * (i % 3 - 1), 0.06 * (i % 4 - 1.5), 0.3 * i])
        extra_s.append([0.22, 0.2, 0.05])
        extra_o.append(0.86)
    return dict(means=np.concatenate([means, extra_m]), quats=np.concatenate([quats, extra_q]), scales=np.concatenate([scales, extra_s]),
                opacities=np.concatenate([opac, extra_o]), viewmats=viewmats, Ks=Ks)


def small_scene(seed=1, n=96):
    """96 splats, short tile lists: the channel and mode sweep.  Opacities scaled down so that few pixels terminate."""
    rs = np.random.RandomState(seed)
    viewmats, Ks = cameras()
    means, quats, scales, opac = _random_splats(rs, n, viewmats)
    return dict(means=means, quats=quats, scales=scales, opacities=opac * 0.8, viewmats=viewmats, Ks=Ks)


def degenerate_scene():
    """Forward only: splats behind the camera, beyond a far plane of 50, below a radius clip, and one exactly edge-on.  A third
    camera (an exact quarter turn about y at the origin) sees splat 9 (identity rotation, mean (2, 0, 0), s_x = 2) edge-on:
    M_w = (2, 0, 2), so M_w,x^2 + M_w,y^2 - M_w,z^2 is exactly zero in float32 as well."""
    rs = np.random.RandomState(2)
    viewmats, Ks = cameras()
    side = np.array([[0.0, 0, -1, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1]])
    viewmats, Ks = np.concatenate([viewmats, side[None]]), np.concatenate([Ks, Ks[:1]])
    means, quats, scales, opac = _random_splats(rs, 40, viewmats[:2], min_facing=0.0)
    means[:5, 2] = [-1.0, -4.0, -0.5, 0.001, 0.0]  # behind cameras 0 and 1 / in front of the near plane
    means[5:9, 2] = [80.0, 120.0, 60.0, 51.0]  # beyond far_plane = 50
    means[9], quats[9], scales[9] = [2.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [2.0, 0.3, 0.1]
    return dict(means=means, quats=quats, scales=scales, opacities=opac, viewmats=viewmats, Ks=Ks)
