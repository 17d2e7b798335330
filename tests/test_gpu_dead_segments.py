"""The depth-segmented compositing backward runs no work item behind a tile's last contributor.

The forward reports, per tile, the last list entry any of its 256 pixels composited (the maximum of its last_ids); the work
list keeps a (tile, segment) item only if that entry lies at or behind the segment's start, the item that holds it ends right
behind it, and the forward writes no checkpoint plane that only a dropped item would read.  Nothing that reaches a gradient
changes: an item is dropped exactly when the kernel's own test "a contributor inside the segment" fails for all four
quadrants, an entry is cut exactly when "not behind the quadrant's last contributor" fails for all four.

Scene (tile 16, 64 x 32 pixels = 4 x 2 tiles, per camera): 600 faint background splats listed in the tile columns 0..2 (lists
of 606 entries = three or four segments of 256; every fourth contributes, the others stay below 1/255), six "plug" splats per
tile whose depth decides where the tile saturates (a flat one of opacity 0.97, then stoppers of 0.999: the pixel ends at
T = 0.03 x the background in front), and 300 ghost splats listed in column 3 that reach no pixel.  Per tile:
  front   the plug in front of everything: every pixel ends at the tile's first entry, the later segments are dead
  hole    a narrow plug that misses a corner of the tile: those pixels stay live to the list's end next to saturated ones
  km1     the plug's depth shifted until the tile's last contributor is list entry k * seg - 1 (a segment's last entry)
  k0      ... until it is entry k * seg (a segment's first entry: the segment in front is complete, the one behind has one entry)
  end     a weak plug behind everything: the last contributor is the list's last entry, range_end - 1
  ghost   a list (two boundaries inside) without any contributor
Every test asserts this premise on the last_ids the library returned, and that the work list holds exactly the live items.

Why the opacities are what they are: the unsegmented route (like the reference and the float32 oracle) restarts every pixel
from T_final = 1 - render_alpha, whose rounding error relative to T_final is 3e-8 / T_final -- 3e-4 on a pixel that saturates
at T_final ~ 1e-4.  With an opacity-0.99 wall and a background that takes the live pixels to T ~ 0.003 the float32 oracle and
the unsegmented route were both 1e-4 .. 2.3e-4 (rel. l2) from float64, the segmented route 1e-6 .. 5e-6
(profiles/r25_dead_segments.txt, section 4): the route comparison would have measured its yardstick.  Here all but a few
pixels on the hole plug's rim end at T_final >= 0.005, and the float32 oracle is within 2e-5 of float64 on every gradient."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity_f64 import _check
from util import N, T, rel_l2, tuned

pytestmark = pytest.mark.gpu

from oracle import gs_oracle as O  # noqa: E402

SEG, TS, W, H, TW, TH = 256, 16, 64, 32, 4, 2
NB, NP, NG = 600, 6, 300  # background, plug splats per tile, ghosts
PLUG_TILES = [(tx, ty) for ty in range(TH) for tx in range(3)]
ROLES = [
    {(0, 0): "hole", (1, 0): "front", (2, 0): "km1", (0, 1): "front", (1, 1): "end", (2, 1): "k0"},
    {(0, 0): "k0", (1, 0): "km1", (2, 0): "end", (0, 1): "hole", (1, 1): "front", (2, 1): "front"},
]
BG_OPAC, BG_SIGMA, HOLE_PLUGS = (0.006, 0.012), (40, 80), 3
PLUG_OPAC = {"front": 0.97, "hole": 0.992, "end": 0.3}
ROUTE_BOUND = 2e-4  # "generic vs segmented" of tests/test_gpu_ops.py


def _splats(cams, shift):
    """The compositing inputs of `cams` cameras; shift[c][tile]: background splats in front of the tile's plug."""
    n = NB + len(PLUG_TILES) * NP + NG
    m2, cn, op = np.zeros((cams, n, 2), np.float32), np.zeros((cams, n, 3), np.float32), np.zeros((cams, n), np.float32)
    radii, depths = np.zeros((cams, n), np.int32), np.zeros((cams, n), np.float32)
    for c in range(cams):
        rs = np.random.RandomState(17 + c)
        sig = rs.uniform(*BG_SIGMA, NB)
        m2[c, :NB] = np.stack([rs.uniform(20, 28, NB), rs.uniform(10, 22, NB)], -1)
        cn[c, :NB] = np.stack([1 / sig**2, 0.1 * rs.uniform(-1, 1, NB) / sig**2, 1 / sig**2], -1)
        op[c, :NB] = np.where(np.arange(NB) % 4 == 3, rs.uniform(*BG_OPAC, NB), 0.002)  # three of four stay below 1/255
        radii[c, :NB] = 19  # tile columns 0..2, both rows
        depths[c, :NB] = 2.0 + 1e-3 * np.arange(NB)
        for t, (tx, ty) in enumerate(PLUG_TILES):
            role, s = ROLES[c][(tx, ty)], slice(NB + t * NP, NB + (t + 1) * NP)
            centre = np.array([16 * tx + 11, 16 * ty + 11] if role == "hole" else [16 * tx + 8, 16 * ty + 8], np.float32)
            sigma = 3.5 if role == "hole" else 200.0
            m2[c, s] = centre + rs.uniform(-0.2, 0.2, (NP, 2))
            cn[c, s] = [1 / sigma**2, 0.0, 1 / sigma**2]
            op[c, s] = PLUG_OPAC.get(role, PLUG_OPAC["front"])
            if role == "hole":
                op[c, s][HOLE_PLUGS:] = 0.0
            elif role != "end":  # the first takes T to 0.03 f, the second would take it below 1e-4: T_final = 0.03 f
                op[c, s][1:] = 0.999
            radii[c, s] = 4 if role == "hole" else 7  # inside the tile
            depths[c, s] = 2.0 + 1e-3 * (shift[c][(tx, ty)] - 0.5) + 1e-5 * np.arange(NP)
        g = slice(n - NG, n)
        m2[c, g] = np.array([56.0, 16.0], np.float32) + rs.uniform(-0.1, 0.1, (NG, 2))  # between the pixel centres
        cn[c, g] = [400.0, 0.0, 400.0]
        op[c, g] = 0.5
        radii[c, g] = 7  # column 3, both rows
        depths[c, g] = 1.0 + 1e-3 * np.arange(NG)
    return m2, cn, op, radii, depths


def _tile_table(offs, n_isects, last_ids, masks=None):
    """Per (camera, tile) with a list and no mask: (lin, range_start, range_end, tile_last)."""
    o = np.append(offs.ravel(), n_isects)
    rows = []
    for lin in range(offs.size):
        c, ty, tx = np.unravel_index(lin, offs.shape)
        if o[lin + 1] > o[lin] and (masks is None or masks[c, ty, tx]):
            rows.append((lin, int(o[lin]), int(o[lin + 1]), int(last_ids[c, ty * TS:(ty + 1) * TS, tx * TS:(tx + 1) * TS].max())))
    return rows


def _segments(rows, seg=SEG):
    """(live, dead) segment counts: a segment is live if the tile's last contributor is not in front of its start."""
    live = dead = 0
    for _, rs, re, tl in rows:
        for k in range(rs // seg, (re - 1) // seg + 1):
            if tl >= max(rs, k * seg):
                live += 1
            else:
                dead += 1
    return live, dead


@functools.lru_cache(maxsize=None)
def _scene(cams):
    """The scene with the km1 / k0 plugs shifted to their targets (last contributor by the float32 oracle)."""
    shift = [{t: {"end": NB}.get(ROLES[c][t], 0) for t in PLUG_TILES} for c in range(cams)]
    for _ in range(8):
        m2, cn, op, radii, depths = _splats(cams, shift)
        _, ids, flat = O.isect_tiles(m2, radii, depths, TS, TW, TH)
        offs = O.isect_offset_encode(ids, cams, TW, TH)
        li = O.rasterize_fwd(m2, cn, np.zeros((cams, m2.shape[1], 1), np.float32), op, W, H, TS, offs, flat)[2]
        moved = False
        for lin, rs, re, tl in _tile_table(offs, flat.shape[0], li):
            c, ty, tx = np.unravel_index(lin, offs.shape)
            role = ROLES[c].get((tx, ty))
            if role in ("km1", "k0"):
                target = -(-(rs + 8) // SEG) * SEG - (role == "km1")
                assert rs < target < re - 8
                if tl != target:
                    shift[c][(tx, ty)] = int(np.clip(shift[c][(tx, ty)] + target - tl, 0, NB))
                    moved = True
        if not moved:
            break
    assert not moved, "the plugs did not settle on their targets"
    return dict(means2d=m2, conics=cn, opacities=op, offs=offs, flat=flat, C=cams)


def _premise(c, last_ids, scratch, masks=None, ghosts=True):
    """The scene does what the test is about, by the last_ids the library returned, and the work list holds the live items."""
    rows = _tile_table(c["offs"], c["flat"].shape[0], N(last_ids), masks)
    live, dead = _segments(rows)
    assert dead >= 2, dead
    assert any(tl >= max(rs, (re - 1) // SEG * SEG) for _, rs, re, tl in rows), "no tile is live to its end"
    li = N(last_ids)
    for lin, rs, re, tl in rows:  # a hole tile: pixels that saturate in the first segment next to one that is live to the end
        cam, ty, tx = np.unravel_index(lin, c["offs"].shape)
        if ROLES[cam].get((tx, ty)) == "hole":
            assert tl >= (re - 1) // SEG * SEG and li[cam, ty * TS + 11, tx * TS + 11] < rs + 64, (lin, rs, re, tl)
    assert any(tl >= rs and tl % SEG < 64 for _, rs, _, tl in rows) and any(tl >= rs and tl % SEG >= SEG - 64 for _, rs, _, tl in rows)
    if masks is None:  # the exact off-by-one cases
        assert any(tl > rs and tl % SEG == SEG - 1 for _, rs, _, tl in rows), "last contributor = k * seg - 1"
        assert any(tl > rs and tl % SEG == 0 for _, rs, _, tl in rows), "last contributor = k * seg"
        assert any(tl == re - 1 for _, _, re, tl in rows), "last contributor = range_end - 1"
    if ghosts:
        assert any(tl < rs for _, rs, _, tl in rows), "no tile without a contributor"
    n_items = int(scratch[:128].view(torch.int32).sum())  # the class counters at the head of the scratch
    print(f"segments: {live} live, {dead} dead; work items {n_items}")
    assert n_items == live, (n_items, live, dead)
    return live, dead


@functools.lru_cache(maxsize=None)
def _reference(cams, channels, masked):
    """Inputs, image gradients and the float32 / float64 oracle gradients, computed once per case."""
    c = _scene(cams)
    rs = np.random.RandomState(100 + channels)
    colors = rs.rand(cams, c["means2d"].shape[1], channels).astype(np.float32)
    bg = rs.rand(cams, channels).astype(np.float32)
    masks = None
    if masked:  # a dead tile, a hole tile and a ghost tile masked out
        masks = np.ones((cams, TH, TW), bool)
        masks[0, 0, 1] = masks[cams - 1, 1, 0] = masks[0, 1, 3] = False
    geo = (c["means2d"], c["conics"], colors, c["opacities"], W, H, TS, c["offs"], c["flat"])
    o_rc, o_ra, o_li, bl32 = O.rasterize_fwd(*geo, backgrounds=bg, masks=masks, return_borderline=True)
    with O.precision(64):
        d_rc, d_ra, d_li, bl64 = O.rasterize_fwd(*geo, backgrounds=bg, masks=masks, return_borderline=True)
    ok = (bl32 == 0) & (bl64 == 0)
    assert ok.mean() > 0.995 and np.array_equal(o_li[ok], d_li[ok])
    v_rc = rs.randn(*o_rc.shape).astype(np.float32) * ok[..., None]
    v_ra = rs.randn(*o_ra.shape).astype(np.float32) * ok[..., None]
    if masks is not None:  # (a masked tile's alphas are not written)
        v_ra *= np.repeat(np.repeat(masks, TS, 1), TS, 2)[..., None]
    g32 = O.rasterize_bwd(*geo, o_ra, o_li, v_rc, v_ra, backgrounds=bg, masks=masks, absgrad=True)
    with O.precision(64):
        g64 = O.rasterize_bwd(*geo, d_ra, d_li, v_rc, v_ra, backgrounds=bg, masks=masks, absgrad=True)
    return dict(c=c, colors=colors, bg=bg, masks=masks, v_rc=v_rc, v_ra=v_ra, g32=g32, g64=g64)


NAMES = ("v_means2d", "v_conics", "v_colors", "v_opacities", "absgrad")


def _run(r, route, absgrad=False, deterministic=False, backwards=1):
    """Forward + `backwards` backward calls under a tuning route -> (gradients of each call, last_ids, scratch)."""
    from gscodec_studio_amd import _wrapper as ops

    c = r["c"]
    leaves = [T(c["means2d"], True), T(c["conics"], True), T(r["colors"], True), T(c["opacities"], True)]
    with tuned(route):
        rc, ra = ops.rasterize_to_pixels(*leaves, W, H, TS, T(c["offs"]), T(c["flat"]), backgrounds=T(r["bg"]),
                                         masks=None if r["masks"] is None else T(r["masks"]), absgrad=absgrad, deterministic=deterministic)
        saved = rc.grad_fn.saved_tensors
        last_ids, scratch = saved[9], saved[10]
        loss = (rc * T(r["v_rc"])).sum() + (ra * T(r["v_ra"])).sum()
        calls = []
        for i in range(backwards):
            g = torch.autograd.grad(loss, leaves, retain_graph=i + 1 < backwards)
            calls.append([N(x) for x in g] + ([N(leaves[0].absgrad)] if absgrad else []))
    return calls, last_ids, scratch


def _against_float64(r, g, absgrad):
    g32, g64 = r["g32"], r["g64"]
    _check("v_means2d", g[0], g32[0], g64[0], cond=g64[4])
    for i in (1, 2, 3):
        _check(NAMES[i], g[i], g32[i], g64[i])
    if absgrad:
        _check("absgrad", g[4], g32[4], g64[4])


def _against_unsegmented(r, g, **kw):
    (u,), _, _ = _run(r, "unsegmented", **kw)
    errs = [(name, rel_l2(x, y)) for name, x, y in zip(NAMES, g, u)]
    print("segmented vs unsegmented:", errs)
    print("against float64, segmented / unsegmented:", [(name, rel_l2(x, d), rel_l2(y, d)) for name, x, y, d in zip(NAMES, g, u, r["g64"])])
    for name, e in errs:
        assert e < ROUTE_BOUND, (name, e)


@pytest.mark.parametrize("cams", [1, 2])
@pytest.mark.parametrize("channels,absgrad", [(3, False), (3, True), (9, False), (9, True)])
def test_dead_segments_gradients(channels, absgrad, cams):
    """RGB and wide kernel, absgrad on and off, one and two cameras, with backgrounds (separate gradient arrays): the premise, the
    item count, the gradients against float64 and against the unsegmented route."""
    r = _reference(cams, channels, False)
    (g,), last_ids, scratch = _run(r, "default", absgrad=absgrad)
    _premise(r["c"], last_ids, scratch)
    _against_float64(r, g, absgrad)
    _against_unsegmented(r, g, absgrad=absgrad)


def test_dead_segments_deterministic_and_repeated_backward():
    """deterministic=True: two backward calls over one forward (retain_graph) reuse the work list and agree bit for bit; the
    same gradients against float64 and the unsegmented route."""
    r = _reference(2, 3, False)
    (g1, g2), last_ids, scratch = _run(r, "default", deterministic=True, backwards=2)
    _premise(r["c"], last_ids, scratch)
    for name, x, y in zip(NAMES, g1, g2):
        assert np.array_equal(x, y), name
    _against_float64(r, g1, False)
    _against_unsegmented(r, g1, deterministic=True)


@pytest.mark.parametrize("channels", [3, 9])
def test_dead_segments_repeated_backward_and_masks(channels):
    """Masked tiles (a dead one, a hole one, a ghost one) and a second backward over the same work list."""
    r = _reference(2, channels, True)
    (g1, g2), last_ids, scratch = _run(r, "default", backwards=2)
    _premise(r["c"], last_ids, scratch, masks=r["masks"])
    for name, x, y in zip(NAMES, g1, g2):
        assert rel_l2(y, x) < 1e-5, (name, "second backward", rel_l2(y, x))  # float atomics: the order of the sums differs
    _against_float64(r, g1, False)
    _against_unsegmented(r, g1)


@pytest.mark.parametrize("seg", [64, 192])
def test_dead_segments_other_segment_lengths(seg):
    """64 (every sub-batch a boundary) and 192 (no power of two): the item count and the route agreement."""
    r = _reference(2, 3, False)
    (g,), last_ids, scratch = _run(r, {"raster_seg": seg})
    live, dead = _segments(_tile_table(r["c"]["offs"], r["c"]["flat"].shape[0], N(last_ids)), seg)
    n_items = int(scratch[:128].view(torch.int32).sum())
    assert dead >= 2 and n_items == live, (n_items, live, dead)
    _against_float64(r, g, False)
    _against_unsegmented(r, g)


# ---- rasterization(): the fast path with packed gradient rows

@functools.lru_cache(maxsize=None)
def _world():
    """Two cameras looking down +z at 600 background splats (z = 2 .. 2.6, every tile, three of four below 1/255): the one at the
    origin through a flat wall at z = 1 (one splat takes T to 0.03, the next would take it below 1e-4: every tile saturates in its
    first entries), the one at z = 1.5 from behind the wall (every tile live to its list's end)."""
    rs = np.random.RandomState(23)
    f, nw = 50.0, 40
    n = nw + NB
    u = np.concatenate([32 + rs.uniform(-1, 1, nw), rs.uniform(0, W, NB)])
    v = np.concatenate([16 + rs.uniform(-1, 1, nw), rs.uniform(0, H, NB)])
    z = np.concatenate([1 + 2e-3 * np.arange(nw), 2 + 1e-3 * np.arange(NB)])
    sig = np.concatenate([np.full(nw, 1000.0), rs.uniform(40, 80, NB)])
    means = np.stack([(u - W / 2) * z / f, (v - H / 2) * z / f, z], -1).astype(np.float32)
    scales = np.stack([sig * z / f, sig * z / f, np.full(n, 0.01)], -1).astype(np.float32)
    quats = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    opac = np.concatenate([[0.97], np.full(nw - 1, 0.999), np.where(np.arange(NB) % 4 == 3, rs.uniform(0.006, 0.012, NB), 0.002)]).astype(np.float32)
    sh = np.concatenate([rs.rand(n, 1, 3), 0.05 * rs.randn(n, 15, 3)], 1).astype(np.float32)
    Ks = np.tile(np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32), (2, 1, 1))
    viewmats = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    viewmats[1, 2, 3] = -1.5
    return dict(means=means, quats=quats, scales=scales, opacities=opac, colors=sh, viewmats=viewmats, Ks=Ks)


def test_dead_segments_rasterization_packed_rows():
    """rasterization() (SH degree 3, packed gradient rows): dead segments by the oracle's last_ids, every parameter's gradient
    against the unsegmented route and against the oracle's hand-chained VJPs (the bars of tests/test_gpu_rasterization.py:
    the compositing inputs are the library's own projection there, not the oracle's)."""
    from gscodec_studio_amd import rasterization

    d = _world()
    keys = ("means", "quats", "scales", "opacities", "colors")
    o_rc, o_ra, om = O.rasterization(*(d[k] for k in keys), d["viewmats"], d["Ks"], W, H, sh_degree=3)
    rows = _tile_table(om["isect_offsets"], om["flatten_ids"].shape[0], om["last_ids"])
    live, dead = _segments(rows)
    assert dead >= 2 and any(tl >= max(rs, (re - 1) // SEG * SEG) for _, rs, re, tl in rows), (live, dead)
    bl = O.rasterize_fwd(om["means2d"], om["conics"], om["colors"], om["opacities"], W, H, TS, om["isect_offsets"], om["flatten_ids"],
                         return_borderline=True)[3]
    rs = np.random.RandomState(29)
    v_rc = rs.randn(*o_rc.shape).astype(np.float32) * (bl == 0)[..., None]
    v_ra = rs.randn(*o_ra.shape).astype(np.float32) * (bl == 0)[..., None]

    def run(route):
        P = {k: T(d[k], True) for k in keys}
        with tuned(route):
            rc, ra, meta = rasterization(*(P[k] for k in keys), T(d["viewmats"]), T(d["Ks"]), W, H, sh_degree=3, packed=False)
            meta["means2d"].retain_grad()
            ((rc * T(v_rc)).sum() + (ra * T(v_ra)).sum()).backward()
        return {k: N(P[k].grad) for k in keys}, N(meta["means2d"].grad)

    g, g_m2 = run("default")
    u, u_m2 = run("unsegmented")
    for k in keys:
        assert rel_l2(g[k], u[k]) < ROUTE_BOUND, (k, "segmented vs unsegmented", rel_l2(g[k], u[k]))
    assert rel_l2(g_m2, u_m2) < ROUTE_BOUND

    C = 2
    v_m2, v_cn, v_col, v_op, _ = O.rasterize_bwd(om["means2d"], om["conics"], om["colors"], om["opacities"], W, H, TS, om["isect_offsets"],
                                                 om["flatten_ids"], o_ra, om["last_ids"], v_rc, v_ra)
    assert rel_l2(g_m2, v_m2) < 5e-4, rel_l2(g_m2, v_m2)
    dirs = d["means"][None] - np.linalg.inv(d["viewmats"].astype(np.float64)).astype(np.float32)[:, None, :3, 3]
    shs = np.ascontiguousarray(np.broadcast_to(d["colors"][None], (C,) + d["colors"].shape))
    sh_raw = O.sh_fwd(3, dirs, shs, om["radii"] > 0)
    v_coeffs, v_dirs = O.sh_bwd(3, dirs, shs, v_col * ((sh_raw + 0.5) > 0), om["radii"] > 0)
    vm, _, vq, vs, _ = O.projection_bwd(d["means"], None, d["quats"], d["scales"], d["viewmats"], d["Ks"], W, H, 0.3, "pinhole", om["radii"],
                                        om["conics"], None, v_m2, np.zeros_like(om["depths"]), v_cn, None, need_viewmats=False)
    vm = vm + v_dirs.sum(0)
    for name, ref in (("means", vm), ("quats", vq), ("scales", vs), ("opacities", v_op.sum(0)), ("colors", v_coeffs.sum(0))):
        assert rel_l2(g[name], ref) < 2e-3, (name, rel_l2(g[name], ref))
