"""One ``rasterization()`` call shape of tests/test_gpu_routes.py's table on the CPU, end to end, forward and hand-chained VJP (TEST
INFRASTRUCTURE: numpy + CPU torch, nothing here touches the GPU or imports the package).

    projection_chain.chain  ->  O.isect_tiles / O.isect_offset_encode  ->  O.rasterize_fwd  ->  [expected depth]
    chain(cot=...)          <-                                             O.rasterize_bwd  <-  [its VJP]

``render_chain(bits, case)`` evaluates it in ``bits`` = 64 (the ground truth) or 32 (the reference's arithmetic in float32: the yardstick)
from the float32 numbers of ``route_scene(**case)``, which is also where tests/test_gpu_routes.run_case takes its inputs from.  The tile
lists of either build are binned by the float32 oracle from that build's own projection rounded to float32 (the binning works on depth
bits; the float64 build of it means nothing).

What is hand-written here is the glue the routes decide about, held against central differences by tests/test_render_chain_cpu.py:
colours that are not the chain's ``[N,3]`` / ``[N,K,3]`` (``[N,5]``, per-camera ``[C,N,3]`` without a camera sum in the VJP, per-camera SH
``[C,N,K,3]``), the ``(sh0, shN)`` pair as two slices of one gradient, the soft mask in front of ``shN`` with its VJP to ``shN`` and the logits,
the depth as last channel, ``ED`` = last / max(alphas, 1e-10) with its VJP into the accumulated depth and the alphas, the backgrounds,
covariances as ``[N,3,3]``, the quantizer in front of ``[N,5]`` colours, the misaligned ``shN`` view, an ``sh_degree`` below the bands of K
and the call options handed on to ``chain``.

The table has two parts.  54 cases choose a route with every argument at its default.  41 more (``BASE`` names the case each is derived
from) change what no route decision reads and every route has to carry: the keys ``camera_model``, ``near_plane``, ``far_plane``,
``radius_clip``, ``eps2d`` (the call's and ``chain``'s), ``backgrounds=True`` (``route_scene`` adds a ``[C,D]`` array, drawn after everything
else, so that no other array moves), ``deg`` (the call's ``sh_degree`` where it is below ``int(sqrt(K)) - 1``) and ``sh_scale`` (multiplies
the SH coefficients of bands >= 1).  Every default is the behaviour without the key: the inputs of the 54 are bit for bit what they were."""
from __future__ import annotations

import math

import numpy as np

from oracle import gs_oracle as O
from projection_chain import DYN_KEYS, GATE_EPS, _grid, _np, chain
from util import garden, garden_sh

N_SPLATS, WIDTH, HEIGHT = 300, 48, 32  # two projection blocks; 3 x 2 tiles of 16 pixels
TIMESTAMP = 0.4
QCOLORS = (0.0, 1.0, 8)  # the colour quantizer of the "qcolors" cases
MASK_TEMPERATURE = 0.7
_TRIU = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])
_DEPTH_ONLY, _WITH_DEPTH, _EXPECTED = ("D", "ED"), ("RGB+D", "RGB+ED"), ("ED", "RGB+ED")


# The table of tests/test_gpu_routes.py (and of tests/test_render_chain_cpu.py's conditions): the keyword arguments of ``run_case`` by name.
MODES = ("RGB", "D", "ED", "RGB+D", "RGB+ED")

# colors: n3 / n5 [N,D] | cn3 [C,N,3] | sh [N,K,3] | csh [C,N,K,3] | pair (sh0, shN) | mask (sh0, MaskedShN) | mask_view (its shN a
# misaligned view); patch: {(module, attribute): value} for the duration of the call
CASES = {
    **{f"rows-{m}": dict(colors="n3", render_mode=m) for m in MODES},
    **{f"packed-{m}": dict(colors="n3", render_mode=m, packed=True) for m in MODES},
    "rows-n5": dict(colors="n5"),
    "rows-cn3": dict(colors="cn3", C=2),
    "packed-n5": dict(colors="n5", packed=True),
    "packed-cn3": dict(colors="cn3", C=2, packed=True),
    **{f"rows-sh{K}": dict(colors="sh", K=K) for K in (4, 9, 16)},
    **{f"rows-csh{K}": dict(colors="csh", K=K, C=2) for K in (4, 9, 16)},
    **{f"rows-pair{K}": dict(colors="pair", K=K) for K in (4, 9, 16)},
    "packed-sh16": dict(colors="sh", K=16, packed=True),
    "packed-csh16": dict(colors="csh", K=16, C=2, packed=True),
    "packed-pair16": dict(colors="pair", K=16, packed=True),
    "mask4": dict(colors="mask", K=4),
    "mask9": dict(colors="mask", K=9),
    "mask16": dict(colors="mask", K=16),
    "mask16-view": dict(colors="mask_view", K=16),
    "mask16-C2": dict(colors="mask", K=16, C=2, render_mode="RGB+D"),
    "packed-sparse_grad": dict(colors="n3", packed=True, sparse_grad=True),
    "covars": dict(colors="sh", K=16, covars=True),
    "pose-sh16": dict(colors="sh", K=16, pose_grads=True),
    "pose-pair16": dict(colors="pair", K=16, pose_grads=True),
    "pose-n3": dict(colors="n3", pose_grads=True),
    "antialiased-sh16": dict(colors="sh", K=16, antialiased=True),
    "antialiased-packed": dict(colors="sh", K=16, antialiased=True, packed=True),
    "absgrad": dict(colors="sh", K=16, absgrad=True),
    "deterministic": dict(colors="n3", deterministic=True),
    "channel_chunk2": dict(colors="n3", channel_chunk=2),
    "tile32": dict(colors="sh", K=16, tile_size=32),
    "rows-sh16-RGB+ED-C2": dict(colors="sh", K=16, C=2, render_mode="RGB+ED"),
    "dynamic-fused": dict(colors="n3", dynamic="plain"),
    "dynamic-fused-qcolors": dict(colors="n3", dynamic="qcolors"),
    "dynamic-detour-qcolors-n5": dict(colors="n5", dynamic="qcolors"),
    "dynamic-detour-sh16": dict(colors="sh", K=16, dynamic="plain"),
    "step-off-sh16": dict(colors="sh", K=16, patch={("_step", "ENABLED"): False}),
    "step-off-n3": dict(colors="n3", patch={("_step", "ENABLED"): False}),
    "two-launch-sh-bwd": dict(colors="sh", K=16, patch={("_wrapper", "_FUSE_SH_BWD"): False}),
    "two-launch-sh-bwd-mask16": dict(colors="mask", K=16, patch={("_wrapper", "_FUSE_SH_BWD"): False}),
    "prefill-off": dict(colors="sh", K=16, patch={("_wrapper", "PREFILL_ENABLED"): False}),
    "prefill-off-operators": dict(colors="sh", K=16, patch={("_wrapper", "PREFILL_ENABLED"): False, ("_step", "ENABLED"): False}),
    "pinned-direct-max-0": dict(colors="sh", K=16, patch={("_readback", "_PINNED_DIRECT_MAX"): 0}),
}

# ---- the call options, partial SH bands and clamped colours: a case of the table above (its BASE) with keys changed.  No option may
# change the route: tests/test_gpu_routes.test_native_call_sequence holds each of these to the recorded sequence of its base.
#   camera_model, near_plane, far_plane, radius_clip, eps2d   the call's; the chain's
#   backgrounds=True   a [C,D] leaf for the colour channels (zero on a depth channel), with its gradient
#   deg                the call's ``sh_degree`` where it is below the bands of K: the gradient of the bands above it is identically zero
#   sh_scale           multiplies the coefficients of bands >= 1: 6.0 gives std 0.3, which puts 5 ... 50 % of the visible colours below the clamp
# The values are those at which both builds of the chain agree on every radius, no colour lies within GATE_EPS of its clamp and at
# most 2 % of the pixels are borderline, and at which the option bites (tests/test_render_chain_cpu.py asserts all of it).
_NEAR_FAR = dict(near_plane=1.0, far_plane=3.0)
_COMBINED = dict(camera_model="fisheye", radius_clip=3.0, eps2d=0.1, backgrounds=True, **_NEAR_FAR)
_OPTIONS = {"ortho": dict(camera_model="ortho"), "fisheye": dict(camera_model="fisheye"), "nearfar": _NEAR_FAR,
            "radius_clip": dict(radius_clip=3.0), "eps2d": dict(eps2d=0.1), "bg": dict(backgrounds=True)}
_DERIVED = {
    # step driver, SH
    **{f"step-sh16-{o}": ("rows-sh16", v) for o, v in _OPTIONS.items()},
    "step-sh16-tile8": ("rows-sh16", dict(tile_size=8)),
    "step-sh16-aa-ortho-eps2d": ("antialiased-sh16", dict(camera_model="ortho", eps2d=0.1)),  # (the compensation depends on eps2d)
    # step driver, [N,3] colours
    **{f"step-n3-{o}": ("rows-RGB", _OPTIONS[o]) for o in ("fisheye", "nearfar", "bg")},
    # every option together, through the operators (a depth channel, whose background is zero; the pair with the step driver off)
    "combined-sh16-RGB+ED-C2": ("rows-sh16-RGB+ED-C2", _COMBINED),
    "combined-pair16": ("step-off-sh16", dict(colors="pair", **_COMBINED)),
    "combined-mask16-C2": ("mask16-C2", _COMBINED),
    # packed
    **{f"packed-sh16-{o}": ("packed-sh16", v) for o, v in _OPTIONS.items()},
    "packed-RGB+D-bg": ("packed-RGB+D", dict(backgrounds=True)),
    # the dynamic kernels
    "dynamic-fused-fisheye": ("dynamic-fused", dict(camera_model="fisheye")),
    "dynamic-fused-nearfar-clip": ("dynamic-fused", dict(radius_clip=3.0, **_NEAR_FAR)),
    "dynamic-fused-bg": ("dynamic-fused", dict(backgrounds=True)),
    # partial bands of K = 16
    **{f"step-sh16-deg{d}": ("rows-sh16", dict(deg=d)) for d in (0, 1, 2)},
    "pair16-deg1": ("rows-pair16", dict(deg=1)),
    "mask16-deg2": ("mask16", dict(deg=2)),
    "packed-sh16-deg1": ("packed-sh16", dict(deg=1)),
    "csh16-deg2": ("rows-csh16", dict(deg=2)),
    "two-launch-sh-bwd-deg1": ("two-launch-sh-bwd", dict(deg=1)),
    "step-off-sh16-deg0": ("step-off-sh16", dict(deg=0)),
    # colours below the clamp
    "clamp-sh16": ("rows-sh16", dict(sh_scale=6.0)),
    "clamp-sh16-C2": ("rows-sh16", dict(sh_scale=6.0, C=2)),  # (the camera sum of a gated gradient)
    "clamp-pair16": ("rows-pair16", dict(sh_scale=6.0)),
    "clamp-mask16": ("mask16", dict(sh_scale=7.0)),  # (at 6.0 the mask leaves one colour 5.8e-5 from its clamp; at 7.0 the nearest is 3.2e-3)
    "clamp-packed-sh16": ("packed-sh16", dict(sh_scale=6.0)),
    "clamp-csh16": ("rows-csh16", dict(sh_scale=6.0)),
    "clamp-sh16-deg1": ("rows-sh16", dict(sh_scale=6.0, deg=1)),
    "clamp-two-launch-sh-bwd": ("two-launch-sh-bwd", dict(sh_scale=6.0)),
}
OLD_CASES = tuple(CASES)
BASE = {name: base for name, (base, _) in _DERIVED.items()}
CASES.update({name: {**CASES[base], **changes} for name, (base, changes) in _DERIVED.items()})
CHAIN_OPTIONS = dict(camera_model="pinhole", eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0)  # (and their defaults)


def channels(colors, render_mode="RGB"):
    """Channels of the rendered image of a case."""
    d = 5 if colors == "n5" else 3
    return 1 if render_mode in _DEPTH_ONLY else d + (render_mode in _WITH_DEPTH)


def sh_degree_of(case):
    """The ``sh_degree`` of a case's call (None without SH): every band of K unless ``deg`` says less."""
    if not case.get("K"):
        return None
    full = int(case["K"] ** 0.5) - 1
    deg = case.get("deg")
    assert deg is None or 0 <= deg <= full, (deg, full)
    return full if deg is None else deg


def sh_band(colors, b):
    """-> (name of the input that holds band ``b`` of the SH coefficients, the index of that band in it)."""
    lo, hi = b * b, (b + 1) ** 2
    if colors in ("sh", "csh"):
        return "colors", (Ellipsis, slice(lo, hi), slice(None))
    assert colors in ("pair", "mask"), colors
    return ("sh0", (Ellipsis, slice(0, 1), slice(None))) if b == 0 else ("shN", (Ellipsis, slice(lo - 1, hi - 1), slice(None)))


def route_scene(colors, K=None, C=1, render_mode="RGB", covars=False, pose_grads=False, dynamic=None, backgrounds=False, sh_scale=None, **_):
    """The float32 numbers of one case of the routes table (the remaining options of a case choose a route or an argument, not an input):
    -> dict(P: the differentiable inputs by ``run_case``'s names, viewmats, Ks, weights [C,H,W,X] of the loss, width, height, and with
    ``backgrounds`` a [C,D] array for the colour channels).  ``sh_scale`` multiplies the SH coefficients of bands >= 1."""
    g = garden(N_SPLATS, scale_mult=4.0)
    n = N_SPLATS
    rs = np.random.RandomState(3)

    def R(*shape):
        return rs.random_sample(shape).astype(np.float32)

    F = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    P = {"means": F(g["means"]), "opacities": F(g["opacities"])}
    if covars:  # R diag(s^2) R^T, [N,3,3]
        q = g["quats"].astype(np.float64)
        w, x, y, z = (q / np.linalg.norm(q, axis=-1, keepdims=True)).T
        rot = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
        M = rot * g["scales"].astype(np.float64)[:, None, :]
        P["covars"] = F(M @ M.transpose(0, 2, 1))
    else:
        P["quats"], P["scales"] = F(g["quats"]), F(g["scales"])
    # (black splats would sit ON the clamp of the SH colour at degree 0 and near it above: their DC coefficient is moved off it)
    sh = garden_sh(np.clip(g["rgb"], 0.05, 1.0), K=K) if K else None
    if sh_scale is not None:
        sh[:, 1:] *= np.float32(sh_scale)
    if colors == "n3":
        P["colors"] = F(g["rgb"])
    elif colors == "n5":
        P["colors"] = F(np.concatenate([g["rgb"], R(n, 2)], 1))
    elif colors == "cn3":
        P["colors"] = F(np.repeat(F(g["rgb"])[None], C, 0) * R(C, 1, 1))
    elif colors == "sh":
        P["colors"] = F(sh)
    elif colors == "csh":
        P["colors"] = F(np.repeat(sh[None], C, 0))
    else:
        assert colors in ("pair", "mask", "mask_view"), colors
        P["sh0"] = F(sh[:, :1])
        P["shN"] = F(np.concatenate([R(1), sh[:, 1:].reshape(-1)])) if colors == "mask_view" else F(sh[:, 1:])
        if colors != "pair":
            P["mask_logits"] = F((R(n, 1, 1) - 0.5) * 4)
    if dynamic:
        P.update(motion=F(0.02 * (R(n, 9) - 0.5)), omega=F(0.1 * (R(n, 4) - 0.5)), trbf_center=R(n, 1), trbf_scale=F(R(n, 1) + 0.5))
    vm = F(g["viewmats"][:C])
    Ks = F(g["Ks"][:C]).copy()
    Ks[:, 0] *= WIDTH / g["width"]
    Ks[:, 1] *= HEIGHT / g["height"]
    if pose_grads:
        P["viewmats"] = vm
    S = dict(P=P, viewmats=vm, Ks=Ks, weights=R(C, HEIGHT, WIDTH, channels(colors, render_mode)), width=WIDTH, height=HEIGHT)
    if backgrounds:  # (drawn last: every other array is what it is without them)
        S["backgrounds"] = R(C, 5 if colors == "n5" else 3)
    return S


def soft_mask(bits, logits):
    """sigmoid(logits / temperature) in ``bits``-bit arithmetic (oracle/ada_mask_oracle.soft_mask is its float32 form), shaped like the logits."""
    f = _np(bits)
    return (f(1) / (f(1) + np.exp(-(np.asarray(logits, f) / f(np.float32(MASK_TEMPERATURE)))))).astype(f)


def render_chain(bits, case, cot=None, scene=None):
    """Forward and, with ``cot`` = dict(render [C,H,W,X], alphas [C,H,W,1]), the VJP of one case in ``bits``-bit arithmetic.

    case    a row of the routes table (the keyword arguments of ``run_case``); ``scene`` replaces ``route_scene(**case)`` (a dict of the same
            form, optionally with ``backgrounds`` [C,D] for the colour channels, which then is a differentiable input too).
    -> (out, grads): ``out`` holds render, alphas, radii, means2d, depths, conics, opacities, tiles_per_gauss, flatten_ids, isect_offsets,
    last_ids, ``borderline`` (bool [C,H,W]: a threshold decision of the compositing within a few ulp of flipping), the SH ``gate`` of
    ``chain`` and ``sh_raw`` (the SH value before + 0.5 and the clamp; None without SH); ``grads`` (None without ``cot``) one array per
    entry of ``P`` (and ``backgrounds``) plus ``means2d`` and ``absgrad`` [C,N,2]."""
    S = route_scene(**case) if scene is None else scene
    f = _np(bits)
    form, K, mode, ts = case["colors"], case.get("K"), case.get("render_mode", "RGB"), case.get("tile_size", 16)
    P, Ks, W, H = S["P"], S["Ks"], S["width"], S["height"]
    pose = "viewmats" in P
    vm = P["viewmats"] if pose else S["viewmats"]
    C, N = vm.shape[0], P["means"].shape[0]
    deg = sh_degree_of(case)

    # ---- what the projection chain takes
    CP = {k: P[k] for k in ("means", "opacities", "quats", "scales") if k in P}
    if "covars" in P:
        CP["covars"] = np.ascontiguousarray(P["covars"][:, _TRIU[0], _TRIU[1]])
    dyn = None
    if case.get("dynamic"):
        CP.update({k: P[k] for k in DYN_KEYS})
        dyn = dict(t=float(np.float32(TIMESTAMP)))
    quantized = case.get("dynamic") == "qcolors"
    mask = shN = None
    if form == "n3":
        CP["colors"] = P["colors"]
        if quantized:
            dyn["quantize"] = {"colors": QCOLORS}
    elif form == "sh":
        CP["sh"] = P["colors"]
    elif form in ("pair", "mask", "mask_view"):
        shN = (P["shN"][1:].reshape(N, K - 1, 3) if form == "mask_view" else P["shN"]).astype(f)
        rest = shN
        if form != "pair":
            mask = soft_mask(bits, P["mask_logits"]).reshape(N, 1, 1)
            rest = (shN * mask).astype(f)
        CP["sh"] = np.concatenate([P["sh0"].astype(f), rest], 1)
    else:
        assert form in ("n5", "cn3", "csh"), form
    assert not (pose and form == "csh"), "per-camera SH with pose gradients: not a case of the table"
    kw = dict(antialiased=bool(case.get("antialiased")), sh_degree=deg if "sh" in CP else None, dynamic=dyn, need_viewmats=pose,
              packed_formula=bool(case.get("packed")),  # (the reference's packed projection has a radius formula of its own)
              **{k: case.get(k, v) for k, v in CHAIN_OPTIONS.items()})
    o, _ = chain(bits, CP, vm, Ks, W, H, **kw)
    seen = o["radii"] > 0
    gate = o["gate"]

    # ---- colours the chain does not know
    dirs = coeffs = sh_raw = None
    if form == "n5":
        c5 = np.asarray(_grid(P["colors"], QCOLORS) if quantized else P["colors"], f)  # (straight-through: identity gradient)
        col = np.broadcast_to(c5[None], (C,) + c5.shape) * seen[..., None]
    elif form == "cn3":
        col = np.asarray(P["colors"], f) * seen[..., None]
    elif form == "csh":
        assert dyn is None
        campos = np.linalg.inv(np.asarray(vm, np.float64))[:, :3, 3].astype(f)
        dirs = np.ascontiguousarray(np.asarray(P["means"], f)[None] - campos[:, None])
        coeffs = np.ascontiguousarray(P["colors"], f)
        with O.precision(bits):
            sh_raw = O.sh_fwd(deg, dirs, coeffs, masks=seen)
        col = np.maximum(sh_raw + f(0.5), 0) * seen[..., None]
        gate = (np.abs(sh_raw + f(0.5)) <= GATE_EPS) & seen[..., None]
    else:
        col, sh_raw = o["colors"], o.get("sh_raw")
    col = np.ascontiguousarray(col, f)
    D = col.shape[-1]

    # ---- render channels, backgrounds
    depth_ch = o["depths"][..., None]
    cols = depth_ch if mode in _DEPTH_ONLY else (np.concatenate([col, depth_ch], -1) if mode in _WITH_DEPTH else col)
    cols = np.ascontiguousarray(cols, f)
    bg = None
    if S.get("backgrounds") is not None:
        b = np.asarray(S["backgrounds"], f)
        bg = np.zeros((C, 1), f) if mode in _DEPTH_ONLY else (np.concatenate([b, np.zeros((C, 1), f)], -1) if mode in _WITH_DEPTH else b)
        bg = np.ascontiguousarray(bg)

    # ---- binning (float32 oracle on this build's projection rounded to float32), compositing
    tw, th = math.ceil(W / ts), math.ceil(H / ts)
    tpg, ids, flat = O.isect_tiles(o["means2d"].astype(np.float32), o["radii"], o["depths"].astype(np.float32), ts, tw, th)
    offs = O.isect_offset_encode(ids, C, tw, th)
    geo = (o["means2d"], o["conics"], cols, np.ascontiguousarray(o["opacities"], f), W, H, ts, offs, flat)
    with O.precision(bits):
        rc, ra, li, bl = O.rasterize_fwd(*geo, backgrounds=bg, return_borderline=True)
    render = rc
    a_c = np.maximum(ra, f(1e-10))
    if mode in _EXPECTED:
        render = np.concatenate([rc[..., :-1], rc[..., -1:] / a_c], -1).astype(f)
    out = dict(render=render, alphas=ra, radii=o["radii"], means2d=o["means2d"], depths=o["depths"], conics=o["conics"], opacities=o["opacities"],
               tiles_per_gauss=tpg, flatten_ids=flat, isect_offsets=offs, last_ids=li, borderline=bl != 0, gate=gate, sh_raw=sh_raw)
    if cot is None:
        return out, None

    # ---- the VJP: expected depth, compositing, colours, projection chain
    v_rc, v_ra = np.array(cot["render"], f), np.array(cot["alphas"], f)
    if mode in _EXPECTED:  # e = d / max(a, 1e-10)
        v_e = v_rc[..., -1:]
        v_ra = v_ra - v_e * rc[..., -1:] / (a_c * a_c) * (ra > f(1e-10))
        v_rc[..., -1:] = v_e / a_c
    with O.precision(bits):
        v_m2, v_cn, v_cols, v_op, v_abs = O.rasterize_bwd(*geo, ra, li, np.ascontiguousarray(v_rc), np.ascontiguousarray(v_ra), backgrounds=bg,
                                                          absgrad=True)
    pcot = dict(means2d=v_m2, conics=v_cn, opacities=v_op)
    v_col = None
    if mode in _DEPTH_ONLY:
        pcot["depths"] = v_cols[..., 0]
    elif mode in _WITH_DEPTH:
        v_col, pcot["depths"] = v_cols[..., :-1], v_cols[..., -1]
    else:
        v_col = v_cols
    if v_col is not None and ("colors" in CP or "sh" in CP):
        pcot["colors"] = v_col
    _, g = chain(bits, CP, vm, Ks, W, H, cot=pcot, **kw)

    G = {k: g[k] for k in P if k in g and k not in ("colors", "covars")}
    if "covars" in P:
        G["covars"] = np.zeros((N, 3, 3), f)
        G["covars"][:, _TRIU[0], _TRIU[1]] = g["covars"]
    vz = np.zeros((C, N, D), f) if v_col is None else v_col * seen[..., None]
    if form == "n3":
        G["colors"] = g["colors"]
    elif form == "sh":
        G["colors"] = g["sh"]
    elif form == "n5":
        G["colors"] = vz.sum(0)
    elif form == "cn3":
        G["colors"] = vz  # per camera: no sum
    elif form == "csh":
        with O.precision(bits):
            v_coeffs, v_dirs = O.sh_bwd(deg, dirs, coeffs, np.ascontiguousarray(vz * (sh_raw + f(0.5) > 0)), masks=seen)
        G["colors"] = v_coeffs
        G["means"] = G["means"] + v_dirs.sum(0)  # dirs = means - campos
    else:
        G["sh0"], v_rest = g["sh"][:, :1], g["sh"][:, 1:]
        if mask is None:
            v_shN = v_rest
        else:
            v_shN = v_rest * mask
            v_m = (v_rest * shN).reshape(N, -1).sum(1).reshape(N, 1, 1)
            G["mask_logits"] = (v_m * (f(1) - mask) * mask / f(np.float32(MASK_TEMPERATURE))).astype(f).reshape(P["mask_logits"].shape)
        G["shN"] = np.concatenate([np.zeros(1, f), v_shN.reshape(-1)]) if form == "mask_view" else v_shN
    if S.get("backgrounds") is not None:  # render = sum + (1 - alpha) background, on the colour channels
        G["backgrounds"] = np.zeros(S["backgrounds"].shape, f) if mode in _DEPTH_ONLY else \
            (v_rc[..., :S["backgrounds"].shape[-1]] * (f(1) - ra)).sum((1, 2)).astype(f)
    G = {k: np.asarray(v, f) for k, v in G.items()}
    G["means2d"], G["absgrad"] = v_m2, v_abs
    assert set(P) <= set(G), (sorted(P), sorted(G))
    return out, G
