"""Every route through the projection backward against the float64 chain of tests/projection_chain.py, at OPERATOR level (no compositing
in between: the only discrete decision left is ``radii > 0``).

    rows      gs_projection_rows_bwd        _wrapper.project_rows: what rasterization() runs for unpacked batches -- gradients read from
                                            64-byte rows, v_opacities / v_compensations when antialiased, per-camera colour sums, the SH VJP in
                                            the same lane or gs_sh_view_bwd's v_means_add, NEED_VIEW block reductions
    rows_dyn  gs_projection_rows_dyn_bwd    the same with the temporal slice, exp / sigmoid and the round STE evaluated in the kernel
    packed    gs_projection_packed_bwd      fully_fused_projection(packed=True): plain stores (C = 1), atomics, sparse values, the NEED_VIEW
                                            wave reduction with camera boundaries in mid-wave
    array     gs_projection_bwd             fully_fused_projection(packed=False) with covars [N, 6], all four cotangents

ONE scene: 549 splats = two full blocks of 256 + a 37-lane partial wave; splats 256..511 lie behind every camera, so block 1 has no visible
lane (the ``s != 0`` skip of the block reductions, the ``any == false`` stores); three cameras, and splats seen by none, one and all of them.

Per case, for every gradient (printed as a table with ``pytest -s``; the MI355X run is profiles/projection_routes_parity.txt):

    e_hip = rel_l2(HIP, f64) <= max(1e-4, 4 e32),   e32 = rel_l2(the chain evaluated in float32, f64)
    max|HIP - f64| <= min(2e-4, max(1e-4, 4 max|f32 - f64| / max|f64|)) max|f64|
    rows of splats no camera sees are exactly zero

and every forward output to 1e-4 of float64 where visible.  The fp32 chain is the REFERENCE's arithmetic in float32, never the code under test:
where it is within 2.5e-5 of float64 the fixed 1e-4 is the bar.  That holds (and is asserted) for every pinhole quats + scales case under the
full set of cotangents, and on this scene for every other case too except v_quats of the three ortho rows cases (e32 3.2e-5 ... 4.0e-5: bar
1.3e-4 ... 1.6e-4) and v_means of pinhole-aa-opacities-only (2.6e-5: the compensation's VJP alone, a determinant that cancels).  The max-norm
bar rides on 4 x the fp32 chain's own worst entry (2.5e-5 ... 5.5e-5 of the largest entry) for v_quats / v_scales / v_omega of the ortho,
fisheye and dynamic cases and for v_covars everywhere; the cap of 2e-4 is reached by ortho-classic v_quats alone."""
import numpy as np
import pytest

from projection_chain import DYN_KEYS, chain
from util import assert_close, garden, rel_l2

pytestmark = pytest.mark.gpu

N_SPLATS, BEHIND = 549, slice(256, 512)
BDS = dict(scales=(-10.0, 2.0, 8), quats=(-1.0, 1.0, 8), opacities=(-7.0, 7.0, 8), colors=(-7.5, 7.5, 8))  # (test_gpu_dynamic_fused.BDS)
FACTOR = 4.0
_SCENE = {}


def _scene():
    """The one scene (float32 numpy), built once and never modified."""
    if _SCENE:
        return _SCENE
    fx = garden(N_SPLATS - 256, scale_mult=3.0)
    rs = np.random.RandomState(17)
    vm = fx["viewmats"][:3].astype(np.float32)
    idx = np.r_[0:256, 512:N_SPLATS]
    S = {k: np.zeros((N_SPLATS,) + fx[k].shape[1:], np.float32) for k in ("means", "quats", "scales", "opacities", "rgb")}
    for k in S:
        S[k][idx] = fx[k]
        S[k][BEHIND] = fx[k][rs.randint(0, fx[k].shape[0], 256)]
    # behind every camera: against the mean viewing direction, four units from the origin (camera z about -1.4)
    fwd = vm[:, 2, :3].sum(0)
    S["means"][BEHIND] = (-4.0 * fwd / np.linalg.norm(fwd) + 0.2 * rs.randn(256, 3)).astype(np.float32)
    S["opacities"] = np.clip(S["opacities"], 1e-3, 1 - 1e-3).astype(np.float32)
    # covariances R diag(s^2) R^T of the same splats, upper triangle [xx, xy, xz, yy, yz, zz]
    q = S["quats"].astype(np.float64)
    w, x, y, z = (q / np.linalg.norm(q, axis=-1, keepdims=True)).T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    M = R * S["scales"].astype(np.float64)[:, None, :]
    cov = M @ M.transpose(0, 2, 1)
    S["covars"] = cov[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]].astype(np.float32)
    S["sh"] = (rs.randn(N_SPLATS, 25, 3) * 0.3).astype(np.float32)
    S["sh"][:, 0] = (np.clip(S["rgb"], 0.05, 1.0) - 0.5) / 0.2820947917738781  # (black splats would sit ON the clamp at degree 0)
    # the temporal tensors, raw (log trbf_scale) -- the activated forms are derived per case
    S.update(trbf_center=rs.uniform(0, 1, (N_SPLATS, 1)).astype(np.float32), trbf_scale=rs.uniform(-1.5, 0.5, (N_SPLATS, 1)).astype(np.float32),
             motion=(0.02 * rs.randn(N_SPLATS, 9)).astype(np.float32), omega=(0.1 * rs.randn(N_SPLATS, 4)).astype(np.float32))
    S.update(viewmats=vm, Ks=fx["Ks"][:3].astype(np.float32), width=fx["width"], height=fx["height"])
    _SCENE.update(S)
    return _SCENE


def _spec(route, name, **kw):
    d = dict(route=route, name=name, geom="qs", cm="pinhole", aa=False, C=3, pose=False, color=None, K=None, deg=None, split=False, fuse=True,
             dyn=None, sparse=False, cot=None)
    assert set(kw) <= set(d), kw
    d.update(kw)
    return pytest.param(d, id=f"{route}-{name}")


def _cases():
    cs = []
    for cm in ("pinhole", "ortho", "fisheye"):
        for aa in (False, True):
            cs.append(_spec("rows", f"{cm}-{'aa' if aa else 'classic'}", cm=cm, aa=aa, color="colors"))
        cs.append(_spec("rows", f"{cm}-aa-pose", cm=cm, aa=True, color="colors", pose=True))
    for cm in ("pinhole", "fisheye"):
        for pose in (False, True):
            cs.append(_spec("rows", f"covars-{cm}-aa{'-pose' if pose else ''}", geom="covars", cm=cm, aa=True, color="colors", pose=pose))
    cs.append(_spec("rows", "C1-pinhole-aa", C=1, aa=True, color="colors"))
    # the SH VJP in the projection backward's own lane
    for deg in (0, 1, 2, 3):
        cs.append(_spec("rows", f"sh-K16-deg{deg}", color="sh", K=16, deg=deg))
    cs.append(_spec("rows", "sh-split-K16-deg3", color="sh", K=16, deg=3, split=True))
    cs.append(_spec("rows", "sh-K4-deg1", color="sh", K=4, deg=1))
    cs.append(_spec("rows", "sh-K16-deg3-fisheye", color="sh", K=16, deg=3, cm="fisheye"))
    cs.append(_spec("rows", "sh-K16-deg2-aa", color="sh", K=16, deg=2, aa=True))
    # gs_sh_view_bwd first, its direction gradient handed over as v_means_add
    cs.append(_spec("rows", "sh-unfused-K9-deg2", color="sh", K=9, deg=2))
    cs.append(_spec("rows", "sh-unfused-K25-deg4", color="sh", K=25, deg=4))
    cs.append(_spec("rows", "sh-unfused-K16-deg3-switch", color="sh", K=16, deg=3, fuse=False))
    # dynamic rows
    for cm in ("pinhole", "fisheye"):
        for aa in (False, True):
            cs.append(_spec("rows_dyn", f"activated-{cm}-{'aa' if aa else 'classic'}", cm=cm, aa=aa, color="colors", dyn=dict(t=0.37)))
    raw = ("scales", "opacities", "trbf_scale")
    cs.append(_spec("rows_dyn", "raw-pinhole-aa", aa=True, color="colors", dyn=dict(t=0.37, raw=raw)))
    cs.append(_spec("rows_dyn", "raw-quantized-pinhole-aa", aa=True, color="colors", dyn=dict(t=0.37, raw=raw, quantize=BDS)))
    cs.append(_spec("rows_dyn", "min_trbf-pinhole-aa", aa=True, color="colors", dyn=dict(t=0.37, min_trbf=0.05)))
    # one cotangent alone, so that a term the full set of cotangents drowns is the whole gradient: v_means is then the SH direction
    # gradient and nothing else (it is 1e-3 of v_means under all five cotangents), v_means / v_quats / v_scales the compensation's VJP
    cs.append(_spec("rows", "sh-K16-deg3-colors-only", color="sh", K=16, deg=3, cot=("colors",)))
    cs.append(_spec("rows", "sh-unfused-K9-deg2-colors-only", color="sh", K=9, deg=2, cot=("colors",)))
    cs.append(_spec("rows", "pinhole-aa-opacities-only", aa=True, color="colors", cot=("opacities",)))
    cs.append(_spec("rows_dyn", "activated-pinhole-aa-opacities-only", aa=True, color="colors", dyn=dict(t=0.37), cot=("opacities",)))
    # packed
    cs.append(_spec("packed", "C1-pinhole", C=1))
    cs.append(_spec("packed", "C3-pinhole"))
    cs.append(_spec("packed", "C3-pinhole-sparse", sparse=True))
    cs.append(_spec("packed", "C3-pinhole-pose", pose=True))
    cs.append(_spec("packed", "C3-pinhole-comp-pose", aa=True, pose=True))
    cs.append(_spec("packed", "C3-covars-pinhole-comp", geom="covars", aa=True))
    cs.append(_spec("packed", "C3-fisheye", cm="fisheye"))
    cs.append(_spec("packed", "C3-covars-fisheye-comp-pose", geom="covars", cm="fisheye", aa=True, pose=True))
    # array form with covars
    for cm in ("pinhole", "ortho", "fisheye"):
        for aa in (False, True):
            for pose in (False, True):
                cs.append(_spec("array", f"covars-{cm}{'-comp' if aa else ''}{'-pose' if pose else ''}", geom="covars", cm=cm, aa=aa, pose=pose))
    return cs


def _inputs(sp):
    """-> (P: the differentiable float32 inputs by the chain's names, kw: the chain's options, cameras)"""
    S = _scene()
    P = {"means": S["means"]}
    if sp["geom"] == "covars":
        P["covars"] = S["covars"]
    else:
        P["quats"], P["scales"] = S["quats"], S["scales"]
    if sp["route"] in ("rows", "rows_dyn"):
        P["opacities"] = S["opacities"]
        if sp["color"] == "colors":
            P["colors"] = S["rgb"]
        else:
            P["sh"] = np.ascontiguousarray(S["sh"][:, :sp["K"]])
    dyn = sp["dyn"]
    if dyn is not None:
        raw = dyn.get("raw", ())
        for k in DYN_KEYS:
            P[k] = S[k]
        if "trbf_scale" not in raw:
            # (narrow lifetimes where the temporal filter is on: many splats are off at t)
            P["trbf_scale"] = np.exp(S["trbf_scale"]) * (0.35 if dyn.get("min_trbf") is not None else 1.0)
        if "scales" in raw:
            P["scales"] = np.log(S["scales"])
        if "opacities" in raw:
            P["opacities"] = np.log(S["opacities"] / (1 - S["opacities"]))
        if dyn.get("quantize"):  # some values beyond the quantizer's range: clamped, with the identity gradient
            P = {k: np.array(v) for k, v in P.items()}
            P["quats"][:5, 1], P["opacities"][:9], P["colors"][:4, 2] = -1.75, 8.0, 7.75
    P = {k: np.ascontiguousarray(v, np.float32) for k, v in P.items()}
    C = sp["C"]
    kw = dict(camera_model=sp["cm"], antialiased=sp["aa"], sh_degree=sp["deg"], dynamic=dyn, packed_formula=sp["route"] == "packed",
              need_viewmats=sp["pose"])
    return P, kw, S["viewmats"][:C], S["Ks"][:C]


OUTPUTS = ("means2d", "depths", "conics", "opacities", "colors", "compensations")


def _hip(sp, P, vm, Ks, W, H):
    """The route's forward on the GPU -> (dense outputs by name incl. radii [C,N], backward(cot) -> gradients by the chain's names)."""
    import torch

    from gscodec_studio_amd import _wrapper as ops
    from gscodec_studio_amd import fully_fused_projection
    from util import N, T

    C, n = vm.shape[0], P["means"].shape[0]
    t = {k: T(v, True) for k, v in P.items()}
    vmt, Kt = T(vm, sp["pose"]), T(Ks)
    cm, aa = sp["cm"], sp["aa"]

    def collect():
        g = {}
        for k, p in t.items():
            assert p.grad is not None, k
            g[k] = p.grad
        if sp["pose"]:
            g["viewmats"] = vmt.grad
        return g

    if sp["route"] in ("rows", "rows_dyn"):
        sh = sh_rest = ds = None
        if "sh" in t:
            if sp["split"]:  # the trainer's (sh0, shN): two leaves whose gradients concatenate to the chain's one
                t0, tN = T(P["sh"][:, :1], True), T(P["sh"][:, 1:], True)
                sh, sh_rest = t0, tN
            else:
                sh = t["sh"]
        if sp["dyn"] is not None:
            from gscodec_studio_amd.dynamic import DynamicSlice

            d = sp["dyn"]
            ds = DynamicSlice(t["motion"], t["omega"], t["trbf_center"], t["trbf_scale"], d["t"], raw=d.get("raw", ()), quantize=d.get("quantize"),
                              min_trbf=d.get("min_trbf"))

        class switch:  # _wrapper._FUSE_SH_BWD as the case wants it, restored afterwards (the backward reads it)
            def __enter__(self):
                self.saved = ops._FUSE_SH_BWD
                ops._FUSE_SH_BWD = self.saved and sp["fuse"]

            def __exit__(self, *a):
                ops._FUSE_SH_BWD = self.saved

        with switch():
            if "sh" in t:
                fusable = ops.sh_bwd_fusable(sp["K"], sh, sh_rest, sp["pose"])
                assert fusable == (sp["fuse"] and sp["K"] % 4 == 0), "the case must take the SH route it is named after"
            radii, m2, dep, cn, op, col, _ = ops.project_rows(
                t["means"], t.get("covars"), t.get("quats"), t.get("scales"), vmt, Kt, W, H, t["opacities"], t.get("colors"), antialiased=aa,
                camera_model=cm, sh_coeffs=sh, sh_degree=sp["deg"], sh_rest=sh_rest, dynamic=ds)
        out = dict(radii=N(radii), means2d=N(m2), depths=N(dep), conics=N(cn), opacities=N(op), colors=N(col))

        def backward(cot):
            with switch():
                torch.autograd.backward([m2, dep, cn, op, col], [T(cot[k]) for k in ("means2d", "depths", "conics", "opacities", "colors")])
            if sp["split"]:
                t["sh"].grad = torch.cat((t0.grad, tN.grad), 1)
            return {k: N(v) for k, v in collect().items()}
        return out, backward

    args = (t["means"], t.get("covars"), t.get("quats"), t.get("scales"), vmt, Kt, W, H)
    if sp["route"] == "array":
        radii, m2, dep, cn, comp = fully_fused_projection(*args, packed=False, calc_compensations=aa, camera_model=cm)
        out = dict(radii=N(radii), means2d=N(m2), depths=N(dep), conics=N(cn))
        outs, names = [m2, dep, cn], ["means2d", "depths", "conics"]
        if aa:
            out["compensations"] = N(comp)
            outs.append(comp)
            names.append("compensations")

        def backward(cot):
            torch.autograd.backward(outs, [T(cot[k]) for k in names])
            return {k: N(v) for k, v in collect().items()}
        return out, backward

    # packed: [nnz] outputs, scattered to [C, N] here; the cotangents are gathered back at (camera, gaussian)
    def run(sparse):
        for p in list(t.values()) + [vmt]:
            p.grad = None
        return fully_fused_projection(*args, packed=True, sparse_grad=sparse, calc_compensations=aa, camera_model=cm)

    res = run(sp["sparse"])
    cam, gau = N(res[0]), N(res[1])
    assert (np.diff(cam * n + gau) > 0).all(), "rows sorted by (camera, gaussian)"
    assert C == 1 or (np.bincount(cam, minlength=C) % 64 != 0).all(), "camera boundaries in mid-wave (as _structure asked of the oracle)"
    names = ["means2d", "depths", "conics"] + (["compensations"] if aa else [])
    out = {"radii": np.zeros((C, n), np.int32)}
    out["radii"][cam, gau] = N(res[2])
    for k, v in zip(names, res[3:]):
        out[k] = np.zeros((C, n) + tuple(v.shape[1:]), np.float32)
        out[k][cam, gau] = N(v)

    def backward(cot):
        def grads_of(r):
            torch.autograd.backward(list(r[3:3 + len(names)]), [T(np.ascontiguousarray(cot[k][cam, gau])) for k in names])
            return collect()

        g = grads_of(res)
        if sp["sparse"]:
            per_splat = {k: v for k, v in g.items() if k != "viewmats"}
            for k, v in per_splat.items():
                assert v.is_sparse and v._values().shape[0] == len(cam), (k, v._values().shape, len(cam))
            g = {k: (v.to_dense() if v.is_sparse else v) for k, v in g.items()}
            g = {k: N(v) for k, v in g.items()}
            dense = {k: N(v) for k, v in grads_of(run(False)).items()}
            for k in per_splat:  # the same sums, added by coalescing here and by atomics there
                assert rel_l2(g[k], dense[k]) <= 1e-6, ("sparse vs dense", k, rel_l2(g[k], dense[k]))
            return g
        return {k: N(v) for k, v in g.items()}
    return out, backward


RHO = 4 * 2.0 ** -24


def _compensation_cond(o64, eps2d=0.3):
    """How far ONE unit of relative roundoff in the 2D covariance moves the antialias compensation sqrt(det / det_blurred), per pair.

    det = xx yy - xy^2 cancels for a needle-shaped splat: entries that each carry a relative error rho leave det with an absolute error of
    up to 2 rho (xx yy + xy^2), and the compensation c = sqrt(det / det_b) with that over 2 c det_b: rho (xx yy + xy^2) / (c det_b).  No float32
    evaluation -- the reference's included -- can promise 1e-4 relative where this factor is in the thousands (it reaches 1500 on this scene
    under the orthographic camera, where the reference's own float32 run is off by 2.2e-4 of the value at one pair and the kernels by
    2.4e-4 at another).  The forward bar of the compensation and of the compensated opacity therefore is 1e-4 relative + RHO x this factor with
    RHO = 4 x 2^-24: every entry of the 2D covariance comes out of two 3 x 3 congruences (a dozen roundings each), so four units of roundoff
    is less than what it may carry.  Evaluated from the float64 run's conics (the inverse of the blurred covariance)."""
    cn, comp = o64["conics"], o64["compensations"]
    seen = o64["radii"] > 0
    det_c = np.where(seen, cn[..., 0] * cn[..., 2] - cn[..., 1] ** 2, 1.0)
    xx, yy, xy = cn[..., 2] / det_c - eps2d, cn[..., 0] / det_c - eps2d, -cn[..., 1] / det_c
    return np.where(seen, (np.abs(xx * yy) + xy * xy) * det_c / np.where(seen, comp, 1.0), 0.0)


def _structure(sp, r64):
    """What the scene must exercise, asserted from the float64 oracle's radii."""
    seen = r64 > 0
    assert not seen[:, BEHIND].any(), "block 1 has no visible lane"
    if sp["C"] == 3:
        per = seen.sum(0)
        front = np.r_[per[:256], per[512:]]
        assert (front == 0).any() and (front == 1).any() and (front == 3).any(), np.bincount(per, minlength=4)
    if sp["route"] == "packed":
        nnz = seen.sum(1)
        assert (nnz % 64 != 0).all() and (nnz > 64).all(), nnz  # camera boundaries fall in mid-wave, the last wave is partial


def run_case(sp, hip=_hip):
    """One case end to end; ``hip`` may be replaced by another evaluation with _hip's interface (the CPU dry run of this file's conditions)."""
    P, kw, vm, Ks = _inputs(sp)
    S = _scene()
    W, H = S["width"], S["height"]
    o32, _ = chain(32, P, vm, Ks, W, H, **kw)
    o64, _ = chain(64, P, vm, Ks, W, H, **kw)
    _structure(sp, o64["radii"])
    if sp["dyn"] is not None and sp["dyn"].get("min_trbf") is not None:
        S0 = dict(sp["dyn"], min_trbf=None)
        full, _ = chain(64, P, vm, Ks, W, H, **dict(kw, dynamic=S0))
        assert ((full["radii"] > 0) & ~(o64["radii"] > 0)).sum() > 20, "the temporal filter must cull splats that are in view"

    out, backward = hip(sp, P, vm, Ks, W, H)
    vis = (out["radii"] > 0) & (o32["radii"] > 0) & (o64["radii"] > 0)
    gate = o32["gate"] | o64["gate"]
    # conditions of the comparison, not measurements
    assert vis.sum() >= 0.99 * (o64["radii"] > 0).sum(), (vis.sum(), (o64["radii"] > 0).sum())
    assert gate[vis].mean() <= 0.01, gate[vis].mean()

    # ---- forward, where visible, against float64
    floors = dict(means2d=(1e-4, 1e-3, 0.0), depths=(1e-5, 1e-6, 0.0), conics=(1e-4, 1e-7, 2e-4), opacities=(1e-4, 1e-7, 0.0),
                  compensations=(1e-4, 1e-7, 0.0), colors=(1e-4, 1e-5, 0.0))
    names = [k for k in OUTPUTS if k in out and k in o64]
    for k in names:
        rtol, atol, bad = floors[k]
        sel = (vis[..., None] & ~gate) if k == "colors" else vis
        a, e = np.asarray(out[k], np.float64), np.asarray(o64[k], np.float64)
        tol = atol + rtol * np.abs(e)
        if sp["aa"] and k in ("opacities", "compensations"):
            scale = e / np.where(vis, o64["compensations"], 1.0) if k == "opacities" else 1.0  # (the opacity the compensation multiplies)
            tol = tol + RHO * _compensation_cond(o64) * scale
        miss = (np.abs(a - e) > tol)[sel]
        i = int(np.argmax((np.abs(a - e) - tol)[sel]))
        assert miss.mean() <= bad, (f"{sp['route']} {sp['name']}: {k} vs f64", int(miss.sum()), miss.size, a[sel][i], e[sel][i])

    # ---- backward: standard normal cotangents on every differentiable output, zero outside vis and on gate-flagged colours
    rs = np.random.RandomState(3)
    cot = {}
    for k in names:
        m = vis.reshape(vis.shape + (1,) * (o64[k].ndim - 2))
        cot[k] = (rs.randn(*o64[k].shape) * m * (sp["cot"] is None or k in sp["cot"])).astype(np.float32)
    if "colors" in cot:
        cot["colors"] = cot["colors"] * ~gate
    _, g32 = chain(32, P, vm, Ks, W, H, cot=cot, vis=vis, **kw)
    _, g64 = chain(64, P, vm, Ks, W, H, cot=cot, vis=vis, **kw)
    g = backward(cot)
    assert set(g) == set(g64), (sorted(g), sorted(g64))
    unseen = ~(out["radii"] > 0).any(0)
    assert unseen[BEHIND].all() and unseen.sum() > 256
    failures = []
    for k in g64:
        h, a, b = np.asarray(g[k], np.float64), np.asarray(g32[k], np.float64), np.asarray(g64[k], np.float64)
        assert h.shape == b.shape, (k, h.shape, b.shape)
        if k == "viewmats":
            assert not h[:, 3].any(), "the bottom row of v_viewmats stays zero"
            h, a, b = h[:, :3, :4], a[:, :3, :4], b[:, :3, :4]
        else:
            assert not h[unseen].any(), (k, "rows of splats no camera sees are exactly zero")
        if sp["cot"] is not None and not b.any():  # (a parameter the one cotangent does not reach)
            assert not h.any(), k
            continue
        assert np.abs(b).max() > 0, k
        e_hip, e32 = rel_l2(h, b), rel_l2(a, b)
        bar = max(1e-4, FACTOR * e32)
        if sp["cm"] == "pinhole" and sp["geom"] == "qs" and sp["cot"] is None:  # (the compensation's VJP alone is at 2.6e-5 in v_means)
            assert e32 <= 2.5e-5, (k, e32, "a pinhole quats + scales case is held to the fixed 1e-4")
        top = np.abs(b).max()
        m_hip, m32 = np.abs(h - b).max() / top, np.abs(a - b).max() / top
        m_bar = min(2e-4, max(1e-4, FACTOR * m32))
        row = f"{sp['route']:9s} {sp['name']:32s} v_{k:12s} e_hip {e_hip:.2e}  e32 {e32:.2e}  bar {bar:.2e} | max {m_hip:.2e}  max32 {m32:.2e}  bar {m_bar:.2e}"
        print(row)
        if not (e_hip <= bar and m_hip <= m_bar):
            failures.append(row)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("sp", _cases())
def test_route_against_the_float64_chain(sp):
    run_case(sp)
